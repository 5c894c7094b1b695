// wm_corr_rule.hpp -- the rule of wm_corr_ransac (include/wavematch.h, "pose from correspondences") where it is
// evaluated more than once: by a lane of k_corr_hypotheses and k_corr_model, by every lane of k_corr_count and the
// selection, and by the host (wm_corr_hypothesis, the refit, the automatic sample distance).  It exists ONCE, for host
// and device: the same operations in the same order give the same bits.  No HIP header of its own: the file compiles
// with a plain C++ compiler (tests/cpp_host/corr_rule_host.cpp runs it under the sanitizers).
//
// Nothing here may be fused: the library is built with -ffp-contract=off on both sides (csrc/Makefile), and a host
// program that includes this file must be built the same way.  Divisions and square roots are the IEEE ones.
#pragma once
#include <float.h>
#include <math.h>

#include "wm_math.hpp"

namespace wm {

enum : unsigned { kCorrSkipped = 0u, kCorrValid = 1u };  // (= kSacSkipped / kSacValid of wm_sac_walk.hpp)

WM_HD bool corr_finite(float v) { return v - v == 0.f; }
WM_HD bool corr_finite(double v) { return v - v == 0.0; }

// (dx dx + dy dy) + dz dz of two points, float
WM_HD float corr_dist2(const float *a, const float *b) {
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// The sample test: p = the three SOURCE points of the sample, x y z each.  true: the entry is skipped.
WM_HD bool corr_sample_bad(const float p[9], float min_d2) {
    if (!(corr_dist2(p, p + 3) > min_d2) || !(corr_dist2(p, p + 6) > min_d2) || !(corr_dist2(p + 3, p + 6) > min_d2)) return true;
    // s = |(p1 - p0) x (p2 - p0)|^2, as the plane rule forms it
    const float ux = p[3] - p[0], uy = p[4] - p[1], uz = p[5] - p[2];
    const float vx = p[6] - p[0], vy = p[7] - p[1], vz = p[8] - p[2];
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    const float s = (cx * cx + cy * cy) + cz * cz;
    return !(corr_finite(s) && s > 0.f);
}

// Entry of the stream: the rigid transform of three pairs (p: source, q: target, sample order) as twelve floats, rows
// 0 ... 2 of [R | t]; kCorrSkipped with T zero, or kCorrValid.
WM_HD unsigned corr_hypothesis(const float p[9], const float q[9], float min_d2, float T[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.f;
    if (corr_sample_bad(p, min_d2)) return kCorrSkipped;
    double st[kStatsLen];
#pragma unroll
    for (int i = 0; i < kStatsLen; ++i) st[i] = 0.0;
    st[kSvdN] = 3.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        st[kSvdSp + a] = ((double) p[a] + (double) p[3 + a]) + (double) p[6 + a];
        st[kSvdSq + a] = ((double) q[a] + (double) q[3 + a]) + (double) q[6 + a];
#pragma unroll
        for (int b = 0; b < 3; ++b)
            st[kSvdSqp + a * 3 + b] = ((double) q[a] * (double) p[b] + (double) q[3 + a] * (double) p[3 + b]) +
                                      (double) q[6 + a] * (double) p[6 + b];
    }
    double Td[16];
    umeyama_from_stats<false>(st, Td);
    bool ok = true;
    float Tf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        Tf[i] = (float) Td[i];
        ok = ok && corr_finite(Tf[i]);
    }
    if (!ok) return kCorrSkipped;
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = Tf[i];
    return kCorrValid;
}

// d2 of a pair under T: x' = ((r00 x + r01 y) + r02 z) + tx, ..., d2 = (dx dx + dy dy) + dz dz with dx = x' - qx.
// 26 float operations.
WM_HD float corr_pair_d2(const float T[12], float x, float y, float z, float qx, float qy, float qz) {
    const float dx = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - qx;
    const float dy = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - qy;
    const float dz = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- the host's steps

inline float corr_min_d2_given(double d) { return (float) (d * d); }  // (min_sample_distance >= 0)

// The automatic sample distance of the nine sums over the mv pairs' source points relative to the first one
// ([0..2] sum dx dy dz, [3..8] sum dxdx dxdy dxdz dydy dydz dzdz): ((sqrt l0 + sqrt l1 + sqrt l2) / 3)^2 with l the
// eigenvalues of the covariance normalised by mv, clamped at 0; 0 when poisoned or not finite.
inline float corr_min_d2_from_sums(const double *sum, bool poison, double mv) {
    if (poison || !(mv > 0)) return 0.f;
    const double mx = sum[0] / mv, my = sum[1] / mv, mz = sum[2] / mv;
    const double cxx = sum[3] / mv - mx * mx, cxy = sum[4] / mv - mx * my, cxz = sum[5] / mv - mx * mz;
    const double cyy = sum[6] / mv - my * my, cyz = sum[7] / mv - my * mz, czz = sum[8] / mv - mz * mz;
    const double C[9] = {cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz};
    for (double v : C)
        if (!corr_finite(v)) return 0.f;
    double U[9], S[3], V[9];
    svd3<false>(C, U, S, V);  // (symmetric: the singular values are the eigenvalues' magnitudes)
    double r = 0.0;
    for (int k = 0; k < 3; ++k) r += sqrt(S[k] > 0.0 ? S[k] : 0.0);
    r /= 3.0;
    const float f = (float) (r * r);
    return corr_finite(f) ? f : 0.f;
}

constexpr int kCorrRefitComps = 15;  // [0..2] sum dp, [3..5] sum dq, [6..14] sum dq_a dp_b (a the row)

// The refit: Umeyama over the model's n inliers from the fifteen sums relative to (p0, q0), t recomposed as
// q0 + t' - R p0.  false: poisoned or not finite, the model stays.
inline bool corr_refit_from_sums(const double *sum, bool poison, double n, const float p0[3], const float q0[3], double T[16]) {
    if (poison || !(n >= 3.0)) return false;
    double st[kStatsLen];
    for (int i = 0; i < kStatsLen; ++i) st[i] = 0.0;
    st[kSvdN] = n;
    for (int i = 0; i < 3; ++i) {
        st[kSvdSp + i] = sum[i];
        st[kSvdSq + i] = sum[3 + i];
    }
    for (int i = 0; i < 9; ++i) st[kSvdSqp + i] = sum[6 + i];
    for (int i = 0; i < kCorrRefitComps; ++i)
        if (!corr_finite(sum[i])) return false;
    double Td[16];
    umeyama_from_stats<false>(st, Td);
    for (int i = 0; i < 3; ++i) {
        const double Rp = (Td[i * 4] * (double) p0[0] + Td[i * 4 + 1] * (double) p0[1]) + Td[i * 4 + 2] * (double) p0[2];
        Td[i * 4 + 3] = ((double) q0[i] + Td[i * 4 + 3]) - Rp;
    }
    for (int i = 0; i < 12; ++i)
        if (!corr_finite(Td[i]) || !corr_finite((float) Td[i])) return false;
    for (int i = 0; i < 16; ++i) T[i] = Td[i];
    return true;
}

}  // namespace wm
