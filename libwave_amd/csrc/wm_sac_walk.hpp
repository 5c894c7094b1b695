// wm_sac_walk.hpp -- the HOST side of the plane segmentation that wm_sac_segment and wm_sac_segment_batch share, so that
// PCL's quirks exist once: the loop of RandomSampleConsensus::computeModel as a walk over the hypothesis stream's
// (flag, count) pairs, and the plane of the refit's nine sums.  No device code and no HIP header: the file compiles
// with a plain C++ compiler (tests/cpp_host/sac_walk_host.cpp runs it under the sanitizers).
//
// Why the walk is host code: k = log(1 - p) / log(q) goes through the host's pow and log.  A device log that differs in
// the last bit can flip `it < k`, and with it iterations, hypotheses, the best entry and every count behind them.
#pragma once
#include <float.h>
#include <math.h>

#include "wm_math.hpp"

#include <algorithm>
#include <cmath>

namespace wm {

// what the device says of a stream entry
enum : unsigned { kSacSkipped = 0u, kSacValid = 1u, kSacAxisInvalid = 2u };

// PCL's bound on the iterations for an inlier fraction w
inline double sac_k(double log_p, double w) {
    double q = 1.0 - std::pow(w, 3.0);
    q = std::max(DBL_EPSILON, std::min(1.0 - DBL_EPSILON, q));
    return log_p / std::log(q);
}

// The loop's state for one cloud (include/wavematch.h, "loop").  The stream is evaluated in rounds; how it is cut into
// rounds changes nothing but `rounds`.
struct SacWalk {
    long long max_it = 0, max_skip = 0;
    double log_p = 0.0, n = 0.0;
    long long it = 0, skipped = 0, best = -1, best_j = -1;
    unsigned long long j = 0;  // the next stream entry = the entries consumed
    double k = 1.0;
    int rounds = 0;
    bool going = false;

    void start(int max_iterations, double probability, size_t n_points) {
        *this = SacWalk{};
        max_it = max_iterations;
        max_skip = 10ll * max_it;
        log_p = std::log(1.0 - probability);
        n = (double) n_points;
        going = (double) it < k && skipped < max_skip;
    }
    // A round never holds more entries than the loop can still count as iterations: only skipped entries make another
    // round necessary.  (going: max_it + 1 - it >= 1)
    unsigned round_size(unsigned round_max) const { return (unsigned) std::min<long long>(round_max, max_it + 1 - it); }

    // One entry, in stream order (going must hold).  true: the entry is the new best model.
    bool feed(unsigned flag, unsigned count) {
        bool improved = false;
        if (flag == kSacSkipped) {
            ++skipped;
        } else {
            const long long c = (long long) count;
            if (flag == kSacValid && c > best) {
                best = c;
                best_j = (long long) j;
                k = sac_k(log_p, (double) c / n);
                improved = true;
            } else if (flag == kSacAxisInvalid && best < 0) {
                k = sac_k(log_p, 0.0);  // (PCL: its count of 0 beats "nothing counted yet" and sets k; it is no model)
            }
            ++it;
            if (it > max_it) {
                ++j;
                going = false;
                return improved;
            }
        }
        ++j;
        going = (double) it < k && skipped < max_skip;
        return improved;
    }

    // A round's pairs; entries behind the stopping point are discarded.  on_best(e): entry e of the round is the new best.
    template <class OnBest>
    void feed_round(const unsigned *flags, const unsigned *counts, unsigned R, OnBest on_best) {
        ++rounds;
        for (unsigned e = 0; e < R && going; ++e)
            if (feed(flags[e], counts[e])) on_best(e);
    }
    void feed_round(const unsigned *flags, const unsigned *counts, unsigned R) {
        feed_round(flags, counts, R, [](unsigned) {});
    }
};

// double -> float toward zero: the normal the refit returns is never longer than the unit eigenvector, so that its
// n' C n does not exceed the smallest eigenvalue by what a longer vector would add
inline float sac_toward_zero(double v) {
    float f = (float) v;
    if (std::fabs((double) f) > std::fabs(v)) f = nextafterf(f, 0.f);
    return f;
}

inline float sac_threshold(double t) {  // the smallest float not below t
    float f = (float) t;
    if ((double) f < t) f = nextafterf(f, INFINITY);
    return f;
}

constexpr int kSacComps = 9;  // the refit's sums: [0..2] sum dx dy dz, [3..8] sum dxdx dxdy dxdz dydy dydz dzdz

// The plane of the nine sums over m inliers (relative to p0): the eigenvector of the covariance's smallest eigenvalue,
// its sign the model's; false: poisoned or not finite, the model stays.
inline bool sac_plane_from_sums(const double *sum, bool poison, const float *p0, double m, const float model[4], float out[4]) {
    if (poison) return false;
    const double mx = sum[0] / m, my = sum[1] / m, mz = sum[2] / m;
    const double cxx = sum[3] / m - mx * mx, cxy = sum[4] / m - mx * my, cxz = sum[5] / m - mx * mz;
    const double cyy = sum[6] / m - my * my, cyz = sum[7] / m - my * mz, czz = sum[8] / m - mz * mz;
    const double C[9] = {cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz};
    for (double v : C)
        if (!std::isfinite(v)) return false;
    double U[9], S[3], V[9];
    svd3<false>(C, U, S, V);  // (symmetric, positive semi-definite: the right singular vectors are the eigenvectors)
    double nx = V[2], ny = V[5], nz = V[8];
    if ((nx * (double) model[0] + ny * (double) model[1]) + nz * (double) model[2] < 0) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    const float fx = sac_toward_zero(nx), fy = sac_toward_zero(ny), fz = sac_toward_zero(nz);
    // d = -n . centroid with the normal as it is returned
    const double gx = (double) p0[0] + mx, gy = (double) p0[1] + my, gz = (double) p0[2] + mz;
    const float fd = (float) -(((double) fx * gx + (double) fy * gy) + (double) fz * gz);
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(fz) && std::isfinite(fd))) return false;
    if (fx == 0.f && fy == 0.f && fz == 0.f) return false;
    out[0] = fx;
    out[1] = fy;
    out[2] = fz;
    out[3] = fd;
    return true;
}

}  // namespace wm
