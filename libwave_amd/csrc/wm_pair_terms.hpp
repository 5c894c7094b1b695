// wm_pair_terms.hpp -- what ONE matched pair contributes, defined once for every path that sums it: PCL's float
// transform of a source point, the iteration's 17 sums (k_icp_stats of wm_icp.hip, the fused search of wm_nn.hip, the
// one-workgroup registrations of wm_small.hip), LUMold's 16 sums, residual and normal matrix (wm_info.hip, wm_small.hip),
// and the load of a caller-layout point with its finiteness test (the one-workgroup ICP, GICP and NDT).  The paths
// agree bit for bit (tests/test_batch_gpu.py, tests/test_small_pinned_gpu.py) because they call the same text.
// The build has -ffp-contract=off: inlining one of these cannot fuse or unfuse a product and a sum.
#pragma once
#include "wm_internal.hpp"

namespace wm {

// PCL's float transform of a source point: ((m00*x + m01*y) + m02*z) + m03
__device__ __forceinline__ void xform_pcl(const float *T, float px, float py, float pz, float &x, float &y, float &z) {
    x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], px), __fmul_rn(T[1], py)), __fmul_rn(T[2], pz)), T[3]);
    y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], px), __fmul_rn(T[5], py)), __fmul_rn(T[6], pz)), T[7]);
    z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], px), __fmul_rn(T[9], py)), __fmul_rn(T[10], pz)), T[11]);
}

// point i of a cloud in the caller's layout (`stride` bytes apart); false: not finite (such points are dropped, as k_pack does)
__device__ __forceinline__ bool load_point_finite(const unsigned char *base, unsigned i, unsigned stride, float &x, float &y,
                                                  float &z) {
    const float *p = reinterpret_cast<const float *>(base + (size_t) i * stride);
    x = p[0], y = p[1], z = p[2];
    return x - x == 0.f && y - y == 0.f && z - z == 0.f;  // finite
}

// ------------------------------------------------- the iteration's sums
// The 17 terms of one MATCHED pair, handed to put(k, term) for k = 0 ... 16: n, sum p, sum t, sum t p^T row by row,
// sum d2 | GN: n, sum p, A^T A, J^T r, sum d2 -- p the query under the current pose, t its match.  What `put` does
// with a term is the caller's: the fused search ASSIGNS (icp_terms below; its wave reduction adds the lanes),
// k_icp_stats and k_icp_small ADD to an accumulator that started at +0.0, which turns a term of -0.0 (-px * pz of a
// cloud with z == 0) into +0.0.  Each caller keeps its form, term by term as it is formed: adding a finished array
// of terms instead cost k_icp_stats 12-16 registers and a wave per SIMD.
// (k_nn_cert's sums, wm_nn_cert.hip, are a copy of the SVD branch hand-scheduled with explicit fma: kept apart on purpose)
template <int STATS, class PUT>
__device__ __forceinline__ void icp_pair_terms(float qx, float qy, float qz, float bqx, float bqy, float bqz, float d2, PUT &&put) {
    const double px = qx, py = qy, pz = qz, tx = bqx, ty = bqy, tz = bqz;
    put(0, 1.0);
    put(1, px);
    put(2, py);
    put(3, pz);
    if constexpr (STATS == WM_ICP_SVD) {
        put(4, tx);
        put(5, ty);
        put(6, tz);
        put(7, tx * px);
        put(8, tx * py);
        put(9, tx * pz);
        put(10, ty * px);
        put(11, ty * py);
        put(12, ty * pz);
        put(13, tz * px);
        put(14, tz * py);
        put(15, tz * pz);
    } else {
        const double rx = px - tx, ry = py - ty, rz = pz - tz;
        put(4, py * py + pz * pz);  // (A^T A)(0,0)
        put(5, -px * py);           // (0,1)
        put(6, -px * pz);           // (0,2)
        put(7, px * px + pz * pz);  // (1,1)
        put(8, -py * pz);           // (1,2)
        put(9, px * px + py * py);  // (2,2)
        put(10, rx);
        put(11, ry);
        put(12, rz);
        put(13, py * rz - pz * ry);  // p x r
        put(14, pz * rx - px * rz);
        put(15, px * ry - py * rx);
    }
    put(16, (double) d2);
}

// this lane's terms of the iteration's sums, for the fused search.
// a[17] counts the queries this rank handled; its fraction (units of 2^-24) counts those whose match
// CHANGED in this search -- what the host decides by whether the next searches can be certified instead
// (wm_icp_align).  Exact in a double, and never carrying into the integer part, because at most 2^23
// queries report: beyond that size only every (IcpDevState::changed_mask + 1)-th does (changed_mask_for,
// wm_icp_step.hpp) and the solve scales the count back up.
constexpr double kChangedUnit = 1.0 / 16777216.0;
template <int STATS>
__device__ __forceinline__ void icp_terms(double (&a)[kAcc], bool mine, bool matched, float qx, float qy, float qz,
                                          float bqx, float bqy, float bqz, float d2, bool changed = false) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) a[k] = 0.0;
    if (mine) {
        a[17] = changed ? 1.0 + kChangedUnit : 1.0;
        if (matched) icp_pair_terms<STATS>(qx, qy, qz, bqx, bqy, bqz, d2, [&](int k, double term) { a[k] = term; });
    }
}

// ------------------------------------------------- estimateLUM / estimateLUMold (icp_pcl_functions.cpp:51-289)
// The reference's float / double mix: float pair averages, differences and products feeding double sums.
struct LumPair {
    float av0, av1, av2;  // (p + t) / 2
    float df0, df1, df2;  // p - t
};
__device__ __forceinline__ LumPair lum_pair(float px, float py, float pz, float tx, float ty, float tz) {
    LumPair u;
    u.av0 = __fmul_rn(0.5f, __fadd_rn(px, tx)), u.av1 = __fmul_rn(0.5f, __fadd_rn(py, ty)), u.av2 = __fmul_rn(0.5f, __fadd_rn(pz, tz));
    u.df0 = __fsub_rn(px, tx), u.df1 = __fsub_rn(py, ty), u.df2 = __fsub_rn(pz, tz);
    return u;
}
// pass 1, added to a: a[0] = n, a[1..3] = sum av, a[4..9] = MM(3,4), (3,5), (4,5), (3,3), (4,4), (5,5) terms, a[10..15] = MZ(0..5)
__device__ __forceinline__ void lum_terms(float px, float py, float pz, float tx, float ty, float tz, double (&a)[16]) {
    const LumPair u = lum_pair(px, py, pz, tx, ty, tz);
    a[0] += 1.0;
    a[1] += u.av0;
    a[2] += u.av1;
    a[3] += u.av2;
    a[4] += __fmul_rn(u.av0, u.av2);                                        // -MM(3,4)
    a[5] += __fmul_rn(u.av0, u.av1);                                        // -MM(3,5)
    a[6] += __fmul_rn(u.av1, u.av2);                                        // -MM(4,5)
    a[7] += __fadd_rn(__fmul_rn(u.av1, u.av1), __fmul_rn(u.av2, u.av2));    // MM(3,3)
    a[8] += __fadd_rn(__fmul_rn(u.av0, u.av0), __fmul_rn(u.av1, u.av1));    // MM(4,4)
    a[9] += __fadd_rn(__fmul_rn(u.av0, u.av0), __fmul_rn(u.av2, u.av2));    // MM(5,5)
    a[10] += u.df0;
    a[11] += u.df1;
    a[12] += u.df2;
    a[13] += __fsub_rn(__fmul_rn(u.av1, u.df2), __fmul_rn(u.av2, u.df1));
    a[14] += __fsub_rn(__fmul_rn(u.av0, u.df1), __fmul_rn(u.av1, u.df0));
    a[15] += __fsub_rn(__fmul_rn(u.av2, u.df0), __fmul_rn(u.av0, u.df2));
}
// pass 2: |diff - (D_t + av x D_r)|^2 of one pair, rounded to float as the reference sums it
__device__ __forceinline__ double lum_residual(float px, float py, float pz, float tx, float ty, float tz, const double *D) {
    const LumPair u = lum_pair(px, py, pz, tx, ty, tz);
    const double e0 = u.df0 - (D[0] + u.av2 * D[5] - u.av1 * D[4]);
    const double e1 = u.df1 - (D[1] + u.av0 * D[4] - u.av2 * D[3]);
    const double e2 = u.df2 - (D[2] + u.av1 * D[3] - u.av0 * D[5]);
    return (double) (float) (e0 * e0 + e1 * e1 + e2 * e2);
}
// M^T M of the normal equations from pass 1's sums (M^T Z is s[10..15])
__host__ __device__ inline void lum_normal_matrix(const double s[16], double MM[36]) {
    for (int k = 0; k < 36; ++k) MM[k] = 0.0;
#define M_(r, c) MM[(r) * 6 + (c)]
    M_(0, 4) = -s[2];
    M_(0, 5) = s[3];
    M_(1, 3) = -s[3];
    M_(1, 4) = s[1];
    M_(2, 3) = s[2];
    M_(2, 5) = -s[1];
    M_(3, 4) = -s[4];
    M_(3, 5) = -s[5];
    M_(4, 5) = -s[6];
    M_(3, 3) = s[7];
    M_(4, 4) = s[8];
    M_(5, 5) = s[9];
    M_(0, 0) = M_(1, 1) = M_(2, 2) = (double) (float) (int) s[0];
    M_(4, 0) = M_(0, 4);
    M_(5, 0) = M_(0, 5);
    M_(3, 1) = M_(1, 3);
    M_(4, 1) = M_(1, 4);
    M_(3, 2) = M_(2, 3);
    M_(5, 2) = M_(2, 5);
    M_(4, 3) = M_(3, 4);
    M_(5, 3) = M_(3, 5);
    M_(5, 4) = M_(4, 5);
#undef M_
}

}  // namespace wm
