// wm_fpfh_pair.hpp -- the pair features of the FPFH rule (include/wavematch.h, "feature descriptors"): ONE text for the
// k form (k_spfh, wm_fpfh.hip) and the radius form (k_spfh_radius, wm_fpfh_radius.hip).  Float32, every operation
// rounded, nothing fused; atan2f is the one function of the rule that is not bit-defined.
#pragma once
#include <hip/hip_runtime.h>

namespace wm {

constexpr int kFpfhBins = 11;
constexpr int kFpfhDim = 3 * kFpfhBins;

__device__ __forceinline__ float f_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}
__device__ __forceinline__ float f_det(float a, float b, float c, float d) { return __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, d)); }
__device__ __forceinline__ int f_bin(float x) {  // floorf(11 x), clamped to 0 ... 10
    return (int) fminf(fmaxf(floorf(__fmul_rn((float) kFpfhBins, x)), 0.f), (float) (kFpfhBins - 1));
}

// The rule's square roots are IEEE ones.  __fsqrt_rn compiles to the bare v_sqrt_f32 (1 ulp) with this toolchain; the k
// form (IEEE_SQRT = false) keeps it, so that its bytes stay what they were -- a bin or a swap choice moves only where a
// root's last bit decides it, which k-neighbourhoods almost never do.  The radius form asks for sqrtf, which the
// compiler's default (correctly rounded divide and sqrt) expands to the exact root: two points a few centimetres apart
// share their radius neighbourhood, their normals agree to the last bit or two, and fabsf(a1) < fabsf(a2) is then
// decided by a1's and a2's last bit in a share of the pairs that a test sees.
template <bool IEEE_SQRT>
__device__ __forceinline__ float f_sqrt(float x) {
    return IEEE_SQRT ? sqrtf(x) : __fsqrt_rn(x);
}

// the three bins of the pair (p, q), d2 = |q - p|^2 > 0; false: the pair is skipped
template <bool IEEE_SQRT = false>
__device__ __forceinline__ bool fpfh_pair(float px, float py, float pz, const float4 &np, const float4 &q, const float4 &nq, float d2,
                                          int (&bin)[3]) {
    if (nq.x == 0.f && nq.y == 0.f && nq.z == 0.f) return false;
    float dx = __fsub_rn(q.x, px), dy = __fsub_rn(q.y, py), dz = __fsub_rn(q.z, pz);
    const float f4 = f_sqrt<IEEE_SQRT>(d2);  // (= sqrtf(dp . dp): the key's d2 is that dot product, its differences negated)
    const float a1 = __fdiv_rn(f_dot(np.x, np.y, np.z, dx, dy, dz), f4);
    const float a2 = __fdiv_rn(f_dot(nq.x, nq.y, nq.z, dx, dy, dz), f4);
    const bool swap = fabsf(a1) < fabsf(a2);
    const float n1x = swap ? nq.x : np.x, n1y = swap ? nq.y : np.y, n1z = swap ? nq.z : np.z;
    const float n2x = swap ? np.x : nq.x, n2y = swap ? np.y : nq.y, n2z = swap ? np.z : nq.z;
    if (swap) dx = -dx, dy = -dy, dz = -dz;
    const float f3 = swap ? -a2 : a1;
    float vx = f_det(dy, n1z, dz, n1y), vy = f_det(dz, n1x, dx, n1z), vz = f_det(dx, n1y, dy, n1x);
    const float vn = f_sqrt<IEEE_SQRT>(f_dot(vx, vy, vz, vx, vy, vz));
    if (vn == 0.f) return false;
    vx = __fdiv_rn(vx, vn), vy = __fdiv_rn(vy, vn), vz = __fdiv_rn(vz, vn);
    const float wx = f_det(n1y, vz, n1z, vy), wy = f_det(n1z, vx, n1x, vz), wz = f_det(n1x, vy, n1y, vx);
    const float f2 = f_dot(vx, vy, vz, n2x, n2y, n2z);
    const float f1 = atan2f(f_dot(wx, wy, wz, n2x, n2y, n2z), f_dot(n1x, n1y, n1z, n2x, n2y, n2z));
    const float kPi = 3.14159265358979323846f, kInv2Pi = (float) (1.0 / (2.0 * 3.14159265358979323846));
    bin[0] = f_bin(__fmul_rn(__fadd_rn(f1, kPi), kInv2Pi));
    bin[1] = f_bin(__fmul_rn(__fadd_rn(f2, 1.0f), 0.5f));
    bin[2] = f_bin(__fmul_rn(__fadd_rn(f3, 1.0f), 0.5f));
    return true;
}

}  // namespace wm
