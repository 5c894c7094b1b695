// wm_iss_sums.hpp -- a product as an INTEGER term of an exact int64 sum: the step k_iss_scatter (wm_iss.hip) and
// k_nr_sums (wm_fpfh_radius.hip) build their order-free sums from.
#pragma once
#include <hip/hip_runtime.h>

namespace wm {

// rint(v) + 2^52 + 2^51 for |v| < 2^51: at that magnitude a double's quantum is 1, so the ADDITION rounds v to the
// nearest integer, ties to even -- exactly rint -- and the integer sits in the low bits of the pattern, two's
// complement.  The patterns are added as they are; iss_unbias takes the constant out, once per sum.
constexpr double kIssMagic = 6755399441055744.0;
constexpr unsigned long long kIssMagicBits = 0x4338000000000000ull;

__device__ __forceinline__ unsigned long long iss_term(double product, double scale) {
    return (unsigned long long) __double_as_longlong(product * scale + kIssMagic);  // (the scaling is exact: a power of two)
}
__device__ __forceinline__ long long iss_unbias(unsigned long long s, unsigned n_s) {
    return (long long) (s - (unsigned long long) n_s * kIssMagicBits);  // (modulo 2^64: the true sum fits)
}

}  // namespace wm
