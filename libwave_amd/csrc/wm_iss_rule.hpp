// wm_iss_rule.hpp -- the saliency step of wm_iss_keypoints (include/wavematch.h, "keypoints"): from a point's six
// integer scatter sums and its neighbour count to its `third` value.  It exists ONCE, for host and device: a lane of
// k_iss_third (wm_iss.hip) and wm_iss_third on the host run this text, and the same operations in the same order give
// the same bits.  No HIP header of its own: the file compiles with a plain C++ compiler
// (tests/cpp_host/iss_rule_host.cpp runs it under the sanitizers).
//
// Nothing here may be fused: the library is built with -ffp-contract=off on both sides (csrc/Makefile), and a host
// program that includes this file must be built the same way.  Divisions and square roots are the IEEE ones.
#pragma once
#include <math.h>

#include "wm_math.hpp"

namespace wm {

constexpr int kIssScaleBits = 36;  // a scatter term is rint(product * 2^(36 - x)), r2s = m 2^x with m in [0.5, 1)

WM_HD bool iss_finite(double v) { return v - v == 0.0; }

// sums: sum dx dx, dx dy, dx dz, dy dy, dy dz, dz dz over the neighbourhood, each term an integer of quantum
// 2^(x - 36).  -> third: the smallest eigenvalue in the cloud's units for a SALIENT point, else 0.
//   n_s < min_neighbors: 0.  Otherwise the sums, converted to double (round to nearest), form the symmetric matrix;
//   jacobi3 as it stands; l1 >= l2 >= l3.  Salient iff the three are finite, l3 > 0, l2 / l1 < gamma_21 and
//   l3 / l2 < gamma_32 (a NaN fails); third = ldexp(l3, x - 36).
WM_HD double iss_third(const long long sums[6], int n_s, int min_neighbors, int x, double gamma_21, double gamma_32) {
    if (n_s < min_neighbors) return 0.0;
    const double xx = (double) sums[0], xy = (double) sums[1], xz = (double) sums[2];
    const double yy = (double) sums[3], yz = (double) sums[4], zz = (double) sums[5];
    double A[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
    double w[3], V[9];
    jacobi3(A, w, V);
    double l1 = w[0], l2 = w[1], l3 = w[2], t;
    // (three compare-exchanges: a NaN stays where it is and fails the finite test below)
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    if (l2 < l3) { t = l2; l2 = l3; l3 = t; }
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    if (!(iss_finite(l1) && iss_finite(l2) && iss_finite(l3))) return 0.0;
    if (!(l3 > 0.0)) return 0.0;
    if (!(l2 / l1 < gamma_21)) return 0.0;
    if (!(l3 / l2 < gamma_32)) return 0.0;
    return ldexp(l3, x - kIssScaleBits);
}

}  // namespace wm
