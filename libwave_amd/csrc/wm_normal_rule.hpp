// wm_normal_rule.hpp -- from a neighbourhood's covariance to a point's normal and curvature, ONCE for host and device:
// k_normals (wm_plane.hip, the k form), k_nr_finish (wm_fpfh_radius.hip, the radius form) and wm_normal_from_sums on
// the host run this text.  The radius form's step from its nine integer sums to the covariance is here as well
// (include/wavematch.h, "feature descriptors").  No HIP header of its own: the file compiles with a plain C++ compiler.
//
// Nothing here may be fused: the library is built with -ffp-contract=off on both sides (csrc/Makefile), and a host
// program that includes this file must be built the same way.  Divisions and square roots are the IEEE ones.
#pragma once
#include <math.h>

#include "wm_math.hpp"

namespace wm {

constexpr int kNormalScaleBits = 36;  // the integer sums' quanta: 2^(e - 36) (first moments), 2^(x - 36) (second), as ISS

// c: the symmetric 3 x 3 covariance, row-major, every entry set.  (px, py, pz): the point itself.  out: the unit
// eigenvector of the smallest eigenvalue (svd3<false>: S descending, its vectors the columns of V), turned towards the
// origin (pcl::flipNormalTowardsViewpoint, viewpoint at the origin: n . (0 - p) >= 0), and the curvature
// S[2] / (S[0] + S[1] + S[2]); a largest value <= 0 gives (0, 0, 0, 0).
WM_HD void normal_finish(const double *c, float px, float py, float pz, float *out) {
    out[0] = out[1] = out[2] = out[3] = 0.f;
    double U[9], S[3], V[9];
    svd3<false>(c, U, S, V);  // S descending: lambda2 = S[0], lambda0 = S[2]
    if (S[0] > 0.0) {
        double nx = V[2], ny = V[5], nz = V[8];
        const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
        nx *= inv, ny *= inv, nz *= inv;
        if (nx * (double) px + ny * (double) py + nz * (double) pz > 0.0) nx = -nx, ny = -ny, nz = -nz;
        out[0] = (float) nx;
        out[1] = (float) ny;
        out[2] = (float) nz;
        out[3] = (float) (S[2] / (S[0] + S[1] + S[2]));
    }
}

// e of the rule: ceil(x / 2) for r2 = m 2^x (x may be negative)
WM_HD int normal_half_exponent(int x) { return x >= 0 ? (x + 1) / 2 : -((-x) / 2); }

// sums: the three first moments (quantum 2^(e - 36)) and the six second moments xx xy xz yy yz zz (quantum 2^(x - 36))
// of the differences to the point over its n_s neighbours, the point included.  PCL's single-pass
// computeMeanAndCovarianceMatrix: mean_c = S1_c 2^(e - 36) / n_s, C_ab = S2_ab 2^(x - 36) / n_s - mean_a mean_b.
WM_HD void normal_from_sums(const long long sums[9], int n_s, int x, float px, float py, float pz, float *out) {
    if (n_s < 3) {
        out[0] = out[1] = out[2] = out[3] = 0.f;
        return;
    }
    const double nn = (double) n_s;
    const double q1 = ldexp(1.0, normal_half_exponent(x) - kNormalScaleBits), q2 = ldexp(1.0, x - kNormalScaleBits);
    const double mx = (double) sums[0] * q1 / nn, my = (double) sums[1] * q1 / nn, mz = (double) sums[2] * q1 / nn;
    double c[9];
    c[0] = (double) sums[3] * q2 / nn - mx * mx;
    c[1] = c[3] = (double) sums[4] * q2 / nn - mx * my;
    c[2] = c[6] = (double) sums[5] * q2 / nn - mx * mz;
    c[4] = (double) sums[6] * q2 / nn - my * my;
    c[5] = c[7] = (double) sums[7] * q2 / nn - my * mz;
    c[8] = (double) sums[8] * q2 / nn - mz * mz;
    normal_finish(c, px, py, pz, out);
}

}  // namespace wm
