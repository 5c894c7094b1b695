// wm_radius_walk.hpp -- the candidates of a fixed-radius neighbourhood, walked by one lane: the loop that
// k_outlier_radius (wm_outlier.hip: it counts the hits) and k_cluster_link (wm_cluster.hip: it joins them) are made of.
#pragma once
#include "wm_gicp_dev.hpp"

namespace wm {

// Every point of the cells covering the box [q - r, q + r] (r_cells = r in cells; the grid's slack is added here) goes
// through visit(position in the grid's order, the point) once.  The box is resolved a batch of kKnnRows rows at a time,
// as knn_search resolves its rows: a row of x-adjacent cells is ONE contiguous run of the cell-sorted points, the
// batch's cell_start look-ups are issued together, the non-empty runs go to the lane's column of `runs` (LDS:
// kKnnRows * col_stride entries) and are walked in one flat loop with the next candidate's load in flight.
// EARLY: visit's return value `true` ends the walk; otherwise it is ignored and every candidate is visited.
template <bool EARLY, class Visit>
__device__ __forceinline__ void radius_walk(const GridDev &g, const float4 &q, float r_cells, uint2 *runs, unsigned lane_col,
                                            unsigned col_stride, Visit &&visit) {
    const float fx = (q.x - g.ox) * g.inv_h, fy = (q.y - g.oy) * g.inv_h, fz = (q.z - g.oz) * g.inv_h;
    const float rc = r_cells + g.slack;
    // (clamped as floats: r may exceed what an int holds)
    const int xa = (int) fmaxf(floorf(fx - rc), 0.f), xb = (int) fminf(floorf(fx + rc), (float) (g.nx - 1));
    const int ya = (int) fmaxf(floorf(fy - rc), 0.f), yb = (int) fminf(floorf(fy + rc), (float) (g.ny - 1));
    const int za = (int) fmaxf(floorf(fz - rc), 0.f), zb = (int) fminf(floorf(fz + rc), (float) (g.nz - 1));
    const bool any = xa <= xb && ya <= yb && za <= zb;
    int yy = ya, zz = any ? za : zb + 1;  // row cursor; zz > zb = past the last row
    bool stop = false;
    while (zz <= zb && !(EARLY && stop)) {
        int n_runs = 0;
        unsigned rs[kKnnRows], re[kKnnRows];
#pragma unroll
        for (int u = 0; u < kKnnRows; ++u) {
            const bool live = zz <= zb;
            const size_t base = ((size_t) (live ? zz : za) * g.ny + (live ? yy : ya)) * g.nx;
            rs[u] = g.cell_start[base + xa];
            re[u] = live ? g.cell_start[base + xb + 1] : 0u;  // dead row: e <= s
            if (++yy > yb) {
                yy = ya;
                ++zz;
            }
        }
#pragma unroll
        for (int u = 0; u < kKnnRows; ++u)
            if (re[u] > rs[u]) {
                runs[n_runs * col_stride + lane_col] = make_uint2(rs[u], re[u]);
                ++n_runs;
            }
        if (n_runs == 0) continue;
        int ri = 0;
        const uint2 r0 = runs[lane_col];
        unsigned j = r0.x, e = r0.y;
        float4 t = g.pts[j];
        for (;;) {
            const unsigned jt = j;  // t's position
            bool more = true;
            if (++j == e) {
                more = ++ri < n_runs;
                if (more) {
                    const uint2 rn = runs[ri * col_stride + lane_col];
                    j = rn.x;
                    e = rn.y;
                }
            }
            const float4 tn = g.pts[more ? j : r0.x];  // (a lane at its end reads a line it has had already)
            stop = visit(jt, t);
            if (!more || (EARLY && stop)) break;
            t = tn;
        }
    }
}

}  // namespace wm
