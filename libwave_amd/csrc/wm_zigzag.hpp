// wm_zigzag.hpp -- the nearest-first visiting order of the grid walks (wm_nn_scan.hpp): plain integer and float
// arithmetic, for the device and for a host compiler alike (tests/test_zigzag_cpu.py checks it on the CPU)
#pragma once

#if defined(__HIPCC__)
#define WM_ZZ_FN __host__ __device__ __forceinline__
#else
#define WM_ZZ_FN inline
#endif

namespace wm {

// Step k = 0, 1, 2, ... of a walk over the cells lo .. hi of one axis that starts at c (lo <= c <= hi) and moves
// outwards: c, c+1, c-1, c+2, c-2, ... while both sides have cells left (k <= 2 m, m = the shorter side's length), then
// straight on along the longer side.  Steps 0 .. hi - lo visit every cell exactly once: no step is wasted on a
// coordinate outside the interval, whatever the position of c in it.
WM_ZZ_FN int zigzag_coord(int k, int lo, int c, int hi) {
    const int dn = c - lo, up = hi - c;
    const int m = dn < up ? dn : up;
    const int zig = (k & 1) ? ((k + 1) >> 1) : -(k >> 1);
    const int tail = up > dn ? k - m : m - k;
    return c + (k <= 2 * m ? zig : tail);
}

// Lower bound of the distance (in cells, along this axis) from a query at offset frac in [0, 1] above the lower face
// of cell c to every cell that steps k, k+1, ... of the walk above visit; 0 for k = 0.  The cells left at step k
// are at least a = (k + 1) / 2 cells from c while the walk alternates and k - m once it runs straight, and a cell a
// away from c is a - frac (above) or a - 1 + frac (below) from the query.  A query outside lo .. hi + 1 has c
// clamped and frac 0 or 1: the bound then undercuts the true distance, which is all a stop needs.
WM_ZZ_FN float zigzag_remaining(int k, int lo, int c, int hi, float frac) {
    const int dn = c - lo, up = hi - c;
    const int m = dn < up ? dn : up;
    const int a = k <= 2 * m ? ((k + 1) >> 1) : k - m;
    const float g = frac < 1.f - frac ? frac : 1.f - frac;
    const float d = (float) (a - 1) + g;
    return d > 0.f ? d : 0.f;
}

}  // namespace wm
