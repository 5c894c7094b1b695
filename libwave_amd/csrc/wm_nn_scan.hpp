// wm_nn_scan.hpp -- device-only code of the correspondence search, all __device__ __forceinline__, for wm_nn.hip (full
// search) and wm_nn_cert.hip (certificate kernel): keys, loads and stores, the grid walks, small shared steps, ICP terms
#pragma once
#include "wm_internal.hpp"
#include "wm_icp_step.hpp"
#include "wm_pair_terms.hpp"
#include "wm_bins.hpp"
#include "wm_wave.hpp"
#include "wm_zigzag.hpp"

namespace wm {

__device__ __forceinline__ unsigned long long make_key(float d2, unsigned idx) {
    return ((unsigned long long) __float_as_uint(d2) << 32) | idx;
}

__device__ __forceinline__ float canon_d2(float qx, float qy, float qz, const float4 &t) {
    const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// Blocks are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8).
// Remap so each XCD works on one contiguous (Morton-compact) eighth of the
// queries and its private L2 holds one spatial region of the target.
__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned nblocks) {
    const unsigned per = (nblocks + 7u) / 8u;
    return (b & 7u) * per + (b >> 3);
}
// The one used: the XCDs take turns in chunks of S blocks (nblocks a multiple of 8 S) of the
// Morton-ordered queries.  A chunk of 32 blocks = 2048 queries is still one compact region for the
// XCD's L2, but a region of EXPENSIVE queries (the far corner of a rotated cloud in the early
// iterations) is now shared by all eight XCDs instead of landing on the one that owns that eighth
// of the cloud: 83.0 -> 79.4 us per launch on the 1M pair (chunks of 8-32 equal, 128: 80.0,
// 512: 84.5, whole eighths: 83.0).
__device__ __forceinline__ unsigned xcd_remap_chunked(unsigned b, unsigned S) {
    const unsigned x = b & 7u, l = b >> 3;
    const unsigned chunk = l / S;
    return (chunk * 8u + x) * S + (l - chunk * S);
}

// ------------------------------------------------- what a search wave needs of the state before it can start
// The head run of IcpDevState (wm_internal.hpp), read through a uniform pointer: two wide scalar loads, requested
// together with the wave's stream loads.  Each kernel has ONE empty asm statement where the wave first waits: it names
// these words as scalar operands (WM_NN_STATE_OPERANDS) -- in k_nn_grid next to the stream loads' registers, in
// k_nn_cert behind a scheduling barrier that keeps the burst above it -- so the compiler can neither put the test of
// `done` in front of the requests (it did, sinking every load behind that branch and making a round trip of each) nor
// fetch a word later, when it is first used.  scripts/dev/nn_prologue_report.py reads the outcome off the code object.
struct NnState {
    float Tf[12];
    int done, have_prev, slab_on;
    float slab_lo, slab_hi;
    unsigned changed_mask;
    float step_disp;
};
__device__ __forceinline__ NnState nn_state(const IcpDevState *st) {
    NnState s;
#pragma unroll
    for (int k = 0; k < 12; ++k) s.Tf[k] = st->Tf[k];
    s.done = st->done;
    s.have_prev = st->have_prev;
    s.slab_on = st->slab_on;
    s.slab_lo = st->slab_lo;
    s.slab_hi = st->slab_hi;
    s.changed_mask = st->changed_mask;
    s.step_disp = st->step_disp;
    return s;
}
// (the scalar operands of that statement: 17 of an asm statement's 30; the last two words of the run arrive in the
// load that brings slab_hi)
#define WM_NN_STATE_OPERANDS(s)                                                                                              \
    "s"((s).Tf[0]), "s"((s).Tf[1]), "s"((s).Tf[2]), "s"((s).Tf[3]), "s"((s).Tf[4]), "s"((s).Tf[5]), "s"((s).Tf[6]),           \
        "s"((s).Tf[7]), "s"((s).Tf[8]), "s"((s).Tf[9]), "s"((s).Tf[10]), "s"((s).Tf[11]), "s"((s).done), "s"((s).have_prev), \
        "s"((s).slab_on), "s"((s).slab_lo), "s"((s).slab_hi)

// The grid tables are reached through pointers read from memory, so the compiler only knows
// them as generic (flat) addresses; they always point into HBM -- say so, and get global_load
// instead of flat_load (no LDS-aperture check, no lgkmcnt coupling).
typedef float f4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) f4v *gp_f4;
typedef const __attribute__((address_space(1))) unsigned *gp_u32;
__device__ __forceinline__ float4 ldp(const float4 *p, size_t j) {
    const f4v v = ((gp_f4) p)[j];
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ unsigned ldc(const unsigned *p, size_t j) { return ((gp_u32) p)[j]; }
// Result stores are non-temporal: the line does not stay (dirty) in the XCD's L2, so the kernel
// boundary behind the search has no write-back to wait for (a search leaves 12-26 MB of results that
// nothing on this XCD reads again before the next iteration)
__device__ __forceinline__ void st_f4(float4 *p, float x, float y, float z, float w) {
    f4v v = {x, y, z, w};
    __builtin_nontemporal_store(v, (f4v *) p);
}
__device__ __forceinline__ void st_u64(unsigned long long *p, unsigned long long v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void st_f64(double *p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ float canon_d2v(float qx, float qy, float qz, const f4v &t) {
    return canon_d2(qx, qy, qz, make_float4(t.x, t.y, t.z, t.w));
}

// ------------------------------------------------------------- grid search
// scan the contiguous run [s, e) of cell-sorted target points, four loads in flight.
// The last group may read up to three entries past e: they are the next cells' points (real
// target points -- a closer one among them is a legitimate find) or the NaN padding at the end
// of the array (a NaN distance has the largest key and never wins), so no clamping is needed
// and the four loads share one address.
__device__ __forceinline__ unsigned long long scan_run(const float4 *__restrict__ pts, unsigned s,
                                                       unsigned e, float qx, float qy, float qz,
                                                       unsigned long long best) {
    for (unsigned j = s; j < e; j += 4) {
        const gp_f4 p = (gp_f4) pts + j;
        const f4v t0 = p[0], t1 = p[1], t2 = p[2], t3 = p[3];
        const unsigned long long k0 = make_key(canon_d2v(qx, qy, qz, t0), __float_as_uint(t0.w));
        const unsigned long long k1 = make_key(canon_d2v(qx, qy, qz, t1), __float_as_uint(t1.w));
        const unsigned long long k2 = make_key(canon_d2v(qx, qy, qz, t2), __float_as_uint(t2.w));
        const unsigned long long k3 = make_key(canon_d2v(qx, qy, qz, t3), __float_as_uint(t3.w));
        const unsigned long long a = k0 < k1 ? k0 : k1, b = k2 < k3 ? k2 : k3;
        const unsigned long long m = a < b ? a : b;
        best = m < best ? m : best;
    }
    return best;
}

// Scan the target points that can lie inside ball(q, min(r, sqrt(best))) on level g and report
// the distance `margin` from the query to the faces of the box of cells covering
// [q - r, q + r]^3: every point NOT scanned is either farther than `margin` or farther than
// the best distance at the time it was skipped.
//   * the box is walked row by row ((y,z) rows; cells are x-fastest, so a row is one
//     contiguous run of the cell-sorted array), kRowChunk rows at a time: the chunk's
//     cell_start look-ups are issued together (one memory round trip per chunk, not per row);
//   * a row is cut down to the chord of ball(q, sqrt(best)) -- with rho the (y,z) distance of
//     the row, a point of the row closer than Rb has
//         |x - qx| <= sqrt(Rb^2 - (rho - slack)^2) <= sqrt(Rb^2 - rho^2 + 2 slack (Rb + slack))
//     (cell units; Rb inflated by 1e-5 against the approximate hardware square roots): rows
//     outside the ball cost nothing, rows near its rim a cell or two.
// Pruning changes the work, never the result.
constexpr int kRowChunk = 6;
constexpr int kLayeredRows = 18;  // boxes with more (y,z) rows than this are walked layer by layer
template <bool COST>
__device__ __forceinline__ unsigned long long scan_box(const GridDev &g, float qx, float qy,
                                                       float qz, float r, unsigned long long best,
                                                       float *margin, uint2 *runs, unsigned lane,
                                                       bool allow_layered, unsigned &cost) {
    const float big = 4.0e6f;  // clamp in float so far-away queries cannot overflow the int cast
    const float fx = fminf(fmaxf((qx - g.ox) * g.inv_h, -big), big);
    const float fy = fminf(fmaxf((qy - g.oy) * g.inv_h, -big), big);
    const float fz = fminf(fmaxf((qz - g.oz) * g.inv_h, -big), big);
    const float rc = r * g.inv_h + g.slack;
    const int x0 = (int) floorf(fx - rc), x1 = (int) floorf(fx + rc);
    const int y0 = (int) floorf(fy - rc), y1 = (int) floorf(fy + rc);
    const int z0 = (int) floorf(fz - rc), z1 = (int) floorf(fz + rc);
    const float mx = fminf(fx - (float) x0, (float) (x1 + 1) - fx);
    const float my = fminf(fy - (float) y0, (float) (y1 + 1) - fy);
    const float mz = fminf(fz - (float) z0, (float) (z1 + 1) - fz);
    *margin = (fminf(mx, fminf(my, mz)) - g.slack) * g.h;
    const int xa = max(x0, 0), xb = min(x1, g.nx - 1);
    const int ya = max(y0, 0), yb = min(y1, g.ny - 1);
    const int za = max(z0, 0), zb = min(z1, g.nz - 1);
    if (xa > xb || ya > yb || za > zb) return best;
    // look-ups of one chunk of rows (addresses a0/a1), then the walk over its non-empty runs
    auto lookup_and_walk = [&](const unsigned (&a0)[kRowChunk], const unsigned (&a1)[kRowChunk]) {
        unsigned rs[kRowChunk], re[kRowChunk];
#pragma unroll
        for (int u = 0; u < kRowChunk; ++u) {
            rs[u] = ldc(g.cell_start, a0[u]);
            re[u] = ldc(g.cell_start, a1[u]);
        }
        // The chunk's non-empty runs go into this lane's column of an LDS list, and the lane
        // walks its own list: it moves on to its next run as soon as the current one is done,
        // so the wave makes max-over-lanes(sum of a lane's trips) trips, not
        // sum-over-runs(max-over-lanes).  With sparse rows (far queries: most rows of the ball
        // are empty) that is several times fewer.  Four points per trip, one address (reads
        // past a run's end are harmless, see scan_run).  No barrier: a lane only reads back
        // what it wrote itself, and LDS operations of one wave execute in order.
        unsigned cnt = 0;
        if constexpr (COST) cost += 1u << 16;  // (developer statistics: chunks in bits 16-23, trips below)
#pragma unroll
        for (int u = 0; u < kRowChunk; ++u)
            if (re[u] > rs[u]) runs[cnt++ * 64u + lane] = make_uint2(rs[u], re[u]);
        // ONE flat loop (a nested per-run loop would make the lanes wait for each other at
        // every run boundary again)
        unsigned idx = 0, j = 0, e = 0;
        if (cnt) {
            const uint2 run = runs[lane];
            j = run.x;
            e = run.y;
        }
        while (j < e) {
            const gp_f4 p = (gp_f4) g.pts + j;
            const f4v t0 = p[0], t1 = p[1], t2 = p[2], t3 = p[3];
            const unsigned long long k0 = make_key(canon_d2v(qx, qy, qz, t0), __float_as_uint(t0.w));
            const unsigned long long k1 = make_key(canon_d2v(qx, qy, qz, t1), __float_as_uint(t1.w));
            const unsigned long long k2 = make_key(canon_d2v(qx, qy, qz, t2), __float_as_uint(t2.w));
            const unsigned long long k3 = make_key(canon_d2v(qx, qy, qz, t3), __float_as_uint(t3.w));
            const unsigned long long a = k0 < k1 ? k0 : k1, b = k2 < k3 ? k2 : k3;
            const unsigned long long m = a < b ? a : b;
            best = m < best ? m : best;
            j += 4;
            if constexpr (COST) cost += 1u;
            if (j >= e && ++idx < cnt) {
                const uint2 run = runs[idx * 64u + lane];
                j = run.x;
                e = run.y;
            }
        }
    };
    // Big boxes (queries still far from their neighbour: dozens of rows, most of them empty
    // space) are walked layer by layer, the z-layers in lock-step across the wave: what depends
    // on the layer only (its z distance, the y chord of the ball in it, its base address) is
    // computed once per layer, and only the rows inside the y chord are enumerated at all.
    const bool layered =
        allow_layered && __popcll(__ballot((yb - ya + 1) * (zb - za + 1) > kLayeredRows)) >= 8;
    if (layered) {
        for (int kz = 0;; ++kz) {
            const int zz = za + kz;
            const bool zact = zz <= zb;
            if (__ballot(zact) == 0ull) break;
            const float Rb =
                __builtin_amdgcn_sqrtf(__uint_as_float((unsigned) (best >> 32))) * g.inv_h * 1.00001f;
            const float lim = Rb + g.slack;
            const float lim2 = lim * lim, c0 = Rb * Rb + 2.f * g.slack * lim;
            const float rz = fmaxf(fmaxf((float) zz - fz, fz - (float) (zz + 1)), 0.f);
            const float rz2 = rz * rz;
            // rows of this layer that can touch the ball: their y distance is <= sqrt(lim^2 - rz^2)
            const float hy = __builtin_amdgcn_sqrtf(fmaxf(lim2 - rz2, 0.f)) * 1.00001f;
            const bool zin = zact && !(rz2 > lim2);
            const int yl = zin ? max(ya, __float2int_rd(fy - hy)) : 1;
            const int yh = zin ? min(yb, __float2int_rd(fy + hy)) : 0;
            const unsigned basez = (unsigned) zz * g.ny * g.nx;
            for (int y0 = yl; __ballot(y0 <= yh) != 0ull; y0 += kRowChunk) {
                unsigned a0[kRowChunk], a1[kRowChunk];
#pragma unroll
                for (int u = 0; u < kRowChunk; ++u) {
                    const int yy = y0 + u;
                    const float yf = (float) yy;
                    const float ry = fmaxf(fmaxf(yf - fy, fy - (yf + 1.f)), 0.f);
                    const float rho2 = ry * ry + rz2;
                    const float hx = __builtin_amdgcn_sqrtf(fmaxf(c0 - rho2, 0.f)) * 1.00001f + g.slack;
                    const int xl = max(xa, __float2int_rd(fx - hx)), xh = min(xb, __float2int_rd(fx + hx));
                    const bool ok = yy <= yh && !(rho2 > lim2) && xl <= xh;
                    const unsigned base = basez + (unsigned) yy * g.nx;
                    a0[u] = ok ? base + xl : 0u;
                    a1[u] = ok ? base + xh + 1 : 0u;
                }
                lookup_and_walk(a0, a1);
            }
        }
        return best;
    }
    int yy = ya, zz = za;  // row cursor
    while (zz <= zb) {
        const float Rb =
            __builtin_amdgcn_sqrtf(__uint_as_float((unsigned) (best >> 32))) * g.inv_h * 1.00001f;
        const float lim = Rb + g.slack;
        const float lim2 = lim * lim, c0 = Rb * Rb + 2.f * g.slack * lim;
        // addresses first, then all look-ups back to back and unconditional (a row outside the
        // ball reads cell_start[0] twice: an empty run) -- with predicated loads the compiler
        // interleaves address arithmetic, branches and waits, and the twelve look-ups of a
        // chunk no longer overlap
        unsigned a0[kRowChunk], a1[kRowChunk];
#pragma unroll
        for (int u = 0; u < kRowChunk; ++u) {
            // distance from the query to row (yy, zz) along y and z, in cells: positive on the
            // far side, 0 inside the query's own row (branch-free form of the three cases)
            const float ry = fmaxf(fmaxf((float) yy - fy, fy - (float) (yy + 1)), 0.f);
            const float rz = fmaxf(fmaxf((float) zz - fz, fz - (float) (zz + 1)), 0.f);
            const float rho2 = ry * ry + rz * rz;
            const float hx = __builtin_amdgcn_sqrtf(fmaxf(c0 - rho2, 0.f)) * 1.00001f + g.slack;
            const int xl = max(xa, __float2int_rd(fx - hx)), xh = min(xb, __float2int_rd(fx + hx));
            const bool ok = zz <= zb && !(rho2 > lim2) && xl <= xh;
            const unsigned base = ((unsigned) zz * g.ny + yy) * g.nx;
            a0[u] = ok ? base + xl : 0u;
            a1[u] = ok ? base + xh + 1 : 0u;
            const bool wrap = yy >= yb;
            yy = wrap ? ya : yy + 1;
            zz += wrap;
        }
        lookup_and_walk(a0, a1);
    }
    return best;
}

// scan_run with runner-up tracking: `second` = d2 bits of the closest point seen other than the best
// (meeting the best again -- the seed, a point read past a run's end -- changes nothing)
__device__ __forceinline__ unsigned long long scan_run_bound(const float4 *__restrict__ pts, unsigned s, unsigned e,
                                                             float qx, float qy, float qz, unsigned long long best,
                                                             unsigned &second) {
    for (unsigned j = s; j < e; j += 4) {
        const gp_f4 p = (gp_f4) pts + j;
        const f4v t[4] = {p[0], p[1], p[2], p[3]};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long k = make_key(canon_d2v(qx, qy, qz, t[u]), __float_as_uint(t[u].w));
            if (k < best) {
                second = min(second, (unsigned) (best >> 32));
                best = k;
            } else if (k != best) {
                second = min(second, (unsigned) (k >> 32));
            }
        }
    }
    return best;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float rl_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ unsigned rl_u(unsigned v, int lane) {
    return (unsigned) __builtin_amdgcn_readlane((int) v, lane);
}

// ------------------------------------------------- balanced walk (wave-level work sharing)
// The lane scan above makes a wavefront wait for its slowest lane: in the aligned state a query
// needs 3.3 trips of the candidate loop on average but the slowest of 64 needs 8.4 (measured:
// scripts/dev/dev_cost_model.py), so 60 % of the lanes idle through the loop that is most of the
// kernel -- on the vector ALU and on the L1 address path alike.  Here the wavefront pools the work
// instead: every lane lists its trips (four consecutive points of one of its runs) in LDS, and
// all 64 lanes then take trips off the pooled list, whoever's they are -- ceil(sum / 64) rounds
// instead of max-over-lanes.  A trip's result goes to its query's slot by an LDS atomic min on
// the 64-bit key, so the order in which candidates are seen still does not matter: same results.
// This needs all control flow around the walk to be wave-uniform (a lane that has finished its
// own search keeps working on the others'): the pass and row loops run while ANY lane has work,
// and a lane without work contributes empty rows.
constexpr int kBalCap = 1024;  // pooled trips per chunk of rows; beyond that (rare) every lane walks its own
// rows per chunk of the balanced walk: 2 / 3 / 4 / 6 / 8 / 12 rows measured 73.1 / 70.8 / 72.7 / 73.5 /
// 79.5 / 101 us per launch on the 1M pair (more rows per chunk = more registers and, with the walk
// balanced anyway, nothing gained from batching more look-ups)
constexpr int kBalRowChunk = 3;
struct BalLds {                // per wavefront
    unsigned items[kBalCap + 1];    // (owner lane << 26) | offset of the trip's first point; [kBalCap] = dump slot
    float4 q[64];                   // the queries
    unsigned long long base[64];    // address of the point array (level) each query scans
    unsigned long long best[64];    // running arg-min per query
    // values a lane needs again only after its search (the key it started from, its seed's
    // coordinates): parked here instead of in five registers the compiler would spill to scratch
    unsigned long long seeded[64];
    float bq[3][64];
};

// inclusive prefix sum over the 64 lanes (DPP row shifts inside rows of 16, then the row totals
// are broadcast into the following rows: no LDS traffic, six dependent VALU steps)
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
    v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true);  // row_shr:8
    v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// ubase: the point array all live lanes scan when they are on the same level (the usual case),
// nullptr when the levels differ (then L.base[owner] says which)
template <bool B>
struct BalHolder {
    BalLds v;
};
template <>
struct BalHolder<false> {
    int unused;
};

// Runner-up tracking (BOUND): besides the arg-min the search then also reports a lower bound s of
// the distance from the query to every target point OTHER than its match -- the smaller of the
// second-smallest distance it saw and the radius it pruned with.  While a later pose moves the
// query by less than s - |q - match| the match is still the nearest neighbour and no search is
// needed (k_nn_cert).  To make s useful the scan prunes with min(runner-up, best + pad) instead of
// best: `pad` is how much room the caller wants (a few times the query's last displacement).
struct Bound {
    unsigned second;  // d2 bits of the runner-up so far (a point other than the current best)
    float pad;        // metres
    unsigned *lds;    // [64] words of LDS: the runner-ups while the wave's pooled walk is under way
    float4 *win;      // [64] LDS slots: coordinates (+ index bits) of a candidate that became a query's best
    bool ok;          // false once a path without runner-up tracking has been taken: no bound to offer
    // squared prune radius, as float bits
    __device__ __forceinline__ float prune_r(unsigned long long best) const {
        const float b = __builtin_amdgcn_sqrtf(__uint_as_float((unsigned) (best >> 32))) * 1.00001f + pad;
        return fminf(b, __builtin_amdgcn_sqrtf(__uint_as_float(second)) * 1.00001f);
    }
};

// The rounds of a pooled walk: all 64 lanes take trips (owner lane << 26 | offset of four consecutive
// points) off `items`, whoever's they are, and merge what they find into the owner's slot.
template <bool BOUND>
__device__ __forceinline__ void pooled_rounds(BalLds &L, const unsigned *items, unsigned T, unsigned lane,
                                              const float4 *ubase, Bound *bnd) {
    for (unsigned k0 = 0; k0 < T; k0 += 64u) {
        const unsigned k = k0 + lane;
        if (k < T) {
            const unsigned it = items[k];
            const unsigned owner = it >> 26, j = it & 0x3FFFFFFu;
            const float4 q = L.q[owner];
            const gp_f4 p = (gp_f4) (ubase ? ubase : (const float4 *) L.base[owner]) + j;
            const f4v t0 = p[0], t1 = p[1], t2 = p[2], t3 = p[3];
            const float d0 = canon_d2v(q.x, q.y, q.z, t0), d1 = canon_d2v(q.x, q.y, q.z, t1);
            const float d2 = canon_d2v(q.x, q.y, q.z, t2), d3 = canon_d2v(q.x, q.y, q.z, t3);
            const unsigned m = min(min(__float_as_uint(d0), __float_as_uint(d1)), min(__float_as_uint(d2), __float_as_uint(d3)));
            if (m <= __float_as_uint(q.w)) {  // (d2 >= 0: bit order = numeric order)
                const unsigned long long k0_ = make_key(d0, __float_as_uint(t0.w)), k1_ = make_key(d1, __float_as_uint(t1.w));
                const unsigned long long k2_ = make_key(d2, __float_as_uint(t2.w)), k3_ = make_key(d3, __float_as_uint(t3.w));
                const unsigned long long a = k0_ < k1_ ? k0_ : k1_, b = k2_ < k3_ ? k2_ : k3_;
                if constexpr (BOUND) {
                    // the trip's smallest key contends for the owner's best; whichever of the two loses
                    // is a runner-up candidate, and so is the trip's own second smallest (the global
                    // runner-up is one trip's winner or the best trip's second).  Meeting the same point
                    // again (old == mine: the seed, or a point read past a run's end) changes nothing.
                    const unsigned long long mn = a < b ? a : b;
                    const unsigned u0 = __float_as_uint(d0), u1 = __float_as_uint(d1), u2 = __float_as_uint(d2),
                                   u3 = __float_as_uint(d3);
                    const unsigned lo01 = min(u0, u1), hi01 = max(u0, u1), lo23 = min(u2, u3), hi23 = max(u2, u3);
                    const unsigned sec = min(max(lo01, lo23), min(hi01, hi23));
                    const unsigned long long old = atomicMin(&L.best[owner], mn);
                    unsigned push = sec;
                    if (old != mn) push = min(push, (unsigned) ((old > mn ? old : mn) >> 32));
                    atomicMin(&bnd->lds[owner], push);
                    if (old > mn && bnd->win) {
                        // a new best: its coordinates go to the owner's slot, tagged with its index, so
                        // that the owner need not fetch them from memory afterwards (a slot written by
                        // two winners of one round may hold the loser's: the tag tells)
                        const f4v c = mn == k0_ ? t0 : (mn == k1_ ? t1 : (mn == k2_ ? t2 : t3));
                        bnd->win[owner] = make_float4(c.x, c.y, c.z, c.w);
                    }
                } else {
                    atomicMin(&L.best[owner], a < b ? a : b);
                }
            }
        }
    }
}

template <bool COST, int RC, bool BOUND = false>
__device__ __forceinline__ void balanced_walk(BalLds &L, const unsigned (&rs)[RC],
                                              const unsigned (&re)[RC], unsigned lane,
                                              const float4 *pts, const float4 *ubase, float qx, float qy,
                                              float qz, unsigned long long &best, unsigned &cost,
                                              unsigned long long *prof, Bound *bnd = nullptr) {
    const unsigned long long prof_t0 = COST ? clock64() : 0ull;
    unsigned len[RC], t = 0, longest = 0;
#pragma unroll
    for (int u = 0; u < RC; ++u) {
        len[u] = (unsigned) max((int) (re[u] - rs[u]), 0);
        t += (len[u] + 3u) >> 2;
        longest = max(longest, len[u]);
    }
    const unsigned incl = wave_incl_scan(t);
    const unsigned T = rl_u(incl, 63);
    if (T == 0u) return;  // (wave-uniform)
    if constexpr (COST) cost += t;
    if (T > (unsigned) kBalCap) {  // too much for the list: every lane for itself
        if constexpr (BOUND) {
#pragma unroll
            for (int u = 0; u < RC; ++u) best = scan_run_bound(pts, rs[u], re[u], qx, qy, qz, best, bnd->second);
        } else {
#pragma unroll
            for (int u = 0; u < RC; ++u) best = scan_run(pts, rs[u], re[u], qx, qy, qz, best);
        }
        return;
    }
    unsigned off = incl - t;
    const unsigned tag = lane << 26;
    if (__ballot(longest > 8u) == 0ull) {
        // every run is one or two trips (the usual case): straight-line code, entries that do not
        // exist go to a dump slot past the list
#pragma unroll
        for (int u = 0; u < RC; ++u) {
            L.items[len[u] > 0u ? off : (unsigned) kBalCap] = tag | rs[u];
            L.items[len[u] > 4u ? off + 1u : (unsigned) kBalCap] = tag | (rs[u] + 4u);
            off += (len[u] + 3u) >> 2;
        }
    } else {
#pragma unroll
        for (int u = 0; u < RC; ++u)
            for (unsigned j = rs[u]; j < re[u]; j += 4u) L.items[off++] = tag | j;
    }
    L.best[lane] = best;
    // the owner's best d2 at the start of the walk rides along with its query: a worker builds the four
    // 64-bit keys and issues the LDS atomic only when one of its candidates can get under it -- rarely,
    // once the clouds are close (the seed is usually the neighbour).  A stale bound lets more through, never less.
    if constexpr (BOUND) {
        // ... under the prune radius, that is: runner-up candidates must get through too
        const float pr = bnd->prune_r(best);
        bnd->lds[lane] = bnd->second;
        reinterpret_cast<unsigned *>(&L.q[lane])[3] = __float_as_uint(pr * pr);
    } else {
        reinterpret_cast<unsigned *>(&L.q[lane])[3] = (unsigned) (best >> 32);
    }
    __builtin_amdgcn_wave_barrier();  // (LDS operations of one wave execute in order; this only stops the compiler)
    pooled_rounds<BOUND>(L, L.items, T, lane, ubase, bnd);
    __builtin_amdgcn_wave_barrier();
    best = L.best[lane];
    if constexpr (BOUND) bnd->second = bnd->lds[lane];
    if constexpr (COST) {
        prof[0] += clock64() - prof_t0;  // walk (list building + rounds)
        prof[1] += (T + 63u) / 64u;      // rounds
        prof[2] += 1;                    // walks
    }
}

// scan_box with wave-uniform loops (see above); `live` = this lane has a search of its own going
template <bool COST, int RC, bool BOUND = false>
__device__ __forceinline__ unsigned long long scan_box_bal(const GridDev &g, bool live, float qx, float qy,
                                                           float qz, float r, unsigned long long best,
                                                           float *margin, BalLds &L, unsigned lane,
                                                           bool allow_layered, const float4 *ubase,
                                                           unsigned &cost, unsigned long long *prof, Bound *bnd = nullptr) {
    const float big = 4.0e6f;
    const float fx = fminf(fmaxf((qx - g.ox) * g.inv_h, -big), big);
    const float fy = fminf(fmaxf((qy - g.oy) * g.inv_h, -big), big);
    const float fz = fminf(fmaxf((qz - g.oz) * g.inv_h, -big), big);
    const float rc = r * g.inv_h + g.slack;
    const int x0 = (int) floorf(fx - rc), x1 = (int) floorf(fx + rc);
    const int y0 = (int) floorf(fy - rc), y1 = (int) floorf(fy + rc);
    const int z0 = (int) floorf(fz - rc), z1 = (int) floorf(fz + rc);
    const float mx = fminf(fx - (float) x0, (float) (x1 + 1) - fx);
    const float my = fminf(fy - (float) y0, (float) (y1 + 1) - fy);
    const float mz = fminf(fz - (float) z0, (float) (z1 + 1) - fz);
    *margin = (fminf(mx, fminf(my, mz)) - g.slack) * g.h;
    const int xa = max(x0, 0), xb = min(x1, g.nx - 1);
    const int ya = max(y0, 0), yb = min(y1, g.ny - 1);
    const int za = max(z0, 0), zb = min(z1, g.nz - 1);
    const bool has = live && !(xa > xb || ya > yb || za > zb);
    auto lookup_and_walk = [&](const unsigned (&a0)[RC], const unsigned (&a1)[RC]) {
        unsigned rs[RC], re[RC];
#pragma unroll
        for (int u = 0; u < RC; ++u) {
            rs[u] = ldc(g.cell_start, a0[u]);
            re[u] = ldc(g.cell_start, a1[u]);
        }
        if constexpr (COST) cost += has ? 1u << 16 : 0u;
        balanced_walk<COST, RC, BOUND>(L, rs, re, lane, g.pts, ubase, qx, qy, qz, best, cost, prof, bnd);
    };
    // radius (cell units) beyond which a point cannot matter: the best distance so far -- or, with
    // runner-up tracking, the prune radius
    auto ball_r = [&]() -> float {
        if constexpr (BOUND) return bnd->prune_r(best) * g.inv_h * 1.00001f;
        else return __builtin_amdgcn_sqrtf(__uint_as_float((unsigned) (best >> 32))) * g.inv_h * 1.00001f;
    };
    const bool layered =
        allow_layered && __popcll(__ballot(has && (yb - ya + 1) * (zb - za + 1) > kLayeredRows)) >= 8;
    // NEAREST FIRST (wm_zigzag.hpp): the layers, and the rows of a layer, are visited outwards from the query's own,
    // so `best` -- and with it the ball every later row is cut to -- shrinks in the first chunks of a pass instead of
    // half-way through it (a pass that starts WITHOUT a candidate has one after its first chunks, which is what
    // lets the first search of a registration walk by layers at all: bottom-up it walked the whole cube), and a
    // lane is finished as soon as the nearest layer (row) it has left is outside the ball: `best` only shrinks and
    // what is left only gets farther, so the stop is final.  Lanes that are finished contribute empty rows.
    if (layered) {
        const int zq = min(max(__float2int_rd(fz), za), zb);
        // (the stops use the bound of a query ANYWHERE in its cell -- frac 0 -- instead of its own offset: a layer or
        // a chunk later at most, and two registers fewer in a kernel that has none to spare)
        for (int kz = 0;; ++kz) {
            const float Rb = ball_r();
            const float lim = Rb + g.slack;
            const float lim2 = lim * lim;
            const float dz = zigzag_remaining(kz, za, zq, zb, 0.f);
            const bool zact = has && kz <= zb - za && !(dz * dz > lim2);
            if (__ballot(zact) == 0ull) break;
            const int zz = zigzag_coord(kz, za, zq, zb);
            const float rz = fmaxf(fmaxf((float) zz - fz, fz - (float) (zz + 1)), 0.f);
            const float rz2 = rz * rz;
            const float hy = __builtin_amdgcn_sqrtf(fmaxf(lim2 - rz2, 0.f)) * 1.00001f;
            const bool zin = zact && !(rz2 > lim2);
            const int yl = zin ? max(ya, __float2int_rd(fy - hy)) : 1;
            const int yh = zin ? min(yb, __float2int_rd(fy + hy)) : 0;
            const int yc = min(max(__float2int_rd(fy), yl), yh);  // (an empty layer: yl > yh, no step below is taken)
            const unsigned basez = (unsigned) zz * g.ny * g.nx;
            for (int ky = 0;; ky += RC) {
                // the ball as it is NOW: a chunk's finds cut the next chunk's rows
                const float Rc = ball_r();
                const float limc = Rc + g.slack;
                const float limc2 = limc * limc, c0 = Rc * Rc + 2.f * g.slack * limc;
                const float dy = zigzag_remaining(ky, yl, yc, yh, 0.f);
                const bool yact = ky <= yh - yl && !(dy * dy + rz2 > limc2);
                if (__ballot(yact) == 0ull) break;
                unsigned a0[RC], a1[RC];
#pragma unroll
                for (int u = 0; u < RC; ++u) {
                    const int yy = zigzag_coord(ky + u, yl, yc, yh);
                    const float yf = (float) yy;
                    const float ry = fmaxf(fmaxf(yf - fy, fy - (yf + 1.f)), 0.f);
                    const float rho2 = ry * ry + rz2;
                    const float hx = __builtin_amdgcn_sqrtf(fmaxf(c0 - rho2, 0.f)) * 1.00001f + g.slack;
                    const int xl = max(xa, __float2int_rd(fx - hx)), xh = min(xb, __float2int_rd(fx + hx));
                    const bool ok = yact && ky + u <= yh - yl && !(rho2 > limc2) && xl <= xh;
                    const unsigned base = basez + (unsigned) yy * g.nx;
                    a0[u] = ok ? base + xl : 0u;
                    a1[u] = ok ? base + xh + 1 : 0u;
                }
                lookup_and_walk(a0, a1);
            }
        }
        return best;
    }
    int yy = ya, zz = has ? za : zb + 1;  // row cursor; a lane without rows is past its last one
    while (__ballot(zz <= zb) != 0ull) {
        const float Rb = ball_r();
        const float lim = Rb + g.slack;
        const float lim2 = lim * lim, c0 = Rb * Rb + 2.f * g.slack * lim;
        unsigned a0[RC], a1[RC];
#pragma unroll
        for (int u = 0; u < RC; ++u) {
            const float ry = fmaxf(fmaxf((float) yy - fy, fy - (float) (yy + 1)), 0.f);
            const float rz = fmaxf(fmaxf((float) zz - fz, fz - (float) (zz + 1)), 0.f);
            const float rho2 = ry * ry + rz * rz;
            const float hx = __builtin_amdgcn_sqrtf(fmaxf(c0 - rho2, 0.f)) * 1.00001f + g.slack;
            const int xl = max(xa, __float2int_rd(fx - hx)), xh = min(xb, __float2int_rd(fx + hx));
            const bool ok = zz <= zb && !(rho2 > lim2) && xl <= xh;
            const unsigned base = ((unsigned) zz * g.ny + yy) * g.nx;
            a0[u] = ok ? base + xl : 0u;
            a1[u] = ok ? base + xh + 1 : 0u;
            const bool wrap = yy >= yb;
            yy = wrap ? ya : yy + 1;
            zz += (wrap && zz <= zb) ? 1 : 0;
        }
        lookup_and_walk(a0, a1);
    }
    return best;
}

// Occupancy probe: does the box scan_box_bal would walk for radius r on level g -- floor(f +- (r inv_h + slack)),
// clamped to the lattice -- hold any target point at all?  Answered from cell_start alone: a (y,z) row of the box is
// one contiguous run of the cell-sorted array, so the two look-ups the walk makes per row give the row's point count,
// and no candidate is touched.  The box covers ball(q, r) by the very argument that certifies a scan of it (every
// level's cells are the level-0 cells shifted right: derive_grid_level, clamped at the lattice's last, possibly
// partial, cell exactly as the points' own cells are), so "empty" means: no target point within r of the query.
// A lane without a candidate uses it to find the radius at which a walk first has something to find (k_nn_grid),
// on a level whose cell is about r: a box of some 3 x 3 rows -- kProbeRows pairs of look-ups, one memory round
// trip -- where the walk's own level has 25 or 81.  A non-empty box also names one of its points (`cand`), for the
// lane to start its walk from.
constexpr int kProbeRows = 9;
struct ProbeBox {  // one lane's box on one level, and its row cursor
    int xa, xb, ya, yb, zb, yy, zz;
    unsigned found;  // != 0: a row of the box holds a point
    unsigned cand;   // a point (place in g.pts) of a non-empty row
    __device__ __forceinline__ ProbeBox(const GridDev &g, bool probing, float qx, float qy, float qz, float r) {
        const float big = 4.0e6f;
        const float fx = fminf(fmaxf((qx - g.ox) * g.inv_h, -big), big);
        const float fy = fminf(fmaxf((qy - g.oy) * g.inv_h, -big), big);
        const float fz = fminf(fmaxf((qz - g.oz) * g.inv_h, -big), big);
        const float rc = r * g.inv_h + g.slack;
        xa = max((int) floorf(fx - rc), 0), xb = min((int) floorf(fx + rc), g.nx - 1);
        ya = max((int) floorf(fy - rc), 0), yb = min((int) floorf(fy + rc), g.ny - 1);
        const int za = max((int) floorf(fz - rc), 0);
        zb = min((int) floorf(fz + rc), g.nz - 1);
        const bool has = probing && !(xa > xb || ya > yb || za > zb);
        found = 0u;
        cand = 0u;
        yy = ya, zz = has ? za : zb + 1;  // (a lane without rows is past its last one)
    }
    __device__ __forceinline__ bool more() const { return zz <= zb && found == 0u; }
    // the next kProbeRows rows' look-ups (cell_start[0] twice for a row that does not exist), all requested together
    __device__ __forceinline__ void request(const GridDev &g, unsigned (&rs)[kProbeRows], unsigned (&re)[kProbeRows]) {
        unsigned a0[kProbeRows], a1[kProbeRows];
        const bool go = found == 0u;
#pragma unroll
        for (int u = 0; u < kProbeRows; ++u) {
            const bool ok = go && zz <= zb;
            const unsigned base = ((unsigned) zz * g.ny + yy) * g.nx;
            a0[u] = ok ? base + xa : 0u;
            a1[u] = ok ? base + xb + 1 : 0u;
            const bool wrap = yy >= yb;
            yy = wrap ? ya : yy + 1;
            zz += (wrap && zz <= zb) ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < kProbeRows; ++u) {
            rs[u] = ldc(g.cell_start, a0[u]);
            re[u] = ldc(g.cell_start, a1[u]);
        }
    }
    __device__ __forceinline__ void take(const unsigned (&rs)[kProbeRows], const unsigned (&re)[kProbeRows]) {
#pragma unroll
        for (int u = 0; u < kProbeRows; ++u) found |= re[u] - rs[u];  // (cell_start ascends: a difference is a count)
        // the middle point of a non-empty row, the box's central rows preferred (3 x 3: centre, edges, corners)
        const int order[kProbeRows] = {8, 6, 2, 0, 7, 5, 3, 1, 4};
#pragma unroll
        for (int k = 0; k < kProbeRows; ++k) {
            const int u = order[k];
            if (re[u] != rs[u]) cand = (rs[u] + re[u]) >> 1;
        }
    }
};
// One rung of a lane's radius ladder: is box (g, r) empty (if not: cand = the place in g.pts of one of its points)?
// Wave-uniform loop (one trip for a box of up to kProbeRows rows): lanes that are not probing, are done with their
// rows or have met a point contribute look-ups of cell_start[0].
__device__ __forceinline__ bool probe_box_empty(const GridDev &g, bool probing, float qx, float qy, float qz, float r, unsigned &cand) {
    ProbeBox b(g, probing, qx, qy, qz, r);
    while (__ballot(b.more()) != 0ull) {
        unsigned rs[kProbeRows], re[kProbeRows];
        b.request(g, rs, re);
        b.take(rs, re);
    }
    cand = b.cand;
    return b.found == 0u;
}

// The same scan for a wave with FEW searches going (the certificate kernel's late iterations: a
// handful of unsettled queries per wave, boxes of one to nine rows).  scan_box_bal makes every lane
// step through its own rows three at a time, so a wave with five live lanes still pays a full step
// -- row chords, look-ups, list, round -- per three rows of its largest box.  Here the ROWS are pooled
// too: the owners list (owner, row) pairs in LDS, every lane takes one pair -- the row's chord and its
// two cell_start look-ups, one memory round trip for the whole wave --, the runs found become the
// pooled trip list, and the rounds follow: one pass over everything, whatever the boxes' shapes.
// Runner-up tracking as in the BOUND walk; the chords are cut with the prune radius at entry.
// Returns false (nothing changed) when the job is not small: more than kRowPool rows in the wave,
// more than kRowsPerLane in one box, or more trips than the list holds; the caller then takes
// scan_box_bal.  All live lanes must be on level g.
constexpr unsigned kRowPool = 128, kRowsPerLane = 16, kRowTrips = 512;
struct RowLds {  // overlays BalLds::items (1025 words)
    unsigned trips[kRowTrips];
    unsigned map[kRowPool];   // owner lane | row number << 8
    int box[5][64];           // per owner: xa, xb, ya, za, rows per z layer
};
static_assert(sizeof(RowLds) <= sizeof(unsigned) * (kBalCap + 1), "RowLds overlays BalLds::items");

__device__ __forceinline__ bool scan_box_rows(const GridDev &g, bool live, float qx, float qy, float qz, float r,
                                              unsigned long long &best, float *margin, BalLds &L, unsigned lane,
                                              Bound *bnd) {
    const float big = 4.0e6f;
    const float fx = fminf(fmaxf((qx - g.ox) * g.inv_h, -big), big);
    const float fy = fminf(fmaxf((qy - g.oy) * g.inv_h, -big), big);
    const float fz = fminf(fmaxf((qz - g.oz) * g.inv_h, -big), big);
    const float rc = r * g.inv_h + g.slack;
    const int x0 = (int) floorf(fx - rc), x1 = (int) floorf(fx + rc);
    const int y0 = (int) floorf(fy - rc), y1 = (int) floorf(fy + rc);
    const int z0 = (int) floorf(fz - rc), z1 = (int) floorf(fz + rc);
    const int xa = max(x0, 0), xb = min(x1, g.nx - 1);
    const int ya = max(y0, 0), yb = min(y1, g.ny - 1);
    const int za = max(z0, 0), zb = min(z1, g.nz - 1);
    const bool has = live && !(xa > xb || ya > yb || za > zb);
    const int wy = yb - ya + 1;
    const unsigned nrows = has ? (unsigned) (wy * (zb - za + 1)) : 0u;
    const unsigned incl = wave_incl_scan(nrows);
    const unsigned R = rl_u(incl, 63);
    if (R > kRowPool || __ballot(nrows > kRowsPerLane) != 0ull) return false;
    {
        const float mx = fminf(fx - (float) x0, (float) (x1 + 1) - fx);
        const float my = fminf(fy - (float) y0, (float) (y1 + 1) - fy);
        const float mz = fminf(fz - (float) z0, (float) (z1 + 1) - fz);
        *margin = (fminf(mx, fminf(my, mz)) - g.slack) * g.h;
    }
    if (R == 0u) return true;
    RowLds &W = *reinterpret_cast<RowLds *>(L.items);
    const float pr = bnd->prune_r(best);
    L.best[lane] = best;
    bnd->lds[lane] = bnd->second;
    reinterpret_cast<unsigned *>(&L.q[lane])[3] = __float_as_uint(pr * pr);
    W.box[0][lane] = xa;
    W.box[1][lane] = xb;
    W.box[2][lane] = ya;
    W.box[3][lane] = za;
    W.box[4][lane] = wy;
    for (unsigned k = 0, off = incl - nrows; k < nrows; ++k) W.map[off + k] = lane | (k << 8);
    __builtin_amdgcn_wave_barrier();
    unsigned ttot = 0;  // trips listed and not yet walked (wave-uniform)
    bool fits = true;
    for (unsigned b0 = 0; b0 < R; b0 += 64u) {
        unsigned rs = 0, re = 0, owner = 0;
        if (b0 + lane < R) {
            const unsigned m = W.map[b0 + lane];
            owner = m & 63u;
            const int k = (int) (m >> 8), wyo = W.box[4][owner];
            const int yy = W.box[2][owner] + k % wyo, zz = W.box[3][owner] + k / wyo;
            const float4 q = L.q[owner];
            const float ofx = fminf(fmaxf((q.x - g.ox) * g.inv_h, -big), big);
            const float ofy = fminf(fmaxf((q.y - g.oy) * g.inv_h, -big), big);
            const float ofz = fminf(fmaxf((q.z - g.oz) * g.inv_h, -big), big);
            // the ball that matters, in cells (q.w = the owner's squared prune radius; cushions for the
            // approximate square roots as in scan_box_bal)
            const float Rb = __builtin_amdgcn_sqrtf(q.w) * g.inv_h * 1.00003f;
            const float lim = Rb + g.slack;
            const float lim2 = lim * lim, c0 = Rb * Rb + 2.f * g.slack * lim;
            const float ry = fmaxf(fmaxf((float) yy - ofy, ofy - (float) (yy + 1)), 0.f);
            const float rz = fmaxf(fmaxf((float) zz - ofz, ofz - (float) (zz + 1)), 0.f);
            const float rho2 = ry * ry + rz * rz;
            const float hx = __builtin_amdgcn_sqrtf(fmaxf(c0 - rho2, 0.f)) * 1.00001f + g.slack;
            const int xl = max(W.box[0][owner], __float2int_rd(ofx - hx)), xh = min(W.box[1][owner], __float2int_rd(ofx + hx));
            if (!(rho2 > lim2) && xl <= xh) {
                const unsigned base = ((unsigned) zz * g.ny + yy) * g.nx;
                rs = ldc(g.cell_start, base + xl);
                re = ldc(g.cell_start, base + xh + 1);
            }
        }
        const unsigned len = (unsigned) max((int) (re - rs), 0), t = (len + 3u) >> 2;
        const unsigned incl2 = wave_incl_scan(t);
        const unsigned Tb = rl_u(incl2, 63);
        if (Tb > kRowTrips) {  // (cells this crowded are not the small job this path is for)
            fits = false;
            break;
        }
        if (ttot + Tb > kRowTrips) {
            __builtin_amdgcn_wave_barrier();
            pooled_rounds<true>(L, W.trips, ttot, lane, g.pts, bnd);
            __builtin_amdgcn_wave_barrier();
            ttot = 0;
        }
        unsigned o = ttot + incl2 - t;
        for (unsigned j = rs; j < re; j += 4u) W.trips[o++] = (owner << 26) | j;
        ttot += Tb;
    }
    __builtin_amdgcn_wave_barrier();
    if (fits) pooled_rounds<true>(L, W.trips, ttot, lane, g.pts, bnd);
    __builtin_amdgcn_wave_barrier();
    // (also after a bail-out: whatever the rounds walked so far has been merged, and stays valid)
    best = L.best[lane];
    bnd->second = bnd->lds[lane];
    return fits;
}

// Wave-cooperative version of scan_box for ONE query (q, r, best are wave-uniform):
// the (y,z) rows of the box are first resolved to point ranges by up to 64 lanes in
// parallel (one memory round trip), then every row is streamed by all 64 lanes with
// coalesced float4 loads.  Used for queries far from their neighbour, whose scans
// would otherwise serialise thousands of dependent loads in one lane.
// second_out != nullptr: also the d2 bits of the closest point seen other than the best (runner-up,
// min'd into *second_out: wave-uniform like best)
__device__ __forceinline__ unsigned long long coop_scan_box(const GridDev &g, float qx, float qy,
                                                            float qz, float r,
                                                            unsigned long long best, unsigned lane,
                                                            float *margin, unsigned *second_out = nullptr,
                                                            float pad = 0.f) {
    const float fx = (qx - g.ox) * g.inv_h, fy = (qy - g.oy) * g.inv_h, fz = (qz - g.oz) * g.inv_h;
    const float rc = r * g.inv_h + g.slack;
    const float big = 4.0e6f;
    const int x0 = (int) floorf(fminf(fmaxf(fx - rc, -big), big));
    const int x1 = (int) floorf(fminf(fmaxf(fx + rc, -big), big));
    const int y0 = (int) floorf(fminf(fmaxf(fy - rc, -big), big));
    const int y1 = (int) floorf(fminf(fmaxf(fy + rc, -big), big));
    const int z0 = (int) floorf(fminf(fmaxf(fz - rc, -big), big));
    const int z1 = (int) floorf(fminf(fmaxf(fz + rc, -big), big));
    const float mx = fminf(fx - (float) x0, (float) (x1 + 1) - fx);
    const float my = fminf(fy - (float) y0, (float) (y1 + 1) - fy);
    const float mz = fminf(fz - (float) z0, (float) (z1 + 1) - fz);
    *margin = (fminf(mx, fminf(my, mz)) - g.slack) * g.h;
    const int xa = max(x0, 0), xb = min(x1, g.nx - 1);
    const int ya = max(y0, 0), yb = min(y1, g.ny - 1);
    const int za = max(z0, 0), zb = min(z1, g.nz - 1);
    if (xa > xb || ya > yb || za > zb) return best;
    const int cy = (int) floorf(fminf(fmaxf(fy, -big), big));
    const int cz = (int) floorf(fminf(fmaxf(fz, -big), big));
    const int wy = yb - ya + 1;
    const int nrows = wy * (zb - za + 1);
    const float bd2 = __uint_as_float((unsigned) (best >> 32));
    // best distance (+ the room asked for above it, for the runner-up bound), in cells
    const float Rb = (__builtin_amdgcn_sqrtf(bd2) + pad) * g.inv_h * 1.00001f;
    unsigned long long mine = best;
    unsigned mine2 = 0x7F800000u;  // this lane's runner-up (second_out)
    for (int k0 = 0; k0 < nrows; k0 += 64) {
        // lanes resolve up to 64 rows at once
        const int k = k0 + (int) lane;
        unsigned s = 0, e = 0;
        if (k < nrows) {
            const int yy = ya + k % wy, zz = za + k / wy;
            const float ry = yy > cy ? (float) yy - fy : (yy < cy ? fy - (float) (yy + 1) : 0.f);
            const float rz = zz > cz ? (float) zz - fz : (zz < cz ? fz - (float) (zz + 1) : 0.f);
            // Only the part of the row inside ball(q, sqrt(best)) can hold a closer point: with
            // rho the (y,z) distance of the row, a point of the row closer than Rb has
            // |x - qx| <= sqrt(Rb^2 - (rho - slack)^2) <= sqrt(Rb^2 - rho^2 + 2 slack (Rb + slack))
            // (cell units; Rb inflated by 1e-5 against the approximate square roots).
            const float rho2 = ry * ry + rz * rz;
            const float lim = Rb + g.slack;
            if (!(rho2 > lim * lim)) {
                const float hx2 = fmaxf(Rb * Rb - rho2 + 2.f * g.slack * lim, 0.f);
                const float hx = __builtin_amdgcn_sqrtf(hx2) * 1.00001f + g.slack;
                const int xl = max(xa, (int) floorf(fminf(fmaxf(fx - hx, -big), big)));
                const int xh = min(xb, (int) floorf(fminf(fmaxf(fx + hx, -big), big)));
                if (xl <= xh) {
                    const size_t base = ((size_t) zz * g.ny + yy) * g.nx;
                    s = ldc(g.cell_start, base + xl);
                    e = ldc(g.cell_start, base + xh + 1);
                }
            }
        }
        unsigned long long rows = __ballot(e > s);
        while (rows) {
            const int rl = __ffsll((long long) rows) - 1;
            rows &= rows - 1;
            const unsigned rs = rl_u(s, rl), re = rl_u(e, rl);
            for (unsigned j = rs + lane; j < re; j += 128u) {
                const float4 t0 = ldp(g.pts, j);
                const float4 t1 = ldp(g.pts, j + 64u < re ? j + 64u : j);
                const unsigned long long a = make_key(canon_d2(qx, qy, qz, t0), __float_as_uint(t0.w));
                const unsigned long long b = make_key(canon_d2(qx, qy, qz, t1), __float_as_uint(t1.w));
                const unsigned long long m = a < b ? a : b;
                if (second_out) {  // (wave-uniform branch)
                    const unsigned long long hi = a < b ? b : a;
                    if (m < mine) {
                        mine2 = min(mine2, min((unsigned) (mine >> 32), hi != m ? (unsigned) (hi >> 32) : 0x7F800000u));
                    } else {
                        if (m != mine) mine2 = min(mine2, (unsigned) (m >> 32));
                        if (hi != mine && hi != m) mine2 = min(mine2, (unsigned) (hi >> 32));
                    }
                }
                mine = m < mine ? m : mine;
            }
        }
    }
    const unsigned long long all = wave_min_u64(mine);
    if (second_out) {
        // the wave's runner-up: the lanes' own runner-ups, and the bests of the lanes that do not hold the winner
        unsigned v = mine != all ? min(mine2, (unsigned) (mine >> 32)) : mine2;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = min(v, (unsigned) __shfl_xor((int) v, off));
        *second_out = min(*second_out, v);
    }
    return all;
}

// ------------------------------------------------- small steps of a search (k_nn_grid and k_nn_cert)
// A scan is certified when every point it did not look at is farther than the best it found (or than the
// gate): the box it covered reaches `margin` beyond the query on every side.
__device__ __forceinline__ bool nn_certified(float margin, float bd2, float thr_d2) {
    return margin > 0.f && (bd2 <= margin * margin || thr_d2 <= margin * margin);
}
// Not certified: the radius must GROW (a query sitting on a cell face can have a non-positive margin however small
// its neighbour distance is): to the best distance found (+ pad, the room k_nn_cert's runner-up bound wants; 0.f is
// the same bits as none: the sum it joins is >= 1e-6, never -0), or to 2 r when nothing was found; by a quarter at least
// (v_sqrt_f32, 1 ulp = 6e-8 relative: the cushion of 1e-4 relative + 1e-6 m covers it, as in k_nn_cert's phase 1; a
// radius steers work, never a result)
__device__ __forceinline__ float nn_grow_radius(unsigned long long best, float bd2, float r, float rmax, float pad = 0.f) {
    const float rn = ((unsigned) best != kNoIdx) ? __builtin_amdgcn_sqrtf(bd2) * 1.0001f + 1e-6f + pad : 2.0f * r;
    return fminf(fmaxf(rn, 1.25f * r), rmax);
}
// the finest level whose cell is >= lf * r (cell sizes double from level to level; hl: the levels' cell sizes)
__device__ __forceinline__ int nn_level_for(const float (&hl)[kMaxLevels], int levels, float lf, float r) {
    int l = 0;
#pragma unroll
    for (int k = 0; k < kMaxLevels - 1; ++k) l += (k < levels - 1 && hl[k] < lf * r) ? 1 : 0;
    return l;
}
// k_nn_cert: entry e of the workgroup's unsettled queries (its waves' lists on end, cum[] = their starts) -> wave, place
constexpr int kCertWaves = 4;
__device__ __forceinline__ void chunk_query(unsigned e, const unsigned (&cum)[kCertWaves + 1], unsigned &w, unsigned &k) {
    w = (e >= cum[1] ? 1u : 0u) + (e >= cum[2] ? 1u : 0u) + (e >= cum[3] ? 1u : 0u);
    k = e - (w == 0u ? cum[0] : (w == 1u ? cum[1] : (w == 2u ? cum[2] : cum[3])));
}
// ... and component c of its waves' sums, added in wave order
__device__ __forceinline__ double add_wave_rows(const double (&rows)[kCertWaves][kAcc], unsigned c) {
    double t = rows[0][c];
#pragma unroll
    for (int w = 1; w < kCertWaves; ++w) t += rows[w][c];
    return t;
}

// ------------------------------------------------- fused ICP statistics
// The search kernel ends with every lane holding its query (under the current pose), its
// match and d2 -- exactly what the statistics of the ICP step are summed from (wm_icp.hip:
// n, sum p, sum q, sum q p^T, sum d2 | GN: n, sum p, A^T A, J^T r, sum d2; + the number of
// points this rank handled).  Summing them here deletes a 40 MB stream and a launch per iteration.
//
// (a lane's terms: icp_terms, wm_pair_terms.hpp; the wave reduction by recursive halving: wm_wave.hpp)

}  // namespace wm
