// wm_nn.hip -- exact 1-nearest-neighbour correspondence search on gfx950.
//
// Replaces pcl::registration::CorrespondenceEstimation::determineCorrespondences
// (one FLANN kd-tree 1-NN query per source point per ICP iteration), which is
// where ~95 % of the reference's ICPMatcher::match() time goes
// (wave_matching/src/icp.cpp:95,116,126 -> icp.align()).
//
// Contract (what a FLANN exact search + PCL's distance gate give): for every
// source point the target point with the smallest float squared distance
//     d2 = (dx*dx + dy*dy) + dz*dz            (no FMA contraction)
// provided d2 <= max_corr^2; ties resolve to the lowest target index.  A result
// is carried as one 64-bit key (d2 bits << 32 | target index): non-negative
// floats order like unsigned ints, so "min over keys" is the exact arg-min with
// the tie rule built in, and "no match" is the initial key (threshold, ~0).
//
// Two kernels:
//   k_nn_grid   one lane per query: a certified radius search over a ladder of uniform
//               grids (cell size x2 per level); small radii are scanned by the query's own
//               lane, large ones by the whole wavefront (see the kernel's comment).
//   k_nn_brute  LDS-tiled all-pairs search (small clouds / cross-check).
// (k_nn_cert, the late iterations' certificate kernel: wm_nn_cert.hip; the device code both share: wm_nn_scan.hpp)
#include "wm_nn_scan.hpp"

namespace wm {

// One lane per query: a certified radius search over a ladder of uniform grids
// (cell size x2 per level).
//   r <- the distance, under the NEW pose, to the point this query matched in the previous
//        iteration (a real candidate, so an upper bound of the answer); when there is none (the first search): the
//        distance to one point of the first box of the ladder half a fine cell, x2, x2, ... that holds any -- found by
//        probing the boxes' occupancy on coarse levels, not by walking them (balanced walk; the lane scan walks the ladder);
//   repeat: scan ball(q, min(r, sqrt(best))) inside the box of cells covering [q - r, q + r]^3,
//           on the finest level whose cell is >= lane_lf * r (0.2 r: many short rows, each cut
//           to the ball's chord); certified when best <= margin(box) or the box already covers
//           max_corr; otherwise r <- best (something was found: the next scan is certain to
//           certify) or 2 r.
// Scans up to r_light (12 fine cells: all but ~1e-3 of the queries of a typical pair) run in the
// query's own lane (scan_box).  Longer ones are handed to the whole wavefront, one query at a
// time (coop_scan_box), seeded with the radius its Morton neighbour needed.
// The radius, level and pruning choices change the work, never the result.
// One wavefront per workgroup (finest dispatch granularity, smallest tail; workgroups of 4 / 5 /
// 10 waves cost the search 7 / 30 / 55 %).  STATS < 0: search only.  STATS = WM_ICP_SVD /
// WM_ICP_GN6: the wave also reduces the ICP statistics of its 64 queries to ONE row of `partials`
// ([gridDim.x][kAcc]).  BAL: the wave pools its lanes' candidate trips (balanced walk, wm_nn_scan.hpp);
// otherwise every lane walks its own (kept for targets of 2^26 points and more, and for comparison).
template <int STATS, bool BAL, bool COST = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
    k_nn_grid(const LevelsDev lv, const float4 *__restrict__ src, unsigned n,
              IcpDevState *__restrict__ st, float thr_d2, unsigned long long *__restrict__ keys,
              float4 *__restrict__ match_pt, const float4 *__restrict__ tgt_orig,
              float r_light_cells, float lane_lf, float coop_lf, float r0_cells, unsigned chunk_sz,
              double *__restrict__ partials, unsigned *__restrict__ cost_out,
              unsigned long long *__restrict__ phase_out, long long *__restrict__ bins, float rmax) {
    // (bins != nullptr: the wave's sums are ADDED into the iteration's bins -- exact integer limbs, any order:
    // wm_bins.hpp -- instead of being stored as a row of `partials` for k_reduce_rows to add up)
    // (the wave's life is a chain of memory round trips, and its start is TWO of them: the kernel arguments -- the
    // level ladder among them, by value -- and then, requested together, the head run of the state (nn_state) and the
    // three streams of its chunk: source point, previous key, previous match, whose addresses need nothing but the
    // block number.  The first wait is at the pin below; `done` is tested behind it: a launch queued behind a `done`
    // has loaded (from clamped indices) and leaves without storing or adding anything.  Before the first search keys /
    // match_pt hold nothing meaningful: loaded, not looked at.  Up to eb9ee33 the compiler had the `done` test in
    // front and the loads sunk behind it: seven dependent trips, two of them vector trips in series.)
    // (rmax: the search radius that covers the gate, sqrt(thr_d2) with its cushion -- wave-uniform, formed on the host)
    // (chunk_sz: the XCDs take turns in chunks of this many workgroups, 0: one eighth of the queries each)
    const unsigned lane = threadIdx.x & 63u;
    // (both remaps are formed and one is chosen: a branch on chunk_sz here would put a wait for that one argument in
    // front of the loads of all the others)
    const unsigned row_c = xcd_remap_chunked(blockIdx.x, max(chunk_sz, 1u)), row_e = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned row = chunk_sz ? row_c : row_e;
    const unsigned i = row * 64u + lane;
    const bool active = i < n;
    const unsigned ic = min(i, n - 1u);
    const float4 p_e = src[ic];
    const unsigned long long prev_e = keys[ic];
    const float4 tp_e = match_pt[ic];
    const NnState S = nn_state(st);
    // the levels' cell sizes (wave-uniform); all six come from the kernel arguments at fixed offsets -- no
    // address that depends on the depth; the unused ones (0: the host leaves them so) are never looked at (nn_level_for)
    const int L = lv.n;
    float hl[kMaxLevels];
#pragma unroll
    for (int k = 0; k < kMaxLevels; ++k) hl[k] = lv.g[k].h;
    asm volatile("" ::WM_NN_STATE_OPERANDS(S), "v"(p_e.x), "v"(p_e.y), "v"(p_e.z), "v"(prev_e), "v"(tp_e.x), "v"(tp_e.y),
                 "v"(tp_e.z), "v"(tp_e.w));
    asm volatile("" ::"s"(L), "s"(hl[0]), "s"(hl[1]), "s"(hl[2]), "s"(hl[3]), "s"(hl[4]), "s"(hl[5]), "s"(r_light_cells),
                 "s"(lane_lf), "s"(r0_cells), "s"(thr_d2), "s"(rmax));
    if (S.done) return;
    unsigned cost = 0;
    // developer (COST): shader-clock cycles of this wave's phases, added into phase_out[8] by lane 0:
    // [0] walk, [1] rounds, [2] walks, [3] prologue, [4] pass loop, [5] cooperative phase + stores,
    // [6] statistics tail, [7] waves
    unsigned long long prof[3] = {0ull, 0ull, 0ull};
    const unsigned long long prof_start = COST ? clock64() : 0ull;
    // per wave: [run][lane] = each lane's pending runs (lane scan), or the pooled trip list (balanced walk)
    __shared__ uint2 s_runs[BAL ? 1 : kRowChunk * 64];
    __shared__ BalHolder<BAL> s_hold;
    const int L_levels = L;
    const float h0 = hl[0];
    // larger radii go to the cooperative path.  (Formed again at every use, from the two scalars: there is no scalar
    // float multiply, and kept in a vector register through the whole search it was one the compiler spilled to scratch)
    auto r_light = [&]() -> float {
        float c = r_light_cells;
        asm volatile("" : "+s"(c));
        return c * h0;
    };
    const bool have_prev = S.have_prev != 0;  // wave-uniform
    float qx = 0.f, qy = 0.f, qz = 0.f, r = 0.f;
    float bqx = 0.f, bqy = 0.f, bqz = 0.f;  // coordinates of the previous iteration's match
    unsigned long long best = make_key(thr_d2, kNoIdx);
    unsigned long long seeded = best;  // the key the search started from
    bool heavy = false;
    bool mine = active;
    unsigned long long prev = ~0ull;
    float4 tp = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        if (have_prev) {
            prev = prev_e;
            tp = tp_e;
        }
        xform_pcl(S.Tf, p_e.x, p_e.y, p_e.z, qx, qy, qz);
        // sharded registration: only the rank owning this x-slab handles the point
        if (S.slab_on && !(qx >= S.slab_lo && qx < S.slab_hi)) mine = false;
    }
    // a point of another rank's slab is left untouched: its key / match keep whatever this
    // rank last found for it (still a valid candidate if it ever comes back)
    if (mine) {
        r = r0_cells * h0;
        if (prev != ~0ull) {
            const unsigned pidx = (unsigned) prev;
            r = rmax;  // nothing (close enough) to start from: the full radius
            if (pidx != kNoIdx) {
                // the point matched in the previous iteration is a real candidate: its
                // distance under the NEW pose is an upper bound of the new NN distance, so
                // one scan of ball(q, that distance) is certain to certify
                const float d2b = canon_d2(qx, qy, qz, tp);
                if (d2b <= thr_d2) {
                    best = seeded = make_key(d2b, pidx);
                    bqx = tp.x;
                    bqy = tp.y;
                    bqz = tp.z;
                    // (v_sqrt_f32, 1 ulp: the cushion of 1e-4 relative + 1e-6 m covers it; the radius steers the
                    // scan, the certificate compares exact d2)
                    r = fmaxf(__builtin_amdgcn_sqrtf(d2b) * 1.0001f + 1e-6f, 0.05f * h0);
                }
            }
        }
        r = fminf(r, rmax);
        heavy = r > r_light();
    }
    const unsigned long long prof_pro = COST ? clock64() : 0ull;
    if constexpr (BAL) {
        BalLds &L = s_hold.v;
        L.q[lane] = make_float4(qx, qy, qz, 0.f);
        // parked until the search is over (see BalLds)
        L.seeded[lane] = seeded;
        L.bq[0][lane] = bqx;
        L.bq[1][lane] = bqy;
        L.bq[2][lane] = bqz;
        asm volatile("" ::: "memory");
        bool live = mine && !heavy;
        // (big boxes are walked by layers in unseeded searches too: nearest-first, the walk has a candidate to cut
        // its rows with after the first chunks -- iteration 0 of the 1M pair 466 -> 367 us)
        const bool allow_layered = true;
        // A lane with nothing to start from finds its radius by PROBING, not by walking: the rungs of its ladder
        // (r0 cells, x2 per rung -- the radii the passes below would try in turn) are tested for an empty box on the
        // coarsest level whose cell is <= the rung (probe_box_empty: a round trip of cell_start look-ups per rung, no
        // candidate trips).  An empty probe box contains the box a pass at that radius would have walked, so only
        // passes that would have found nothing are left out.  At the first rung whose box holds a point the lane
        // FETCHES one -- the middle point of a central row of the box -- and, if that is inside the gate and within
        // the lane scan's reach, starts like a seeded query: the point is its candidate and its distance the radius
        // of a pass that is certain to certify, its rows cut to the ball from the first chunk (without a candidate
        // the first pass walked uncut rows until it met a point, certified for 44 % of the queries of the 1M pair,
        // and a second pass walked the ball again for the rest).  A candidate out of reach changes nothing: the
        // lane's first pass is made at the rung's radius, as the ladder would have.  Radii and candidates steer work,
        // never a result, and the lanes that end up heavy are the ladder's.  A seeded launch pays the ballot (a lane
        // whose previous match is out of range starts at rmax and is not probed).
        bool probing = live && (unsigned) best == kNoIdx && r < rmax;
        if (__ballot(probing) != 0ull) {
            float rp = r0_cells * h0;  // the rung: every probing lane's r (wave-uniform)
            for (int rung = 0; rung < 16 && __ballot(probing) != 0ull; ++rung) {
                int lp = 0;
#pragma unroll
                for (int k = 1; k < kMaxLevels; ++k) lp += (k < L_levels && hl[k] <= rp) ? 1 : 0;
                const GridDev g = lv.g[lp];
                unsigned cand;  // a place in g.pts (below the level's point count: a row that holds points)
                const bool empty = probe_box_empty(g, probing, qx, qy, qz, rp, cand);
                const bool hit = probing && !empty;
                const f4v ct = ((gp_f4) g.pts)[hit ? cand : 0u];
                if (hit) {
                    // (a NaN target point fails the comparison; the radius is formed as a seeded query's is)
                    const float d2c = canon_d2v(qx, qy, qz, ct);
                    const float rc = fmaxf(__builtin_amdgcn_sqrtf(d2c) * 1.0001f + 1e-6f, 0.05f * h0);
                    if (d2c <= thr_d2 && rc <= r_light()) {
                        best = make_key(d2c, __float_as_uint(ct.w));
                        r = fminf(rc, rmax);
                    }
                }
                if (probing) {
                    if constexpr (COST) cost += ((cost >> 28) & 7u) < 7u ? 1u << 28 : 0u;  // probe rungs: bits 28-30
                    if (empty) {
                        r = nn_grow_radius(best, 0.f, r, rmax);
                        heavy = r > r_light();
                        live = !heavy;
                    }
                    probing = empty && live && r < rmax;
                }
                rp = fminf(2.0f * rp, rmax);
            }
        }
        for (int pass = 0; pass < 32 && __ballot(live) != 0ull; ++pass) {
            const int l = nn_level_for(hl, L_levels, lane_lf, r);
            // all live lanes on one level (always, once the clouds are close): the level's
            // description comes through scalar loads into SGPRs instead of eleven VGPRs per lane
            // (one level at a time, lanes of the other levels working along, was slower: 77.6 vs
            // 73.4 us per launch)
            const unsigned long long lv_mask = __ballot(live);
            const int l0 = __builtin_amdgcn_readlane(l, __ffsll((long long) lv_mask) - 1);
            float margin;
            if (__ballot(live && l != l0) == 0ull) {
                const GridDev g = lv.g[l0];
                best = scan_box_bal<COST, kBalRowChunk>(g, live, qx, qy, qz, r, best, &margin, L, lane, allow_layered, g.pts, cost, prof);
            } else {
                const GridDev g = lv.g[l];
                L.base[lane] = (unsigned long long) g.pts;
                best = scan_box_bal<COST, kBalRowChunk>(g, live, qx, qy, qz, r, best, &margin, L, lane, allow_layered, nullptr, cost, prof);
            }
            if (live) {
                if constexpr (COST) cost += ((cost >> 24) & 15u) < 15u ? 1u << 24 : 0u;  // passes: bits 24-27
                const float bd2 = __uint_as_float((unsigned) (best >> 32));
                if (nn_certified(margin, bd2, thr_d2)) {
                    live = false;
                } else {
                    r = nn_grow_radius(best, bd2, r, rmax);
                    heavy = r > r_light();
                    live = !heavy;
                }
            }
        }
    } else if (mine) {
        for (int pass = 0; !heavy && pass < 32; ++pass) {
            const int l = nn_level_for(hl, L_levels, lane_lf, r);
            const GridDev g = lv.g[l];
            float margin;
            best = scan_box<COST>(g, qx, qy, qz, r, best, &margin, s_runs, lane, have_prev, cost);
            if constexpr (COST) cost += ((cost >> 24) & 15u) < 15u ? 1u << 24 : 0u;  // passes: bits 24-27
            const float bd2 = __uint_as_float((unsigned) (best >> 32));
            if (nn_certified(margin, bd2, thr_d2)) break;
            // not certified: the radius must GROW (a query sitting on a cell face can have a
            // non-positive margin however small its neighbour distance is)
            r = nn_grow_radius(best, bd2, r, rmax);
            heavy = r > r_light();
        }
    }
    const unsigned long long prof_pass = COST ? clock64() : 0ull;
    // ---- cooperative phase: the wave takes its heavy queries one at a time
    unsigned long long todo = __ballot(heavy);
    const unsigned n_heavy = __popcll(todo);
    float seed = 0.f;  // radius the previous heavy query of this wave ended with
    while (todo) {
        const int sl = __ffsll((long long) todo) - 1;
        todo &= todo - 1;
        const float ux = rl_f(qx, sl), uy = rl_f(qy, sl), uz = rl_f(qz, sl);
        float ur = rl_f(r, sl);
        unsigned long long ub = ((unsigned long long) rl_u((unsigned) (best >> 32), sl) << 32) |
                                rl_u((unsigned) best, sl);
        if ((unsigned) ub == kNoIdx && seed > ur) ur = fminf(seed, rmax);  // neighbour's radius
        for (int pass = 0; pass < 64; ++pass) {
            const int l = nn_level_for(hl, L_levels, coop_lf, ur);
            const GridDev g = lv.g[l];
            float margin;
            ub = coop_scan_box(g, ux, uy, uz, ur, ub, lane, &margin);
            const float bd2 = __uint_as_float((unsigned) (ub >> 32));
            if (nn_certified(margin, bd2, thr_d2)) break;
            if (ur >= rmax) break;
            ur = nn_grow_radius(ub, bd2, ur, rmax);
        }
        seed = ((unsigned) ub != kNoIdx) ? 1.25f * sqrtf(__uint_as_float((unsigned) (ub >> 32))) : ur;
        if ((int) lane == sl) best = ub;
    }
    // (the lane number and the query index are formed again here, from mbcnt: kept from the top of
    // the kernel they -- and the LDS addresses derived from them -- were three registers the
    // compiler spilled to scratch, 16 MB of extra writes and reads per launch)
    const unsigned lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const unsigned i_e = BAL ? row * 64u + lane_e : i;
    if constexpr (BAL) {
        asm volatile("" ::: "memory");
        BalLds &L = s_hold.v;
        seeded = L.seeded[lane_e];
        bqx = L.bq[0][lane_e];
        bqy = L.bq[1][lane_e];
        bqz = L.bq[2][lane_e];
    }
    if (mine) {
        st_u64(&keys[i_e], best);
        // the match's coordinates ride along for the statistics kernel and for the next
        // iteration's seed; a new winner's are read from the caller-ordered target copy
        // (its key carries the original index)
        if (best != seeded && (unsigned) best != kNoIdx) {
            const f4v c = ((gp_f4) tgt_orig)[(unsigned) best];
            bqx = c.x;
            bqy = c.y;
            bqz = c.z;
        }
        // (.w: the match's index, for k_nn_cert.)  A query that KEPT its match -- the seed's key, formed from match_pt[i]
        // itself under this pose, is still the best -- finds match_pt[i] already holding these very coordinates and
        // this index: no store (16 of the 24 result bytes of most queries once the clouds are close)
        if (!(best == seeded && (unsigned) best != kNoIdx))
            st_f4(&match_pt[i_e], bqx, bqy, bqz, __uint_as_float((unsigned) best));
    }
    if (lane == 0 && n_heavy) atomicAdd(&st->queue_count[1], n_heavy);  // stats only
    const unsigned long long prof_store = COST ? clock64() : 0ull;
    if constexpr (COST) {
        if (active) cost_out[i_e] = mine ? (cost | (heavy ? 0x80000000u : 0u)) : 0u;
    }
    if constexpr (STATS >= 0) {
        double a[kAcc];
        icp_terms<STATS>(a, mine, (unsigned) best != kNoIdx, qx, qy, qz, bqx, bqy, bqz,
                         __uint_as_float((unsigned) (best >> 32)),
                         (unsigned) best != (unsigned) seeded && (i_e & st->changed_mask) == 0u);
        acc_halve<kAcc, 32>(a, lane);
        const int comp = acc_comp_of_lane(lane);
        if (comp >= 0) {
            if (bins) bins_add(bins, row % (unsigned) kBinCount, (unsigned) comp, a[0]);
            else st_f64(&partials[(size_t) row * kAcc + comp], a[0]);
        }
    }
    if constexpr (COST) {
        if (lane_e == 0 && phase_out) {
            const unsigned long long t_end = clock64();
            atomicAdd(&phase_out[0], prof[0]);
            atomicAdd(&phase_out[1], prof[1]);
            atomicAdd(&phase_out[2], prof[2]);
            atomicAdd(&phase_out[3], prof_pro - prof_start);
            atomicAdd(&phase_out[4], prof_pass - prof_pro);
            atomicAdd(&phase_out[5], prof_store - prof_pass);
            atomicAdd(&phase_out[6], t_end - prof_store);
            atomicAdd(&phase_out[7], 1ull);
        }
    }
}

// ----------------------------------------------------------- brute force
constexpr int kBruteTile = 1024;

__global__ void __launch_bounds__(kBlock) k_init_keys(unsigned long long *keys, unsigned n,
                                                       const IcpDevState *st, float thr_d2) {
    if (st->done) return;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) keys[i] = make_key(thr_d2, kNoIdx);
}

// grid = (ceil(n / 256), splits); block y scans target slice y.  Every lane
// holds one (transformed) query; the target streams through a float4 LDS tile
// that all lanes read at the same address (LDS broadcast, no bank conflicts).
__global__ void __launch_bounds__(kBlock)
    k_nn_brute(const float4 *__restrict__ tgt, unsigned m, const float4 *__restrict__ src,
               unsigned n, const IcpDevState *__restrict__ st, float thr_d2,
               unsigned long long *__restrict__ keys) {
    if (st->done) return;
    __shared__ float4 tile[kBruteTile];
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned per = (m + gridDim.y - 1) / gridDim.y;
    const unsigned m0 = blockIdx.y * per, m1 = min(m0 + per, m);
    float qx = 0, qy = 0, qz = 0;
    if (i < n) xform_pcl(st->Tf, src[i].x, src[i].y, src[i].z, qx, qy, qz);
    const bool mine = !(st->slab_on && !(qx >= st->slab_lo && qx < st->slab_hi));
    unsigned long long best = make_key(thr_d2, kNoIdx);
    for (unsigned t0 = m0; t0 < m1; t0 += kBruteTile) {
        const unsigned cnt = min((unsigned) kBruteTile, m1 - t0);
        __syncthreads();
        for (unsigned k = threadIdx.x; k < cnt; k += kBlock) tile[k] = tgt[t0 + k];
        __syncthreads();
        for (unsigned k = 0; k < cnt; ++k) {
            const float4 t = tile[k];
            // non-finite target points were packed as NaN: their key (0x7FC0....)
            // exceeds every finite threshold and never wins
            const unsigned long long key = make_key(canon_d2(qx, qy, qz, t), __float_as_uint(t.w));
            best = key < best ? key : best;
        }
    }
    if (i < n && mine && best < make_key(thr_d2, kNoIdx)) atomicMin(&keys[i], best);
}

// after the all-pairs search: coordinates of every match (the grid search tracks them itself)
__global__ void __launch_bounds__(kBlock)
    k_fill_match(const unsigned long long *__restrict__ keys, unsigned n,
                 const float4 *__restrict__ tgt, const IcpDevState *__restrict__ st,
                 float4 *__restrict__ match_pt) {
    if (st->done) return;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned idx = (unsigned) keys[i];
    match_pt[i] = idx == kNoIdx ? make_float4(0.f, 0.f, 0.f, __uint_as_float(kNoIdx)) : tgt[idx];
}

// largest float whose value, compared as PCL does ((double) d2 > max_corr^2 -> reject), is still accepted;
// strict: accepted iff (double) d2 < max_corr^2 (estimateLUMold's gate)
static float threshold_below(double max_corr, bool strict) {
    const double m2 = max_corr * max_corr;
    if (!(m2 < 3.0e38)) return 3.0e38f;
    float f = (float) m2;
    if (strict ? (double) f >= m2 : (double) f > m2) f = nextafterf(f, 0.0f);
    return f;
}
float threshold_d2(double max_corr) { return threshold_below(max_corr, false); }
float threshold_d2_strict(double max_corr) { return threshold_below(max_corr, true); }

// where a search kernel's sums go (stats_mode >= 0): into the iteration's bins (use_bins; *rows_out, which the caller
// has set to 0, is left alone), or into `blocks` rows of ctx->partials (*rows_out = blocks)
int nn_sums_target(wm_ctx *ctx, int stats_mode, bool use_bins, unsigned blocks, long long **bins, unsigned *rows_out) {
    *bins = nullptr;
    if (stats_mode >= 0 && use_bins) {
        if (!ctx->bins.p) return WM_ERR_STATE;  // (the caller's loop made them ready: bins_ready, wm_icp.hip)
        *bins = ctx->bins.as<long long>();
    } else if (stats_mode >= 0) {
        WM_HIP(ctx, ctx->partials.reserve((size_t) blocks * kAcc * sizeof(double)));
        if (rows_out) *rows_out = blocks;
    }
    return WM_OK;
}

template <int STATS, bool BAL, bool COST = false>
static void launch_nn_grid_t(wm_ctx *ctx, unsigned blocks, float thr_d2, unsigned xcd_chunk, long long *bins = nullptr) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nn_grid<STATS, BAL, COST>), dim3(blocks), dim3(64), 0, ctx->stream,
                       ctx->levels_dev, ctx->src_sorted.as<float4>(), (unsigned) ctx->n_src,
                       ctx->d_state.as<IcpDevState>(), thr_d2, ctx->keys.as<unsigned long long>(),
                       ctx->match_pt.as<float4>(), ctx->tgt_orig.as<float4>(), ctx->tune_r_light,
                       ctx->tune_lane_lf, ctx->tune_coop_lf, ctx->tune_r0, xcd_chunk, ctx->partials.as<double>(),
                       ctx->cost_log.p ? ctx->cost_log.as<unsigned>() + (size_t) ctx->cost_log_iter * ctx->n_src : nullptr,
                       ctx->phase_log.p ? ctx->phase_log.as<unsigned long long>() + 8 * (size_t) ctx->cost_log_iter : nullptr, bins,
                       sqrtf(thr_d2) * 1.0001f + 1e-6f);
}

// stats_mode < 0: search only.  WM_ICP_SVD / WM_ICP_GN6: the search kernel also leaves the ICP
// statistics of this iteration as *rows_out rows of kAcc doubles in ctx->partials.
// use_bins (with a stats_mode): the sums go into the iteration's bins (wm_bins.hpp) -- *rows_out is 0 then, and the
// solve is launch_bins_solve
int launch_nn_grid(wm_ctx *ctx, float thr_d2, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2,
                   int stats_mode, unsigned *rows_out, bool use_bins) {
    const unsigned n = (unsigned) ctx->n_src;
    if (rows_out) *rows_out = 0;
    if (n == 0) return WM_OK;
    unsigned blocks = (n + 63u) / 64u;
    blocks = (blocks + 7u) & ~7u;  // xcd_remap needs a multiple of 8
    unsigned xcd_chunk = 0;
    if (ctx->tune_xcd_chunk > 0 && blocks >= 32u * (unsigned) ctx->tune_xcd_chunk) {
        // the chunked remap (big grids only: it pads the grid to a multiple of 8 chunks)
        xcd_chunk = (unsigned) ctx->tune_xcd_chunk;
        const unsigned m = 8u * xcd_chunk;
        blocks = (blocks + m - 1u) / m * m;
    }
    long long *bins = nullptr;
    const int rc = nn_sums_target(ctx, stats_mode, use_bins, blocks, &bins, rows_out);
    if (rc != WM_OK) return rc;
    // the balanced walk packs (lane, point offset) into 32 bits: targets below 2^26 points
    const bool bal = ctx->tune_nn_balanced && ctx->n_tgt_input < (1u << 26) - 8u;
    if (ev0) WM_HIP(ctx, hipEventRecord(ev0, ctx->stream));
    if (stats_mode == WM_ICP_SVD && ctx->cost_log.p && ctx->cost_log_iter < ctx->cost_log_cap) {
        if (bal) launch_nn_grid_t<WM_ICP_SVD, true, true>(ctx, blocks, thr_d2, xcd_chunk, bins);  // developer statistics
        else launch_nn_grid_t<WM_ICP_SVD, false, true>(ctx, blocks, thr_d2, xcd_chunk, bins);
        ctx->cost_log_iter++;
    } else if (stats_mode < 0) {
        if (bal) launch_nn_grid_t<-1, true>(ctx, blocks, thr_d2, xcd_chunk);
        else launch_nn_grid_t<-1, false>(ctx, blocks, thr_d2, xcd_chunk);
    } else if (stats_mode == WM_ICP_SVD) {
        if (bal) launch_nn_grid_t<WM_ICP_SVD, true>(ctx, blocks, thr_d2, xcd_chunk, bins);
        else launch_nn_grid_t<WM_ICP_SVD, false>(ctx, blocks, thr_d2, xcd_chunk, bins);
    } else {
        if (bal) launch_nn_grid_t<WM_ICP_GN6, true>(ctx, blocks, thr_d2, xcd_chunk, bins);
        else launch_nn_grid_t<WM_ICP_GN6, false>(ctx, blocks, thr_d2, xcd_chunk, bins);
    }
    if (ev1) WM_HIP(ctx, hipEventRecord(ev1, ctx->stream));
    if (ev2) WM_HIP(ctx, hipEventRecord(ev2, ctx->stream));
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

int launch_nn_brute(wm_ctx *ctx, float thr_d2, hipEvent_t ev0, hipEvent_t ev1) {
    const unsigned n = (unsigned) ctx->n_src, m = (unsigned) ctx->n_tgt_input;
    if (n == 0) return WM_OK;
    const IcpDevState *st = ctx->d_state.as<IcpDevState>();
    unsigned long long *keys = ctx->keys.as<unsigned long long>();
    const unsigned bx = (n + kBlock - 1) / kBlock;
    unsigned splits = 1;
    if (m > 0) {
        // enough workgroups to fill 256 CUs several times over
        splits = (2048 + bx - 1) / bx;
        const unsigned max_splits = (m + kBruteTile - 1) / kBruteTile;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
    }
    if (ev0) WM_HIP(ctx, hipEventRecord(ev0, ctx->stream));
    hipLaunchKernelGGL(k_init_keys, dim3(bx), dim3(kBlock), 0, ctx->stream, keys, n, st, thr_d2);
    if (m > 0)
        hipLaunchKernelGGL(k_nn_brute, dim3(bx, splits), dim3(kBlock), 0, ctx->stream,
                           ctx->tgt_orig.as<float4>(), m, ctx->src_sorted.as<float4>(), n, st,
                           thr_d2, keys);
    hipLaunchKernelGGL(k_fill_match, dim3(bx), dim3(kBlock), 0, ctx->stream, keys, n,
                       ctx->tgt_orig.as<float4>(), st, ctx->match_pt.as<float4>());
    if (ev1) WM_HIP(ctx, hipEventRecord(ev1, ctx->stream));
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

}  // namespace wm
