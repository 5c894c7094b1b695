// wm_nn_cert.hip -- the certificate kernel of the late ICP iterations, launched and resident (device code shared
// with the full search, wm_nn.hip: wm_nn_scan.hpp)
#include "wm_nn_scan.hpp"

#include <atomic>

namespace wm {

// ------------------------------------------------- certified correspondences (late iterations)
// Once the clouds are nearly aligned an ICP step moves a source point by far less than the spacing of
// the target, and almost every query keeps its neighbour.  That can be PROVED per query without a
// search: the last search of the query left, besides its match m, the query's position and a lower
// bound s on its distance, there, to every target point other than m (runner-up tracking, `Bound`,
// wm_nn_scan.hpp).  If now, with disp the distance moved since,
//     |q - m| < s - disp        (with float-rounding cushions)
// then every other point is strictly farther than m: m is the exact nearest neighbour, ties
// included, and the query is SETTLED by three stream reads (source point, match, position + bound:
// 48 B) and NO write: its key keeps the match's index, and the distance in it is brought up to date
// once, when the registration ends (k_fix_keys).  Queries that fail the test are searched with the
// pooled walk of k_nn_grid, pruning with min(runner-up, best + pad) so that the bound they leave is
// worth something (pad = pad_mul x the size of the last step, at most pad_frac x the seed distance).
// Same keys, bit for bit, as a full search of every query.
//
// A workgroup of four waves handles 4 x NB x 64 consecutive (Morton-ordered) queries:
//   phase 1  every wave: NB batches of 64 -- certificate test, the settled queries' terms of the
//            iteration's sums (two batches added lane by lane, then a wave reduction); the unsettled
//            ones are listed, in query order, in the wave's LDS (the first 64 with their data);
//   phase 2  the unsettled queries of the whole workgroup in chunks of 64, chunk c by wave c mod 4:
//            the search, stores, sums.  Once aligned a workgroup has a handful of them: ONE wave
//            runs one chunk instead of four waves running one each -- the kernel is bound by
//            instruction issue, and a chunk costs the same whether 3 or 60 of its lanes are live;
//   the four waves' sums are added in wave order: one row of partial sums per workgroup (a 1M cloud
//   leaves 984 rows: the solve kernel adds them itself, no row-reduction launch).
// bounds_valid = 0: no usable bounds (the previous iteration was searched by k_nn_grid): every query
// is searched and leaves its bound.

// ---- the RESIDENT form of the certificate kernel (LATE = true): the late iterations of one registration
// in ONE launch.  Every workgroup keeps its 4 x NB x 64 queries from iteration to iteration (their three
// streams -- source point, match, position + bound -- are requested again while the solver works: L2 /
// Infinity Cache hits that cost no time of their own), the
// iteration's sums meet in device memory (one row per workgroup, written through; a ticket per workgroup),
// and ONE extra workgroup -- the solver, a kernel of its own on a second stream -- adds the rows in a fixed order,
// runs the solve and PCL's stopping rules (icp_apply_stats: what k_reduce_solve runs), publishes the
// iteration's record to the host and hands the new pose to the workers through a 64-byte slot.  What a
// launched certified iteration pays around its ~6 us of work -- two kernel boundaries, 48 MB of streams,
// the dispatch of 4 000 waves -- is gone.  Every workgroup has to be resident at once (checked on the
// host against the kernel's occupancy and the device's budget of resident workgroups); every wait gives
// up after kLateGuardTicks and sets `abandoned`, after which everybody leaves and the host continues with
// launched iterations from the state the solver wrote back.  No agent-scope fences anywhere (an XCD-wide
// L2 write-back each): rows, pose and counters are written through / read at agent scope.
// (every word that is polled or hammered sits in a 128-byte line of its own, and the word the thousand
// workers wait on exists sixteen times: a worker that has delivered its row looks at copy (workgroup mod
// 16) -- a thousand pollers of ONE line keep its memory channel so busy that the ticket atomics and row
// stores of the workgroups still working queue up behind them)
constexpr int kLateGenCopies = 16;
struct LateCtl {            // device memory
    unsigned ticket;        // rows delivered so far (monotonic over the iterations of one launch)
    unsigned pad0[31];
    unsigned abandoned;     // a wait timed out somewhere: everybody leaves
    unsigned pad1[31];
    float bc[2][16];        // by parity of the iteration: Tf[12], step size, flags (bit 0: stop), 2 spare
    struct {
        unsigned gen;       // iterations whose result the solver has handed out (0xFFFFFFFF: leave, a wait gave up)
        unsigned pad[31];
    } g[kLateGenCopies];
};
static_assert(sizeof(LateCtl) == 384 + 128 * kLateGenCopies, "layout");
struct LateArgs {
    LateCtl *ctl;
    unsigned long long *pub;     // pinned: the iterations' records (as k_reduce_solve writes them)
    int pub_slots;
    unsigned long long *h_exit;  // pinned: [exit_seq : 32 | reason : 8 | iterations done inside : 24], written last
    unsigned exit_seq;
    float stop_unsettled;        // leave when an iteration had to search more than this share of the queries ...
    float stop_disp;             // ... or a step moved the points by more than this (metres)
    int max_inside;              // ... or after this many iterations
    unsigned long long *dbg;     // developer (WM_LATE_DEBUG): 4 wall-clock stamps per iteration from the solver
    unsigned long long *dbg_w;   // ... and 8 per WORKER for iteration dbg_li
    unsigned dbg_li;
};
constexpr unsigned long long kLateGuardTicks = 20000000ull;  // 0.2 s of the 100 MHz wall clock
constexpr int kLateRow = 20;  // doubles per workgroup row: the kAcc sums, the queries it searched, one spare
enum { kLateDone = 1, kLatePolicy = 2, kLateAbandoned = 3, kLateBudget = 4 };

__device__ __forceinline__ unsigned ld_agent_u32(const unsigned *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the solver workgroup of the resident kernel: see above
struct LateSolverLds {
    IcpDevState st;
    double part[12][kLateRow];
    double tot[kLateRow];
    unsigned go, flags;
};
__global__ void __launch_bounds__(64 * kCertWaves) __attribute__((amdgpu_waves_per_eu(4, 4)))
    k_late_solver(const double *partials, unsigned workers, IcpDevState *st, LateArgs la) {
    // (a kernel of its own, on a second stream beside the workers': its f64 solve and its 28 loads in flight per
    // thread would otherwise set the register allocation of the search loop.  One workgroup, and no bigger than
    // a worker's in threads / registers / LDS: it fits wherever a worker fits)
    __shared__ LateSolverLds S;
    LateCtl *ctl = la.ctl;
    constexpr unsigned kWords = sizeof(IcpDevState) / 4;
    for (unsigned w = threadIdx.x; w < kWords; w += 64u * kCertWaves)
        reinterpret_cast<unsigned *>(&S.st)[w] = reinterpret_cast<const unsigned *>(st)[w];
    __syncthreads();
    unsigned reason = 0, inside = 0;
    if (S.st.done) reason = kLateDone;  // (queued behind a `done`: nothing to do -- the workers have left too)
    for (unsigned li = 0; reason == 0u; ++li) {
        // ---- all rows of this iteration in?
        if (threadIdx.x < 64u) {
            const unsigned want = (li + 1u) * workers;
            const unsigned long long t0 = wall_clock64();
            bool ok = true;
            for (;;) {
                if ((int) (ld_agent_u32(&ctl->ticket) - want) >= 0) break;
                if (ld_agent_u32(&ctl->abandoned) != 0u || wall_clock64() - t0 > kLateGuardTicks) {
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (threadIdx.x == 0) S.go = ok ? 1u : 0u;
            if (threadIdx.x == 0 && la.dbg && li < 64u) la.dbg[li * 4u + 0u] = wall_clock64();  // all rows in
        }
        __syncthreads();
        if (!S.go) {
            if (threadIdx.x == 0) __hip_atomic_store(&ctl->abandoned, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            reason = kLateAbandoned;
        } else {
            // ---- the rows, in a fixed order: thread (r, c) adds rows r, r + 12, ... of column c (28 loads in
            // flight per thread: three round trips for a thousand rows), one thread per column adds the 12
            const unsigned c = threadIdx.x % (unsigned) kLateRow, r = threadIdx.x / (unsigned) kLateRow;
            if (r < 12u) {
                double acc = 0.0;
                constexpr int U = 28;
                for (unsigned b = r; b < workers; b += 12u * U) {
                    double v[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const unsigned bb = b + 12u * (unsigned) u;
                        v[u] = bb < workers ? __hip_atomic_load(partials + (size_t) bb * kLateRow + c, __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT)
                                            : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) acc += v[u];
                }
                S.part[r][c] = acc;
            }
            __syncthreads();
            if (threadIdx.x < (unsigned) kLateRow) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 12; ++k) t += S.part[k][threadIdx.x];
                S.tot[threadIdx.x] = t;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                if (la.dbg && li < 64u) la.dbg[li * 4u + 1u] = wall_clock64();  // rows added
                double a[kAcc], ex[kStatsLen];
#pragma unroll
                for (int k = 0; k < kAcc; ++k) a[k] = S.tot[k];
                expand_stats(S.st.mode, a, ex, S.st.changed_mask);
                S.st.local_handled = ex[kStatsLen - 1];
#pragma unroll
                for (int k = 0; k < kStatsLen; ++k) S.st.stats[k] = ex[k];
                icp_apply_stats(&S.st, ex, (long long) S.tot[kAcc]);
                // (the rule to leave, on this iteration's unquantised values; the host's rule for the launched
                // iterations reads the quantised record of an earlier one: CertPolicy::decide, wm_icp_ctl.hpp)
                unsigned fl = 0;
                if (S.st.done) fl = kLateDone;
                else if ((li > 0u || S.st.frac_unsettled < 0.999f) && S.st.frac_unsettled > la.stop_unsettled) fl = kLatePolicy;
                else if (S.st.step_disp > la.stop_disp) fl = kLatePolicy;
                else if ((int) (li + 1u) >= la.max_inside) fl = kLateBudget;
                S.flags = fl;
                if (la.dbg && li < 64u) la.dbg[li * 4u + 2u] = wall_clock64();  // solved
                publish_step(&S.st, la.pub, la.pub_slots);  // (the record k_reduce_solve publishes)
            }
            __syncthreads();
            reason = S.flags;
            inside = li + 1u;
        }
        // ---- the pose of the next iteration (or the word to leave) for the workers: data, wait, then the number
        if (threadIdx.x < 16u) {
            const unsigned t = threadIdx.x;
            const float v = t < 12u ? S.st.Tf[t] : (t == 12u ? S.st.step_disp : (t == 13u ? __uint_as_float(reason) : 0.f));
            __hip_atomic_store(&ctl->bc[(li + 1u) & 1u][t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (threadIdx.x < (unsigned) kLateGenCopies)
            __hip_atomic_store(&ctl->g[threadIdx.x].gen, reason == (unsigned) kLateAbandoned ? ~0u : li + 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x == 0 && la.dbg && li < 64u) la.dbg[li * 4u + 3u] = wall_clock64();  // handed out
    }
    // ---- the state goes back to memory for the kernels behind this one; the host learns how it ended
    __syncthreads();
    for (unsigned w = threadIdx.x; w < kWords; w += 64u * kCertWaves)
        reinterpret_cast<unsigned *>(st)[w] = reinterpret_cast<const unsigned *>(&S.st)[w];
    if (threadIdx.x == 0 && la.h_exit)
        __hip_atomic_store(la.h_exit, ((unsigned long long) la.exit_seq << 32) | ((unsigned long long) (reason & 0xFFu) << 24) |
                                          (unsigned long long) (inside & 0xFFFFFFu),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// developer (WM_LATE_DEBUG): wall-clock stamp k of this worker, for iteration la.dbg_li of the resident form
template <bool LATE>
__device__ __forceinline__ void late_wstamp(unsigned long long *dbg_w, unsigned dbg_li, unsigned li, unsigned k) {
    if constexpr (LATE)
        if (dbg_w && li == dbg_li && threadIdx.x == 0) dbg_w[(size_t) blockIdx.x * 8u + k] = wall_clock64();
}

template <int STATS, int NB, int RC, bool LATE = false>
__global__ void __launch_bounds__(64 * kCertWaves) __attribute__((amdgpu_waves_per_eu(4, 4)))
    k_nn_cert(const LevelsDev lv, const LevelsDev *__restrict__ lvp, const float4 *__restrict__ src, unsigned n,
              IcpDevState *__restrict__ st, float thr_d2, unsigned long long *__restrict__ keys,
              float4 *__restrict__ match_pt, float4 *__restrict__ bound, const float4 *__restrict__ tgt_orig,
              float r_light_cells, float lane_lf, float coop_lf, float r0_cells,
              double *__restrict__ partials, int bounds_valid, float pad_mul, float pad_frac,
              unsigned *__restrict__ uns_count, unsigned long long *__restrict__ prof_out, LateArgs la,
              long long *__restrict__ bins, float rmax) {
    // (bins != nullptr, launched form only: the workgroup's sums and its count of searched queries are ADDED into
    // the iteration's bins -- exact integer limbs, any order: wm_bins.hpp -- instead of stored as a row of `partials`)
    // (a wave's life is a chain of memory round trips, and its start is TWO of them: the kernel arguments -- the level
    // ladder among them, by value -- and then, requested together, the head run of the state (nn_state, wm_nn_scan.hpp)
    // and the phase's three streams, whose addresses need nothing but the block number.  The first wait is at the
    // pin below and `done` is tested behind it (up to eb9ee33 the compiler had that test, a round trip of its own, in
    // front of the loads): a launch queued behind a `done` has loaded, from clamped indices, and leaves without
    // storing or adding anything)
    // (lvp: the ladder's copy in device memory, for a level above 0 chosen at run time.  Looked up in the by-value
    // copy, as k_nn_grid does, it costs this kernel a stack slot: 20 bytes of scratch where it had none)
    // (rmax: the search radius that covers the gate, sqrt(thr_d2) with its cushion -- wave-uniform, formed on the host)
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const unsigned row = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned gbase = row * (64u * NB * kCertWaves);  // the workgroup's first query
    const unsigned base = gbase + wave * (64u * NB);        // the wave's
    // (the stream loads' clamp is made to wait for `st` as well: the kernel arguments come in ONE batch and the state
    // is requested with the streams -- left alone the compiler fetches `st` behind them, one more wait)
    unsigned n_st = n;
    asm("" : "+s"(n_st) : "s"(st));
    const NnState S = nn_state(st);
    float4 p[NB], mp[NB], rf[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const unsigned i = min(base + (unsigned) j * 64u + lane, n_st - 1u);
        p[j] = src[i];
        mp[j] = match_pt[i];  // (meaningless before the first search, and then not looked at)
        rf[j] = bound[i];
    }
    // the levels' cell sizes (wave-uniform: scalar registers); all six come from the kernel arguments at fixed offsets
    // -- no address that depends on the depth; the unused ones (0: the host leaves them so) are never looked at (nn_level_for)
    const int Ln = lv.n;
    float hl[kMaxLevels];
#pragma unroll
    for (int k = 0; k < kMaxLevels; ++k) hl[k] = lv.g[k].h;
    // (the requests above stay above this line, the first wait below it: the state's words, then the kernel arguments
    // the searches use)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::WM_NN_STATE_OPERANDS(S), "s"(S.step_disp), "s"(S.changed_mask));
    asm volatile("" ::"s"(Ln), "s"(hl[0]), "s"(hl[1]), "s"(hl[2]), "s"(hl[3]), "s"(hl[4]), "s"(hl[5]), "s"(r_light_cells),
                 "s"(lane_lf), "s"(r0_cells), "s"(thr_d2), "s"(rmax));
    // `done` (uniform over the workgroup) is tested BEHIND phase 1 in the launched form: in front of it the test either
    // pulls the stream loads behind its branch (the compiler's choice up to eb9ee33: a round trip for `done` alone in
    // front of the burst) or, with the loads held in front of it, makes phase 1 wait for the last of the twelve loads
    // before it may touch the first batch (+0.4 us per launch, measured).  Phase 1 writes nothing but this workgroup's
    // LDS, so a launch queued behind a `done` still stores nothing and adds nothing.
    if constexpr (LATE) {
        if (S.done) return;  // (the solver tells the host)
    }
    // LATE: the three streams of the later iterations come through buffer loads the compiler cannot hoist out
    // of the iteration loop (kept in registers across the searches they would be spilled to scratch: the
    // searches need every register); the match and the bound at agent scope (sc1), past this compute unit's
    // L1 -- the workgroup's own searches of the previous iteration rewrote some of them
    const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void *) src, 0, LATE ? n * 16u : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_mp = __builtin_amdgcn_make_buffer_rsrc((void *) match_pt, 0, LATE ? n * 16u : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_rf = __builtin_amdgcn_make_buffer_rsrc((void *) bound, 0, LATE ? n * 16u : 0u, 0x00020000);
    // developer (prof_out): shader-clock stamps of wave 0 of every 256th workgroup, 16 per sample
    // (the phases between them: scripts/dev/dev_cert_prof.py); nothing is recorded otherwise
    const bool stamp_on = prof_out != nullptr && (blockIdx.x & 255u) == 0u && wave == 0u;
    unsigned long long pt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pt[k] = 0ull;
    if (stamp_on) pt[0] = clock64();
    __shared__ BalLds s_L[kCertWaves];
    __shared__ unsigned s_second[kCertWaves][64];
    __shared__ float4 s_win[kCertWaves][64];
    __shared__ unsigned short s_list[kCertWaves][64 * NB];
    __shared__ unsigned s_cnt[kCertWaves];
    __shared__ double s_rows[kCertWaves][kAcc];
    __shared__ float s_bc[20];  // LATE: this iteration's pose, step size, flags, [16] = a wait gave up
    BalLds &L = s_L[wave];
    s_win[wave][lane] = make_float4(0.f, 0.f, 0.f, __uint_as_float(kNoIdx));  // (no winner recorded)
    const GridDev g0 = lv.g[0];  // (what the late searches scan)
    const float h0 = hl[0];
    const float r_light = r_light_cells * h0;
    const bool have_prev = S.have_prev != 0;
    // sharded registration: this rank handles the queries whose transformed x lies in its slab (a query
    // it does not own is skipped: no test, no search, nothing stored -- whatever this rank knew about
    // it stays consistent for the day it comes back)
    const bool slab_on = S.slab_on != 0;
    const float slab_lo = S.slab_lo, slab_hi = S.slab_hi;
    const unsigned changed_mask = S.changed_mask;
    const int comp = acc_comp_of_lane(lane);
    if (stamp_on) pt[1] = clock64();  // state in
    // (LATE: one trip per iteration of the registration; otherwise one trip)
    for (unsigned li = 0;; ++li) {
        // ---- this iteration's pose, step size, and whether bounds exist
        if constexpr (LATE) {
            if (li > 0u) {
                // (requested BEFORE the wait for the solver: they arrive while it works)
                typedef unsigned u4v __attribute__((ext_vector_type(4)));
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const unsigned i = min(base + (unsigned) j * 64u + lane, n - 1u);
                    const u4v a = __builtin_amdgcn_raw_buffer_load_b128(rs_src, i * 16u, 0, 0);
                    const u4v b = __builtin_amdgcn_raw_buffer_load_b128(rs_mp, i * 16u, 0, 16);
                    const u4v c = __builtin_amdgcn_raw_buffer_load_b128(rs_rf, i * 16u, 0, 16);
                    p[j] = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
                    mp[j] = make_float4(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w));
                    rf[j] = make_float4(__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w));
                }
                if (wave == 0u) {  // wave 0 waits for the solver's word (one request per look), then fetches the slot
                    // (the solver needs ~9 us from the last row to its word: a first long nap, then a look every ~0.5 us)
                    const unsigned *my_gen = &la.ctl->g[blockIdx.x & (unsigned) (kLateGenCopies - 1)].gen;
                    const unsigned long long t0 = wall_clock64();
                    bool ok = true;
                    __builtin_amdgcn_s_sleep(100);
                    for (;;) {
                        const unsigned g = ld_agent_u32(my_gen);
                        if (g == ~0u || wall_clock64() - t0 > kLateGuardTicks) {
                            ok = false;
                            break;
                        }
                        if ((int) (g - li) >= 0) break;
                        __builtin_amdgcn_s_sleep(20);
                    }
                    if (lane < 16u)
                        s_bc[lane] = __uint_as_float(ld_agent_u32(reinterpret_cast<const unsigned *>(&la.ctl->bc[li & 1u][lane])));
                    if (lane == 16u) s_bc[16] = ok ? 0.f : 1.f;
                    if (!ok && lane == 0u) __hip_atomic_store(&la.ctl->abandoned, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else if (threadIdx.x < 17u) {
                s_bc[threadIdx.x] = threadIdx.x < 12u ? st->Tf[threadIdx.x] : (threadIdx.x == 12u ? st->step_disp : 0.f);
            }
            __syncthreads();
            if (s_bc[16] != 0.f || __float_as_uint(s_bc[13]) != 0u) return;  // (uniform: gave up, or told to leave)
        }
        late_wstamp<LATE>(la.dbg_w, la.dbg_li, li, 0);  // pose in
        // (one launch per iteration: the pose is read where it is used, as before; resident: from this iteration's slot)
        float Tl_loc[12];
        if constexpr (LATE) {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                Tl_loc[k] = __uint_as_float((unsigned) __builtin_amdgcn_readfirstlane((int) __float_as_uint(s_bc[k])));
        }
        const float *Tl = LATE ? Tl_loc : S.Tf;
        const float step_now = LATE ? __uint_as_float((unsigned) __builtin_amdgcn_readfirstlane((int) __float_as_uint(s_bc[12])))
                                    : S.step_disp;
        const bool valid = (LATE && li > 0u) || (bounds_valid != 0 && have_prev);
        // room a search leaves above its result for the runner-up bound: a few of the last step's sizes
        // (what the following steps will add up to while the registration converges)
        const float pad_room = have_prev ? pad_mul * step_now : 0.f;
        double rowacc = 0.0;
        unsigned n_uns = 0;    // (wave-uniform)
        // ---- phase 1: the certificate
        {
            double acc[kAcc];
#pragma unroll
            for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
            bool any = false;
            if (stamp_on) {  // (when the first batch's three loads have landed)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                pt[2] = clock64();
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const unsigned i = base + (unsigned) j * 64u + lane;
                const bool act = i < n;
                bool settled = false, owned = act;
                float qx = 0.f, qy = 0.f, qz = 0.f, d2 = 0.f;
                if (act) {
                    xform_pcl(Tl, p[j].x, p[j].y, p[j].z, qx, qy, qz);
                    if (slab_on && !(qx >= slab_lo && qx < slab_hi)) owned = false;
                }
                if (owned && valid) {
                    // where the query is now, how far that is from where its bound was taken, and how far
                    // its match is: no stores -- a settled query costs three stream reads
                    const float ex = qx - rf[j].x, ey = qy - rf[j].y, ez = qz - rf[j].z;
                    // (v_sqrt_f32, 1 ulp: the comparison carries 1e-4 relative + 1e-6 m of cushion on either side;
                    // the library sqrtf is a twenty-instruction sequence, and this phase is bound by issue)
                    const float disp = __builtin_amdgcn_sqrtf(ex * ex + ey * ey + ez * ez);
                    const unsigned idx = __float_as_uint(mp[j].w);
                    d2 = canon_d2(qx, qy, qz, mp[j]);
                    settled = idx != kNoIdx && d2 <= thr_d2 &&
                              __builtin_amdgcn_sqrtf(d2) * 1.0001f + 1e-6f < rf[j].w - disp * 1.0001f - 1e-6f;
                }
                if constexpr (STATS >= 0) {
                    // the settled queries' terms: two batches are added lane by lane, then one wave reduction
                    // (all four at once needs 36 more live registers than the kernel has: 92 B of scratch per lane)
                    if ((j & 1) == 0) any = false;
                    any = any || settled;
                    if constexpr (STATS == WM_ICP_SVD) {
                        // (the first batch of a pair assigns, the second accumulates with fused multiply-adds:
                        // half the f64 instructions of forming the terms and adding them)
                        const double m = settled ? 1.0 : 0.0;
                        const double px = settled ? (double) qx : 0.0, py = settled ? (double) qy : 0.0,
                                     pz = settled ? (double) qz : 0.0;
                        const double tx = settled ? (double) mp[j].x : 0.0, ty = settled ? (double) mp[j].y : 0.0,
                                     tz = settled ? (double) mp[j].z : 0.0;
                        const double dd = settled ? (double) d2 : 0.0;
                        // (k_icp_stats' order: 1, p, t, t p^T row by row, d2, 1)
                        const double t[kAcc] = {m, px, py, pz, tx, ty, tz, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, dd, m};
                        const double u[3] = {tx, ty, tz}, v[3] = {px, py, pz};
#pragma unroll
                        for (int k = 0; k < kAcc; ++k) {
                            if (k < 7 || k > 15) acc[k] = (j & 1) == 0 ? t[k] : acc[k] + t[k];
                            else if ((j & 1) == 0) acc[k] = u[(k - 7) / 3] * v[(k - 7) % 3];
                            else acc[k] = fma(u[(k - 7) / 3], v[(k - 7) % 3], acc[k]);
                        }
                    } else {
                        double a[kAcc];
                        icp_terms<STATS>(a, settled, settled, qx, qy, qz, mp[j].x, mp[j].y, mp[j].z, d2);
#pragma unroll
                        for (int k = 0; k < kAcc; ++k) acc[k] = ((j & 1) == 0 ? 0.0 : acc[k]) + a[k];
                    }
                    if ((j & 1) == 1 || j == NB - 1) {
                        if (__ballot(any) != 0ull) {
                            acc_halve<kAcc, 32>(acc, lane);
                            rowacc += comp >= 0 ? acc[0] : 0.0;
                        }
                    }
                }
                const bool uns = owned && !settled;
                const unsigned long long umask = __ballot(uns);
                if (uns) {
                    const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned) (umask >> 32),
                                                                      __builtin_amdgcn_mbcnt_lo((unsigned) umask, 0u));
                    const unsigned e = n_uns + before;
                    s_list[wave][e] = (unsigned short) ((unsigned) j * 64u + lane);
                    // the wave's first 64 are parked (pose applied, match) where its pooled walk will keep
                    // its list: phase 2 starts without another round trip to memory
                    if (valid && e < 64u) {
                        float4 *park = reinterpret_cast<float4 *>(L.items);
                        park[2u * e] = make_float4(qx, qy, qz, 0.f);
                        park[2u * e + 1u] = mp[j];
                    }
                }
                n_uns += (unsigned) __popcll(umask);
            }
        }
        if (lane == 0) s_cnt[wave] = n_uns;
        if (stamp_on) pt[3] = clock64();  // phase 1 done
        __syncthreads();
        if constexpr (!LATE) {
            if (S.done) return;  // (a launch queued behind a `done`: nothing stored, nothing added -- see the top)
        }
        late_wstamp<LATE>(la.dbg_w, la.dbg_li, li, 1);  // phase 1 done (all waves)
        // ---- phase 2: what is left in the workgroup, 64 queries at a time, chunk c by wave c mod 4
        unsigned cum[kCertWaves + 1];
        cum[0] = 0;
#pragma unroll
        for (int w = 0; w < kCertWaves; ++w) cum[w + 1] = cum[w] + s_cnt[w];
        const unsigned U = cum[kCertWaves];
        if (uns_count && threadIdx.x == 0 && U) atomicAdd(&uns_count[blockIdx.x & 63u], U);  // developer statistics
        // how many queries this launch had to search: the solve kernel hands it to the host (one atomic per
        // workgroup, spread over 64 words)
        // (with bins the count is one of their components)
        if (!LATE && !bins && threadIdx.x == 0 && U) atomicAdd(&st->cert_unsettled[blockIdx.x & 63u], U);
        const unsigned nchunks = (U + 63u) / 64u;
        unsigned cost = 0;
        unsigned long long prof[3] = {0ull, 0ull, 0ull};
        // The wave's first chunk is gathered from the four waves' parked entries BEFORE any wave scans (a
        // scan overwrites its wave's parking area), and set down again in the wave's own area after the
        // barrier: query (pose applied), its index, its match.
        {
            float gx = 0.f, gy = 0.f, gz = 0.f;
            float4 gtp = make_float4(0.f, 0.f, 0.f, __uint_as_float(kNoIdx));
            unsigned gi = kNoIdx;
            const unsigned e = wave * 64u + lane;
            if (wave < nchunks && e < U) {
                unsigned w, k;
                chunk_query(e, cum, w, k);
                gi = gbase + w * (64u * NB) + (unsigned) s_list[w][k];
                if (valid && k < 64u) {
                    const float4 *park = reinterpret_cast<const float4 *>(s_L[w].items);
                    const float4 a = park[2u * k];
                    gtp = park[2u * k + 1u];
                    gx = a.x;
                    gy = a.y;
                    gz = a.z;
                } else {
                    const float4 p1 = src[gi];
                    if (have_prev) gtp = match_pt[gi];
                    xform_pcl(Tl, p1.x, p1.y, p1.z, gx, gy, gz);
                }
            }
            __syncthreads();
            float4 *own = reinterpret_cast<float4 *>(L.items);
            own[2u * lane] = make_float4(gx, gy, gz, __uint_as_float(gi));
            own[2u * lane + 1u] = gtp;
        }
        for (unsigned c = wave; c < nchunks; c += kCertWaves) {
            bool mine;
            unsigned i;
            float qx = 0.f, qy = 0.f, qz = 0.f, r = 0.f, pad = 0.f;
            float bqx = 0.f, bqy = 0.f, bqz = 0.f;
            float4 tp = make_float4(0.f, 0.f, 0.f, __uint_as_float(kNoIdx));
            bool from_mem = false;
            if (c == wave) {
                const float4 *own = reinterpret_cast<const float4 *>(L.items);
                const float4 a = own[2u * lane];
                tp = own[2u * lane + 1u];
                i = __float_as_uint(a.w);
                mine = i != kNoIdx;
                qx = a.x;
                qy = a.y;
                qz = a.z;
                __builtin_amdgcn_wave_barrier();  // (read before the walk reuses this LDS)
            } else {
                const unsigned e = c * 64u + lane;
                mine = e < U;
                i = 0;
                if (mine) {
                    unsigned w, k;
                    chunk_query(e, cum, w, k);
                    i = gbase + w * (64u * NB) + (unsigned) s_list[w][k];
                }
                from_mem = mine;
            }
            unsigned long long best = make_key(thr_d2, kNoIdx);
            unsigned long long seeded = best;
            bool heavy = false;
            if (from_mem) {
                const float4 p1 = src[i];
                if (have_prev) tp = match_pt[i];
                xform_pcl(Tl, p1.x, p1.y, p1.z, qx, qy, qz);
            }
            if (mine) {
                r = r0_cells * h0;
                if (have_prev) {
                    const unsigned pidx = __float_as_uint(tp.w);
                    r = rmax;
                    if (pidx != kNoIdx) {
                        const float d2b = canon_d2(qx, qy, qz, tp);
                        if (d2b <= thr_d2) {
                            best = seeded = make_key(d2b, pidx);
                            bqx = tp.x;
                            bqy = tp.y;
                            bqz = tp.z;
                            // (v_sqrt_f32, 1 ulp: the cushion of 1e-4 relative + 1e-6 m below covers it, as in phase 1;
                            // the pad is whatever it comes to here: the radius and the bound use the same one)
                            const float sd = __builtin_amdgcn_sqrtf(d2b);
                            pad = fminf(pad_room, pad_frac * sd);
                            r = fmaxf(sd * 1.0001f + 1e-6f, 0.05f * h0) + pad;
                        }
                    }
                }
                r = fminf(r, rmax);
                heavy = r > r_light;
            }
            if (c == wave && stamp_on) pt[4] = clock64();  // first chunk: seeds ready
            Bound bnd;
            bnd.second = 0x7F800000u;
            bnd.pad = pad;
            bnd.lds = s_second[wave];
            bnd.win = s_win[wave];
            bnd.ok = true;
            float margin_last = 0.f;
            L.q[lane] = make_float4(qx, qy, qz, 0.f);
            L.seeded[lane] = seeded;
            L.bq[0][lane] = bqx;
            L.bq[1][lane] = bqy;
            L.bq[2][lane] = bqz;
            asm volatile("" ::: "memory");
            bool live = mine && !heavy;
            for (int pass = 0; pass < 32 && __ballot(live) != 0ull; ++pass) {
                const int l = nn_level_for(hl, Ln, lane_lf, r);
                const unsigned long long lv_mask = __ballot(live);
                const int l0 = __builtin_amdgcn_readlane(l, __ffsll((long long) lv_mask) - 1);
                float margin;
                if (__ballot(live && l != l0) == 0ull) {
                    const GridDev g = l0 == 0 ? g0 : lvp->g[l0];
                    if (!scan_box_rows(g, live, qx, qy, qz, r, best, &margin, L, lane, &bnd))
                        best = scan_box_bal<false, RC, true>(g, live, qx, qy, qz, r, best, &margin, L, lane, have_prev,
                                                              g.pts, cost, prof, &bnd);
                } else {
                    const GridDev g = lvp->g[l];
                    L.base[lane] = (unsigned long long) g.pts;
                    best = scan_box_bal<false, RC, true>(g, live, qx, qy, qz, r, best, &margin, L, lane, have_prev,
                                                          nullptr, cost, prof, &bnd);
                }
                if (live) {
                    const float bd2 = __uint_as_float((unsigned) (best >> 32));
                    margin_last = margin;
                    if (nn_certified(margin, bd2, thr_d2)) {
                        live = false;
                    } else {
                        r = nn_grow_radius(best, bd2, r, rmax, pad);
                        heavy = r > r_light;
                        live = !heavy;
                    }
                }
            }
            if (c == wave && stamp_on) pt[5] = clock64();  // first chunk: pass loop done
            // cooperative phase for radii beyond r_light (k_nn_grid's), with the runner-up tracked as well: the
            // ball scanned is the query's whole search ball, so the bound is min(runner-up, margin of the last box)
            unsigned long long todo = __ballot(heavy);
            float seed = 0.f;
            while (todo) {
                const int sl = __ffsll((long long) todo) - 1;
                todo &= todo - 1;
                const float ux = rl_f(qx, sl), uy = rl_f(qy, sl), uz = rl_f(qz, sl);
                float ur = rl_f(r, sl);
                unsigned long long ub = ((unsigned long long) rl_u((unsigned) (best >> 32), sl) << 32) |
                                        rl_u((unsigned) best, sl);
                unsigned usec = 0x7F800000u;
                float umargin = 0.f;
                const float upad = rl_f(pad, sl);
                if ((unsigned) ub == kNoIdx && seed > ur) ur = fminf(seed, rmax);
                for (int pass = 0; pass < 64; ++pass) {
                    const int l = nn_level_for(hl, Ln, coop_lf, ur);
                    const GridDev g = lvp->g[l];
                    float margin;
                    ub = coop_scan_box(g, ux, uy, uz, ur, ub, lane, &margin, &usec, upad);
                    umargin = margin;
                    const float bd2 = __uint_as_float((unsigned) (ub >> 32));
                    if (nn_certified(margin, bd2, thr_d2)) break;
                    if (ur >= rmax) break;
                    ur = nn_grow_radius(ub, bd2, ur, rmax);
                }
                seed = ((unsigned) ub != kNoIdx) ? 1.25f * sqrtf(__uint_as_float((unsigned) (ub >> 32))) : ur;
                if ((int) lane == sl) {
                    best = ub;
                    // (a scan cuts its rows to the chord of ball(q, best at its entry + pad): what it skipped is
                    // farther than that, hence farther than the final best + pad)
                    bnd.second = usec;
                    margin_last = umargin;
                    heavy = false;
                }
            }
            asm volatile("" ::: "memory");
            seeded = L.seeded[lane];
            bqx = L.bq[0][lane];
            bqy = L.bq[1][lane];
            bqz = L.bq[2][lane];
            if (c == wave && stamp_on) pt[6] = clock64();  // first chunk: cooperative phase done
            if (mine) {
                st_u64(&keys[i], best);
                if (best != seeded && (unsigned) best != kNoIdx) {
                    // the new match's coordinates: left in LDS by the lane that found it (the tag says whether
                    // the slot really is this point's), else from the caller-ordered target copy
                    const float4 w = s_win[wave][lane];
                    if (__float_as_uint(w.w) == (unsigned) best) {
                        bqx = w.x;
                        bqy = w.y;
                        bqz = w.z;
                    } else {
                        const f4v cc = ((gp_f4) tgt_orig)[(unsigned) best];
                        bqx = cc.x;
                        bqy = cc.y;
                        bqz = cc.z;
                    }
                }
                st_f4(&match_pt[i], bqx, bqy, bqz, __uint_as_float((unsigned) best));
                // every point but the match is farther than: the runner-up seen, the radius pruned with, and
                // the faces of the last box scanned
                float s = 0.f;
                if (bnd.ok && !heavy && (unsigned) best != kNoIdx && margin_last > 0.f) {
                    const float bd = sqrtf(__uint_as_float((unsigned) (best >> 32)));
                    s = fminf(fminf(sqrtf(__uint_as_float(bnd.second)), bd + pad), margin_last) * 0.9999f - 1e-6f;
                }
                st_f4(&bound[i], qx, qy, qz, s);  // ... seen from HERE
            }
            if (c == wave && stamp_on) pt[7] = clock64();  // first chunk: winners fetched, results stored
            if constexpr (STATS >= 0) {
                double a[kAcc];
                icp_terms<STATS>(a, mine, (unsigned) best != kNoIdx, qx, qy, qz, bqx, bqy, bqz,
                                 __uint_as_float((unsigned) (best >> 32)),
                                 (unsigned) best != (unsigned) seeded && (i & changed_mask) == 0u);
                acc_halve<kAcc, 32>(a, lane);
                rowacc += comp >= 0 ? a[0] : 0.0;
            }
            if (c == wave && stamp_on) pt[8] = clock64();  // first chunk: sums reduced
            __builtin_amdgcn_wave_barrier();
        }
        if (stamp_on) pt[10] = clock64();
        if constexpr (LATE) {
            late_wstamp<LATE>(la.dbg_w, la.dbg_li, li, 2);  // wave 0's searches done
            // the four waves' sums in wave order -> the workgroup's row, written through; when the stores have
            // been performed, the ticket.  (Every wave first waits for its own result stores: the next
            // iteration's loads of the match and the bound, by other waves, come behind the barrier.)
            if (comp >= 0) s_rows[wave][comp] = rowacc;
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            late_wstamp<LATE>(la.dbg_w, la.dbg_li, li, 3);  // all waves' searches done, result stores performed
            if (threadIdx.x == 0 && la.dbg_w && li == la.dbg_li) la.dbg_w[(size_t) blockIdx.x * 8u + 6u] = U;
            if (threadIdx.x < (unsigned) kAcc + 1u) {
                const double t = threadIdx.x < (unsigned) kAcc ? add_wave_rows(s_rows, threadIdx.x) : (double) U;
                __hip_atomic_store(partials + (size_t) row * kLateRow + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            late_wstamp<LATE>(la.dbg_w, la.dbg_li, li, 4);  // row stored
            if (threadIdx.x == 0) (void) __hip_atomic_fetch_add(&la.ctl->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            late_wstamp<LATE>(la.dbg_w, la.dbg_li, li, 5);  // ticket drawn
        } else if constexpr (STATS >= 0) {
            // the four waves' sums, added in wave order
            if (comp >= 0) s_rows[wave][comp] = rowacc;
            __syncthreads();
            if (bins) {
                if (threadIdx.x < (unsigned) kAcc) {
                    bins_add(bins, row % (unsigned) kBinCount, threadIdx.x, add_wave_rows(s_rows, threadIdx.x));
                } else if (threadIdx.x == (unsigned) kAcc && U) {
                    bins_add_count(bins, row % (unsigned) kBinCount, (unsigned) kAcc, (long long) U);
                }
            } else if (threadIdx.x < (unsigned) kAcc) {
                st_f64(&partials[(size_t) row * kAcc + threadIdx.x], add_wave_rows(s_rows, threadIdx.x));
            }
        }
        if (stamp_on && lane == 0) {
            pt[11] = clock64();
            unsigned long long *o = prof_out + 16 * (blockIdx.x >> 8);
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = pt[k];
            o[12] = U;
        }
        if constexpr (!LATE) break;
    }  // (iterations)
}

// After a registration whose last searches were certified: the settled queries' keys still carry the
// distance of their last real search.  Bring every key up to date with the pose of the last search
// (same arithmetic as the search: same bits as if every query had been searched).
__global__ void __launch_bounds__(kBlock)
    k_fix_keys(const float4 *__restrict__ src, unsigned n, const IcpDevState *__restrict__ st, float thr_d2,
               const float4 *__restrict__ match_pt, unsigned long long *__restrict__ keys) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = src[i], m = match_pt[i];
    const unsigned idx = __float_as_uint(m.w);
    float qx, qy, qz;
    xform_pcl(st->Tf_search, p.x, p.y, p.z, qx, qy, qz);
    keys[i] = idx == kNoIdx ? make_key(thr_d2, kNoIdx) : make_key(canon_d2(qx, qy, qz, m), idx);
}

int launch_fix_keys(wm_ctx *ctx, float thr_d2) {
    const unsigned n = (unsigned) ctx->n_src;
    if (n == 0) return WM_OK;
    hipLaunchKernelGGL(k_fix_keys, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream,
                       ctx->src_sorted.as<float4>(), n, ctx->d_state.as<IcpDevState>(), thr_d2,
                       ctx->match_pt.as<float4>(), ctx->keys.as<unsigned long long>());
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

constexpr int kCertNB = 4;  // batches of 64 queries per workgroup of k_nn_cert
constexpr int kLateNB = 4;  // ... and of its resident form
// the one launch of k_nn_cert<STATS, NB, 3, LATE>: the launched form (la empty; developer counters, bins) and the
// resident form (la filled in; neither)
template <int STATS, int NB, bool LATE>
static void launch_cert_kernel(wm_ctx *ctx, unsigned blocks, float thr_d2, bool bounds_valid, const LateArgs &la,
                               long long *bins) {
    const bool log = !LATE && ctx->cert_log_iter < ctx->cert_log_cap;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nn_cert<STATS, NB, 3, LATE>), dim3(blocks), dim3(64 * kCertWaves), 0, ctx->stream,
                       ctx->levels_dev, ctx->d_levels.as<LevelsDev>(), ctx->src_sorted.as<float4>(), (unsigned) ctx->n_src,
                       ctx->d_state.as<IcpDevState>(), thr_d2, ctx->keys.as<unsigned long long>(),
                       ctx->match_pt.as<float4>(), ctx->nn_bound.as<float4>(), ctx->tgt_orig.as<float4>(),
                       ctx->tune_r_light, ctx->tune_lane_lf, ctx->tune_coop_lf, ctx->tune_r0,
                       ctx->partials.as<double>(), bounds_valid ? 1 : 0, ctx->tune_cert_pad_mul,
                       ctx->tune_cert_pad_frac,
                       log && ctx->cert_count.p ? ctx->cert_count.as<unsigned>() + 64 * (size_t) ctx->cert_log_iter : nullptr,
                       log && ctx->cert_prof.p ? ctx->cert_prof.as<unsigned long long>() + 64 * (size_t) ctx->cert_log_iter
                                               : nullptr,
                       la, bins, sqrtf(thr_d2) * 1.0001f + 1e-6f);
}

// use_bins (with a stats_mode): sums and the searched-queries count go into the iteration's bins (wm_bins.hpp) --
// *rows_out is 0 then, and the solve is launch_bins_solve
int launch_nn_cert(wm_ctx *ctx, float thr_d2, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2, int stats_mode,
                   unsigned *rows_out, bool bounds_valid, bool use_bins) {
    const unsigned n = (unsigned) ctx->n_src;
    if (rows_out) *rows_out = 0;
    if (n == 0) return WM_OK;
    const unsigned per = 64u * (unsigned) kCertNB * (unsigned) kCertWaves;
    unsigned blocks = (n + per - 1u) / per;
    blocks = (blocks + 7u) & ~7u;  // xcd_remap needs a multiple of 8
    WM_HIP(ctx, ctx->nn_bound.reserve(((size_t) n + 64) * sizeof(float4)));
    long long *bins = nullptr;
    const int rc = nn_sums_target(ctx, stats_mode, use_bins, blocks, &bins, rows_out);
    if (rc != WM_OK) return rc;
    if (ev0) WM_HIP(ctx, hipEventRecord(ev0, ctx->stream));
    if (stats_mode < 0) launch_cert_kernel<-1, kCertNB, false>(ctx, blocks, thr_d2, bounds_valid, LateArgs{}, nullptr);
    else if (stats_mode == WM_ICP_SVD) launch_cert_kernel<WM_ICP_SVD, kCertNB, false>(ctx, blocks, thr_d2, bounds_valid, LateArgs{}, bins);
    else launch_cert_kernel<WM_ICP_GN6, kCertNB, false>(ctx, blocks, thr_d2, bounds_valid, LateArgs{}, bins);
    if (ctx->cert_count.p && ctx->cert_log_iter < ctx->cert_log_cap) ctx->cert_log_iter++;
    if (ev1) WM_HIP(ctx, hipEventRecord(ev1, ctx->stream));
    if (ev2) WM_HIP(ctx, hipEventRecord(ev2, ctx->stream));
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// ---- the resident form (k_nn_cert<.., LATE = true>)
template <int STATS>
static const void *late_kernel() {
    return (const void *) k_nn_cert<STATS, kLateNB, 3, true>;
}

// workgroups of resident kernels (this one, GICP's evaluators) a device may hold at once, per process:
// resident kernels that each hold part of the GPU while waiting must never keep each other's remaining
// workgroups from starting
// (in 1/1024ths of the device: a kernel of nb workgroups of which `capacity` fit at once takes
// ceil(1024 nb / capacity) -- the kernels differ in what a workgroup occupies)
static std::atomic<int> g_resident[64];
int resident_admit(int device, int nb, int capacity) {
    if (device < 0 || device >= 64 || capacity <= 0 || nb > capacity) return 0;
    const int share = (int) (((long long) nb * 1024 + capacity - 1) / capacity);
    int cur = g_resident[device].load();
    while (cur + share <= 1024)
        if (g_resident[device].compare_exchange_weak(cur, cur + share)) return share;
    return 0;
}
void resident_release(int device, int share) {
    if (device >= 0 && device < 64 && share > 0) g_resident[device].fetch_sub(share);
}

size_t late_ctl_bytes() { return sizeof(LateCtl); }

// Can the late iterations of this align run in one resident launch?  (*blocks_out: its grid)
bool late_possible(wm_ctx *ctx, int stats_mode, unsigned *blocks_out) {
    const unsigned n = (unsigned) ctx->n_src;
    if (n == 0 || (stats_mode != WM_ICP_SVD && stats_mode != WM_ICP_GN6)) return false;
    if (ctx->late_capacity == 0) {  // first use: how many of its workgroups fit on the device at once?
        ctx->late_capacity = -1;
        int cus = 0, per_cu = 0, per_cu2 = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) return false;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, late_kernel<WM_ICP_SVD>(), 64 * kCertWaves, 0) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu2, late_kernel<WM_ICP_GN6>(), 64 * kCertWaves, 0) != hipSuccess) {
            (void) hipGetLastError();
            return false;
        }
        ctx->late_capacity = cus * (per_cu < per_cu2 ? per_cu : per_cu2);
    }
    if (ctx->late_capacity <= 0) return false;
    const unsigned per = 64u * (unsigned) kLateNB * (unsigned) kCertWaves;
    unsigned workers = (n + per - 1u) / per;
    workers = (workers + 7u) & ~7u;  // xcd_remap needs a multiple of 8
    if ((int) workers + 1 > ctx->late_capacity) return false;  // (+ 1: the solver's workgroup)
    if (blocks_out) *blocks_out = workers;
    return true;
}

// Enqueue the resident kernel: iterations from the state's current one until done / the policy says leave
// / max_inside.  The caller holds `blocks` of the device's resident budget until the kernel has finished.
int launch_nn_late(wm_ctx *ctx, float thr_d2, int stats_mode, unsigned blocks, bool bounds_valid, unsigned exit_seq,
                   float stop_unsettled, float stop_disp, int max_inside) {
    const unsigned n = (unsigned) ctx->n_src;
    const unsigned workers = blocks;
    if (!ctx->side_stream || !ctx->ev_fork || !ctx->ev_join) return WM_ERR_STATE;
    WM_HIP(ctx, ctx->nn_bound.reserve(((size_t) n + 64) * sizeof(float4)));
    WM_HIP(ctx, ctx->partials.reserve((size_t) workers * kLateRow * sizeof(double)));
    WM_HIP(ctx, ctx->late_ctl.reserve(sizeof(LateCtl) + 64 * 4 * sizeof(unsigned long long)));
    if (!ctx->h_late) {
        WM_HIP(ctx, hipHostMalloc((void **) &ctx->h_late, 64, hipHostMallocDefault));
        *ctx->h_late = 0ull;
    }
    WM_HIP(ctx, hipMemsetAsync(ctx->late_ctl.p, 0, sizeof(LateCtl) + 64 * 4 * sizeof(unsigned long long), ctx->stream));
    LateArgs la;
    la.ctl = ctx->late_ctl.as<LateCtl>();
    la.pub = ctx->h_pub;
    la.pub_slots = ctx->h_pub_slots;
    la.h_exit = ctx->h_late;
    la.exit_seq = exit_seq;
    la.stop_unsettled = stop_unsettled;
    la.stop_disp = stop_disp;
    la.max_inside = max_inside;
    la.dbg = ctx->late_debug_iter >= 0 ? (unsigned long long *) ((char *) ctx->late_ctl.p + sizeof(LateCtl)) : nullptr;
    la.dbg_w = nullptr;
    la.dbg_li = 0;
    if (la.dbg) {
        WM_HIP(ctx, ctx->cert_prof.reserve((size_t) workers * 8 * sizeof(unsigned long long)));
        WM_HIP(ctx, hipMemsetAsync(ctx->cert_prof.p, 0, (size_t) workers * 8 * sizeof(unsigned long long), ctx->stream));
        la.dbg_w = ctx->cert_prof.as<unsigned long long>();
        la.dbg_li = (unsigned) ctx->late_debug_iter;
    }
    // the solver beside the workers, on the second stream: both start when what is on the main stream now is done
    WM_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    WM_HIP(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    hipLaunchKernelGGL(k_late_solver, dim3(1), dim3(64 * kCertWaves), 0, ctx->side_stream, ctx->partials.as<double>(),
                       workers, ctx->d_state.as<IcpDevState>(), la);
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->side_stream));
    if (stats_mode == WM_ICP_SVD) launch_cert_kernel<WM_ICP_SVD, kLateNB, true>(ctx, blocks, thr_d2, bounds_valid, la, nullptr);
    else launch_cert_kernel<WM_ICP_GN6, kLateNB, true>(ctx, blocks, thr_d2, bounds_valid, la, nullptr);
    WM_HIP(ctx, hipGetLastError());
    // (what follows on the main stream needs the state the solver writes back when it leaves)
    WM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    return WM_OK;
}

}  // namespace wm
