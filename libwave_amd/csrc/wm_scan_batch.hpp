// wm_scan_batch.hpp -- the front of a call over a queue of scans: what wm_cluster_extract_batch and
// wm_outlier_filter_batch do before their own kernels run.  The scans' points stand one after the other ("batch
// positions", scan-major), each scan has a lattice of its own whose cells are numbered scan after scan, so one count,
// one exclusive scan and one scatter give ONE cell-sorted array, scan-major again ("grid positions").  A scan's GridDev
// points at its own slice of cell_start and at the shared array, so a walk never meets a point of another scan.
//
// On the context's stream: wm_scan_table.hpp's first half (the table's first half and the host clouds up, k_cluster_pack:
// the packed cloud, per scan the box and the finite count) and their fetch; on the host per scan the finite count, the caller's
// say on it (how many of its points are searched), the box and the cell; then k_cluster_count over the lattices, the
// occupancies' fetch and at most one recount, the exclusive scan and k_cluster_scatter.  Two host waits, whatever the
// number of scans.
//
// Included by the units that run a batch (each gets kernels of its own: the names are the cluster extraction's, where
// they were written).  The buffers (ScanBatchBufs) belong to the caller's workspace: two callers share nothing.
#pragma once
#include <string.h>

#include "wm_scan_table.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace wm {

namespace {

__device__ __forceinline__ unsigned cl_by_grid(const ClScan *tab, unsigned S, unsigned x) {
    return cl_find(tab, S, x, [](const ClScan &s) { return s.g0; });
}
__device__ __forceinline__ unsigned cl_by_search(const ClScan *tab, unsigned S, unsigned b) {
    return cl_find(tab, S, b, [](const ClScan &s) { return s.lblk0; });
}

__device__ __forceinline__ unsigned cl_cell(const GridDev &g, const float4 &p) {  // (wm_grid.hip: LinearKey)
    int cx = (int) floorf((p.x - g.ox) * g.inv_h);
    int cy = (int) floorf((p.y - g.oy) * g.inv_h);
    int cz = (int) floorf((p.z - g.oz) * g.inv_h);
    cx = min(max(cx, 0), g.nx - 1);
    cy = min(max(cy, 0), g.ny - 1);
    cz = min(max(cz, 0), g.nz - 1);
    return (unsigned) ((cz * g.ny + cy) * g.nx + cx);
}

// k_count of wm_grid.hip with the scan's lattice and its first cell; the lane that finds a cell empty counts it as
// occupied (occ[k]: what build_call_grid's occupancy check fetches, here for every scan at once)
__global__ void __launch_bounds__(kBlock)
    k_cluster_count(const ClScan *__restrict__ tab, unsigned S, const float4 *__restrict__ pts, unsigned *__restrict__ cell_of,
                    unsigned *__restrict__ rank_of, unsigned *counts, unsigned *occ) {
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    unsigned first = 0u;
    if (i < me.n) {
        const float4 p = pts[me.off + i];
        unsigned c = kNoIdx, r = 0u;
        if (p.x == p.x) {
            c = cl_cell(me.g, p);
            r = atomicAdd(&counts[me.cell0 + c], 1u);
            first = r == 0u ? 1u : 0u;
        }
        cell_of[me.off + i] = c;
        rank_of[me.off + i] = r;
    }
    for (int off = 32; off > 0; off >>= 1) first += __shfl_down(first, off);
    if ((threadIdx.x & 63) == 0 && first) atomicAdd(&occ[k], first);
}

// k_scatter of wm_grid.hip: the batch's cell-sorted array and the four NaN entries behind its last point
__global__ void __launch_bounds__(kBlock)
    k_cluster_scatter(const ClScan *__restrict__ tab, unsigned S, const float4 *__restrict__ pts,
                      const unsigned *__restrict__ cell_of, const unsigned *__restrict__ rank_of,
                      const unsigned *__restrict__ cell_start, float4 *__restrict__ out, size_t ncells) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned end = cell_start[ncells];
        const float nanv = __builtin_nanf("");
#pragma unroll
        for (int u = 0; u < 4; ++u) out[end + u] = make_float4(nanv, nanv, nanv, __uint_as_float(kNoIdx));
    }
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    if (i >= me.n) return;
    const unsigned c = cell_of[me.off + i];
    if (c == kNoIdx) return;
    out[cell_start[me.cell0 + c] + rank_of[me.off + i]] = pts[me.off + i];
}

// ------------------------------------------------------------------ a batch's lattices (host)
uint64_t cl_cells_of(const Bbox &bb, float h) {  // (wm_grid.hip: build_grid_level's lattice)
    uint64_t c = 1;
    for (int d = 0; d < 3; ++d) c *= (uint64_t) floor(((double) bb.hi[d] - bb.lo[d]) / h) + 1;
    return c;
}

// build_call_grid's automatic cell of a scan (occ == 0) or its second choice from the measured occupancy, under the
// scan's share of the batch's cells
float cl_cell_size(const Bbox &bb, size_t n_finite, float floor_h, uint64_t cell_cap, float h_prev, double occ) {
    float h;
    if (occ > 0) {
        h = fmaxf((float) (h_prev * sqrt(3.0 / occ)), floor_h);
    } else {
        double vol = 1;
        for (int d = 0; d < 3; ++d) vol *= fmax((double) bb.hi[d] - bb.lo[d], 1e-3);
        h = fmaxf((float) fmax(cbrt(vol / (double) n_finite) * 1.5, 1e-4), floor_h);
    }
    while (cl_cells_of(bb, h) > cell_cap) h *= 1.26f;
    return h;
}

void cl_lattice(const Bbox &bb, float h, GridDev *g) {  // (wm_grid.hip: build_grid_level)
    g->nx = (int) floor((bb.hi[0] - bb.lo[0]) / h) + 1;
    g->ny = (int) floor((bb.hi[1] - bb.lo[1]) / h) + 1;
    g->nz = (int) floor((bb.hi[2] - bb.lo[2]) / h) + 1;
    const float extent = fmaxf(fmaxf(bb.hi[0] - bb.lo[0], bb.hi[1] - bb.lo[1]), bb.hi[2] - bb.lo[2]);
    float amax = 0;
    for (int d = 0; d < 3; ++d) amax = fmaxf(amax, fmaxf(fabsf(bb.lo[d]), fabsf(bb.hi[d])));
    const float ulp = fmaxf(amax, extent) * 1.2e-7f;
    g->ox = bb.lo[0];
    g->oy = bb.lo[1];
    g->oz = bb.lo[2];
    g->h = h;
    g->inv_h = 1.0f / h;
    g->slack = fmaxf(1e-3f, 8.0f * ulp / h);
}

float cl_from_orderable(unsigned u) {
    const unsigned b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// The buffers a front works in; a workspace owns one.  `pts` and `grid` serve the workspace's single call too (the
// packed cloud, build_call_grid's level).
struct ScanBatchBufs {
    DevBuf pts;                  // the packed clouds, batch positions
    DevBuf bb, cell_of, counts;  // a batch's boxes and occupancies, and its counting sort
    GridLevel grid;              // pts: the cell-sorted array; cell_start: the lattices one after the other
    PairStage stage;             // a batch's scan table and host clouds up (wm_stage.hpp)
    PinnedBuf h_bb;              // the boxes and finite counts, then the occupancies
    void release() {
        DevBuf *bufs[] = {&pts, &bb, &cell_of, &counts, &grid.pts, &grid.cell_start};
        for (DevBuf *b : bufs) b->release();
        stage.release();
        h_bb.release();
    }
};

// What a front hands to the kernels behind it.
struct ScanBatch {
    ClScan *tab = nullptr;          // the host mirror (pinned; valid until the workspace's next batch)
    const ClScan *d_tab = nullptr;  // the device table
    unsigned S = 0;
    size_t total = 0, blocks = 0;          // batch positions and their workgroups of kBlock
    size_t nf_total = 0;                   // grid positions; 0: nothing finite, no grid was built and the table
                                           // on the device is the first half only (raw, n, off, blk0)
    size_t search_blocks = 0;              // the search workgroups of all scans
};

// The front.  `scans`: the caller's {pts, n} rows, checked by the caller (no null cloud with points, the points in
// all below 2^31).  floor_h: no cell is smaller (what bounds the rows a radius walk spans).  search_block: the threads
// of the caller's search workgroup, in which lblk0 is counted.  per_scan(k, row) is called once per scan, in order,
// with the row's n, off, nf and g0 set: it returns whether the scan's points are searched and may set row.aux0.
// ev_a is recorded behind the upload (PairStage::submit); the stream is idle on return only where nf_total == 0.
template <class Scan, class PerScan>
int scan_batch_front(wm_ctx *ctx, ScanBatchBufs &w, const Scan *scans, unsigned S, size_t stride, int mem, float floor_h,
                     unsigned search_block, PerScan per_scan, ScanBatch *out) {
    PairStage &stg = w.stage;
    hipStream_t st = ctx->stream;

    // the table's first half and the clouds; pack, the boxes and the finite counts (wm_scan_table.hpp); their fetch
    WM_HIP(ctx, w.h_bb.reserve((size_t) S * 8 * 4));
    ScanTable T;
    WM_TRY(scan_table_pack(ctx, stg, scans, S, stride, mem, w.pts, w.bb, (size_t) S * 8 * 4, &T));
    ClScan *tab = T.tab;
    const ClScan *d_tab = T.d_tab;
    const size_t total = T.total, blocks = T.blocks, table_bytes = T.table_bytes;
    unsigned *bb = w.bb.as<unsigned>(), *occ = bb + 7 * (size_t) S, *h_bb = w.h_bb.as<unsigned>();
    WM_TRY(fast_fetch(ctx, h_bb, bb, (size_t) S * 7 * 4));

    // per scan: the finite count, the box, its grid positions and search workgroups
    std::vector<Bbox> box(S);
    std::vector<float> cell(S, 0.f);
    std::vector<uint64_t> cell_cap(S, 0);
    size_t nf_total = 0, lblk = 0;
    for (unsigned k = 0; k < S; ++k) {
        ClScan &t = tab[k];
        t.nf = h_bb[6 * (size_t) S + k];
        t.g0 = (unsigned) nf_total;
        t.lblk0 = (unsigned) lblk;
        t.searched = per_scan(k, t) ? t.nf : 0u;
        nf_total += t.nf;
        lblk += (t.searched + search_block - 1) / search_block;
        if (!t.nf) continue;
        for (int d = 0; d < 3; ++d) {
            box[k].lo[d] = cl_from_orderable(h_bb[3 * (size_t) k + d]);
            box[k].hi[d] = cl_from_orderable(h_bb[3 * (size_t) S + 3 * (size_t) k + d]);
        }
        // the single call's cap is 2^26 + 8 n cells; a batch shares ONE 2^26 among its scans
        cell_cap[k] = std::min<uint64_t>(8ull * t.n + std::max<uint64_t>(((uint64_t) 1 << 26) / S, 4096), 0x7FFFFFFFull);
        cell[k] = cl_cell_size(box[k], t.nf, floor_h, cell_cap[k], 0.f, 0.0);
    }
    out->tab = tab;
    out->d_tab = d_tab;
    out->S = S;
    out->total = total;
    out->blocks = blocks;
    out->nf_total = nf_total;
    out->search_blocks = lblk;
    if (nf_total == 0) return WM_OK;

    // the lattices, cells numbered scan after scan: count, (the occupancies' fetch, at most one recount), scan, scatter
    WM_HIP(ctx, w.grid.pts.reserve((total + 4) * sizeof(float4)));
    WM_HIP(ctx, w.cell_of.reserve(2 * total * 4));
    unsigned *cell_of = w.cell_of.as<unsigned>(), *rank_of = cell_of + total;
    uint64_t ncells = 0;
    for (int attempt = 0;; ++attempt) {
        ncells = 0;
        for (unsigned k = 0; k < S; ++k) {
            ClScan &t = tab[k];
            t.cell0 = ncells;
            if (!t.nf) continue;
            cl_lattice(box[k], cell[k], &t.g);
            ncells += (uint64_t) t.g.nx * t.g.ny * t.g.nz;
        }
        // (the stream is idle here -- both fetches have been waited for -- so growing a buffer frees nothing in use)
        WM_HIP(ctx, w.grid.cell_start.reserve((ncells + 1) * 4));
        WM_HIP(ctx, w.counts.reserve(ncells * 4));
        for (unsigned k = 0; k < S; ++k) {
            tab[k].g.pts = w.grid.pts.as<float4>();
            tab[k].g.cell_start = w.grid.cell_start.as<unsigned>() + tab[k].cell0;
        }
        WM_HIP(ctx, hipMemcpyAsync(stg.up.dev.p, stg.up.host.p, table_bytes, hipMemcpyHostToDevice, st));
        WM_HIP(ctx, hipMemsetAsync(w.counts.p, 0, ncells * 4, st));
        hipLaunchKernelGGL(k_cluster_count, dim3((unsigned) blocks), dim3(kBlock), 0, st, d_tab, S,
                           (const float4 *) w.pts.as<float4>(), cell_of, rank_of, w.counts.as<unsigned>(), occ);
        WM_HIP(ctx, hipGetLastError());
        if (attempt) break;
        WM_TRY(fast_fetch(ctx, h_bb, occ, (size_t) S * 4));
        bool again = false;
        for (unsigned k = 0; k < S; ++k) {
            if (!tab[k].nf || !h_bb[k]) continue;
            const double o = (double) tab[k].nf / h_bb[k];
            if (o > 6.0 || o < 1.5) {
                const float h2 = cl_cell_size(box[k], tab[k].nf, floor_h, cell_cap[k], cell[k], o);
                again = again || h2 != cell[k];
                cell[k] = h2;
            }
        }
        if (!again) break;
    }
    WM_TRY(exclusive_scan(ctx, w.counts.as<unsigned>(), ncells, w.grid.cell_start.as<unsigned>()));
    hipLaunchKernelGGL(k_cluster_scatter, dim3((unsigned) blocks), dim3(kBlock), 0, st, d_tab, S,
                       (const float4 *) w.pts.as<float4>(), (const unsigned *) cell_of, (const unsigned *) rank_of,
                       (const unsigned *) w.grid.cell_start.as<unsigned>(), w.grid.pts.as<float4>(), (size_t) ncells);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

}  // namespace

}  // namespace wm
