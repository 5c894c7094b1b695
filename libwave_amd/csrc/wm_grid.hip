// wm_grid.hip -- building the HBM-resident spatial index that replaces PCL's FLANN
// kd-tree (pcl::Registration::initCompute -> KdTreeFLANN::setInputCloud, triggered
// by icp.align at wave_matching/src/icp.cpp:95,116,126):
//   pack (AoS stride -> float4 + index, non-finite filter)  -> bbox reduction
//   -> cell histogram -> exclusive scan -> scatter (counting sort by cell), or, on a large lattice, the same tables
//   band of rows by band of rows (counting_sort_rows; rows_apply says where)
// Target levels are sorted x-fastest so that x-adjacent cells are contiguous in
// memory; the source cloud is counting-sorted by a Morton cell code so that a
// wavefront's 64 consecutive queries stay spatially compact under any rigid T.
#include <cstring>  // before rocprim (its headers use memcpy unqualified)

#include <rocprim/rocprim.hpp>

#include "wm_internal.hpp"
#include "wm_sort.hpp"

#include <math.h>
#include <vector>
#include <string.h>

namespace wm {

// ------------------------------------------------------------------ pack
__global__ void __launch_bounds__(kBlock) k_pack(const unsigned char *in, size_t n, size_t stride,
                                                  float4 *out) {
    size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *p = reinterpret_cast<const float *>(in + i * stride);
    float x = p[0], y = p[1], z = p[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
        x = y = z = __builtin_nanf("");
    }
    out[i] = make_float4(x, y, z, __uint_as_float((unsigned) i));
}

// A HOST cloud in PINNED memory (hipHostMalloc / hipHostRegister: what a caller that cares about the upload hands over)
// can cross PCIe on a DMA engine while this thread does something else: the copy into the slot-1 staging buffer is
// started here, asynchronously, on the side stream; pack_cloud(..., slot 1, staged = true) later waits for it -- on the
// HOST, so that the caller's memory is not read after the call that was given it has returned -- and packs from there.
// false: not pinned (or no side stream): the caller takes the blocking path.
template <bool PACK>
__global__ void k_bbox(float4 *pts, size_t n, float *out, const unsigned char *raw, size_t rstride);  // (below)

bool upload_begin_async(wm_ctx *ctx, const void *pts, size_t bytes) {
    if (!ctx->side_stream || bytes == 0) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, pts) != hipSuccess) {  // (plain pageable memory is unknown to the runtime: an error, cleared here)
        (void) hipGetLastError();
        return false;
    }
    if (at.type != hipMemoryTypeHost) return false;
    DevBuf &stage = ctx->staging2;
    if (stage.cap < bytes) {  // (growing it frees the old one: nothing of ours may still read it)
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || stage.reserve(bytes) != hipSuccess) return false;
    }
    if (hipMemcpyAsync(stage.p, pts, bytes, hipMemcpyHostToDevice, ctx->side_stream) != hipSuccess) {
        (void) hipGetLastError();
        (void) hipStreamSynchronize(ctx->side_stream);
        return false;
    }
    return true;
}

int pack_cloud(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, float4 *out, int slot, bool staged,
               float *bbox_partials, unsigned *bbox_blocks) {
    if (bbox_blocks) {
        unsigned b = (unsigned) ((n + kBlock - 1) / kBlock);
        *bbox_blocks = b > (unsigned) kBboxBlocks ? (unsigned) kBboxBlocks : b;
    }
    if (n == 0) return WM_OK;
    const unsigned char *dptr = nullptr;
    if (mem == WM_MEM_HOST && staged) {
        // (upload_begin_async put the cloud on its way into the slot-1 staging buffer: wait for the copy engine)
        WM_HIP(ctx, hipStreamSynchronize(ctx->side_stream));
        dptr = ctx->staging2.as<unsigned char>();
    } else if (mem == WM_MEM_HOST) {
        // Caller memory is pageable: a blocking copy.  Slot 0 (the source, and every other caller): after the
        // stream has drained -- the staging buffer may still feed the previous cloud's k_pack.  Slot 1 (the
        // target, when the source of the same registration was uploaded just before): a staging buffer of
        // its own and NO wait -- the source's bounding box, Morton sort and gather run on the stream while
        // this cloud crosses PCIe (wm_set_target).
        DevBuf &stage = slot == 1 ? ctx->staging2 : ctx->staging;
        if (slot != 1) WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (stage.cap < n * stride) {  // (growing it frees the old one: nothing of ours may still read it)
            WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
            WM_HIP(ctx, stage.reserve(n * stride));
        }
        WM_HIP(ctx, hipMemcpy(stage.p, pts, n * stride, hipMemcpyHostToDevice));
        dptr = stage.as<unsigned char>();
    } else {
        dptr = static_cast<const unsigned char *>(pts);
    }
    unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    if (bbox_partials && bbox_blocks) {  // (the cloud's box in the same launch: k_bbox<true>)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bbox<true>), dim3(*bbox_blocks), dim3(kBlock), 0, ctx->stream, out, n, bbox_partials, dptr, stride);
        WM_HIP(ctx, hipGetLastError());
        return WM_OK;
    }
    hipLaunchKernelGGL(k_pack, dim3(blocks), dim3(kBlock), 0, ctx->stream, dptr, n, stride, out);
    WM_HIP(ctx, hipGetLastError());
    if (bbox_partials && bbox_blocks) return launch_bbox(ctx, out, n, bbox_partials, bbox_blocks);
    return WM_OK;
}

// ------------------------------------------------------------------ bbox
// One partial per workgroup: out[8 b + 0..2] = min, [3..5] = max (as floats), [6] = valid count.
// The host reduces the partials (it waits for the result anyway); no same-address atomics.
// PACK: the cloud is packed on the way (k_pack's conversion of the caller's records at `raw`, byte stride `rstride`, into
// pts) -- one launch instead of two at the head of every registration's chain of dependent launches; the box and the count
// are the same numbers either way (minima, maxima and an integer do not care about the order they are formed in).
template <bool PACK>
__global__ void __launch_bounds__(kBlock) k_bbox(float4 *pts, size_t n, float *out, const unsigned char *raw, size_t rstride) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned cnt = 0;
    const size_t stride = (size_t) gridDim.x * kBlock;
    for (size_t i0 = (size_t) blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += 4 * stride) {
        float4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // four loads in flight
            const size_t i = i0 + u * stride;
            if (PACK) {
                p[u] = make_float4(NAN, 0.f, 0.f, 0.f);
                if (i < n) {
                    const float *q = reinterpret_cast<const float *>(raw + i * rstride);
                    float x = q[0], y = q[1], z = q[2];
                    if (!(isfinite(x) && isfinite(y) && isfinite(z))) x = y = z = __builtin_nanf("");
                    p[u] = make_float4(x, y, z, __uint_as_float((unsigned) i));
                }
            } else {
                p[u] = i < n ? pts[i] : make_float4(NAN, 0.f, 0.f, 0.f);
            }
        }
        if (PACK) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t i = i0 + u * stride;
                if (i < n) pts[i] = p[u];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p[u].x == p[u].x) {  // not NaN
                lo[0] = fminf(lo[0], p[u].x);
                lo[1] = fminf(lo[1], p[u].y);
                lo[2] = fminf(lo[2], p[u].z);
                hi[0] = fmaxf(hi[0], p[u].x);
                hi[1] = fmaxf(hi[1], p[u].y);
                hi[2] = fmaxf(hi[2], p[u].z);
                ++cnt;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], __shfl_down(lo[d], off));
            hi[d] = fmaxf(hi[d], __shfl_down(hi[d], off));
        }
        cnt += __shfl_down(cnt, off);
    }
    __shared__ float s_lo[kBlock / 64][3], s_hi[kBlock / 64][3];
    __shared__ unsigned s_cnt[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int d = 0; d < 3; ++d) {
            s_lo[wave][d] = lo[d];
            s_hi[wave][d] = hi[d];
        }
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            for (int d = 0; d < 3; ++d) {
                lo[d] = fminf(lo[d], s_lo[w][d]);
                hi[d] = fmaxf(hi[d], s_hi[w][d]);
            }
            cnt += s_cnt[w];
        }
        float *o = out + 8 * (size_t) blockIdx.x;
        for (int d = 0; d < 3; ++d) {
            o[d] = lo[d];
            o[3 + d] = hi[d];
        }
        o[6] = __uint_as_float(cnt);
    }
}

int launch_bbox(wm_ctx *ctx, const float4 *pts, size_t n, float *partials_dev, unsigned *blocks_out) {
    unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    if (blocks > (unsigned) kBboxBlocks) blocks = kBboxBlocks;
    *blocks_out = blocks;
    if (n == 0) return WM_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bbox<false>), dim3(blocks), dim3(kBlock), 0, ctx->stream, const_cast<float4 *>(pts), n, partials_dev,
                       (const unsigned char *) nullptr, (size_t) 0);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

void finish_bbox(const float *res, unsigned blocks, Bbox *out, size_t *n_valid) {
    for (int d = 0; d < 3; ++d) out->lo[d] = out->hi[d] = 0.f;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    size_t cnt = 0;
    for (unsigned b = 0; b < blocks; ++b) {
        const float *o = res + 8 * b;
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], o[d]);
            hi[d] = fmaxf(hi[d], o[3 + d]);
        }
        unsigned c;
        memcpy(&c, &o[6], 4);
        cnt += c;
    }
    *n_valid = cnt;
    if (cnt > 0)
        for (int d = 0; d < 3; ++d) {
            out->lo[d] = lo[d];
            out->hi[d] = hi[d];
        }
}

int compute_bbox(wm_ctx *ctx, const float4 *pts, size_t n, Bbox *out, size_t *n_valid) {
    for (int d = 0; d < 3; ++d) out->lo[d] = out->hi[d] = 0.f;
    *n_valid = 0;
    if (n == 0) return WM_OK;
    // partials in device memory, fetched into pinned memory by one wavefront (fast_fetch)
    float *res = (float *) pinned_scratch(ctx, 8 * sizeof(float) * kBboxBlocks);
    if (!res) return WM_ERR_HIP;
    WM_HIP(ctx, ctx->bbox_buf.reserve(8 * sizeof(float) * kBboxBlocks));
    unsigned blocks = 0;
    WM_TRY(launch_bbox(ctx, pts, n, ctx->bbox_buf.as<float>(), &blocks));
    WM_TRY(fast_fetch(ctx, res, ctx->bbox_buf.p, 8 * sizeof(float) * blocks));
    finish_bbox(res, blocks, out, n_valid);
    return WM_OK;
}

// -------------------------------------------------- counting sort by cell
struct LinearKey {  // x-fastest dense cell index (target levels)
    float ox, oy, oz, inv_h;
    int nx, ny, nz;
    // THE cell of a point: every kernel that needs it (the counting sorts, k_coarse_move) asks here
    __device__ void cell(const float4 &p, int *cx, int *cy, int *cz) const {
        *cx = min(max((int) floorf((p.x - ox) * inv_h), 0), nx - 1);
        *cy = min(max((int) floorf((p.y - oy) * inv_h), 0), ny - 1);
        *cz = min(max((int) floorf((p.z - oz) * inv_h), 0), nz - 1);
    }
    // ... as its (y, z) row and its place along x: the cell index is row * nx + cx
    __device__ void row_x(const float4 &p, unsigned *row, unsigned *cx) const {
        int x, y, z;
        cell(p, &x, &y, &z);
        *row = (unsigned) (z * ny + y);
        *cx = (unsigned) x;
    }
    __device__ unsigned operator()(const float4 &p) const {
        unsigned row, cx;
        row_x(p, &row, &cx);
        return row * (unsigned) nx + cx;
    }
};

__device__ inline unsigned spread3(unsigned v) {  // 10 bits -> every third bit
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

struct MortonKey {  // Morton code of a 2^bits-per-axis cell (source ordering)
    float ox, oy, oz, sx, sy, sz;
    int cells;  // 2^bits
    __device__ unsigned operator()(const float4 &p) const {
        int cx = min(max((int) ((p.x - ox) * sx), 0), cells - 1);
        int cy = min(max((int) ((p.y - oy) * sy), 0), cells - 1);
        int cz = min(max((int) ((p.z - oz) * sz), 0), cells - 1);
        return spread3((unsigned) cx) | (spread3((unsigned) cy) << 1) |
               (spread3((unsigned) cz) << 2);
    }
};

// histogram of the cells; the value the atomic returns is the point's rank inside its cell, so the
// scatter needs no second round of atomics (the order inside a cell is the atomics' arrival order:
// arbitrary, and irrelevant -- the search's keys carry the original index)
template <class KeyFn>
__global__ void __launch_bounds__(kBlock) k_count(const float4 *pts, size_t n, KeyFn key,
                                                   unsigned *cell_of, unsigned *rank_of, unsigned *counts) {
    size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float4 p = pts[i];
    unsigned c = kNoIdx, r = 0;
    if (p.x == p.x) {
        c = key(p);
        r = atomicAdd(&counts[c], 1u);
    }
    cell_of[i] = c;
    rank_of[i] = r;
}

// (thread 0 also writes the four NaN entries behind the last point: the search reads groups of four
// entries and may run past the end of the last run -- see k_pad_tail, which does it for an empty level)
__global__ void __launch_bounds__(kBlock) k_scatter(const float4 *pts, size_t n,
                                                     const unsigned *cell_of, const unsigned *rank_of,
                                                     const unsigned *cell_start, float4 *out, size_t ncells) {
    size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        const unsigned end = cell_start[ncells];
        const float nanv = __builtin_nanf("");
#pragma unroll
        for (int u = 0; u < 4; ++u) out[end + u] = make_float4(nanv, nanv, nanv, __uint_as_float(kNoIdx));
    }
    if (i >= n) return;
    unsigned c = cell_of[i];
    if (c == kNoIdx) return;
    out[cell_start[c] + rank_of[i]] = pts[i];
}

// ------------------------------------------------------- exclusive scan
struct ScanIn {  // in[i] for i < n, 0 at i = n (exclusive_scan below)
    const unsigned *in;
    size_t n;
    __device__ unsigned operator()(size_t i) const { return i < n ? in[i] : 0u; }
};

// out must hold n+1 entries (out[n] = the total).  rocPRIM's single-pass look-back scan: 5 M cell counts in ~17 us
// (a three-kernel tiles / tile sums / add scan took 41 us).
int exclusive_scan(wm_ctx *ctx, const unsigned *in, size_t n, unsigned *out) {
    if (n == 0) {
        WM_HIP(ctx, hipMemsetAsync(out, 0, sizeof(unsigned), ctx->stream));
        return WM_OK;
    }
    // n + 1 items through an iterator that reads in[i] below n and 0 at n: out[n] comes out as the
    // total, without a one-thread kernel behind the scan (a dependent launch of its own: ~5 us)
    auto it = rocprim::make_transform_iterator(rocprim::counting_iterator<size_t>(0), ScanIn{in, n});
    // (32 items per thread: 54 us for the 14 M cell counts of a 1M-point level 0 against 67 with rocPRIM's default
    // tuning; 17 against 19 at 2 M -- scripts/dev/scan_probe.hip)
    using scan_cfg = rocprim::scan_config<256, 32, rocprim::block_load_method::block_load_transpose,
                                          rocprim::block_store_method::block_store_transpose,
                                          rocprim::block_scan_algorithm::using_warp_scan>;
    size_t bytes = 0;
    WM_HIP(ctx, rocprim::exclusive_scan<scan_cfg>(nullptr, bytes, it, out, 0u, n + 1, rocprim::plus<unsigned>(), ctx->stream));
    WM_HIP(ctx, ctx->block_sums.reserve(bytes + 64));
    WM_HIP(ctx, rocprim::exclusive_scan<scan_cfg>(ctx->block_sums.p, bytes, it, out, 0u, n + 1, rocprim::plus<unsigned>(),
                                                  ctx->stream));
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

template <class KeyFn>
static int counting_sort(wm_ctx *ctx, const float4 *pts, size_t n, KeyFn key, size_t ncells,
                         unsigned *cell_start /* ncells+1 */, float4 *out) {
    WM_HIP(ctx, ctx->cell_of.reserve(2 * n * sizeof(unsigned)));
    WM_HIP(ctx, ctx->counts.reserve(ncells * sizeof(unsigned)));
    unsigned *counts = ctx->counts.as<unsigned>();
    unsigned *cell_of = ctx->cell_of.as<unsigned>(), *rank_of = cell_of + n;
    WM_HIP(ctx, hipMemsetAsync(counts, 0, ncells * sizeof(unsigned), ctx->stream));
    unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_count<KeyFn>), dim3(blocks), dim3(kBlock), 0, ctx->stream,
                       pts, n, key, cell_of, rank_of, counts);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, counts, ncells, cell_start));
    hipLaunchKernelGGL(k_scatter, dim3(blocks), dim3(kBlock), 0, ctx->stream, pts, n, cell_of, rank_of,
                       cell_start, out, ncells);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// ------------------------------------------- counting sort by cell, row by row
// A level is ordered by cell index row * nx + cx, so a (y, z) ROW of cells is one contiguous run of the point array and
// of cell_start.  On a large lattice only a few per cent of the cells hold a point, and the sort above pays for every
// cell three times (the memset, the scan's read, the scan's write) and for a returning atomic per point scattered over
// the whole table.  By rows every cell costs one store and no atomic leaves a compute unit: the points are first put
// in order of their BAND -- 2^k consecutive rows, few enough that a counter per cell of the band fits a workgroup's
// LDS --, then a workgroup per band counts its points per cell in LDS, scans the counters there and writes the band's
// stretch of cell_start and the points' final places.  The order by band is one pass of a radix sort with a band per
// digit (wm_sort.hpp, whose scan it uses), its tiles' ranks taken in LDS.  Four launches:
//   k_rows_hist     per tile of 4 096 points: how many fall in each band        -> hist[band][tile]
//   k_rs_scan       a workgroup per band: its tiles' counts -> their exclusive prefix, the band's total
//   k_rows_scatter  the bands' first slots (a scan of the totals, in LDS, by every tile; tile 0 leaves it for the last
//                   kernel), then the tile's points to band start + prefix + rank in the tile, into a temporary
//   k_rows_finish   cell_start and the level's point array
// (Counters per row in device memory, a returning atomic each, were tried first: atomics run at the memory side, and a
// million of them on the 80 KB table of a 1M-point level took 85 us, against 48 us for k_count's over its 56 MB.)
// The order inside a cell is the atomics' arrival order, as above; cell_start is the same table.
constexpr int kRowThreads = 512;              // of all three kernels
constexpr int kRowTile = kRowThreads * 8;     // points per tile
constexpr unsigned kRowNxCap = 4000;          // cells along x up to which a band's counters fit the LDS budget ...
constexpr unsigned kRowCounterWords = 16000;  // ... of this many counters per workgroup (62.5 KB)
constexpr unsigned kRowBandRows = 8;          // rows per band, unless nx or the number of bands asks otherwise
constexpr unsigned kRowMaxBands = 8192;       // bands (counters in the LDS of k_rows_hist and k_rows_scatter)
constexpr uint64_t kRowMaxTable = 1ull << 22; // entries of hist[band][tile]

// exclusive prefix sums of a[0 .. n) in LDS, in place, by the whole workgroup (a[] complete and visible on entry: the
// caller's barrier; visible again on return); returns the total.  s_wave: kRowThreads / 64 words.
__device__ __forceinline__ unsigned rows_lds_scan(unsigned *a, unsigned n, unsigned *s_wave) {
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned per = (n + kRowThreads - 1) / kRowThreads;
    const unsigned b = min(tid * per, n), e = min(b + per, n);
    unsigned sum = 0;
    for (unsigned i = b; i < e; ++i) sum += a[i];
    const unsigned incl = wave_incl_scan(sum, lane);
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum, all = 0;
    for (unsigned w = 0; w < (unsigned) (kRowThreads / 64); ++w) {
        if (w < wave) run += s_wave[w];
        all += s_wave[w];
    }
    for (unsigned i = b; i < e; ++i) {
        const unsigned v = a[i];
        a[i] = run;
        run += v;
    }
    __syncthreads();
    return all;
}

__global__ void __launch_bounds__(kRowThreads) k_rows_hist(const float4 *__restrict__ pts, unsigned n, LinearKey key, unsigned rshift,
                                                            unsigned bands, unsigned tiles, unsigned *__restrict__ hist) {
    extern __shared__ unsigned s_mem[];  // [bands]
    const unsigned tid = threadIdx.x, tile = blockIdx.x;
    for (unsigned b = tid; b < bands; b += kRowThreads) s_mem[b] = 0u;
    __syncthreads();
    float4 p[8];
#pragma unroll
    for (unsigned r = 0; r < 8u; ++r) {  // eight loads in flight
        const unsigned i = tile * (unsigned) kRowTile + r * kRowThreads + tid;
        p[r] = i < n ? pts[i] : make_float4(NAN, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (unsigned r = 0; r < 8u; ++r)
        if (p[r].x == p[r].x) {
            unsigned row, cx;
            key.row_x(p[r], &row, &cx);
            atomicAdd(&s_mem[row >> rshift], 1u);
        }
    __syncthreads();
    for (unsigned b = tid; b < bands; b += kRowThreads) hist[(size_t) b * tiles + tile] = s_mem[b];
}

__global__ void __launch_bounds__(kRowThreads) k_rows_scatter(const float4 *__restrict__ pts, unsigned n, LinearKey key, unsigned rshift,
                                                               unsigned bands, unsigned tiles, const unsigned *__restrict__ hist,
                                                               const unsigned *__restrict__ totals, unsigned *__restrict__ band_start,
                                                               float4 *__restrict__ tmp) {
    extern __shared__ unsigned s_mem[];  // [bands]: the cursor of each band's run for this tile
    __shared__ unsigned s_wave[kRowThreads / 64];
    const unsigned tid = threadIdx.x, tile = blockIdx.x;
    float4 p[8];
#pragma unroll
    for (unsigned r = 0; r < 8u; ++r) {
        const unsigned i = tile * (unsigned) kRowTile + r * kRowThreads + tid;
        p[r] = i < n ? pts[i] : make_float4(NAN, 0.f, 0.f, 0.f);
    }
    for (unsigned b = tid; b < bands; b += kRowThreads) s_mem[b] = totals[b];
    __syncthreads();
    const unsigned all = rows_lds_scan(s_mem, bands, s_wave);
    if (tile == 0) {
        for (unsigned b = tid; b < bands; b += kRowThreads) band_start[b] = s_mem[b];
        if (tid == 0) band_start[bands] = all;
    }
    for (unsigned b = tid; b < bands; b += kRowThreads) s_mem[b] += hist[(size_t) b * tiles + tile];
    __syncthreads();
#pragma unroll
    for (unsigned r = 0; r < 8u; ++r)
        if (p[r].x == p[r].x) {
            unsigned row, cx;
            key.row_x(p[r], &row, &cx);
            tmp[atomicAdd(&s_mem[row >> rshift], 1u)] = p[r];
        }
}

// A workgroup takes a band, i.e. ONE contiguous stretch of the band-ordered points, and all its threads walk that stretch
// together -- whether it is eight rows of fifty points or one of them holds seventy thousand.  Pass 1 counts the points
// per cell in LDS; a scan turns the counts into the cells' offsets in the stretch; the band's stretch of cell_start
// leaves in coalesced runs (an empty band's words too); pass 2 reads the points again (from the cache) and draws each
// one's slot from its cell's offset, now a cursor.  The last band's workgroup also writes cell_start[ncells] and the four
// NaN entries behind the last point (see k_pad_tail).
__global__ void __launch_bounds__(kRowThreads) k_rows_finish(const float4 *__restrict__ tmp, const unsigned *__restrict__ band_start,
                                                              LinearKey key, unsigned nrows, unsigned rshift,
                                                              unsigned *__restrict__ cell_start, float4 *__restrict__ out) {
    extern __shared__ unsigned s_mem[];  // [rows of the band][nx]
    __shared__ unsigned s_wave[kRowThreads / 64];
    const unsigned nx = (unsigned) key.nx, tid = threadIdx.x;
    const unsigned r0 = blockIdx.x << rshift;
    const unsigned cells = min(1u << rshift, nrows - r0) * nx;
    const unsigned s = band_start[blockIdx.x], e = band_start[blockIdx.x + 1];
    for (unsigned k = tid; k < cells; k += kRowThreads) s_mem[k] = 0u;
    __syncthreads();
    for (unsigned j0 = s + tid; j0 < e; j0 += 4u * kRowThreads) {
        float4 p[4];
#pragma unroll
        for (unsigned u = 0; u < 4u; ++u) {  // four loads in flight
            const unsigned j = j0 + u * kRowThreads;
            p[u] = j < e ? tmp[j] : make_float4(NAN, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (unsigned u = 0; u < 4u; ++u)
            if (j0 + u * kRowThreads < e) {
                unsigned row, cx;
                key.row_x(p[u], &row, &cx);
                atomicAdd(&s_mem[min((row - r0) * nx + cx, cells - 1u)], 1u);
            }
    }
    __syncthreads();
    if (e != s) rows_lds_scan(s_mem, cells, s_wave);  // (an empty band's counters are its offsets already)
    unsigned *cs = cell_start + (size_t) r0 * nx;
    for (unsigned k = tid; k < cells; k += kRowThreads) cs[k] = s + s_mem[k];
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        cs[cells] = e;
        const float nanv = __builtin_nanf("");
#pragma unroll
        for (int u = 0; u < 4; ++u) out[e + u] = make_float4(nanv, nanv, nanv, __uint_as_float(kNoIdx));
    }
    __syncthreads();
    for (unsigned j0 = s + tid; j0 < e; j0 += 4u * kRowThreads) {
        float4 p[4];
#pragma unroll
        for (unsigned u = 0; u < 4u; ++u) {
            const unsigned j = j0 + u * kRowThreads;
            p[u] = j < e ? tmp[j] : make_float4(NAN, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (unsigned u = 0; u < 4u; ++u)
            if (j0 + u * kRowThreads < e) {
                unsigned row, cx;
                key.row_x(p[u], &row, &cx);
                out[s + atomicAdd(&s_mem[min((row - r0) * nx + cx, cells - 1u)], 1u)] = p[u];
            }
    }
}

// WHERE the row-wise sort is taken, and with how many rows per band (2^*rshift): a pure function of the option
// (grid_rows), the lattice and the number of points.
//   structurally: a band's counters must fit the finish kernel's LDS budget (nx <= kRowNxCap), the bands' counters that
//   of the other two kernels (kRowMaxBands), and the table of the tiles' counts stays small beside the points;
//   where it pays (option 1): rows of at least 3 cells, enough bands to give every compute unit a workgroup of
//   k_rows_finish, and enough points that the four launches' fixed cost is not the whole of it
constexpr unsigned kRowMinRows = 2048, kRowMinPoints = 32768;
static bool rows_apply(int option, int nx, int ny, int nz, size_t n, unsigned *rshift) {
    if (option == 0 || n == 0 || (unsigned) nx > kRowNxCap) return false;
    const uint64_t nrows = (uint64_t) ny * nz;
    unsigned sh = 0;
    while ((2u << sh) <= kRowBandRows && (2u << sh) * (unsigned) nx <= kRowCounterWords) ++sh;
    while (((nrows - 1) >> sh) + 1 > kRowMaxBands && (2u << sh) * (unsigned) nx <= kRowCounterWords) ++sh;
    const uint64_t bands = ((nrows - 1) >> sh) + 1, tiles = (n + kRowTile - 1) / kRowTile;
    if (bands > kRowMaxBands || bands * tiles > kRowMaxTable) return false;
    *rshift = sh;
    if (option == 2) return true;
    return nx >= 3 && nrows >= kRowMinRows && n >= kRowMinPoints;
}
static_assert(kRowCounterWords / kRowNxCap >= 1 && kRowCounterWords * sizeof(unsigned) + 64 <= 65536, "k_rows_finish's LDS");

static int counting_sort_rows(wm_ctx *ctx, const float4 *pts, size_t n, const LinearKey &key, unsigned rshift,
                              unsigned *cell_start /* ncells+1 */, float4 *out) {
    const unsigned nrows = (unsigned) key.ny * (unsigned) key.nz;
    const unsigned bands = ((nrows - 1) >> rshift) + 1, tiles = (unsigned) ((n + kRowTile - 1) / kRowTile);
    WM_HIP(ctx, ctx->row_tmp.reserve(n * sizeof(float4)));
    WM_HIP(ctx, ctx->row_hist.reserve(((size_t) bands * tiles + 2 * (size_t) bands + 1) * sizeof(unsigned)));
    unsigned *hist = ctx->row_hist.as<unsigned>(), *totals = hist + (size_t) bands * tiles, *band_start = totals + bands;
    float4 *tmp = ctx->row_tmp.as<float4>();
    const size_t band_lds = (size_t) bands * sizeof(unsigned);
    hipLaunchKernelGGL(k_rows_hist, dim3(tiles), dim3(kRowThreads), band_lds, ctx->stream, pts, (unsigned) n, key, rshift, bands, tiles, hist);
    WM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rs_scan, dim3(bands), dim3(kRsThreads), 0, ctx->stream, hist, tiles, totals);
    WM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rows_scatter, dim3(tiles), dim3(kRowThreads), band_lds, ctx->stream, pts, (unsigned) n, key, rshift, bands, tiles,
                       (const unsigned *) hist, (const unsigned *) totals, band_start, tmp);
    WM_HIP(ctx, hipGetLastError());
    const size_t cell_lds = ((size_t) key.nx << rshift) * sizeof(unsigned);
    hipLaunchKernelGGL(k_rows_finish, dim3(bands), dim3(kRowThreads), cell_lds, ctx->stream, (const float4 *) tmp,
                       (const unsigned *) band_start, key, nrows, rshift, cell_start, out);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// occupied-cell count (for choosing the level-0 cell size): one partial per workgroup,
// summed by the host
// occupied-cell count (for choosing the level-0 cell size): one partial per workgroup,
// summed by the host
constexpr int kOccBlocks = 1024;
__global__ void __launch_bounds__(kBlock) k_count_occupied(const unsigned *cell_start,
                                                            size_t ncells, unsigned *out) {
    unsigned c = 0;
    for (size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x; i < ncells;
         i += (size_t) gridDim.x * kBlock)
        c += (cell_start[i + 1] != cell_start[i]);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    __shared__ unsigned s_c[kBlock / 64];
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) c += s_c[w];
        out[blockIdx.x] = c;
    }
}

// Four NaN entries after the last point of a level's cell-sorted array: the search reads
// groups of four entries and may run past the end of the last run.
__global__ void k_pad_tail(const unsigned *cell_start, size_t ncells, float4 *pts) {
    const unsigned end = cell_start[ncells];
    const float nanv = __builtin_nanf("");
    if (threadIdx.x < 4) pts[end + threadIdx.x] = make_float4(nanv, nanv, nanv, __uint_as_float(kNoIdx));
}

static void grid_dims(const Bbox &bb, float h, int *nx, int *ny, int *nz) {
    *nx = (int) floor((bb.hi[0] - bb.lo[0]) / h) + 1;
    *ny = (int) floor((bb.hi[1] - bb.lo[1]) / h) + 1;
    *nz = (int) floor((bb.hi[2] - bb.lo[2]) / h) + 1;
}

int build_grid_level(wm_ctx *ctx, const float4 *pts, size_t n, const Bbox &bb, float h,
                     GridLevel *lvl, double *avg_occupancy) {
    int nx, ny, nz;
    grid_dims(bb, h, &nx, &ny, &nz);
    uint64_t ncells = (uint64_t) nx * ny * nz;
    lvl->ncells = ncells;
    WM_HIP(ctx, lvl->pts.reserve((n + 4) * sizeof(float4)));
    WM_HIP(ctx, lvl->cell_start.reserve((ncells + 1) * sizeof(unsigned)));
    LinearKey key{bb.lo[0], bb.lo[1], bb.lo[2], 1.0f / h, nx, ny, nz};
    unsigned rshift = 0;
    if (rows_apply(ctx->tune_grid_rows, nx, ny, nz, n, &rshift)) {
        WM_TRY(counting_sort_rows(ctx, pts, n, key, rshift, lvl->cell_start.as<unsigned>(), lvl->pts.as<float4>()));
    } else if (n > 0) {
        WM_TRY(counting_sort(ctx, pts, n, key, ncells, lvl->cell_start.as<unsigned>(),
                             lvl->pts.as<float4>()));
    } else {
        WM_HIP(ctx, hipMemsetAsync(lvl->cell_start.p, 0, (ncells + 1) * sizeof(unsigned),
                                   ctx->stream));
        hipLaunchKernelGGL(k_pad_tail, dim3(1), dim3(64), 0, ctx->stream, lvl->cell_start.as<unsigned>(),
                           (size_t) ncells, lvl->pts.as<float4>());
    }
    // float cell assignment can be off by the rounding of (p - origin) * inv_h:
    // keep a cell-unit margin in every geometric bound that relies on it.
    float extent = fmaxf(fmaxf(bb.hi[0] - bb.lo[0], bb.hi[1] - bb.lo[1]), bb.hi[2] - bb.lo[2]);
    float amax = 0;
    for (int d = 0; d < 3; ++d) amax = fmaxf(amax, fmaxf(fabsf(bb.lo[d]), fabsf(bb.hi[d])));
    float ulp = fmaxf(amax, extent) * 1.2e-7f;
    lvl->d.ox = bb.lo[0];
    lvl->d.oy = bb.lo[1];
    lvl->d.oz = bb.lo[2];
    lvl->d.h = h;
    lvl->d.inv_h = 1.0f / h;
    lvl->d.slack = fmaxf(1e-3f, 8.0f * ulp / h);
    lvl->d.nx = nx;
    lvl->d.ny = ny;
    lvl->d.nz = nz;
    lvl->d.pts = lvl->pts.as<float4>();
    lvl->d.cell_start = lvl->cell_start.as<unsigned>();
    lvl->built = true;
    if (avg_occupancy) {
        unsigned blocks = (unsigned) ((ncells + kBlock - 1) / kBlock);
        if (blocks > (unsigned) kOccBlocks) blocks = kOccBlocks;
        unsigned *part = (unsigned *) pinned_scratch(ctx, sizeof(unsigned) * kOccBlocks);
        if (!part) return WM_ERR_HIP;
        WM_HIP(ctx, ctx->bbox_buf.reserve(sizeof(unsigned) * kOccBlocks));
        hipLaunchKernelGGL(k_count_occupied, dim3(blocks), dim3(kBlock), 0, ctx->stream,
                           lvl->cell_start.as<unsigned>(), (size_t) ncells, ctx->bbox_buf.as<unsigned>());
        WM_TRY(fast_fetch(ctx, part, ctx->bbox_buf.p, sizeof(unsigned) * blocks));
        uint64_t occ = 0;
        for (unsigned b = 0; b < blocks; ++b) occ += part[b];
        *avg_occupancy = occ ? (double) n / occ : 0.0;
    }
    return WM_OK;
}

static uint64_t cells_of(const Bbox &bb, float h) {  // (build_grid_level's lattice)
    uint64_t c = 1;
    for (int d = 0; d < 3; ++d) c *= (uint64_t) floor(((double) bb.hi[d] - bb.lo[d]) / h) + 1;
    return c;
}

// The grid of one call over an arbitrary packed cloud (wm_outlier_filter, wm_cluster_extract).  The automatic cell is
// source_grid's (wm_gicp.hip): 1.5 x the cube root of the box's volume per point, rebuilt once when the occupied
// cells hold more than 6 or fewer than 1.5 points on average.  A fixed-radius search's box [q - r, q + r] must span a
// bounded number of rows, so its cell is never smaller than `floor_h` (r / 2 by default: at most 6 x 6 rows of at most
// 6 cells); 0 for a search without a radius.
int build_call_grid(wm_ctx *ctx, const float4 *pts, size_t n, size_t n_finite, const Bbox &bb, float floor_h,
                    GridLevel *grid) {
    double vol = 1;
    for (int d = 0; d < 3; ++d) vol *= fmax((double) bb.hi[d] - bb.lo[d], 1e-3);
    float h = fmaxf((float) fmax(cbrt(vol / (double) n_finite) * 1.5, 1e-4), floor_h);
    const uint64_t cell_cap = ((uint64_t) 1 << 26) + 8 * (uint64_t) n;  // (a lattice far beyond the points pays for nothing)
    while (cells_of(bb, h) > cell_cap) h *= 1.26f;
    double occ = 0;
    WM_TRY(build_grid_level(ctx, pts, n, bb, h, grid, &occ));
    if (occ > 6.0 || (occ > 0 && occ < 1.5)) {
        float h2 = fmaxf((float) (h * sqrt(3.0 / occ)), floor_h);
        while (cells_of(bb, h2) > cell_cap) h2 *= 1.26f;
        if (h2 != h) WM_TRY(build_grid_level(ctx, pts, n, bb, h2, grid, nullptr));
    }
    return WM_OK;
}

// Source ordering: stable radix sort of (Morton cell code, original index) pairs, then a
// gather.  Stable => points of one Morton cell keep ascending original index, so every
// downstream sum over the source runs in a reproducible order.  Non-finite points get the
// key past the last cell and fall off the end (n_valid comes from the bbox pass).
__global__ void __launch_bounds__(kBlock) k_morton_keys(const float4 *pts, unsigned n, MortonKey key,
                                                         unsigned invalid, unsigned *keys,
                                                         unsigned *vals) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    keys[i] = p.x == p.x ? key(p) : invalid;
    vals[i] = i;
}

__global__ void __launch_bounds__(kBlock) k_gather(const float4 *pts, const unsigned *vals,
                                                    unsigned n, float4 *out) {
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) out[j] = pts[vals[j]];
}

int morton_sort(wm_ctx *ctx, const float4 *pts, size_t n, const Bbox &bb, size_t n_valid,
                float4 *out) {
    if (n == 0 || n_valid == 0) return WM_OK;
    int bits = (int) ceil(log2(cbrt((double) n)));
    if (bits < 3) bits = 3;
    if (bits > 8) bits = 8;
    const int cells = 1 << bits;
    float ext[3];
    for (int d = 0; d < 3; ++d) ext[d] = fmaxf(bb.hi[d] - bb.lo[d], 1e-6f);
    MortonKey key{bb.lo[0], bb.lo[1], bb.lo[2], cells / ext[0], cells / ext[1], cells / ext[2],
                  cells};
    WM_HIP(ctx, ctx->vg_idx.reserve(n * 4));
    WM_HIP(ctx, ctx->vg_idx2.reserve(n * 4));
    WM_HIP(ctx, ctx->vg_perm.reserve(n * 4));
    WM_HIP(ctx, ctx->vg_perm2.reserve(n * 4));
    unsigned *k1 = ctx->vg_idx.as<unsigned>(), *k2 = ctx->vg_idx2.as<unsigned>();
    unsigned *v1 = ctx->vg_perm.as<unsigned>(), *v2 = ctx->vg_perm2.as<unsigned>();
    const unsigned blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_morton_keys, dim3(blocks), dim3(kBlock), 0, ctx->stream, pts, (unsigned) n,
                       key, 1u << (3 * bits), k1, v1);
    size_t tmp_bytes = 0;
    WM_HIP(ctx, sort_pairs_low_bits(nullptr, tmp_bytes, k1, k2, v1, v2, n, 3 * bits + 1, ctx->stream,
                                    (size_t) ctx->tune_radix_min));
    WM_HIP(ctx, ctx->vg_tmp.reserve(tmp_bytes));
    WM_HIP(ctx, sort_pairs_low_bits(ctx->vg_tmp.p, tmp_bytes, k1, k2, v1, v2, n, 3 * bits + 1, ctx->stream,
                                    (size_t) ctx->tune_radix_min));
    const unsigned gblocks = (unsigned) ((n_valid + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_gather, dim3(gblocks), dim3(kBlock), 0, ctx->stream, pts, v2,
                       (unsigned) n_valid, out);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// ---- coarser levels derived from the next finer one (cell size exactly x2, same origin):
// a coarse cell is the union of 2x2x2 fine cells, i.e. of 4 contiguous runs of the fine
// cell-sorted array (the two x-children of a row are adjacent).  Counting is a handful of
// cell_start reads per coarse cell and the copy moves whole runs: no atomics, no keys.
__device__ __forceinline__ void child_run(const unsigned *fs, int fnx, int fny, int fnz, int X,
                                          int Y, int Z, int r, unsigned *s, unsigned *e) {
    const int y = 2 * Y + (r & 1), z = 2 * Z + (r >> 1);
    *s = *e = 0;
    if (y >= fny || z >= fnz) return;
    const size_t base = ((size_t) z * fny + y) * fnx;
    const int xa = 2 * X, xb = min(2 * X + 2, fnx);
    *s = fs[base + xa];
    *e = fs[base + xb];
}

__global__ void __launch_bounds__(kBlock)
    k_coarse_count(const unsigned *__restrict__ fs, int fnx, int fny, int fnz, int cnx, int cny,
                   size_t ncells, unsigned *__restrict__ counts) {
    const size_t c = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (c >= ncells) return;
    const int X = (int) (c % cnx), Y = (int) ((c / cnx) % cny), Z = (int) (c / ((size_t) cnx * cny));
    unsigned total = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        unsigned s, e;
        child_run(fs, fnx, fny, fnz, X, Y, Z, r, &s, &e);
        total += e - s;
    }
    counts[c] = total;
}

// One lane per POINT of the fine array: its level-0 cell (recomputed from its coordinates,
// exactly as the level-0 sort did) shifted right gives its fine and coarse cells; its slot in
// the coarse array is the coarse cell's start + the lengths of the child runs before its own
// + its offset in its run.  Reads and writes are coalesced (a run moves as a block) and the
// order inside a coarse cell is fixed: child runs in (y, z) order, fine order inside a run.
__global__ void __launch_bounds__(kBlock)
    k_coarse_move(const unsigned *__restrict__ fs, const float4 *__restrict__ fpts, size_t fncells,
                  LinearKey key0, int shift, int fnx, int fny, int fnz, int cnx, int cny,
                  const unsigned *__restrict__ cs, float4 *__restrict__ out, size_t cncells) {
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    if (j == 0) {  // the four NaN entries behind the last point (see k_scatter)
        const unsigned end = cs[(size_t) cncells];
        const float nanv = __builtin_nanf("");
#pragma unroll
        for (int u = 0; u < 4; ++u) out[end + u] = make_float4(nanv, nanv, nanv, __uint_as_float(kNoIdx));
    }
    if (j >= fs[fncells]) return;
    const float4 p = fpts[j];
    int x, y, z;
    key0.cell(p, &x, &y, &z);
    x >>= shift;
    y >>= shift;
    z >>= shift;
    const int X = x >> 1, Y = y >> 1, Z = z >> 1, r = (y & 1) + 2 * (z & 1);
    unsigned dst = cs[((size_t) Z * cny + Y) * cnx + X];
    for (int q = 0; q < r; ++q) {
        unsigned s, e;
        child_run(fs, fnx, fny, fnz, X, Y, Z, q, &s, &e);
        dst += e - s;
    }
    unsigned s, e;
    child_run(fs, fnx, fny, fnz, X, Y, Z, r, &s, &e);
    out[dst + (j - s)] = p;
}

static int derive_grid_level(wm_ctx *ctx, const GridLevel &fine, int fine_index, GridLevel *lvl,
                             size_t n) {
    const GridDev &f = fine.d;
    const int nx = (f.nx + 1) / 2, ny = (f.ny + 1) / 2, nz = (f.nz + 1) / 2;
    const uint64_t ncells = (uint64_t) nx * ny * nz;
    lvl->ncells = ncells;
    WM_HIP(ctx, lvl->pts.reserve((n + 4) * sizeof(float4)));
    WM_HIP(ctx, lvl->cell_start.reserve((ncells + 1) * sizeof(unsigned)));
    WM_HIP(ctx, ctx->counts.reserve(ncells * sizeof(unsigned)));
    unsigned *counts = ctx->counts.as<unsigned>();
    const unsigned blocks = (unsigned) ((ncells + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_coarse_count, dim3(blocks), dim3(kBlock), 0, ctx->stream, f.cell_start, f.nx,
                       f.ny, f.nz, nx, ny, (size_t) ncells, counts);
    WM_TRY(exclusive_scan(ctx, counts, ncells, lvl->cell_start.as<unsigned>()));
    {
        const GridDev &g0 = ctx->levels[0].d;
        const LinearKey key0{g0.ox, g0.oy, g0.oz, g0.inv_h, g0.nx, g0.ny, g0.nz};
        const unsigned pblocks = (unsigned) ((n + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_coarse_move, dim3(pblocks), dim3(kBlock), 0, ctx->stream, f.cell_start,
                           f.pts, (size_t) fine.ncells, key0, fine_index, f.nx, f.ny, f.nz, nx, ny,
                           lvl->cell_start.as<unsigned>(), lvl->pts.as<float4>(), (size_t) ncells);
    }
    WM_HIP(ctx, hipGetLastError());
    lvl->d = f;
    lvl->d.h = 2.0f * f.h;  // exact in float
    lvl->d.inv_h = 1.0f / lvl->d.h;
    lvl->d.nx = nx;
    lvl->d.ny = ny;
    lvl->d.nz = nz;
    lvl->d.pts = lvl->pts.as<float4>();
    lvl->d.cell_start = lvl->cell_start.as<unsigned>();
    // a point sits in coarse cell (fine cell >> 1): the fine level's geometric margin
    // (slack_f * h_f) is slack_f / 2 coarse cells; keep the fine value (conservative)
    lvl->built = true;
    return WM_OK;
}

// Level 0: cell size from the measured density (a few points per occupied cell).
// Levels >= 1: cell size x4 per level until one ring of cells covers max_corr.
static int build_level0(wm_ctx *ctx) {
    const float4 *pts = ctx->tgt_orig.as<float4>();
    const Bbox &bb = ctx->tgt_bbox;
    const size_t n = ctx->n_tgt_input;
    double ext[3], vol = 1;
    for (int d = 0; d < 3; ++d) {
        ext[d] = fmax((double) bb.hi[d] - bb.lo[d], 1e-3);
        vol *= ext[d];
    }
    const uint64_t kMaxCells = 96ull << 20;
    auto clamp_h = [&](double h) {
        for (;;) {
            int nx, ny, nz;
            grid_dims(bb, (float) h, &nx, &ny, &nz);
            if ((uint64_t) nx * ny * nz <= kMaxCells) return h;
            h *= 1.26;
        }
    };
    double h;
    if (ctx->grid_cell_override > 0) {
        h = clamp_h(ctx->grid_cell_override);
        return build_grid_level(ctx, pts, n, bb, (float) h, &ctx->levels[0], nullptr);
    }
    const double target_occ = 3.0;
    // first guess assumes points spread over surfaces: occupancy ~ h^2 ...
    h = clamp_h(fmax(cbrt(vol / fmax((double) ctx->n_tgt, 1.0)) * 1.5, 1e-4));
    // ... unless the previous target looked alike (consecutive scans of one sensor do):
    // then its tuned cell size is the first guess and usually passes the check at once
    if (ctx->tuned_h > 0 && ctx->tuned_n > 0) {
        const double rn = (double) ctx->n_tgt / (double) ctx->tuned_n;
        const double rv = vol / ctx->tuned_vol;
        if (rn > 0.8 && rn < 1.25 && rv > 0.6 && rv < 1.6) h = clamp_h(ctx->tuned_h);
        // a cloud this close to the one the cell size was measured on: build with it and skip the
        // occupancy check (a device -> host round trip) -- but look again every 16th time.  The cell
        // size only steers the search's work, never its result.
        if (rn > 0.9 && rn < 1.1 && rv > 0.8 && rv < 1.25 && ++ctx->tuned_uses < 16)
            return build_grid_level(ctx, pts, n, bb, (float) h, &ctx->levels[0], nullptr);
    }
    ctx->tuned_uses = 0;
    double occ = 0;
    for (int it = 0; it < 3; ++it) {
        WM_TRY(build_grid_level(ctx, pts, n, bb, (float) h, &ctx->levels[0], &occ));
        if (occ <= 0) break;
        if (occ > target_occ * 0.6 && occ < target_occ * 1.6) break;
        double scale = sqrt(target_occ / occ);
        if (scale > 4) scale = 4;
        if (scale < 0.25) scale = 0.25;
        double nh = clamp_h(h * scale);
        if (fabs(nh - h) < 0.05 * h) break;
        h = nh;
    }
    if (!ctx->levels[0].built || ctx->levels[0].d.h != (float) h)
        WM_TRY(build_grid_level(ctx, pts, n, bb, (float) h, &ctx->levels[0], nullptr));
    ctx->tuned_h = h;
    ctx->tuned_n = ctx->n_tgt;
    ctx->tuned_vol = vol;
    return WM_OK;
}

int ensure_levels(wm_ctx *ctx, double max_corr) {
    if (!ctx->levels[0].built) {
        WM_TRY(build_level0(ctx));
        ctx->n_levels = 1;
        ctx->levels_max_corr = -1;
    }
    if (ctx->levels_max_corr == max_corr) return WM_OK;
    const float4 *pts = ctx->tgt_orig.as<float4>();
    double h = ctx->levels[0].d.h;
    int L = 1;
    // cell size x2 per level until a level's cells reach max_corr / 5: the search picks the
    // finest level whose cells are >= 0.2 r (lane scan) or 0.5 r (cooperative scan) and walks
    // boxes of cells, so coarser levels than that would never be chosen by the former and save
    // the latter (rare far-out queries) only a few row look-ups
    while (h < 0.2 * max_corr && L < kMaxLevels) {
        h *= 2.0;
        WM_TRY(derive_grid_level(ctx, ctx->levels[L - 1], L - 1, &ctx->levels[L], ctx->n_tgt_input));
        ++L;
    }
    (void) pts;
    ctx->n_levels = L;
    ctx->levels_max_corr = max_corr;
    // publish the ladder for the search kernels: every launch takes it by value, as a kernel argument (levels_dev),
    // and looks a level chosen at run time up in the copy in device memory
    LevelsDev host{};
    for (int l = 0; l < L; ++l) host.g[l] = ctx->levels[l].d;
    host.n = L;
    ctx->levels_dev = host;
    WM_HIP(ctx, ctx->d_levels.reserve(sizeof(LevelsDev)));
    // staged in pinned memory the ctx owns: the copy is asynchronous and needs no wait (the
    // next user of the scratch waits on the stream before touching it)
    LevelsDev *stage = (LevelsDev *) ((char *) pinned_scratch(ctx, 0) + (32u << 10));
    if (!ctx->h_scratch) return WM_ERR_HIP;
    *stage = host;
    WM_HIP(ctx, hipMemcpyAsync(ctx->d_levels.p, stage, sizeof(host), hipMemcpyHostToDevice,
                               ctx->stream));
    return WM_OK;
}

}  // namespace wm

extern "C" int wm_debug_sort_pairs(wm_ctx *ctx, const void *keys, int key_bytes, size_t n, unsigned bits, unsigned *values_out) {
    using namespace wm;
    if (!ctx || (n > 0 && (!keys || !values_out)) || (key_bytes != 4 && key_bytes != 8) || bits > 8u * (unsigned) key_bytes ||
        n >= (size_t) 0xFFFF0000u)
        return WM_ERR_ARG;
    if (n == 0) return WM_OK;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    struct Scoped : DevBuf {  // (DevBuf frees nothing by itself: the context owns its buffers; these are this call's)
        ~Scoped() { release(); }
    } k1, k2, v1, v2, tmp;
    WM_HIP(ctx, k1.reserve(n * (size_t) key_bytes));
    WM_HIP(ctx, k2.reserve(n * (size_t) key_bytes));
    WM_HIP(ctx, v1.reserve(n * 4));
    WM_HIP(ctx, v2.reserve(n * 4));
    WM_HIP(ctx, tmp.reserve(rs_temp_bytes(n)));
    std::vector<unsigned> iota(n);
    for (size_t i = 0; i < n; ++i) iota[i] = (unsigned) i;
    WM_HIP(ctx, hipMemcpy(k1.p, keys, n * (size_t) key_bytes, hipMemcpyHostToDevice));
    WM_HIP(ctx, hipMemcpy(v1.p, iota.data(), n * 4, hipMemcpyHostToDevice));
    if (key_bytes == 4)
        WM_HIP(ctx, rs_sort_pairs(tmp.p, k1.as<unsigned>(), k2.as<unsigned>(), v1.as<unsigned>(), v2.as<unsigned>(), n, bits, ctx->stream));
    else
        WM_HIP(ctx, rs_sort_pairs(tmp.p, k1.as<unsigned long long>(), k2.as<unsigned long long>(), v1.as<unsigned>(), v2.as<unsigned>(), n,
                                  bits, ctx->stream));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    WM_HIP(ctx, hipMemcpy(values_out, v2.p, n * 4, hipMemcpyDeviceToHost));
    return WM_OK;
}
