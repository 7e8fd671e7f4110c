// segmaploss.hip -- the segment loss of the per-segment regression modules LitZ / LitEZ (the reference's
// LitBase._calc_segment_loss) on the device: a dense prediction map [B, planes, nx, ny] scored against the targets of the
// ACTIVE segments only, sum-reduced criterion divided by the number of rows.
//
// A row of coords = (x, y, event) is COUNTED when it lies below the valid count, inside [nx, ny, B] and (with a mask) on a
// segment whose mask entry is 1.0.  For a counted row and plane p: d = map[event, p, x, y] - target[row, cols[p]].
//
//   k_sml_forward    ONE launch, the shape of segquant.hip's k_mrl_forward: the rows are cut into chunks of SML_CHUNK by
//                    row index, whatever the grid; a workgroup sums a chunk in a fixed shape (every thread its rows in
//                    row order, then a fixed tree) and stores the chunk's per-plane sums and count; the workgroup that
//                    draws the last ticket folds the chunk sums in chunk order and writes out[0 .. planes - 1] = sum / count,
//                    out[planes] = their fp64 sum rounded once, and the count.  d and every sum are fp64, there is no
//                    floating-point atomic: the result repeats bit for bit and does not depend on the grid, the rows'
//                    capacity (a chunk beyond the valid rows adds an exact 0) or B.
//   k_sml_backward   ONE launch that writes ALL of dmap, so nothing clears it first.  A workgroup takes SML_EVENTS
//                    consecutive events, one wavefront each.  The wavefront finds its event's row range among the valid
//                    rows by bisection on the event column (rows are grouped by event in ascending order, as the rulebook
//                    builds take them), the workgroup clears a [SML_EVENTS, planes, nx, ny] tile in LDS, every counted row
//                    writes grad * s / count into its cell, and the tile goes out in 16-byte lanes: SML_EVENTS = 4 events
//                    of 14 x 11 cells are a multiple of 16 bytes in every dtype, one event is not.  Cells without a
//                    counted row -- events without rows, events beyond the batch's own -- are the tile's zeros.
//                    Segments are unique within an event; a duplicated one is found by an integer LDS minimum over the
//                    cell's rows (its first row owns the cell), and only then the owner lane walks the event's rows again
//                    and sums the cell's values in row order, so the result is deterministic there too.
//
// A row that is not counted is SELECTED out: none of its values, and no map cell outside the counted rows, is loaded into
// the arithmetic (beyond the valid count not even its coordinates).  With no row counted the losses are NaN (0 / 0) and
// dmap is all zeros.
#include "wfs_common.h"
#include "wfs_rows.h"                         // ldt: rows of a runtime dtype

namespace {

constexpr int SML_THREADS = 256;
constexpr int SML_ROWS = 4;                   // rows per thread and chunk
constexpr int SML_CHUNK = SML_THREADS * SML_ROWS;
constexpr int SML_MAX_BLOCKS = 256;
constexpr int SML_HEAD = 16;                  // workspace: the ticket (and padding), then (planes + 1) x 8 bytes per chunk
constexpr int SML_PLANES = 4;                 // at most
constexpr int SML_EVENTS = SML_THREADS / WFS_WAVE;   // events per workgroup of the backward launch
constexpr int SML_CELLS = 256;                // nx * ny at most (14 x 11 = 154)

struct SmlIn {
    const void *map, *target;
    const int *coords;
    const float *mask;                        // [nx, ny] or NULL
    const long long *n_dev;
    long long n_cap, B;
    int map_dtype, target_dtype, n_cols, planes, nx, ny, kind;
    int cols[SML_PLANES];
};

// row r (below the valid count): its cell x * ny + y and its event when it is counted, else cell < 0
__device__ __forceinline__ int sml_cell(const SmlIn &in, long long r, int &e) {
    const int x = in.coords[r * 3], y = in.coords[r * 3 + 1];
    e = in.coords[r * 3 + 2];
    if (x < 0 || x >= in.nx || y < 0 || y >= in.ny || e < 0 || e >= in.B) return -1;
    const int cell = x * in.ny + y;
    if (in.mask && in.mask[cell] != 1.0f) return -1;
    return cell;
}

__device__ __forceinline__ double sml_diff(const SmlIn &in, long long r, int e, int cell, int p) {
    const long long at = ((long long)e * in.planes + p) * (in.nx * in.ny) + cell;
    return (double)ldt(in.map, at, in.map_dtype) - (double)ldt(in.target, r * in.n_cols + in.cols[p], in.target_dtype);
}

// fixed tree over the workgroup's threads; the results are in every thread
__device__ __forceinline__ void sml_tree(double (*sa)[SML_THREADS], long long *sc, int planes, double *a, long long &c) {
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < SML_PLANES; ++p)
        if (p < planes) sa[p][t] = a[p];
    sc[t] = c;
    __syncthreads();
    for (int s = SML_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int p = 0; p < planes; ++p) sa[p][t] += sa[p][t + s];
            sc[t] += sc[t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < SML_PLANES; ++p)
        if (p < planes) a[p] = sa[p][0];
    c = sc[0];
    __syncthreads();
}

__global__ void __launch_bounds__(SML_THREADS)
k_sml_forward(SmlIn in, long long n_chunks, unsigned *__restrict__ ticket, double *__restrict__ part,
              float *__restrict__ out, long long *__restrict__ count) {
    __shared__ double sa[SML_PLANES][SML_THREADS];
    __shared__ long long sc[SML_THREADS];
    const long long nv = wfs_valid_rows_nonneg(in.n_cap, in.n_dev);
    const int t = threadIdx.x, planes = in.planes, stride = planes + 1;
    for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        double a[SML_PLANES] = {0.0, 0.0, 0.0, 0.0};
        long long c = 0;
#pragma unroll
        for (int j = 0; j < SML_ROWS; ++j) {
            const long long r = ch * SML_CHUNK + (long long)j * SML_THREADS + t;
            if (r >= nv) continue;
            int e;
            const int cell = sml_cell(in, r, e);
            if (cell < 0) continue;
#pragma unroll
            for (int p = 0; p < SML_PLANES; ++p) {
                if (p < planes) {
                    const double d = sml_diff(in, r, e, cell, p);
                    a[p] += in.kind == WFS_LOSS_L1 ? fabs(d) : d * d;
                }
            }
            ++c;
        }
        sml_tree(sa, sc, planes, a, c);
        if (t == 0) {
#pragma unroll
            for (int p = 0; p < SML_PLANES; ++p)
                if (p < planes) part[ch * stride + p] = a[p];
            reinterpret_cast<long long *>(part)[ch * stride + planes] = c;
        }
    }
    // hand-off: the chunk stores drain, one agent-scope release, then the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sc[0] = drawn == gridDim.x - 1 ? 1 : 0;
        if (sc[0]) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    const bool last = sc[0] != 0;
    __syncthreads();
    if (!last) return;
    double a[SML_PLANES] = {0.0, 0.0, 0.0, 0.0};
    long long c = 0;
    for (long long ch = t; ch < n_chunks; ch += SML_THREADS) {
#pragma unroll
        for (int p = 0; p < SML_PLANES; ++p)
            if (p < planes) a[p] += part[ch * stride + p];
        c += reinterpret_cast<const long long *>(part)[ch * stride + planes];
    }
    sml_tree(sa, sc, planes, a, c);
    if (t == 0) {
        double total = 0.0;
#pragma unroll
        for (int p = 0; p < SML_PLANES; ++p) {
            if (p < planes) {
                const double v = a[p] / (double)c;  // no row counted: 0 / 0 = NaN
                out[p] = (float)v;
                total += v;
            }
        }
        out[planes] = (float)total;
        *count = c;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the first row at or above `from` (below nv) whose event is >= e; every lane of the wavefront walks the same path
__device__ __forceinline__ long long sml_lower(const int *coords, long long from, long long nv, long long e) {
    long long lo = from, hi = nv;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (coords[mid * 3 + 2] < e) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the value a counted row leaves in its cell of plane p
__device__ __forceinline__ float sml_grad(const SmlIn &in, long long r, int e, int cell, int p, double g_over_count) {
    const double d = sml_diff(in, r, e, cell, p);
    const double s = in.kind == WFS_LOSS_L1 ? (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : (d == d ? 0.0 : d))) : 2.0 * d;
    return (float)(g_over_count * s);
}

// T: the map's element type.  The tile is laid out as dmap is: [event of the workgroup][plane][cell].
template <typename T>
__global__ void __launch_bounds__(SML_THREADS)
k_sml_backward(SmlIn in, const long long *__restrict__ count, const float *__restrict__ grad, T *__restrict__ dmap) {
    __shared__ __attribute__((aligned(16))) float tile[SML_EVENTS * SML_PLANES * SML_CELLS];
    __shared__ int owner[SML_EVENTS * SML_CELLS];
    __shared__ int dup[SML_EVENTS];
    const int t = threadIdx.x, w = t / WFS_WAVE, lane = t % WFS_WAVE;
    const int planes = in.planes, cells = in.nx * in.ny;
    const long long e0 = (long long)blockIdx.x * SML_EVENTS;
    const int n_ev = (int)(in.B - e0 < SML_EVENTS ? in.B - e0 : SML_EVENTS);
    const int n_el = n_ev * planes * cells;   // elements of dmap this workgroup writes
    for (int i = t; i < n_el; i += SML_THREADS) tile[i] = 0.f;
    for (int i = t; i < SML_EVENTS * cells; i += SML_THREADS) owner[i] = 0x7fffffff;
    if (t < SML_EVENTS) dup[t] = 0;
    const long long cnt = *count;
    const long long nv = cnt > 0 ? wfs_valid_rows_nonneg(in.n_cap, in.n_dev) : 0;
    const long long e = e0 + w;
    long long lo = 0, hi = 0;
    if (w < n_ev && nv > 0) {
        lo = sml_lower(in.coords, 0, nv, e);
        hi = sml_lower(in.coords, lo, nv, e + 1);
    }
    const double g_over_count = cnt > 0 ? (double)*grad / (double)cnt : 0.0;
    __syncthreads();
    // the first counted row of a cell owns it
    for (long long r = lo + lane; r < hi; r += WFS_WAVE) {
        int re;
        const int cell = sml_cell(in, r, re);
        if (cell >= 0 && re == e) atomicMin(&owner[w * cells + cell], (int)(r - lo));
    }
    __syncthreads();
    for (long long r = lo + lane; r < hi; r += WFS_WAVE) {
        int re;
        const int cell = sml_cell(in, r, re);
        if (cell < 0 || re != e) continue;
        if (owner[w * cells + cell] == (int)(r - lo)) {
            for (int p = 0; p < planes; ++p) tile[(w * planes + p) * cells + cell] = sml_grad(in, r, re, cell, p, g_over_count);
        } else {
            dup[w] = 1;                       // a later row of a cell that has an owner: a duplicated segment
        }
    }
    __syncthreads();
    if (dup[w]) {
        // duplicated segments: the cell's lane sums its rows' values in row order
        for (int cell = lane; cell < cells; cell += WFS_WAVE) {
            const int first = owner[w * cells + cell];
            if (first == 0x7fffffff) continue;
            double sum[SML_PLANES] = {0.0, 0.0, 0.0, 0.0};
            for (long long r = lo + first; r < hi; ++r) {
                int re;
                if (sml_cell(in, r, re) != cell || re != e) continue;
#pragma unroll
                for (int p = 0; p < SML_PLANES; ++p)
                    if (p < planes) sum[p] += (double)sml_grad(in, r, re, cell, p, g_over_count);
            }
#pragma unroll
            for (int p = 0; p < SML_PLANES; ++p)
                if (p < planes) tile[(w * planes + p) * cells + cell] = (float)sum[p];
        }
    }
    __syncthreads();
    // the tile goes out as it lies: 16-byte lanes where the workgroup's span of dmap is a multiple of 16 bytes
    T *dst = dmap + e0 * planes * cells;
    constexpr int PER = 16 / (int)sizeof(T);
    if (((long long)SML_EVENTS * planes * cells) % PER == 0 && n_el % PER == 0) {
        for (int i = t; i < n_el / PER; i += SML_THREADS) {
            const float4 a = reinterpret_cast<const float4 *>(tile)[i * (PER / 4)];
            if constexpr (std::is_same<T, float>::value) {
                reinterpret_cast<float4 *>(dst)[i] = a;
            } else {
                const float4 b = reinterpret_cast<const float4 *>(tile)[i * 2 + 1];
                uint4 v;
                v.x = wfs_pack2<T>(a.x, a.y), v.y = wfs_pack2<T>(a.z, a.w);
                v.z = wfs_pack2<T>(b.x, b.y), v.w = wfs_pack2<T>(b.z, b.w);
                reinterpret_cast<uint4 *>(dst)[i] = v;
            }
        }
    } else {
        for (int i = t; i < n_el; i += SML_THREADS) wfs_st(dst + i, tile[i]);
    }
}

bool sml_args(const void *map, int32_t map_dtype, int64_t B, int32_t planes, int32_t nx, int32_t ny, const int32_t *coords,
              const void *target, int32_t target_dtype, int32_t n_cols, const int32_t *cols, const float *se_mask,
              int64_t n_cap, const int64_t *n_dev, int32_t kind, SmlIn *in) {
    if (!wfs_dtype_ok(map_dtype) || !wfs_dtype_ok(target_dtype) || planes < 1 || planes > SML_PLANES || !cols) return false;
    if (n_cols < 1 || nx < 1 || ny < 1 || (long long)nx * ny > SML_CELLS || B < 0 || B >= (1ll << 31)) return false;
    if (n_cap < 0 || n_cap >= (1ll << 31) || (kind != WFS_LOSS_L1 && kind != WFS_LOSS_MSE)) return false;
    if (n_cap > 0 && (!coords || !target)) return false;
    if (B > 0 && !map) return false;
    *in = SmlIn{map, target, coords, se_mask, (const long long *)n_dev, n_cap, B, map_dtype, target_dtype, n_cols, planes, nx,
                ny, kind, {0, 0, 0, 0}};
    for (int p = 0; p < planes; ++p) {
        if (cols[p] < 0 || cols[p] >= n_cols) return false;
        in->cols[p] = cols[p];
    }
    return true;
}

}  // namespace

extern "C" size_t wfs_segment_map_loss_workspace_bytes(int64_t n_cap, int32_t planes) {
    if (n_cap < 0 || planes < 1 || planes > SML_PLANES) return 0;
    return (size_t)SML_HEAD + (size_t)(n_cap > 0 ? wfs_cdiv(n_cap, SML_CHUNK) : 1) * (planes + 1) * sizeof(double);
}

#define SML_ARGS_MESSAGE(name)                                                                                    \
    name ": dtypes %d / %d, map [%lld, %d, %d, %d] (at most %d planes, %d cells), %d columns, n_cap = %lld, kind %d", \
        map_dtype, target_dtype, (long long)B, planes, nx, ny, SML_PLANES, SML_CELLS, n_cols, (long long)n_cap, kind

extern "C" int wfs_segment_map_loss(const void *map, int32_t map_dtype, int64_t B, int32_t planes, int32_t nx, int32_t ny,
                                    const int32_t *coords, const void *target, int32_t target_dtype, int32_t n_cols,
                                    const int32_t *cols, const float *se_mask, int64_t n_cap, const int64_t *n_dev,
                                    int32_t kind, int32_t max_blocks, void *workspace, size_t workspace_bytes, float *out,
                                    int64_t *count, void *stream) {
    SmlIn in;
    WFS_REQUIRE(sml_args(map, map_dtype, B, planes, nx, ny, coords, target, target_dtype, n_cols, cols, se_mask, n_cap, n_dev,
                         kind, &in),
                WFS_EINVAL, SML_ARGS_MESSAGE("wfs_segment_map_loss"));
    WFS_REQUIRE(workspace && out && count && max_blocks >= 0, WFS_EINVAL, "wfs_segment_map_loss: NULL argument");
    WFS_REQUIRE(workspace_bytes >= wfs_segment_map_loss_workspace_bytes(n_cap, planes), WFS_EWORKSPACE,
                "wfs_segment_map_loss: workspace of %zu bytes, %zu needed", workspace_bytes,
                wfs_segment_map_loss_workspace_bytes(n_cap, planes));
    const long long n_chunks = wfs_cdiv(n_cap, SML_CHUNK);       // 0 rows: no chunk, the fold writes NaN and count 0
    long long blocks = n_chunks < 1 ? 1 : n_chunks;
    const long long cap = max_blocks > 0 ? max_blocks : SML_MAX_BLOCKS;
    if (blocks > cap) blocks = cap;
    k_sml_forward<<<(unsigned)blocks, SML_THREADS, 0, (hipStream_t)stream>>>(
        in, n_chunks, (unsigned *)workspace, (double *)((char *)workspace + SML_HEAD), out, (long long *)count);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_segment_map_loss_backward(const void *map, int32_t map_dtype, int64_t B, int32_t planes, int32_t nx,
                                             int32_t ny, const int32_t *coords, const void *target, int32_t target_dtype,
                                             int32_t n_cols, const int32_t *cols, const float *se_mask, int64_t n_cap,
                                             const int64_t *n_dev, int32_t kind, const int64_t *count, const float *grad,
                                             void *dmap, void *stream) {
    SmlIn in;
    WFS_REQUIRE(sml_args(map, map_dtype, B, planes, nx, ny, coords, target, target_dtype, n_cols, cols, se_mask, n_cap, n_dev,
                         kind, &in),
                WFS_EINVAL, SML_ARGS_MESSAGE("wfs_segment_map_loss_backward"));
    WFS_REQUIRE(count && grad && (B == 0 || dmap), WFS_EINVAL, "wfs_segment_map_loss_backward: NULL argument");
    WFS_REQUIRE(((uintptr_t)dmap & 15) == 0, WFS_EINVAL, "wfs_segment_map_loss_backward: dmap must be 16-byte aligned");
    if (B == 0) return WFS_OK;
    const unsigned blocks = (unsigned)wfs_cdiv(B, SML_EVENTS);
    return wfs_with_dtype(map_dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_sml_backward<T><<<blocks, SML_THREADS, 0, (hipStream_t)stream>>>(in, (const long long *)count, grad, (T *)dmap);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}
