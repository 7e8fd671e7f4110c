// segloss.hip -- the two fused regression losses of the captured training step, both on the fold of wfs_lossfold.h (one
// forward launch, fp64 sums, no floating-point atomic: the result repeats bit for bit and does not depend on the grid).
//
// Masked regression loss (the reference's LitSegQuantifier): the mean of |d| (L1) or d^2 (MSE), d = pred - target[:, col],
// over the rows below the valid count that lie on a single-ended segment (when a mask is given), with the mean of d^2 over
// the same rows beside it.
//
//   k_mrl_forward    ONE launch: the fold over (sum of terms, sum of squares); writes loss, mse and the count.
//   k_mrl_backward   ONE launch, one thread per row: dpred = g * s / count in pred's type, s = sign(d) (sign(0) = 0) or 2 d.
//
// A row that is not counted is SELECTED out: none of its values is loaded into the arithmetic (beyond the valid count not
// even its coordinates), so a NaN, an Inf or the captured step's padding value there cannot reach the loss, and its
// gradient is a stored 0.  With no row counted the loss is NaN (0 / 0, torch's mean over nothing) and dpred is all zeros.
//
// Segment map loss (LitZ / LitEZ, the reference's LitBase._calc_segment_loss): a dense prediction map [B, planes, nx, ny]
// scored against the targets of the ACTIVE segments only, sum-reduced criterion divided by the number of rows.  A row of
// coords = (x, y, event) is COUNTED when it lies below the valid count, inside [nx, ny, B] and (with a mask) on a segment
// whose mask entry is 1.0.  For a counted row and plane p: d = map[event, p, x, y] - target[row, cols[p]].
//
//   k_sml_forward    ONE launch: the fold over the per-plane sums; writes out[0 .. planes - 1] = sum / count,
//                    out[planes] = their fp64 sum rounded once, and the count.  The result does not depend on B either.
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
// Here too a row that is not counted is selected out, and no map cell outside the counted rows is loaded into the
// arithmetic.  With no row counted the losses are NaN (0 / 0) and dmap is all zeros.
#include "wfs_common.h"
#include "wfs_lossfold.h"
#include "wfs_rows.h"                         // ldt / stt: rows of a runtime dtype

namespace {

// ---- masked regression loss ------------------------------------------------------------------------------------------
struct MrlIn {
    const void *pred, *target;
    const int *coords;
    const float *mask;                        // [nx, ny] or NULL
    const long long *n_dev;
    long long n_cap;
    int pred_dtype, target_dtype, n_cols, col, nx, ny, kind;
};

// row r (below the valid count) is counted: on a single-ended segment when there is a mask
__device__ __forceinline__ bool mrl_counted(const MrlIn &in, long long r) {
    if (!in.mask) return true;
    const int x = in.coords[r * 3], y = in.coords[r * 3 + 1];
    return x >= 0 && x < in.nx && y >= 0 && y < in.ny && in.mask[x * in.ny + y] == 1.0f;
}

__device__ __forceinline__ double mrl_diff(const MrlIn &in, long long r) {
    return (double)ldt(in.pred, r, in.pred_dtype) - (double)ldt(in.target, r * in.n_cols + in.col, in.target_dtype);
}

__global__ void __launch_bounds__(LF_THREADS)
k_mrl_forward(MrlIn in, long long n_chunks, unsigned *__restrict__ ticket, double *__restrict__ part,
              float *__restrict__ out, long long *__restrict__ count) {
    lossfold_forward<2>(
        2, wfs_valid_rows_nonneg(in.n_cap, in.n_dev), n_chunks, ticket, part,
        [&](long long r, double *a) {
            if (!mrl_counted(in, r)) return false;
            const double d = mrl_diff(in, r);
            const double q = d * d;           // formed once: both sums take the same rounded product
            a[0] += in.kind == WFS_LOSS_L1 ? fabs(d) : q;
            a[1] += q;
            return true;
        },
        [&](const double *a, long long c) {
            out[0] = (float)(a[0] / (double)c);   // no row counted: 0 / 0 = NaN
            out[1] = (float)(a[1] / (double)c);
            *count = c;
        });
}

__global__ void __launch_bounds__(LF_THREADS)
k_mrl_backward(MrlIn in, const long long *__restrict__ count, const float *__restrict__ grad, void *__restrict__ dpred) {
    const long long r = (long long)blockIdx.x * LF_THREADS + threadIdx.x;
    if (r >= in.n_cap) return;
    const long long nv = wfs_valid_rows_nonneg(in.n_cap, in.n_dev), cnt = *count;
    float v = 0.f;
    if (cnt > 0 && r < nv && mrl_counted(in, r))
        v = (float)((double)*grad * lossfold_sign(in.kind, mrl_diff(in, r)) / (double)cnt);
    stt(dpred, r, in.pred_dtype, v);
}

bool mrl_args(const void *pred, int32_t pred_dtype, const void *target, int32_t target_dtype, int32_t n_cols, int32_t col,
              const int32_t *coords, const float *se_mask, int32_t nx, int32_t ny, int64_t n_cap, const int64_t *n_dev,
              int32_t kind, MrlIn *in) {
    if (!wfs_dtype_ok(pred_dtype) || !wfs_dtype_ok(target_dtype) || n_cols < 1 || col < 0 || col >= n_cols) return false;
    if (n_cap < 0 || n_cap >= (1ll << 31) || (kind != WFS_LOSS_L1 && kind != WFS_LOSS_MSE)) return false;
    if (n_cap > 0 && (!pred || !target)) return false;
    if (se_mask && (!coords || nx < 1 || ny < 1)) return false;
    *in = MrlIn{pred, target, coords, se_mask, (const long long *)n_dev, n_cap, pred_dtype, target_dtype, n_cols, col, nx, ny,
                kind};
    return true;
}

// ---- segment map loss ------------------------------------------------------------------------------------------------
constexpr int SML_THREADS = LF_THREADS;
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

__global__ void __launch_bounds__(SML_THREADS)
k_sml_forward(SmlIn in, long long n_chunks, unsigned *__restrict__ ticket, double *__restrict__ part,
              float *__restrict__ out, long long *__restrict__ count) {
    const int planes = in.planes;
    lossfold_forward<SML_PLANES>(
        planes, wfs_valid_rows_nonneg(in.n_cap, in.n_dev), n_chunks, ticket, part,
        [&](long long r, double *a) {
            int e;
            const int cell = sml_cell(in, r, e);
            if (cell < 0) return false;
#pragma unroll
            for (int p = 0; p < SML_PLANES; ++p)
                if (p < planes) a[p] += lossfold_term(in.kind, sml_diff(in, r, e, cell, p));
            return true;
        },
        [&](const double *a, long long c) {
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
        });
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
    return (float)(g_over_count * lossfold_sign(in.kind, sml_diff(in, r, e, cell, p)));
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

extern "C" size_t wfs_masked_regression_loss_workspace_bytes(int64_t n_cap) {
    return n_cap < 0 ? 0 : lossfold_workspace_bytes(n_cap, 2);
}

#define MRL_ARGS_MESSAGE(name)                                                                                        \
    name ": dtypes %d / %d, column %d of %d, n_cap = %lld, kind %d, mask %d x %d", pred_dtype, target_dtype, col, n_cols, \
        (long long)n_cap, kind, nx, ny

extern "C" int wfs_masked_regression_loss(const void *pred, int32_t pred_dtype, const void *target, int32_t target_dtype,
                                          int32_t n_cols, int32_t col, const int32_t *coords, const float *se_mask,
                                          int32_t nx, int32_t ny, int64_t n_cap, const int64_t *n_dev, int32_t kind,
                                          int32_t max_blocks, void *workspace, size_t workspace_bytes, float *out,
                                          int64_t *count, void *stream) {
    MrlIn in;
    WFS_REQUIRE(mrl_args(pred, pred_dtype, target, target_dtype, n_cols, col, coords, se_mask, nx, ny, n_cap, n_dev, kind,
                         &in),
                WFS_EINVAL, MRL_ARGS_MESSAGE("wfs_masked_regression_loss"));
    WFS_REQUIRE(workspace && out && count && max_blocks >= 0, WFS_EINVAL, "wfs_masked_regression_loss: NULL argument");
    WFS_REQUIRE(workspace_bytes >= wfs_masked_regression_loss_workspace_bytes(n_cap), WFS_EWORKSPACE,
                "wfs_masked_regression_loss: workspace of %zu bytes, %zu needed", workspace_bytes,
                wfs_masked_regression_loss_workspace_bytes(n_cap));
    const LossfoldGrid g = lossfold_grid(n_cap, max_blocks);
    k_mrl_forward<<<g.blocks, LF_THREADS, 0, (hipStream_t)stream>>>(
        in, g.n_chunks, (unsigned *)workspace, (double *)((char *)workspace + LF_HEAD), out, (long long *)count);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_masked_regression_loss_backward(const void *pred, int32_t pred_dtype, const void *target,
                                                   int32_t target_dtype, int32_t n_cols, int32_t col,
                                                   const int32_t *coords, const float *se_mask, int32_t nx, int32_t ny,
                                                   int64_t n_cap, const int64_t *n_dev, int32_t kind,
                                                   const int64_t *count, const float *grad, void *dpred, void *stream) {
    MrlIn in;
    WFS_REQUIRE(mrl_args(pred, pred_dtype, target, target_dtype, n_cols, col, coords, se_mask, nx, ny, n_cap, n_dev, kind,
                         &in),
                WFS_EINVAL, MRL_ARGS_MESSAGE("wfs_masked_regression_loss_backward"));
    WFS_REQUIRE(count && grad && (n_cap == 0 || dpred), WFS_EINVAL, "wfs_masked_regression_loss_backward: NULL argument");
    if (n_cap == 0) return WFS_OK;
    k_mrl_backward<<<(unsigned)wfs_cdiv(n_cap, LF_THREADS), LF_THREADS, 0, (hipStream_t)stream>>>(
        in, (const long long *)count, grad, dpred);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" size_t wfs_segment_map_loss_workspace_bytes(int64_t n_cap, int32_t planes) {
    return n_cap < 0 || planes < 1 || planes > SML_PLANES ? 0 : lossfold_workspace_bytes(n_cap, planes);
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
    const LossfoldGrid g = lossfold_grid(n_cap, max_blocks);
    k_sml_forward<<<g.blocks, SML_THREADS, 0, (hipStream_t)stream>>>(
        in, g.n_chunks, (unsigned *)workspace, (double *)((char *)workspace + LF_HEAD), out, (long long *)count);
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
