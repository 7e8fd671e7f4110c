// voxelize.hip -- the hybrid 3-D net's hand-over from waveform rows to voxels, on the device.
//
// The 3-D PSD nets take one voxel per (segment, sample) where either PMT saw something (the reference's 3-D datasets are
// voxelised offline: PulseDataset3D over *Waveform3DPairSim.h5, src/datasets/PulseDataset.py:543-625).  The hybrid form
// (BASELINE configs[4]: feat [n, 1, 2T] -> TCN -> voxelise -> SubM3d head) puts the TCN in front, so the voxels have to be
// cut out of the TCN's output rows inside the step:
//
//   sample t of row r is ACTIVE iff rows[r][t] > thr || rows[r][T + t] > thr     (the RAW input rows: the voxel set does
//                                                                                not depend on the weights)
//   voxel v = (r, t), numbered row-major, t ascending:  indices[v] = (evt, x, y, t),  feats[v] = (Y[r][t], Y[r][T + t])
//
//   k_vox_count   one wave per 64-sample SLICE of a row (S = ceil(T / 64) slices per row): __ballot of the activity,
//                 popcount -> the slice's count.  (One wave walking a whole row was latency-bound: 16 dependent
//                 load-ballot steps per wave at T = 1024 took 12.5 us for 787 rows.)
//   k_vox_scan    ONE block: exclusive prefix over the slices' counts (in place), the voxel count, the sticky overflow
//                 flag, and the voxel-level event table (wfs_event_offsets format, from the offsets of each event's first
//                 row)
//   k_vox_emit    one wave per slice again: the same ballot, v = slice offset + mbcnt(ballot) -> 16-byte index store and
//                 one feature pair per active lane.  Deterministic: no atomic anywhere, the order is the rows' order.
//   k_vox_bwd     one block per row up to the CAPACITY: the row's voxels' gradients are placed into an LDS copy of the row
//                 (zeros elsewhere), which is then written whole with 16-byte stores.  Rows without voxels -- padding rows
//                 included -- are written as exact zeros (the TCN backward sums tap partials over every row it is given).
#include "wfs_common.h"

namespace {

constexpr int VB = 256;             // 4 waves per block, one 64-sample slice per wave (count / emit)
constexpr int VSCAN = 1024;         // the prefix block
constexpr int VSEG = 16;            // slices per prefix thread held in registers (12.6 k slices at 256 events, T = 1024)


template <typename T>
__device__ __forceinline__ bool active(const T *row, int T_, int t, float thr) {
    return t < T_ && (wfs_ld(row + t) > thr || wfs_ld(row + T_ + t) > thr);
}

template <typename T>
__global__ void __launch_bounds__(VB) k_vox_count(const T *__restrict__ rows, long long n_cap, int T_,
                                                   const long long *__restrict__ n_dev, float thr, int *__restrict__ off) {
    const long long w = (long long)blockIdx.x * (VB / WFS_WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int S = (T_ + WFS_WAVE - 1) / WFS_WAVE;
    const long long r = w / S;
    if (r >= n_cap) return;
    int cnt = 0;
    if (r < wfs_valid_rows(n_cap, n_dev))
        cnt = __popcll(__ballot(active(rows + r * 2 * T_, T_, (int)(w - r * S) * WFS_WAVE + lane, thr)));
    if (lane == 0) off[w] = cnt;          // rows beyond the valid count: no voxels, whatever they hold
}

// exclusive prefix of off[0 .. n_cap S) in place, off[n_cap S] = V (the true total), *v_dev = min(V, V_cap), sticky
// overflow; the event table ev[0 .. B] (+ WFS_EVENT_FLAG_WORDS flag words) of the voxels when ev != NULL
__global__ void __launch_bounds__(VSCAN) k_vox_scan(int *__restrict__ off, long long n_cap, int S,
                                                    const int *__restrict__ coords,
                                                    const long long *__restrict__ n_dev, int B, long long V_cap,
                                                    long long *__restrict__ v_dev, int *__restrict__ overflow,
                                                    int *__restrict__ ev) {
    __shared__ long long wsum[VSCAN / WFS_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long n_off = n_cap * S;
    const long long per = (n_off + VSCAN - 1) / VSCAN;
    const long long j0 = tid * per < n_off ? tid * per : n_off, j1 = j0 + per < n_off ? j0 + per : n_off;
    // a thread's counts are loaded back to back into registers when they fit (one memory latency, not `per` of them)
    const bool in_regs = per <= VSEG;
    int cnts[VSEG];
    long long own = 0;
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < VSEG; ++k) cnts[k] = j0 + k < j1 ? off[j0 + k] : 0;
#pragma unroll
        for (int k = 0; k < VSEG; ++k) own += cnts[k];
    } else {
        for (long long j = j0; j < j1; ++j) own += off[j];
    }
    // block-wide exclusive scan of the per-thread sums: inside the wave by shuffles, then over the 16 wave totals
    long long inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < VSCAN / WFS_WAVE; ++w) {
        before += w < wid ? wsum[w] : 0;
        total += wsum[w];
    }
    long long run = before + inc - own;
    const long long nv = wfs_valid_rows(n_cap, n_dev);
    const long long vc = total < V_cap ? total : V_cap;
    int bad = 0;
    // slice j = (row r, slice c of the row): r and c are stepped, not divided out per slice
    long long r = j0 / S;
    int c = (int)(j0 - r * S);
    auto visit = [&](long long j, long long cnt) {
        off[j] = (int)run;
        if (ev && c == 0 && r < nv) {
            // the event table of the voxels from the rows': event e starts at the first voxel of its first row (rows of
            // one event are contiguous; an event without rows starts where the next one does)
            const int b = coords[r * 3 + 2];
            const int bp = r > 0 ? coords[(r - 1) * 3 + 2] : -1;
            const bool ok = b >= 0 && b < B && b >= bp && bp >= -1 && bp < B;
            bad |= ok ? 0 : 1;
            if (ok) {
                const int at = (int)(run < V_cap ? run : V_cap);
                for (int e = bp + 1; e <= b; ++e) ev[e] = at;
            }
        }
        run += cnt;
        if (++c == S) {
            c = 0;
            ++r;
        }
    };
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < VSEG; ++k)
            if (j0 + k < j1) visit(j0 + k, cnts[k]);
    } else {
        for (long long j = j0; j < j1; ++j) visit(j, off[j]);
    }
    bad = __syncthreads_or(bad);
    if (ev) {
        // events after the last valid row's start at the voxel count -- filled by the whole block (B may be the row
        // capacity when the caller only knows an upper bound on the events)
        const int bl = nv > 0 ? coords[(nv - 1) * 3 + 2] : -1;
        if (bl >= -1 && bl < B)
            for (int e = bl + 1 + tid; e <= B; e += VSCAN) ev[e] = nv > 0 ? (int)vc : 0;
        if (tid < WFS_EVENT_FLAG_WORDS) ev[B + 1 + tid] = tid == 0 ? bad : 0;
    }
    if (tid == 0) {
        off[n_off] = (int)total;
        *v_dev = vc;
        if (total > V_cap) *overflow = 1;         // sticky: set, never cleared here
    }
}

template <typename T>
__device__ __forceinline__ void store_pair(T *f, long long v, const T *y, int t, int T_) {
    wfs_st(f + 2 * v, wfs_ld(y + t));
    wfs_st(f + 2 * v + 1, wfs_ld(y + T_ + t));
}
template <>
__device__ __forceinline__ void store_pair<float>(float *f, long long v, const float *y, int t, int T_) {
    *reinterpret_cast<float2 *>(f + 2 * v) = make_float2(y[t], y[T_ + t]);
}
template <>
__device__ __forceinline__ void store_pair<wfs_bf16>(wfs_bf16 *f, long long v, const wfs_bf16 *y, int t, int T_) {
    *reinterpret_cast<unsigned *>(f + 2 * v) = (unsigned)y[t] | ((unsigned)y[T_ + t] << 16);
}
template <>
__device__ __forceinline__ void store_pair<wfs_f16>(wfs_f16 *f, long long v, const wfs_f16 *y, int t, int T_) {
    *reinterpret_cast<unsigned *>(f + 2 * v) = (unsigned)y[t].bits | ((unsigned)y[T_ + t].bits << 16);
}

template <typename T>
__global__ void __launch_bounds__(VB) k_vox_emit(const T *__restrict__ rows, const T *__restrict__ vals,
                                                  const int *__restrict__ coords, long long n_cap, int T_, float thr,
                                                  const int *__restrict__ off, long long V_cap, int4 *__restrict__ idx,
                                                  T *__restrict__ feat) {
    const long long w = (long long)blockIdx.x * (VB / WFS_WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int S = (T_ + WFS_WAVE - 1) / WFS_WAVE;
    const long long r = w / S;
    if (r >= n_cap) return;
    const long long base = off[w];
    long long end = off[w + 1];           // the plan's count of this slice (0 for rows beyond the valid count)
    end = end < V_cap ? end : V_cap;      // voxels beyond the capacity are not written
    if (base >= end) return;
    const T *row = rows + r * 2 * T_;
    const int t = (int)(w - r * S) * WFS_WAVE + lane;
    const bool a = active(row, T_, t, thr);
    const unsigned long long m = __ballot(a);
    const long long v = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (a && v < end) {
        idx[v] = make_int4(coords[r * 3 + 2], coords[r * 3], coords[r * 3 + 1], t);
        store_pair(feat, v, vals + r * 2 * T_, t, T_);
    }
}

// U: the store unit (uint4 / unsigned / unsigned short), chosen by the host from the row's byte length and dY's alignment
template <typename T, typename U>
__global__ void __launch_bounds__(VB) k_vox_bwd(const T *__restrict__ dfeat, const int4 *__restrict__ idx,
                                                 const int *__restrict__ off, int T_, long long V_cap, T *__restrict__ dY) {
    extern __shared__ uint4 lds_row[];
    const long long r = blockIdx.x;
    const int tid = threadIdx.x;
    const int units = (int)((2 * T_ * sizeof(T)) / sizeof(U));
    U *dst = reinterpret_cast<U *>(dY + r * 2 * T_);
    const int S = (T_ + WFS_WAVE - 1) / WFS_WAVE;
    long long lo = off[r * S], hi = off[(r + 1) * S];
    hi = hi < V_cap ? hi : V_cap;
    const U zero = U();
    if (lo >= hi) {                        // no voxel in this row (padding rows included): exact zeros
        for (int i = tid; i < units; i += VB) dst[i] = zero;
        return;
    }
    U *buf = reinterpret_cast<U *>(lds_row);
    for (int i = tid; i < units; i += VB) buf[i] = zero;
    __syncthreads();
    T *row = reinterpret_cast<T *>(lds_row);
    for (long long v = lo + tid; v < hi; v += VB) {
        const int t = idx[v].w;
        if (t >= 0 && t < T_) {
            row[t] = dfeat[2 * v];
            row[T_ + t] = dfeat[2 * v + 1];
        }
    }
    __syncthreads();
    for (int i = tid; i < units; i += VB) dst[i] = buf[i];
}

template <typename T>
int launch_bwd(const void *dfeat, const int32_t *indices, const int32_t *off, int64_t n_cap, int32_t T_, int64_t V_cap,
               void *dY, hipStream_t stream) {
    const size_t bytes = (size_t)2 * T_ * sizeof(T);
    const size_t lds = wfs_align_up(bytes, 16);
    const dim3 grid((unsigned)n_cap), block(VB);
    const uintptr_t a = (uintptr_t)dY | (uintptr_t)bytes;
    if (a % 16 == 0)
        k_vox_bwd<T, uint4><<<grid, block, lds, stream>>>((const T *)dfeat, (const int4 *)indices, off, T_, V_cap, (T *)dY);
    else if (a % 4 == 0)
        k_vox_bwd<T, unsigned><<<grid, block, lds, stream>>>((const T *)dfeat, (const int4 *)indices, off, T_, V_cap,
                                                             (T *)dY);
    else
        k_vox_bwd<T, unsigned short><<<grid, block, lds, stream>>>((const T *)dfeat, (const int4 *)indices, off, T_, V_cap,
                                                                   (T *)dY);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

}  // namespace

extern "C" size_t wfs_voxelize_offsets_ints(int64_t n_cap, int32_t T_) {
    return (size_t)(n_cap > 0 ? n_cap : 0) * (size_t)wfs_cdiv(T_ > 0 ? T_ : 1, WFS_WAVE) + 1;
}

static int vox_shape_ok(int64_t n_cap, int32_t T_, int32_t dtype) {
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    WFS_REQUIRE(T_ >= 1 && T_ <= WFS_VOXELIZE_MAX_SAMPLES, WFS_EINVAL, "%d samples per PMT not in [1, %d]", T_,
                WFS_VOXELIZE_MAX_SAMPLES);
    WFS_REQUIRE(n_cap >= 0 && n_cap * (int64_t)T_ < (1ll << 31) && n_cap < (1ll << 31) - 1, WFS_EINVAL,
                "%lld rows x %d samples: voxel numbers must fit int32", (long long)n_cap, T_);
    return WFS_OK;
}

extern "C" int wfs_voxelize_plan(const void *rows, const int32_t *coords, int64_t n_cap, int32_t T_, const int64_t *n_dev,
                                 float threshold, int32_t batch_size, int64_t V_cap, int32_t *row_offsets, int64_t *v_dev,
                                 int32_t *event_offsets, int32_t *overflow_dev, int32_t dtype, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = vox_shape_ok(n_cap, T_, dtype);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(V_cap >= 0 && V_cap < (1ll << 31), WFS_EINVAL, "voxel capacity %lld not in [0, 2^31)", (long long)V_cap);
    WFS_REQUIRE(row_offsets && v_dev && overflow_dev && (rows || n_cap == 0), WFS_EINVAL, "NULL device pointer");
    WFS_REQUIRE(!event_offsets || (coords && batch_size >= 1), WFS_EINVAL, "the event table needs coords and batch_size >= 1");
    const long long *nd = (const long long *)n_dev;
    if (n_cap > 0) {
        const dim3 grid((unsigned)wfs_cdiv(n_cap * wfs_cdiv(T_, WFS_WAVE), VB / WFS_WAVE)), block(VB);
        const int rc_count = wfs_with_dtype(dtype, [&](auto t) -> int {
            using T = decltype(t);
            k_vox_count<T><<<grid, block, 0, stream>>>((const T *)rows, n_cap, T_, nd, threshold, row_offsets);
            WFS_LAUNCH_CHECK();
            return WFS_OK;
        });
        if (rc_count != WFS_OK) return rc_count;
    }
    k_vox_scan<<<dim3(1), dim3(VSCAN), 0, stream>>>(row_offsets, n_cap, (int)wfs_cdiv(T_, WFS_WAVE), coords, nd, batch_size, V_cap,
                                                    (long long *)v_dev, overflow_dev, event_offsets);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_voxelize_emit(const void *rows, const void *values, const int32_t *coords, int64_t n_cap, int32_t T_,
                                 float threshold, const int32_t *row_offsets, int64_t V_cap, int32_t *indices, void *feats,
                                 int32_t dtype, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = vox_shape_ok(n_cap, T_, dtype);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(V_cap >= 0 && V_cap < (1ll << 31), WFS_EINVAL, "voxel capacity %lld not in [0, 2^31)", (long long)V_cap);
    if (n_cap == 0 || V_cap == 0) return WFS_OK;
    WFS_REQUIRE(rows && values && coords && row_offsets && indices && feats, WFS_EINVAL, "NULL device pointer");
    WFS_REQUIRE((uintptr_t)indices % 16 == 0 && (uintptr_t)feats % (2 * wfs_dtype_bytes(dtype)) == 0, WFS_EINVAL,
                "indices must be 16-byte and feats pair aligned");
    const dim3 grid((unsigned)wfs_cdiv(n_cap * wfs_cdiv(T_, WFS_WAVE), VB / WFS_WAVE)), block(VB);
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_vox_emit<T><<<grid, block, 0, stream>>>((const T *)rows, (const T *)values, coords, n_cap, T_, threshold,
                                                  row_offsets, V_cap, (int4 *)indices, (T *)feats);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_voxelize_bwd(const void *dfeat, const int32_t *indices, const int32_t *row_offsets, int64_t n_cap,
                                int32_t T_, int64_t V_cap, void *dY, int32_t dtype, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = vox_shape_ok(n_cap, T_, dtype);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(V_cap >= 0 && V_cap < (1ll << 31), WFS_EINVAL, "voxel capacity %lld not in [0, 2^31)", (long long)V_cap);
    if (n_cap == 0) return WFS_OK;
    WFS_REQUIRE(row_offsets && dY && (V_cap == 0 || (dfeat && indices)), WFS_EINVAL, "NULL device pointer");
    WFS_REQUIRE((uintptr_t)indices % 16 == 0, WFS_EINVAL, "indices must be 16-byte aligned");
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        return launch_bwd<decltype(t)>(dfeat, indices, row_offsets, n_cap, T_, V_cap, dY, stream);
    });
}
