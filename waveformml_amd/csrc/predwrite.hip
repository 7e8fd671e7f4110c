// predwrite.hip -- the device half of the prediction writers (include/wfsparse.h "prediction writers"; reference
// src/datasets/PredictionWriter.py swap_values on src/utils/SparseUtils.py normalize_waveforms / swap_sparse_from_dense /
// swap_sparse_from_event, which walk a chunk row by row on the host).  A chunk's RAW compound records are on the device;
// wfs_predict_prepare cuts the net's input out of them, wfs_predict_scatter patches the net's output into them.  Both are
// memory-bound copies with awkward strides: records are 324 / 584 bytes, members start at any even offset, so every
// access to a record goes through ld32 / st32, which are one dword access when the call's layout is 4-byte friendly and
// two 16-bit accesses when it is not (decided once per call, a template parameter).
#include "wfs_common.h"

namespace {

constexpr int T = WFS_PREDICT_ROWS_PER_BLOCK;

template <bool A4>
__device__ __forceinline__ unsigned ld32(const unsigned char *p) {
    if (A4) return *reinterpret_cast<const unsigned *>(p);
    const unsigned short *h = reinterpret_cast<const unsigned short *>(p);
    return (unsigned)h[0] | ((unsigned)h[1] << 16);
}

template <bool A4>
__device__ __forceinline__ void st32(unsigned char *p, unsigned v) {
    if (A4) {
        *reinterpret_cast<unsigned *>(p) = v;
    } else {
        unsigned short *h = reinterpret_cast<unsigned short *>(p);
        h[0] = (unsigned short)(v & 0xFFFFu);
        h[1] = (unsigned short)(v >> 16);
    }
}

// change flag of a row: its event number differs from the previous row's; row 0 always starts an event
template <bool A4>
__device__ __forceinline__ int change_flag(const unsigned char *ev, long long row, long long item) {
    if (row == 0) return 1;
    return ld32<A4>(ev + row * item) != ld32<A4>(ev + (row - 1) * item) ? 1 : 0;
}

// launch 1: number of change flags of every block of T rows
template <bool A4>
__global__ void __launch_bounds__(T) k_pp_flags(const unsigned char *__restrict__ ev, long long n, long long item,
                                                int *__restrict__ block_sums) {
    const long long row = (long long)blockIdx.x * T + threadIdx.x;
    const int flag = row < n ? change_flag<A4>(ev, row, item) : 0;
    const int total = __syncthreads_count(flag);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// launch 2: coordinates.  Event of a row = (flags in the blocks before) + (flags up to the row inside the block) - 1:
// integer sums in a fixed order.  Blocks past the valid rows write the padding.
template <bool A4>
__global__ void __launch_bounds__(T) k_pp_coords(const unsigned char *__restrict__ rec, long long n, long long item,
                                                 long long coord_off, long long cap, const int *__restrict__ block_sums,
                                                 int *__restrict__ coords, long long *__restrict__ n_valid) {
    __shared__ int part[T / WFS_WAVE];
    __shared__ int base_s;
    const int t = threadIdx.x, lane = t & (WFS_WAVE - 1), wave = t / WFS_WAVE;
    const long long row = (long long)blockIdx.x * T + t;
    if (blockIdx.x == 0 && t == 0 && n_valid) *n_valid = n;
    if ((long long)blockIdx.x * T >= n) {                       // block-uniform: padding rows only
        if (row < cap) {
            coords[row * 3 + 0] = 0;
            coords[row * 3 + 1] = 0;
            coords[row * 3 + 2] = 0;
        }
        return;
    }
    int s = 0;
    for (int b = t; b < (int)blockIdx.x; b += T) s += block_sums[b];
    for (int d = WFS_WAVE / 2; d > 0; d >>= 1) s += __shfl_down(s, d, WFS_WAVE);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (t == 0) {
        int b = 0;
        for (int w = 0; w < T / WFS_WAVE; ++w) b += part[w];
        base_s = b;
    }
    __syncthreads();
    const int base = base_s;
    const unsigned char *p = rec + row * item + coord_off;
    const int flag = row < n ? change_flag<A4>(rec + coord_off + 8, row, item) : 0;
    const unsigned long long mask = __ballot(flag);
    const int in_wave = __popcll(mask & ((2ull << lane) - 1ull));           // inclusive
    __syncthreads();                                                        // part[] is reused
    if (lane == 0) part[wave] = __popcll(mask);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += part[w];
    if (row < n) {
        coords[row * 3 + 0] = (int)ld32<A4>(p);
        coords[row * 3 + 1] = (int)ld32<A4>(p + 4);
        coords[row * 3 + 2] = base + before + in_wave - 1;
    } else if (row < cap) {
        coords[row * 3 + 0] = 0;
        coords[row * 3 + 1] = 0;
        coords[row * 3 + 2] = 0;
    }
}

template <typename H>
__device__ __forceinline__ void store_pair(H *feats, long long pair, float a, float b) {
    reinterpret_cast<unsigned *>(feats)[pair] = wfs_pack2<H>(a, b);
}
template <>
__device__ __forceinline__ void store_pair<float>(float *feats, long long pair, float a, float b) {
    reinterpret_cast<float2 *>(feats)[pair] = float2{a, b};
}

// launch 3: features, one PAIR of neighbouring elements per thread (width is even, so pairs never straddle rows and
// consecutive threads store consecutive 8 / 4 bytes).  With an odd L = width / 2 the pair in the middle holds one
// element of either PMT side: the gain side is chosen per ELEMENT.
template <int KIND, bool A4, typename H>
__global__ void __launch_bounds__(256) k_pp_feats(const unsigned char *__restrict__ rec, long long n, long long item,
                                                  long long coord_off, long long feat_off, int half,
                                                  const double *__restrict__ gain, int nx, int ny, long long cap,
                                                  H *__restrict__ feats, int small) {
    const long long total = cap * half, step = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += step) {
        const long long row = small ? (long long)((unsigned)p / (unsigned)half) : p / half;
        const int jp = (int)(p - row * half);
        float a = 0.f, b = 0.f;
        if (row < n) {
            const unsigned char *r = rec + row * item;
            if (KIND == WFS_PREDICT_WAVEFORM) {
                const unsigned w = ld32<A4>(r + feat_off + 4ll * jp);
                const int lo = (short)(w & 0xFFFFu), hi = (short)(w >> 16);
                const int x = (int)ld32<A4>(r + coord_off), y = (int)ld32<A4>(r + coord_off + 4);
                if (x >= 0 && x < nx && y >= 0 && y < ny) {
                    const double *g = gain + ((long long)x * ny + y) * 2;
                    const int j = 2 * jp;
                    a = (float)((double)lo * g[j >= half ? 1 : 0]);
                    b = (float)((double)hi * g[j + 1 >= half ? 1 : 0]);
                    // the fp32 value is what the reference stores: a 16-bit row rounds THAT once more.  Without the
                    // barrier the compiler narrows fp64 -> fp16 in one step, which differs where the fp32 value is a
                    // half-way case of the 16-bit format (seen: -0x1.91200047acap+5 -> fp32 -0x1.912p+5 -> fp16).
                    asm volatile("" : "+v"(a), "+v"(b));
                } else {
                    a = b = __builtin_nanf("");
                }
            } else {
                a = __uint_as_float(ld32<A4>(r + feat_off + 8ll * jp));
                b = __uint_as_float(ld32<A4>(r + feat_off + 8ll * jp + 4));
            }
        }
        store_pair<H>(feats, p, a, b);
    }
}

template <bool A4, typename S>
__global__ void __launch_bounds__(256) k_ps_scatter(unsigned char *__restrict__ rec, long long n, long long item,
                                                    long long member_off, int col0, int L,
                                                    const int *__restrict__ coords, const S *__restrict__ src, int mode,
                                                    long long B, int nx, int ny, int affine, float sub, float mul,
                                                    int small) {
    const long long total = n * L, step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long long row = small ? (long long)((unsigned)i / (unsigned)L) : i / L;
        const int l = (int)(i - row * L);
        long long at;
        if (mode == WFS_PREDICT_ROWS) {
            at = i;
        } else {
            const int e = coords[row * 3 + 2];
            if (e < 0 || e >= B) continue;
            if (mode == WFS_PREDICT_EVENT) {
                at = (long long)e * L + l;
            } else {
                const int x = coords[row * 3 + 0], y = coords[row * 3 + 1];
                if (x < 0 || x >= nx || y < 0 || y >= ny) continue;
                at = (((long long)e * L + l) * nx + x) * ny + y;
            }
        }
        float v = wfs_ld(src + at);
        if (affine) v = __fmul_rn(__fsub_rn(v, sub), mul);       // two roundings, as numpy's (a - 0.5) * scale
        st32<A4>(rec + row * item + member_off + 4ll * (col0 + l), __float_as_uint(v));
    }
}

unsigned grid_for(long long work) {
    long long blocks = wfs_cdiv(work > 0 ? work : 1, 256);
    return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

template <int KIND, bool A4>
void launch_feats(const unsigned char *rec, long long n, long long item, long long coord_off, long long feat_off, int half,
                  const double *gain, int nx, int ny, long long cap, void *feats, int dtype, hipStream_t stream) {
    const long long total = cap * half;
    const int small = total < (1ll << 31) ? 1 : 0;
    const dim3 grid(grid_for(total)), block(256);
    wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_pp_feats<KIND, A4, T><<<grid, block, 0, stream>>>(rec, n, item, coord_off, feat_off, half, gain, nx, ny, cap,
                                                            (T *)feats, small);
        return WFS_OK;
    });
}

template <bool A4>
void launch_scatter(unsigned char *rec, long long n, long long item, long long member_off, int col0, int L,
                    const int *coords, const void *src, int dtype, int mode, long long B, int nx, int ny, int affine,
                    float sub, float mul, hipStream_t stream) {
    const long long total = n * L;
    const int small = total < (1ll << 31) ? 1 : 0;
    const dim3 grid(grid_for(total)), block(256);
    wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_ps_scatter<A4, T><<<grid, block, 0, stream>>>(rec, n, item, member_off, col0, L, coords, (const T *)src, mode, B, nx,
                                                        ny, affine, sub, mul, small);
        return WFS_OK;
    });
}

}  // namespace

extern "C" size_t wfs_predict_workspace_ints(int64_t n) { return (size_t)wfs_cdiv(n > 0 ? n : 1, T); }

extern "C" int wfs_predict_prepare(const void *records, int64_t n, int64_t item_size, int64_t coord_offset,
                                   int64_t feat_offset, int32_t feat_kind, int32_t width, const double *gain_factors,
                                   int32_t nx, int32_t ny, int64_t cap, int32_t *coords, void *feats, int32_t feat_dtype,
                                   int64_t *n_valid, int32_t *workspace, size_t workspace_ints, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    WFS_REQUIRE(n >= 0 && cap >= n && cap >= 1, WFS_EINVAL, "%lld rows into a capacity of %lld", (long long)n, (long long)cap);
    WFS_REQUIRE(cap < (1ll << 31), WFS_EOVERFLOW, "capacity %lld rows: event numbers are int32", (long long)cap);
    WFS_REQUIRE(feat_kind == WFS_PREDICT_WAVEFORM || feat_kind == WFS_PREDICT_PULSE, WFS_EINVAL, "feature kind %d", feat_kind);
    WFS_REQUIRE(wfs_dtype_ok(feat_dtype), WFS_EINVAL, "feature dtype %d", feat_dtype);
    WFS_REQUIRE(width >= 2 && width % 2 == 0, WFS_EINVAL, "feature width %d must be even (two PMT sides)", width);
    const int64_t elem = feat_kind == WFS_PREDICT_WAVEFORM ? 2 : 4;
    WFS_REQUIRE(item_size > 0 && item_size % 2 == 0 && coord_offset >= 0 && coord_offset % 2 == 0 && feat_offset >= 0 &&
                    feat_offset % 2 == 0 && coord_offset + 12 <= item_size && feat_offset + elem * width <= item_size,
                WFS_EINVAL, "members at %lld (coord) / %lld (%d features) do not fit 2-byte aligned into records of %lld bytes",
                (long long)coord_offset, (long long)feat_offset, width, (long long)item_size);
    WFS_REQUIRE(coords && feats && (n == 0 || records), WFS_EINVAL, "NULL device pointer");
    WFS_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)feats % 8 == 0 && (uintptr_t)coords % 4 == 0, WFS_EINVAL,
                "records must be 4-byte aligned, feature rows 8-byte aligned");
    WFS_REQUIRE(feat_kind != WFS_PREDICT_WAVEFORM || (gain_factors && nx > 0 && ny > 0), WFS_EINVAL,
                "waveform records need a gain table [nx, ny, 2]");
    const size_t nb = wfs_predict_workspace_ints(n);
    WFS_REQUIRE(n == 0 || (workspace && workspace_ints >= nb), WFS_EWORKSPACE, "workspace of %zu ints, %zu needed",
                workspace_ints, nb);
    const unsigned char *rec = (const unsigned char *)records;
    const bool a4 = item_size % 4 == 0 && coord_offset % 4 == 0 && feat_offset % 4 == 0;
    const int half = width / 2;
    const dim3 block(T), cgrid((unsigned)wfs_cdiv(cap, T));
    if (a4) {
        if (n > 0) k_pp_flags<true><<<dim3((unsigned)nb), block, 0, stream>>>(rec + coord_offset + 8, n, item_size, workspace);
        k_pp_coords<true><<<cgrid, block, 0, stream>>>(rec, n, item_size, coord_offset, cap, workspace, coords,
                                                       (long long *)n_valid);
        if (feat_kind == WFS_PREDICT_WAVEFORM)
            launch_feats<WFS_PREDICT_WAVEFORM, true>(rec, n, item_size, coord_offset, feat_offset, half, gain_factors, nx, ny,
                                                     cap, feats, feat_dtype, stream);
        else
            launch_feats<WFS_PREDICT_PULSE, true>(rec, n, item_size, coord_offset, feat_offset, half, gain_factors, nx, ny, cap,
                                                  feats, feat_dtype, stream);
    } else {
        if (n > 0) k_pp_flags<false><<<dim3((unsigned)nb), block, 0, stream>>>(rec + coord_offset + 8, n, item_size, workspace);
        k_pp_coords<false><<<cgrid, block, 0, stream>>>(rec, n, item_size, coord_offset, cap, workspace, coords,
                                                        (long long *)n_valid);
        if (feat_kind == WFS_PREDICT_WAVEFORM)
            launch_feats<WFS_PREDICT_WAVEFORM, false>(rec, n, item_size, coord_offset, feat_offset, half, gain_factors, nx, ny,
                                                      cap, feats, feat_dtype, stream);
        else
            launch_feats<WFS_PREDICT_PULSE, false>(rec, n, item_size, coord_offset, feat_offset, half, gain_factors, nx, ny,
                                                   cap, feats, feat_dtype, stream);
    }
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_predict_scatter(void *records, int64_t n, int64_t item_size, int64_t member_offset, int32_t member_cols,
                                   int32_t col0, int32_t L, const int32_t *coords, const void *src, int32_t src_dtype,
                                   int32_t mode, int64_t B, int32_t nx, int32_t ny, int32_t affine, float sub, float mul,
                                   void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    WFS_REQUIRE(n >= 0 && n < (1ll << 31), WFS_EINVAL, "%lld rows", (long long)n);
    WFS_REQUIRE(mode == WFS_PREDICT_DENSE || mode == WFS_PREDICT_EVENT || mode == WFS_PREDICT_ROWS, WFS_EINVAL, "mode %d", mode);
    WFS_REQUIRE(wfs_dtype_ok(src_dtype), WFS_EINVAL, "source dtype %d", src_dtype);
    WFS_REQUIRE(L >= 1 && col0 >= 0 && member_cols >= 1 && col0 + (int64_t)L <= member_cols, WFS_EINVAL,
                "columns [%d, %d) of a member of %d", col0, col0 + L, member_cols);
    WFS_REQUIRE(item_size > 0 && item_size % 2 == 0 && member_offset >= 0 && member_offset % 2 == 0 &&
                    member_offset + 4ll * member_cols <= item_size,
                WFS_EINVAL, "a float32 member of %d at %lld does not fit 2-byte aligned into records of %lld bytes", member_cols,
                (long long)member_offset, (long long)item_size);
    WFS_REQUIRE(mode == WFS_PREDICT_ROWS || (B >= 1 && (mode == WFS_PREDICT_EVENT || (nx > 0 && ny > 0))), WFS_EINVAL,
                "source of %lld events on a %d x %d grid", (long long)B, nx, ny);
    if (n == 0) return WFS_OK;
    WFS_REQUIRE(records && src && (mode == WFS_PREDICT_ROWS || coords), WFS_EINVAL, "NULL device pointer");
    WFS_REQUIRE((uintptr_t)records % 4 == 0, WFS_EINVAL, "records must be 4-byte aligned");
    if (item_size % 4 == 0 && member_offset % 4 == 0)
        launch_scatter<true>((unsigned char *)records, n, item_size, member_offset, col0, L, coords, src, src_dtype, mode, B, nx,
                             ny, affine, sub, mul, stream);
    else
        launch_scatter<false>((unsigned char *)records, n, item_size, member_offset, col0, L, coords, src, src_dtype, mode, B,
                              nx, ny, affine, sub, mul, stream);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
