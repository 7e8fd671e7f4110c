// pool.hip -- SparseMaxPool2d / 3d of spconv 1.2.1 (indice_maxpool / indice_maxpool_backward) as two gathers.
//
// spconv's pool walks the rulebook's pairs input-stationary: forward `if X[in] > Y[out]: Y[out] = X[in]` on an output
// that starts at ZERO, backward `dX[in] += dY[out] where X[in] == Y[out]`.  Here, as for the convolutions
// (gather_conv.hip), both directions are stationary in the rows they WRITE: the forward owns an output row and gathers
// its <= K inputs through the by-output table, the backward owns an input row and gathers the <= K outputs it reached
// through the by-input table.  Every row is written once, nothing is scattered or atomically accumulated, the sums of
// the backward run in fixed offset order: results are run-to-run reproducible.
//
// There is no arithmetic to speak of: both kernels are bound by bytes and round trips.  A row of C channels is C *
// sizeof(T) / 16 lanes of 16 bytes each, several rows share a wave, the table entries of a group of offsets are read
// first and the group's gathers are then all in flight together.  The gathered rows go through raw buffers sized by the
// rows that exist: a missing neighbour (-1) -- or an entry outside the buffer, as an overflowed build can leave --
// reads as 0, which is the identity of both kernels (the output starts at 0; a gradient of 0 adds nothing).
#include <vector>

#include "wfs_common.h"

namespace {

constexpr int TB = 256;
constexpr int GROUP = 9;         // offsets whose gathers are in flight together (27 = 3 groups; a packed 9-row table = 1)

// R = capacity (strides, grid); the number of valid rows comes from device memory when r_dev is given (wfs_valid_rows)

template <typename T>
struct Chunk {                   // 16 bytes of a row
    static constexpr int NE = 16 / sizeof(T);
};

__device__ __forceinline__ void unpack16(const float *, uint4 v, float (&f)[4]) {
    f[0] = __uint_as_float(v.x);
    f[1] = __uint_as_float(v.y);
    f[2] = __uint_as_float(v.z);
    f[3] = __uint_as_float(v.w);
}
template <typename H>
__device__ __forceinline__ void unpack16(const H *, uint4 v, float (&f)[8]) {
    wfs_unpack2<H>(v.x, f[0], f[1]);
    wfs_unpack2<H>(v.y, f[2], f[3]);
    wfs_unpack2<H>(v.z, f[4], f[5]);
    wfs_unpack2<H>(v.w, f[6], f[7]);
}
// rounds to the row type (the backward's sums)
__device__ __forceinline__ uint4 pack16(const float *, const float (&f)[4]) {
    return uint4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])};
}
template <typename H>
__device__ __forceinline__ uint4 pack16(const H *, const float (&f)[8]) {
    return uint4{wfs_pack2<H>(f[0], f[1]), wfs_pack2<H>(f[2], f[3]), wfs_pack2<H>(f[4], f[5]), wfs_pack2<H>(f[6], f[7])};
}
// the forward's results are input elements widened to fp32 (or +0): narrowing them again rounds nothing.  bf16 is the
// upper half of the fp32 pattern -- taken as such, no conversion instruction in between.
__device__ __forceinline__ uint4 pack16_exact(const float *p, const float (&f)[4]) { return pack16(p, f); }
__device__ __forceinline__ uint4 pack16_exact(const wfs_f16 *p, const float (&f)[8]) { return pack16(p, f); }
__device__ __forceinline__ uint4 pack16_exact(const wfs_bf16 *, const float (&f)[8]) {
    auto two = [](float lo, float hi) { return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xFFFF0000u); };
    return uint4{two(f[0], f[1]), two(f[2], f[3]), two(f[4], f[5]), two(f[6], f[7])};
}
__device__ __forceinline__ void st_exact(float *p, float v) { *p = v; }
__device__ __forceinline__ void st_exact(wfs_f16 *p, float v) { wfs_st(p, v); }
__device__ __forceinline__ void st_exact(wfs_bf16 *p, float v) { *p = (wfs_bf16)(__float_as_uint(v) >> 16); }

// an entry of the by-input table: the dense form holds the row, the packed form (include/wfsparse.h "packed tables")
// the row in the bits above its three offset bits -- which offset it was does not matter to a pool
template <bool PACKED>
__device__ __forceinline__ int entry_row(int e) {
    return PACKED ? (e >= 0 ? (e >> 3) : -1) : e;
}

// byte offset of 16-byte chunk `sub` of row `nb` in a raw buffer of `rows` rows; anything else -> past every buffer
__device__ __forceinline__ int chunk_offset(int nb, long long rows, unsigned row_bytes, int sub) {
    return ((unsigned long long)(long long)nb < (unsigned long long)rows) ? (int)((unsigned)nb * row_bytes + (unsigned)sub * 16u)
                                                                           : (int)0x80000000;
}

// ------------------------------------------------------------------------------------------ forward
// Y[r] = max(0, max_k X[table[k][r]]): thread = (row, 16-byte chunk), L chunks per row, rows_pb rows per block.
// The table column a k stands for (kmap) does not matter to a maximum: the columns are walked in storage order.
template <typename T>
__global__ void __launch_bounds__(TB) k_maxpool_fwd(const int *__restrict__ table, int K, long long R,
                                                    const long long *__restrict__ r_dev, const T *__restrict__ X,
                                                    long long X_rows, int L, int rows_pb, T *__restrict__ Y) {
    constexpr int NE = Chunk<T>::NE;
    const int rloc = (int)threadIdx.x / L, sub = (int)threadIdx.x - rloc * L;
    const long long row = (long long)blockIdx.x * rows_pb + rloc;
    if (rloc >= rows_pb || row >= wfs_valid_rows(R, r_dev)) return;
    const unsigned row_bytes = (unsigned)L * 16u;
    // byte offsets below 2 GiB: the dispatcher checks X_rows * row_bytes
    const __amdgpu_buffer_rsrc_t rsrcX = __builtin_amdgcn_make_buffer_rsrc((void *)X, 0, (int)(X_rows * row_bytes), 0x00020000);
    float y[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) y[i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += GROUP) {
        int nb[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) nb[g] = k0 + g < K ? table[(long long)(k0 + g) * R + row] : -1;
        uint4 v[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g)
            v[g] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrcX, chunk_offset(nb[g], X_rows, row_bytes, sub), 0, 0));
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            float x[NE];
            unpack16((const T *)nullptr, v[g], x);
#pragma unroll
            for (int i = 0; i < NE; ++i) y[i] = x[i] > y[i] ? x[i] : y[i];       // spconv's comparison: NaN and -0 never win
        }
    }
    reinterpret_cast<uint4 *>(Y)[row * L + sub] = pack16_exact((const T *)nullptr, y);
}

// every other channel count (rows that are not whole 16-byte chunks, e.g. the first layer's 2 channels): thread =
// (row, channel)
template <typename T>
__global__ void __launch_bounds__(TB) k_maxpool_fwd_any(const int *__restrict__ table, int K, long long R,
                                                        const long long *__restrict__ r_dev, const T *__restrict__ X,
                                                        long long X_rows, int C, T *__restrict__ Y) {
    const long long e = (long long)blockIdx.x * TB + threadIdx.x;
    const long long row = e / C;
    const int c = (int)(e - row * C);
    if (row >= wfs_valid_rows(R, r_dev)) return;
    float y = 0.f;
    for (int k = 0; k < K; ++k) {
        const int nb = table[(long long)k * R + row];
        if ((unsigned long long)(long long)nb >= (unsigned long long)X_rows) continue;
        const float x = wfs_ld(X + (long long)nb * C + c);
        y = x > y ? x : y;
    }
    st_exact(Y + row * C + c, y);
}

// ------------------------------------------------------------------------------------------ backward
// dX[j] = sum_k (X[j] == Y[o]) ? dY[o] : 0 with o = table[k][j] >= 0, fp32 sums in ascending k.  TR = rows of the
// table: K for the dense form, K / kl for the packed one (an input reaches at most one output per packed row, and the
// packed rows are in offset order: the same terms in the same order as through the dense table).
template <typename T, bool PACKED>
__global__ void __launch_bounds__(TB) k_maxpool_bwd(const int *__restrict__ table, int TR, long long N,
                                                    const long long *__restrict__ n_dev, const T *__restrict__ X,
                                                    const T *__restrict__ Y, const T *__restrict__ dY, long long M_rows,
                                                    int L, int rows_pb, T *__restrict__ dX) {
    constexpr int NE = Chunk<T>::NE;
    const int rloc = (int)threadIdx.x / L, sub = (int)threadIdx.x - rloc * L;
    const long long row = (long long)blockIdx.x * rows_pb + rloc;
    if (rloc >= rows_pb || row >= wfs_valid_rows(N, n_dev)) return;
    const unsigned row_bytes = (unsigned)L * 16u;
    const __amdgpu_buffer_rsrc_t rsrcY = __builtin_amdgcn_make_buffer_rsrc((void *)Y, 0, (int)(M_rows * row_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcG = __builtin_amdgcn_make_buffer_rsrc((void *)dY, 0, (int)(M_rows * row_bytes), 0x00020000);
    float x[NE], acc[NE];
    unpack16((const T *)nullptr, reinterpret_cast<const uint4 *>(X)[row * L + sub], x);
#pragma unroll
    for (int i = 0; i < NE; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < TR; k0 += GROUP) {
        int off[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            const int e = k0 + g < TR ? table[(long long)(k0 + g) * N + row] : -1;
            off[g] = chunk_offset(entry_row<PACKED>(e), M_rows, row_bytes, sub);
        }
        uint4 yv[GROUP], gv[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            yv[g] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrcY, off[g], 0, 0));
            gv[g] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrcG, off[g], 0, 0));
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            float yf[NE], gf[NE];
            unpack16((const T *)nullptr, yv[g], yf);
            unpack16((const T *)nullptr, gv[g], gf);
            // no neighbour: both read as 0 -- whatever the comparison says, the term is 0
#pragma unroll
            for (int i = 0; i < NE; ++i) acc[i] += (x[i] == yf[i]) ? gf[i] : 0.f;
        }
    }
    reinterpret_cast<uint4 *>(dX)[row * L + sub] = pack16((const T *)nullptr, acc);
}

template <typename T, bool PACKED>
__global__ void __launch_bounds__(TB) k_maxpool_bwd_any(const int *__restrict__ table, int TR, long long N,
                                                        const long long *__restrict__ n_dev, const T *__restrict__ X,
                                                        const T *__restrict__ Y, const T *__restrict__ dY,
                                                        long long M_rows, int C, T *__restrict__ dX) {
    const long long e = (long long)blockIdx.x * TB + threadIdx.x;
    const long long row = e / C;
    const int c = (int)(e - row * C);
    if (row >= wfs_valid_rows(N, n_dev)) return;
    const float x = wfs_ld(X + row * C + c);
    float acc = 0.f;
    for (int k = 0; k < TR; ++k) {
        const int o = entry_row<PACKED>(table[(long long)k * N + row]);
        if ((unsigned long long)(long long)o >= (unsigned long long)M_rows) continue;
        if (x == wfs_ld(Y + (long long)o * C + c)) acc += wfs_ld(dY + (long long)o * C + c);
    }
    wfs_st(dX + row * C + c, acc);
}

// rows as whole 16-byte chunks, at most one block wide, gathered rows addressable through 32-bit byte offsets
inline bool vector_rows(int C, int dtype, long long gathered_rows) {
    const long long row_bytes = (long long)C * wfs_dtype_bytes(dtype);
    return row_bytes % 16 == 0 && row_bytes / 16 <= TB && gathered_rows * row_bytes < (1ll << 31);
}

}  // namespace

extern "C" int wfs_maxpool_fwd(const int32_t *table, const int32_t *kmap_host, int32_t K, int64_t R, const void *X,
                               int64_t X_rows, int32_t C, void *Y, int32_t dtype, const int64_t *r_dev_, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const long long *r_dev = (const long long *)r_dev_;
    WFS_REQUIRE(K >= 1 && K <= 65535, WFS_EINVAL, "kernel volume %d not in [1,65535]", K);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    WFS_REQUIRE(C >= 1 && R >= 0 && X_rows >= 0, WFS_EINVAL, "bad shape: %d channels, %lld rows gathering from %lld", C,
                (long long)R, (long long)X_rows);
    if (kmap_host) {                 // a maximum does not care which offset a column stands for -- but every column must be one
        std::vector<char> seen((size_t)K, 0);
        for (int k = 0; k < K; ++k) {
            WFS_REQUIRE(kmap_host[k] >= 0 && kmap_host[k] < K && !seen[kmap_host[k]], WFS_EINVAL,
                        "kmap is not a permutation of the %d offsets (entry %d)", K, k);
            seen[kmap_host[k]] = 1;
        }
    }
    if (R == 0) return WFS_OK;
    WFS_REQUIRE(table && Y && (X || X_rows == 0), WFS_EINVAL, "NULL device pointer");
    if (vector_rows(C, dtype, X_rows)) {
        WFS_REQUIRE((((uintptr_t)X | (uintptr_t)Y) & 15) == 0, WFS_EINVAL, "rows must be 16-byte aligned");
        const int L = C * wfs_dtype_bytes(dtype) / 16, rows_pb = TB / L;
        const dim3 grid((unsigned)wfs_cdiv(R, rows_pb)), block(TB);
        return wfs_with_dtype(dtype, [&](auto t) -> int {
            using T = decltype(t);
            k_maxpool_fwd<T><<<grid, block, 0, stream>>>(table, K, R, r_dev, (const T *)X, X_rows, L, rows_pb, (T *)Y);
            WFS_LAUNCH_CHECK();
            return WFS_OK;
        });
    }
    const long long blocks = wfs_cdiv((long long)R * C, TB);
    WFS_REQUIRE(blocks < (1ll << 31), WFS_EINVAL, "%lld x %d elements are too many for one launch", (long long)R, C);
    const dim3 grid((unsigned)blocks), block(TB);
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        k_maxpool_fwd_any<T><<<grid, block, 0, stream>>>(table, K, R, r_dev, (const T *)X, X_rows, C, (T *)Y);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

// does wfs_maxpool_bwd take the packed by-input table [K / kl, N] of wfs_event_rulebook_conv as it is?
extern "C" int wfs_maxpool_packed_ok(int32_t packed_kl, int32_t K, int32_t C, int32_t dtype) {
    return packed_kl >= 1 && packed_kl <= 8 && K >= 1 && K % packed_kl == 0 && C >= 1 && wfs_dtype_ok(dtype);
}

extern "C" int wfs_maxpool_bwd(const int32_t *table, int32_t K, int32_t packed_kl, int64_t N, const void *X, const void *Y,
                               const void *dY, int64_t M_rows, int32_t C, void *dX, int32_t dtype, const int64_t *n_dev_,
                               void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const long long *n_dev = (const long long *)n_dev_;
    WFS_REQUIRE(K >= 1 && K <= 65535, WFS_EINVAL, "kernel volume %d not in [1,65535]", K);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    WFS_REQUIRE(C >= 1 && N >= 0 && M_rows >= 0, WFS_EINVAL, "bad shape: %d channels, %lld rows gathering from %lld", C,
                (long long)N, (long long)M_rows);
    WFS_REQUIRE(packed_kl == 0 || wfs_maxpool_packed_ok(packed_kl, K, C, dtype), WFS_EINVAL,
                "a packed table (kl %d) does not fit %d offsets (wfs_maxpool_packed_ok)", packed_kl, K);
    if (N == 0) return WFS_OK;
    WFS_REQUIRE(table && X && dX && ((Y && dY) || M_rows == 0), WFS_EINVAL, "NULL device pointer");
    const int TR = packed_kl ? K / packed_kl : K;
    if (vector_rows(C, dtype, M_rows)) {
        WFS_REQUIRE((((uintptr_t)X | (uintptr_t)Y | (uintptr_t)dY | (uintptr_t)dX) & 15) == 0, WFS_EINVAL,
                    "rows must be 16-byte aligned");
        const int L = C * wfs_dtype_bytes(dtype) / 16, rows_pb = TB / L;
        const dim3 grid((unsigned)wfs_cdiv(N, rows_pb)), block(TB);
        return wfs_with_dtype(dtype, [&](auto t) -> int {
            using T = decltype(t);
            if (packed_kl)
                k_maxpool_bwd<T, true><<<grid, block, 0, stream>>>(table, TR, N, n_dev, (const T *)X, (const T *)Y,
                                                                   (const T *)dY, M_rows, L, rows_pb, (T *)dX);
            else
                k_maxpool_bwd<T, false><<<grid, block, 0, stream>>>(table, TR, N, n_dev, (const T *)X, (const T *)Y,
                                                                    (const T *)dY, M_rows, L, rows_pb, (T *)dX);
            WFS_LAUNCH_CHECK();
            return WFS_OK;
        });
    }
    const long long blocks = wfs_cdiv((long long)N * C, TB);
    WFS_REQUIRE(blocks < (1ll << 31), WFS_EINVAL, "%lld x %d elements are too many for one launch", (long long)N, C);
    const dim3 grid((unsigned)blocks), block(TB);
    return wfs_with_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (packed_kl)
            k_maxpool_bwd_any<T, true><<<grid, block, 0, stream>>>(table, TR, N, n_dev, (const T *)X, (const T *)Y,
                                                                   (const T *)dY, M_rows, C, (T *)dX);
        else
            k_maxpool_bwd_any<T, false><<<grid, block, 0, stream>>>(table, TR, N, n_dev, (const T *)X, (const T *)Y,
                                                                    (const T *)dY, M_rows, C, (T *)dX);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}
