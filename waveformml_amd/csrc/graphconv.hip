// graphconv.hip -- GraphNet's FiLM message passing on an event-local kNN graph (reference src/models/GraphNet.py with
// graph_class_index 11: torch_geometric's FiLMConv behind torch_cluster's knn_graph, both RESTATED -- DESIGN.md 7).
//
//   k_graph_knn      one thread per row: the run of rows of its event (the grouped event column), then the brute-force
//                    selection of wfs_graphknn.h -> nbr [N, KMAX] (-1 padded), deg [N].
//   k_graph_rev      one thread per row: which rows name it as a neighbour, in ascending row order, as a CSR inside the
//                    event's own slice of rev_rows (an event's in-edges are its out-edges: <= rows * KMAX) -> rev_pos
//                    [N, 2] = (start, count).  Two walks over the event's lists: count what lies in front, then write.
//   k_film_fwd       out_i = relu(gs_i * s_i + bs_i) + (1 / deg_i) sum_j relu(g_i * h_j + b_i) from the six column blocks
//                    (s | bs | gs | h | b | g) of the product row P [N, 6 D]; lanes over channels, rows over threadIdx.y.
//   k_film_bwd       the gradient of the six blocks from dout: the target side walks nbr (db, dg), the source side walks
//                    the reverse list in its fixed order (dh); the masks are recomputed from the same stored P with the
//                    same fused multiply-add.  fp32 accumulators, no atomics.
//   k_zero_tail      rows at and beyond the valid count := 0 (what a net hands back for a captured batch's padding).
//   k_event_max_*    per-event maximum over the rows of each event (global_max_pool): the first row wins a tie and is
//                    kept per (event, channel); an event without rows gives zeros and passes no gradient.  Event numbers
//                    ascend with the rows (a binary search finds an event's run).
//
// Every kernel is bound by the rows it streams: P is read once per direction plus one h row per edge (forward, target side)
// and one (b, g, dout) triple per reverse edge.  Nothing here assumes an alignment beyond the element size: D runs from 1
// to 374 and is often odd.  Rows at and beyond the device-side count have no edges, are nobody's neighbour and are
// written as zeros by the forward kernel.
#include "wfs_common.h"
#include "wfs_graphknn.h"

namespace {

constexpr int KB = 256;          // threads of the table kernels
constexpr int KMAX = WFS_GRAPH_KMAX;

__global__ void __launch_bounds__(KB)
k_graph_knn(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev, int k, int self_loop,
            int *__restrict__ nbr, int *__restrict__ deg) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long r = (long long)blockIdx.x * KB + threadIdx.x;
    if (r >= n_cap) return;
    int mine[KMAX];
    int n = 0;
    if (r < nv) {
        long long first, last;
        graph_event_run(coords, nv, r, &first, &last);
        n = graph_knn_select(coords, first, last, r, k, self_loop, mine);
    }
    for (int q = 0; q < KMAX; ++q) nbr[r * KMAX + q] = q < n ? mine[q] : -1;
    deg[r] = n;
}

__global__ void __launch_bounds__(KB)
k_graph_rev(const int *__restrict__ coords, long long n_cap, const long long *__restrict__ n_dev,
            const int *__restrict__ nbr, const int *__restrict__ deg, int *__restrict__ rev_pos,
            int *__restrict__ rev_rows) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long j = (long long)blockIdx.x * KB + threadIdx.x;
    if (j >= n_cap) return;
    if (j >= nv) {
        rev_pos[2 * j] = 0;
        rev_pos[2 * j + 1] = 0;
        return;
    }
    long long first, last;
    graph_event_run(coords, nv, j, &first, &last);
    int front = 0, count = 0;
    for (long long t = first; t < last; ++t) {
        const int d = deg[t];
        for (int q = 0; q < d; ++q) {
            const int s = nbr[t * KMAX + q];
            front += (s >= first && s < j) ? 1 : 0;
            count += s == j ? 1 : 0;
        }
    }
    // the event's slice is [first * KMAX, last * KMAX) and holds sum(deg) <= (last - first) * KMAX entries
    const long long start = first * KMAX + front;
    int w = 0;
    for (long long t = first; t < last && w < count; ++t) {
        const int d = deg[t];
        for (int q = 0; q < d; ++q)
            if (nbr[t * KMAX + q] == j && start + w < last * KMAX) rev_rows[start + w++] = (int)t;
    }
    rev_pos[2 * j] = (int)start;
    rev_pos[2 * j + 1] = w;
}

// the argument of an edge's (or the skip term's) ReLU: ONE expression for forward and backward, so that the mask the
// backward recomputes is the forward's
__device__ __forceinline__ float film_arg(float gamma, float v, float beta) { return __fmaf_rn(gamma, v, beta); }

struct Tile {
    int tx, ty;          // lanes over channels, rows per block
};
static inline Tile film_tile(int D) {
    const int tx = D <= 64 ? 64 : (D <= 128 ? 128 : 256);
    return Tile{tx, 256 / tx};
}

template <typename T>
__global__ void __launch_bounds__(256)
k_film_fwd(const T *__restrict__ P, const int *__restrict__ nbr, const int *__restrict__ deg, long long n_cap, int D,
           T *__restrict__ out, const long long *__restrict__ n_dev) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long i = (long long)blockIdx.x * blockDim.y + threadIdx.y;
    if (i >= n_cap) return;
    if (i >= nv) {
        for (int c = threadIdx.x; c < D; c += blockDim.x) wfs_st(out + i * D + c, 0.f);
        return;
    }
    const long long W = 6ll * D;
    const T *Pi = P + i * W;
    const int d = deg[i];
    int js[KMAX];
    for (int q = 0; q < KMAX; ++q) js[q] = q < d ? nbr[i * KMAX + q] : -1;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        const float s = wfs_ld(Pi + c), bs = wfs_ld(Pi + D + c), gs = wfs_ld(Pi + 2 * D + c);
        const float b = wfs_ld(Pi + 4 * D + c), g = wfs_ld(Pi + 5 * D + c);
        const float a = film_arg(gs, s, bs);
        float o = a > 0.f ? a : 0.f;
        float acc = 0.f;
        for (int q = 0; q < KMAX; ++q) {
            if (q >= d) break;
            const long long j = js[q];
            if (j < 0 || j >= nv) continue;
            const float v = film_arg(g, wfs_ld(P + j * W + 3 * D + c), b);
            acc += v > 0.f ? v : 0.f;
        }
        if (d > 0) o += acc / (float)d;
        wfs_st(out + i * D + c, o);
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
k_film_bwd(const T *__restrict__ P, const T *__restrict__ dout, const int *__restrict__ nbr, const int *__restrict__ deg,
           const int *__restrict__ rev_pos, const int *__restrict__ rev_rows, long long n_cap, int D,
           T *__restrict__ dP, const long long *__restrict__ n_dev) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long i = (long long)blockIdx.x * blockDim.y + threadIdx.y;
    if (i >= nv) return;
    const long long W = 6ll * D;
    const T *Pi = P + i * W;
    T *dPi = dP + i * W;
    const int d = deg[i];
    int js[KMAX];
    for (int q = 0; q < KMAX; ++q) js[q] = q < d ? nbr[i * KMAX + q] : -1;
    const long long rstart = rev_pos[2 * i];
    const int rcount = rev_pos[2 * i + 1];
    const long long rlimit = n_cap * KMAX;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        const float s = wfs_ld(Pi + c), bs = wfs_ld(Pi + D + c), gs = wfs_ld(Pi + 2 * D + c);
        const float h = wfs_ld(Pi + 3 * D + c), b = wfs_ld(Pi + 4 * D + c), g = wfs_ld(Pi + 5 * D + c);
        const float go = wfs_ld(dout + i * D + c);
        // the skip term: no 1 / deg
        const float gsk = film_arg(gs, s, bs) > 0.f ? go : 0.f;
        wfs_st(dPi + c, gsk * gs);
        wfs_st(dPi + D + c, gsk);
        wfs_st(dPi + 2 * D + c, gsk * s);
        // target side: this row's modulation over its neighbours' h
        const float gi = d > 0 ? go / (float)d : 0.f;
        float db = 0.f, dg = 0.f;
        for (int q = 0; q < KMAX; ++q) {
            if (q >= d) break;
            const long long j = js[q];
            if (j < 0 || j >= nv) continue;
            const float hj = wfs_ld(P + j * W + 3 * D + c);
            if (film_arg(g, hj, b) > 0.f) {
                db += gi;
                dg += gi * hj;
            }
        }
        wfs_st(dPi + 4 * D + c, db);
        wfs_st(dPi + 5 * D + c, dg);
        // source side: the rows that name this one, in ascending row order
        float dh = 0.f;
        for (int e = 0; e < rcount; ++e) {
            if (rstart + e < 0 || rstart + e >= rlimit) break;
            const long long t = rev_rows[rstart + e];
            if (t < 0 || t >= nv) continue;
            const int dt = deg[t];
            const float gt = wfs_ld(P + t * W + 5 * D + c), bt = wfs_ld(P + t * W + 4 * D + c);
            if (dt > 0 && film_arg(gt, h, bt) > 0.f) dh += (wfs_ld(dout + t * D + c) / (float)dt) * gt;
        }
        wfs_st(dPi + 3 * D + c, dh);
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
k_zero_tail(T *__restrict__ X, long long n_cap, int C, const long long *__restrict__ n_dev) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long total = (n_cap - nv) * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
        wfs_st(X + nv * C + e, 0.f);
}

// first row of [0, nv) whose event number is >= e (event numbers ascend with the rows)
__device__ __forceinline__ long long event_lower_bound(const int *coords, long long nv, int e) {
    long long lo = 0, hi = nv;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (coords[3 * mid + 2] < e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_event_max_fwd(const int *__restrict__ coords, const T *__restrict__ X, long long n_cap, int D, int B, T *__restrict__ Y,
                int *__restrict__ arg, const long long *__restrict__ n_dev) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const int e = blockIdx.x * blockDim.y + threadIdx.y;
    if (e >= B) return;
    const long long first = event_lower_bound(coords, nv, e), last = event_lower_bound(coords, nv, e + 1);
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float best = 0.f;
        int at = -1;
        for (long long r = first; r < last; ++r) {
            const float v = wfs_ld(X + r * D + c);
            if (at < 0 || v > best) {            // strictly greater: the first row keeps a tie
                best = v;
                at = (int)r;
            }
        }
        wfs_st(Y + (long long)e * D + c, best);
        arg[(long long)e * D + c] = at;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
k_event_max_bwd(const int *__restrict__ coords, const T *__restrict__ dY, const int *__restrict__ arg, long long n_cap,
                int D, int B, T *__restrict__ dX, const long long *__restrict__ n_dev) {
    const long long nv = wfs_valid_rows_nonneg(n_cap, n_dev);
    const long long i = (long long)blockIdx.x * blockDim.y + threadIdx.y;
    if (i >= n_cap) return;
    const int e = i < nv ? coords[3 * i + 2] : -1;
    const bool in = e >= 0 && e < B;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float v = 0.f;
        if (in && arg[(long long)e * D + c] == (int)i) v = wfs_ld(dY + (long long)e * D + c);
        wfs_st(dX + i * D + c, v);
    }
}

}  // namespace

extern "C" int wfs_graph_kmax(void) { return KMAX; }

extern "C" int wfs_graph_knn_host(const int32_t *coords, int64_t n, int64_t n_valid, int32_t k, int32_t self_loop,
                                  int32_t *nbr, int32_t *deg) {
    WFS_REQUIRE(k >= 1 && k <= KMAX, WFS_EINVAL, "wfs_graph_knn_host: k = %d (1 .. %d)", k, KMAX);
    WFS_REQUIRE(n >= 0 && n < (1ll << 28) && (n == 0 || (coords && nbr && deg)), WFS_EINVAL,
                "wfs_graph_knn_host: bad row count or NULL argument");
    const long long nv = n_valid < 0 ? 0 : (n_valid < n ? n_valid : n);
    for (long long r = 0; r < n; ++r) {
        int32_t mine[KMAX];
        int cnt = 0;
        if (r < nv) {
            long long first, last;
            graph_event_run(coords, nv, r, &first, &last);
            cnt = graph_knn_select(coords, first, last, r, k, self_loop ? 1 : 0, mine);
        }
        for (int q = 0; q < KMAX; ++q) nbr[r * KMAX + q] = q < cnt ? mine[q] : -1;
        deg[r] = cnt;
    }
    return WFS_OK;
}

extern "C" int wfs_graph_knn(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t k, int32_t self_loop,
                             int32_t *nbr, int32_t *deg, int32_t *rev_pos, int32_t *rev_rows, void *stream) {
    WFS_REQUIRE(k >= 1 && k <= KMAX, WFS_EINVAL, "wfs_graph_knn: k = %d (1 .. %d)", k, KMAX);
    WFS_REQUIRE(n_cap >= 0 && n_cap < (1ll << 28), WFS_EINVAL, "wfs_graph_knn: %lld rows (below 2^28)", (long long)n_cap);
    if (n_cap == 0) return WFS_OK;
    WFS_REQUIRE(coords && nbr && deg && rev_pos && rev_rows, WFS_EINVAL, "wfs_graph_knn: NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)wfs_cdiv(n_cap, KB);
    k_graph_knn<<<blocks, KB, 0, s>>>(coords, n_cap, (const long long *)n_dev, k, self_loop ? 1 : 0, nbr, deg);
    WFS_LAUNCH_CHECK();
    k_graph_rev<<<blocks, KB, 0, s>>>(coords, n_cap, (const long long *)n_dev, nbr, deg, rev_pos, rev_rows);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

#define WFS_REQUIRE_GRAPH_ROWS(name, n_cap, D)                                                                        \
    do {                                                                                                              \
        WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, name ": bad dtype %d", dtype);                                   \
        WFS_REQUIRE((D) >= 1 && (D) <= 65536, WFS_EINVAL, name ": %d channels (1 .. 65536)", (int)(D));               \
        WFS_REQUIRE((n_cap) >= 0 && (n_cap) < (1ll << 28), WFS_EINVAL, name ": %lld rows (below 2^28)",               \
                    (long long)(n_cap));                                                                              \
    } while (0)

extern "C" int wfs_film_message_fwd(const void *P, const int32_t *nbr, const int32_t *deg, int64_t n_cap, int32_t D,
                                    void *out, int32_t dtype, const int64_t *n_dev, void *stream) {
    WFS_REQUIRE_GRAPH_ROWS("wfs_film_message_fwd", n_cap, D);
    if (n_cap == 0) return WFS_OK;
    WFS_REQUIRE(P && nbr && deg && out, WFS_EINVAL, "wfs_film_message_fwd: NULL device pointer");
    const Tile t = film_tile(D);
    const dim3 block(t.tx, t.ty), grid((unsigned)wfs_cdiv(n_cap, t.ty));
    return wfs_with_dtype(dtype, [&](auto z) -> int {
        using T = decltype(z);
        k_film_fwd<T><<<grid, block, 0, (hipStream_t)stream>>>((const T *)P, nbr, deg, n_cap, D, (T *)out,
                                                                (const long long *)n_dev);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_film_message_bwd(const void *P, const void *dout, const int32_t *nbr, const int32_t *deg,
                                    const int32_t *rev_pos, const int32_t *rev_rows, int64_t n_cap, int32_t D, void *dP,
                                    int32_t dtype, const int64_t *n_dev, void *stream) {
    WFS_REQUIRE_GRAPH_ROWS("wfs_film_message_bwd", n_cap, D);
    if (n_cap == 0) return WFS_OK;
    WFS_REQUIRE(P && dout && nbr && deg && rev_pos && rev_rows && dP, WFS_EINVAL,
                "wfs_film_message_bwd: NULL device pointer");
    const Tile t = film_tile(D);
    const dim3 block(t.tx, t.ty), grid((unsigned)wfs_cdiv(n_cap, t.ty));
    return wfs_with_dtype(dtype, [&](auto z) -> int {
        using T = decltype(z);
        k_film_bwd<T><<<grid, block, 0, (hipStream_t)stream>>>((const T *)P, (const T *)dout, nbr, deg, rev_pos, rev_rows,
                                                                n_cap, D, (T *)dP, (const long long *)n_dev);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_rows_zero_tail(void *X, int64_t n_cap, int32_t C, int32_t dtype, const int64_t *n_dev, void *stream) {
    WFS_REQUIRE_GRAPH_ROWS("wfs_rows_zero_tail", n_cap, C);
    if (n_cap == 0 || !n_dev) return WFS_OK;          // an exact row count: there is no tail
    WFS_REQUIRE(X, WFS_EINVAL, "wfs_rows_zero_tail: NULL device pointer");
    const long long want = wfs_cdiv((long long)n_cap * C, 256);
    const unsigned grid = (unsigned)(want < 1024 ? want : 1024);
    return wfs_with_dtype(dtype, [&](auto z) -> int {
        using T = decltype(z);
        k_zero_tail<T><<<grid, 256, 0, (hipStream_t)stream>>>((T *)X, n_cap, C, (const long long *)n_dev);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_event_max_fwd(const int32_t *coords, const void *X, int64_t n_cap, int32_t D, int32_t B, void *Y,
                                 int32_t *arg, int32_t dtype, const int64_t *n_dev, void *stream) {
    WFS_REQUIRE_GRAPH_ROWS("wfs_event_max_fwd", n_cap, D);
    WFS_REQUIRE(B >= 0 && (long long)B * D < (1ll << 31), WFS_EINVAL, "wfs_event_max_fwd: %d events", B);
    if (B == 0) return WFS_OK;
    WFS_REQUIRE((coords && X) || n_cap == 0, WFS_EINVAL, "wfs_event_max_fwd: NULL device pointer");
    WFS_REQUIRE(Y && arg, WFS_EINVAL, "wfs_event_max_fwd: NULL output");
    const Tile t = film_tile(D);
    const dim3 block(t.tx, t.ty), grid((unsigned)wfs_cdiv(B, t.ty));
    return wfs_with_dtype(dtype, [&](auto z) -> int {
        using T = decltype(z);
        k_event_max_fwd<T><<<grid, block, 0, (hipStream_t)stream>>>(coords, (const T *)X, n_cap, D, B, (T *)Y, arg,
                                                                     (const long long *)n_dev);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}

extern "C" int wfs_event_max_bwd(const int32_t *coords, const void *dY, const int32_t *arg, int64_t n_cap, int32_t D,
                                 int32_t B, void *dX, int32_t dtype, const int64_t *n_dev, void *stream) {
    WFS_REQUIRE_GRAPH_ROWS("wfs_event_max_bwd", n_cap, D);
    WFS_REQUIRE(B >= 0 && (long long)B * D < (1ll << 31), WFS_EINVAL, "wfs_event_max_bwd: %d events", B);
    if (n_cap == 0) return WFS_OK;
    WFS_REQUIRE(coords && dX && (B == 0 || (dY && arg)), WFS_EINVAL, "wfs_event_max_bwd: NULL device pointer");
    const Tile t = film_tile(D);
    const dim3 block(t.tx, t.ty), grid((unsigned)wfs_cdiv(n_cap, t.ty));
    return wfs_with_dtype(dtype, [&](auto z) -> int {
        using T = decltype(z);
        k_event_max_bwd<T><<<grid, block, 0, (hipStream_t)stream>>>(coords, (const T *)dY, arg, n_cap, D, B, (T *)dX,
                                                                     (const long long *)n_dev);
        WFS_LAUNCH_CHECK();
        return WFS_OK;
    });
}
