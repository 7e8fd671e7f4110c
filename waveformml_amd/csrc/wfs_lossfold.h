// wfs_lossfold.h -- the deterministic chunk fold under the fused regression losses of segloss.hip (k_mrl_forward,
// k_sml_forward): up to MAX fp64 sums and an int64 count over the counted rows, in ONE launch, without a floating-point atomic.
//
// The rows are cut into chunks of LF_CHUNK by row index, whatever the grid: a workgroup sums a chunk in a fixed shape (every
// thread its LF_ROWS rows in row order, then a fixed tree over the threads) and stores the chunk's record: `sums` doubles, then
// the count as an int64 in the last slot.  The workgroup that draws the last ticket folds the records -- every thread its
// chunks in chunk order, then the same tree -- and hands sums and count to the caller's finish in its thread 0.  So the result
// repeats bit for bit and does not depend on the grid, nor on the rows' capacity: a chunk beyond the valid rows adds an exact 0.
//
// The hand-off is one agent-scope release in each workgroup (after its chunk stores have drained) in front of a relaxed
// ticket add, and one agent-scope acquire in the last one; the last one puts the ticket back to 0.  The ticket word must be
// 0 before the first launch: the workspace is LF_HEAD bytes (the ticket and padding), then the records.
#pragma once
#include "wfs_common.h"

constexpr int LF_THREADS = 256;
constexpr int LF_ROWS = 4;                    // rows per thread and chunk
constexpr int LF_CHUNK = LF_THREADS * LF_ROWS;
constexpr int LF_MAX_BLOCKS = 256;
constexpr int LF_HEAD = 16;                   // workspace: the ticket (and padding), then (sums + 1) x 8 bytes per chunk

// what a counted row with difference d adds to a sum-reduced L1 / MSE loss
__device__ __forceinline__ double lossfold_term(int kind, double d) { return kind == WFS_LOSS_L1 ? fabs(d) : d * d; }

// d term / d d: sign(d) with sign(0) = 0 and a NaN passed through, or 2 d
__device__ __forceinline__ double lossfold_sign(int kind, double d) {
    return kind == WFS_LOSS_L1 ? (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : (d == d ? 0.0 : d))) : 2.0 * d;
}

// fixed tree over the workgroup's threads; the results are in every thread
template <int MAX>
__device__ __forceinline__ void lossfold_tree(double (*sa)[LF_THREADS], long long *sc, int sums, double *a, long long &c) {
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < MAX; ++p)
        if (p < sums) sa[p][t] = a[p];
    sc[t] = c;
    __syncthreads();
    for (int s = LF_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int p = 0; p < sums; ++p) sa[p][t] += sa[p][t + s];
            sc[t] += sc[t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < MAX; ++p)
        if (p < sums) a[p] = sa[p][0];
    c = sc[0];
    __syncthreads();
}

// The body of a forward kernel of LF_THREADS threads.  row(r, a) -> bool: whether row r (below the valid count nv) is
// counted, and if so its terms added to the thread's sums a[0 .. sums - 1] (added there, term by term, so that no kernel
// holds MAX terms in registers); finish(a, c): thread 0 of the last workgroup writes the outputs from the sums and the count.
template <int MAX, typename Row, typename Finish>
__device__ __forceinline__ void lossfold_forward(int sums, long long nv, long long n_chunks, unsigned *__restrict__ ticket,
                                                 double *__restrict__ part, Row row, Finish finish) {
    __shared__ double sa[MAX][LF_THREADS];
    __shared__ long long sc[LF_THREADS];
    const int t = threadIdx.x, stride = sums + 1;
    for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        double a[MAX] = {};
        long long c = 0;
#pragma unroll
        for (int j = 0; j < LF_ROWS; ++j) {
            const long long r = ch * LF_CHUNK + (long long)j * LF_THREADS + t;
            if (r < nv && row(r, a)) ++c;
        }
        lossfold_tree<MAX>(sa, sc, sums, a, c);
        if (t == 0) {
#pragma unroll
            for (int p = 0; p < MAX; ++p)
                if (p < sums) part[ch * stride + p] = a[p];
            reinterpret_cast<long long *>(part)[ch * stride + sums] = c;
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
    double a[MAX] = {};
    long long c = 0;
    for (long long ch = t; ch < n_chunks; ch += LF_THREADS) {
#pragma unroll
        for (int p = 0; p < MAX; ++p)
            if (p < sums) a[p] += part[ch * stride + p];
        c += reinterpret_cast<const long long *>(part)[ch * stride + sums];
    }
    lossfold_tree<MAX>(sa, sc, sums, a, c);
    if (t == 0) {
        finish(a, c);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static inline size_t lossfold_workspace_bytes(int64_t n_cap, int sums) {
    return (size_t)LF_HEAD + (size_t)(n_cap > 0 ? wfs_cdiv(n_cap, LF_CHUNK) : 1) * (sums + 1) * sizeof(double);
}

// the launch of a forward over n_cap rows: every chunk a workgroup, at most max_blocks (0: LF_MAX_BLOCKS) of them
struct LossfoldGrid {
    long long n_chunks;                       // 0 rows: no chunk, the fold writes NaN and count 0
    unsigned blocks;
};
static inline LossfoldGrid lossfold_grid(int64_t n_cap, int32_t max_blocks) {
    const long long n_chunks = wfs_cdiv(n_cap, LF_CHUNK);
    long long blocks = n_chunks < 1 ? 1 : n_chunks;
    const long long cap = max_blocks > 0 ? max_blocks : LF_MAX_BLOCKS;
    if (blocks > cap) blocks = cap;
    return {n_chunks, (unsigned)blocks};
}
