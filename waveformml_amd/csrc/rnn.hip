// rnn.hip -- the multi-layer Elman RNN of torch.nn.RNN(I, H, layers, nonlinearity, bias, dropout, bidirectional,
// batch_first=True) on rows X [N][T][I], forward and backward.
//
// Reference: RecurrentNet (src/models/RecurrentBlocks.py) runs nn.RNN(1, hidden, n_layers, 'relu') over [N, n_samples, 1]
// pulse rows.  Per layer l and direction d
//
//   h[t] = act(W_ih in_l[t] + b_ih + W_hh h[t -+ 1] + b_hh),  h[start] = 0,  in_0 = X,  in_l = drop(out_{l-1})
//
// is a chain of T dependent steps per row, so rows are the parallel axis: ONE LANE PER (row, direction) carries the H
// hidden values in registers through the chain (k_rnn_scan_fwd / k_rnn_scan_bwd, H a compile-time constant: 4 / 8 / 16 /
// 32 with zero-padded weights), W_hh read from LDS at lane-uniform addresses.  Everything that is not on the chain is
// taken off it and runs as a pass over all (t, row) positions:
//   forward,  per layer: k_rnn_mix   P[t] = W_ih (in_l[t] m) + b_ih + b_hh, both directions, into the layer's slot of `saved`
//                        k_rnn_scan_fwd   h[t] = act(P[t] + W_hh h[t -+ 1]) IN PLACE (P[t + 1] is fetched while step t computes)
//   backward, per layer (top first): k_rnn_scan_bwd   delta[t] = act'(h[t]) (G[t] + W_hh^T delta[t +- 1]) in place of G
//                        k_rnn_dw    dW_ih, dW_hh, db as per-block partial sums over (t, row)
//                        k_rnn_mix   G of the layer below = m (sum over directions of W_ih^T delta)   (layer 0: dX)
//   then ONE k_rnn_dw_final for every parameter of the net.
// Layout: per-lane reads of [N][T][C] rows would put neighbouring lanes T C elements apart, so all state the kernels
// keep is LANE-CONTIGUOUS, [t][c][Npad] fp32 (Npad = N rounded up to 64): `saved` = X transposed, then every layer's
// outputs (before dropout).  Only the ends torch sees are [N][T][C]: k_rnn_tin / k_rnn_tout transpose X, dY in and Y, dX
// out through 32 x 32 LDS tiles.
// Dropout: torch's placement (the outputs of every layer but the last, training only), this project's generator: the
// counter hash of wfs_rows.h over (row, layer, channel, t).  No mask is stored; the next layer's input projection, its
// dW pass and the backward's mix rebuild it from the seed.
// Weight gradients: each dW block sums a fixed set of position tiles in a fixed order, and the partial sums are added
// block by block in index order -- no atomics, bit-identical reruns.
#include "wfs_rows.h"

namespace {

constexpr int MAXI = WFS_RNN_MAX_INPUT, MAXH = WFS_RNN_MAX_HIDDEN, MAXLY = WFS_RNN_MAX_LAYERS;
constexpr int MAXC = 2 * MAXH;   // channels of a bidirectional layer's output
constexpr int SCAN_TB = 64;      // one wave per scan block: 1024 rows spread over 16 CUs
constexpr int MIX_TB = 256;
constexpr int MIX_CH = 8;        // output channels per thread of the mix pass
constexpr int DW_TB = 256;
constexpr int DW_TP = 32;        // positions per staged tile of the dW pass
constexpr int DW_MAXBLK = 1024;  // dW blocks (partial sums per layer and direction)
constexpr int DW_MAXCOL = MAXC + MAXH + 1;
constexpr int TT = 32;           // transpose tile

// element (row, layer, channel ch of the layer's output, sample t): t < 2^12, ch < 2^6, layer < 2^3 (include/wfsparse.h)
__device__ __forceinline__ float drop_mult(const Drop &d, long long row, int layer, int ch, int t) {
    return wfs_drop_mult(d, ((((unsigned long long)row << 3 | (unsigned)layer) << 6 | (unsigned)ch) << 12) | (unsigned)t);
}

struct Rec {  // one (layer, direction): device addresses (0 = absent)
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float *dw_ih, *dw_hh, *db_ih, *db_hh;
};

// src [N][M] (dt) -> dst [M][Npad] fp32; the lanes N .. Npad of every row of dst are zero
__global__ void __launch_bounds__(TT * 8) k_rnn_tin(const void *__restrict__ src, int dt, float *__restrict__ dst,
                                                    long long N, long long Npad, long long M) {
    __shared__ float tile[TT][TT + 1];
    const long long m0 = (long long)blockIdx.x * TT;
    for (long long n0 = (long long)blockIdx.y * TT; n0 < Npad; n0 += (long long)gridDim.y * TT) {
        __syncthreads();
        for (int r = threadIdx.y; r < TT; r += 8) {
            const long long n = n0 + r, m = m0 + threadIdx.x;
            tile[r][threadIdx.x] = (n < N && m < M) ? ldt(src, n * M + m, dt) : 0.f;
        }
        __syncthreads();
        for (int r = threadIdx.y; r < TT; r += 8) {
            const long long m = m0 + r, n = n0 + threadIdx.x;
            if (m < M && n < Npad) dst[m * Npad + n] = tile[threadIdx.x][r];
        }
    }
}

// src [M][Npad] fp32 -> dst [N][M] (dt)
__global__ void __launch_bounds__(TT * 8) k_rnn_tout(const float *__restrict__ src, void *__restrict__ dst, int dt,
                                                     long long N, long long Npad, long long M) {
    __shared__ float tile[TT][TT + 1];
    const long long m0 = (long long)blockIdx.x * TT;
    for (long long n0 = (long long)blockIdx.y * TT; n0 < N; n0 += (long long)gridDim.y * TT) {
        __syncthreads();
        for (int r = threadIdx.y; r < TT; r += 8) {
            const long long m = m0 + r, n = n0 + threadIdx.x;
            tile[r][threadIdx.x] = (m < M && n < N) ? src[m * Npad + n] : 0.f;
        }
        __syncthreads();
        for (int r = threadIdx.y; r < TT; r += 8) {
            const long long n = n0 + r, m = m0 + threadIdx.x;
            if (n < N && m < M) stt(dst, n * M + m, dt, tile[threadIdx.x][r]);
        }
    }
}

// One layer's W_ih of every direction applied at every (t, row):
//   forward  (transposed == 0): R = IN inputs, Q = dirs H outputs:  out[t][d H + j] = b_ih[j] + b_hh[j] + sum_c W_ih_d[j][c] (in[t][c] m_pre)
//   backward (transposed == 1): R = dirs H,    Q = IN:              out[t][c] = m_post sum_{d, j} W_ih_d[j][c] in[t][d H + j]
// m_pre / m_post: the dropout multipliers of layer `drop_layer`'s outputs (-1: none).  Grid (row blocks, T, Q / 8).
__global__ void __launch_bounds__(MIX_TB) k_rnn_mix(const Rec *__restrict__ recs, int layer, int dirs, int H, int IN,
                                                    int transposed, const float *__restrict__ in, float *__restrict__ out,
                                                    long long N, long long Npad, int drop_layer, float drop_p,
                                                    const long long *__restrict__ seed_dev) {
    __shared__ float Ms[MAXC * MAXC];  // [R][Qp]
    __shared__ float Bs[MAXC];
    const int C = dirs * H, R = transposed ? C : IN, Q = transposed ? IN : C;
    const int Qp = (Q + MIX_CH - 1) / MIX_CH * MIX_CH;
    for (int i = threadIdx.x; i < R * Qp; i += MIX_TB) Ms[i] = 0.f;
    for (int i = threadIdx.x; i < MAXC; i += MIX_TB) Bs[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < C * IN; i += MIX_TB) {
        const int dj = i / IN, c = i - dj * IN, d = dj / H, j = dj - d * H;
        const float w = recs[layer * dirs + d].w_ih[j * IN + c];
        if (transposed)
            Ms[dj * Qp + c] = w;
        else
            Ms[c * Qp + dj] = w;
    }
    if (!transposed)
        for (int dj = threadIdx.x; dj < C; dj += MIX_TB) {
            const Rec rc = recs[layer * dirs + dj / H];
            const int j = dj % H;
            Bs[dj] = (rc.b_ih ? rc.b_ih[j] : 0.f) + (rc.b_hh ? rc.b_hh[j] : 0.f);
        }
    __syncthreads();
    const long long n = (long long)blockIdx.x * MIX_TB + threadIdx.x;
    if (n >= N) return;
    const Drop dr = make_drop(drop_layer >= 0 ? drop_p : 0.f, seed_dev);
    const int t = blockIdx.y, q0 = blockIdx.z * MIX_CH;
    float acc[MIX_CH];
#pragma unroll
    for (int c = 0; c < MIX_CH; ++c) acc[c] = Bs[q0 + c];
    const float *ip = in + (long long)t * R * Npad + n;
    for (int r = 0; r < R; ++r) {
        float x = ip[r * Npad];
        if (!transposed) x *= drop_mult(dr, n, drop_layer, r, t);
        const float *m = Ms + r * Qp + q0;
#pragma unroll
        for (int c = 0; c < MIX_CH; ++c) acc[c] = fmaf(m[c], x, acc[c]);
    }
    float *op = out + (long long)t * Q * Npad + n;
#pragma unroll
    for (int c = 0; c < MIX_CH; ++c) {
        const int q = q0 + c;
        if (q >= Q) break;
        float v = acc[c];
        if (transposed) v *= drop_mult(dr, n, drop_layer, q, t);
        op[q * Npad] = v;
    }
}

// W_hh of (layer, direction) into LDS as Ws[k][j], zero outside H x H.  forward: Ws[k][j] = W_hh[j][k] (h[t] = .. + sum_k
// W_hh[j][k] h[k]); backward: Ws[k][j] = W_hh[k][j] (a[j] = .. + sum_k W_hh[k][j] delta[k]).
template <int HP>
__device__ __forceinline__ void stage_whh(float *Ws, const float *w_hh, int H, bool fwd) {
    for (int i = threadIdx.x; i < HP * HP; i += SCAN_TB) {
        const int k = i / HP, j = i - k * HP;
        Ws[i] = (k < H && j < H) ? (fwd ? w_hh[j * H + k] : w_hh[k * H + j]) : 0.f;
    }
    __syncthreads();
}

// channel j of one (t, lane) of a [t][c][Npad] buffer, 0 for the padding channels j >= H: the load itself is
// unconditional (of channel H - 1), so that HP loads issue back to back with no branch between them
template <int HP>
__device__ __forceinline__ float ldrow(const float *at_t, int j, int H, long long Npad) {
    const float v = at_t[(j < H ? j : H - 1) * Npad];
    return j < H ? v : 0.f;
}

// a[j] += sum_k Ws[k][j] v[k]; a and v are registers (HP is a compile-time constant, every index below is static).
// HP <= 8: everything unrolled, and the compiler keeps the HP x HP weights in registers across the time loop (64 VGPRs).
// Above that they do not fit (32 x 32 weights: unrolled, they are fetched ahead of their use and spill to scratch), so
// the loop over k stays ROLLED: the lane parks v in its own LDS column Vs[k][lane] (a runtime k may index LDS, not
// registers), and each turn reads one v[k] and one row of weights (lane-uniform addresses: a broadcast) for HP FMAs.
template <int HP>
__device__ __forceinline__ void matvec(const float *Ws, float *Vs, const float (&v)[HP], float (&a)[HP]) {
    if (HP <= 8) {
#pragma unroll
        for (int k = 0; k < HP; ++k) {
#pragma unroll
            for (int j = 0; j < HP; ++j) a[j] = fmaf(Ws[k * HP + j], v[k], a[j]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < HP; ++k) Vs[k * SCAN_TB + threadIdx.x] = v[k];
#pragma unroll 2
        for (int k = 0; k < HP; ++k) {
            const float vk = Vs[k * SCAN_TB + threadIdx.x];
#pragma unroll
            for (int j = 0; j < HP; ++j) a[j] = fmaf(Ws[k * HP + j], vk, a[j]);
        }
    }
}

// Lane = (row, direction = blockIdx.y).  S is the layer's slot [T][C][Npad]: it holds P on entry and h on return.
// hidden (may be NULL) [layers dirs][N][H] (dt): the last state of the chain.
template <int HP, bool TANH>
__global__ void __launch_bounds__(SCAN_TB) k_rnn_scan_fwd(const Rec *__restrict__ recs, int layer, int dirs, int H,
                                                          float *__restrict__ S, long long N, long long Npad, int T,
                                                          void *__restrict__ hidden, int dt) {
    __shared__ __attribute__((aligned(16))) float Ws[HP * HP];
    __shared__ float Vs[HP > 8 ? HP * SCAN_TB : 1];
    const int d = blockIdx.y, C = dirs * H;
    stage_whh<HP>(Ws, recs[layer * dirs + d].w_hh, H, true);
    const long long n = (long long)blockIdx.x * SCAN_TB + threadIdx.x;
    if (n >= N) return;
    float *base = S + (long long)d * H * Npad + n;
    const long long tstride = (long long)C * Npad;
    float h[HP], p[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) h[j] = 0.f;
    int t = d ? T - 1 : 0;
    const int dt_ = d ? -1 : 1;
#pragma unroll
    for (int j = 0; j < HP; ++j) p[j] = ldrow<HP>(base + t * tstride, j, H, Npad);
    for (int s = 0; s < T; ++s, t += dt_) {
        float pn[HP];  // the next step's projection travels while this step computes
        const int tn = s + 1 < T ? t + dt_ : t;
#pragma unroll
        for (int j = 0; j < HP; ++j) pn[j] = ldrow<HP>(base + tn * tstride, j, H, Npad);
        float a[HP];
#pragma unroll
        for (int j = 0; j < HP; ++j) a[j] = p[j];
        matvec<HP>(Ws, Vs, h, a);
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            h[j] = TANH ? tanhf(a[j]) : (a[j] > 0.f ? a[j] : 0.f);
            if (j < H) base[t * tstride + j * Npad] = h[j];
            p[j] = pn[j];
        }
    }
    if (hidden) {
#pragma unroll
        for (int j = 0; j < HP; ++j)
            if (j < H) stt(hidden, ((long long)(layer * dirs + d) * N + n) * H + j, dt, h[j]);
    }
}

// G [T][C][Npad]: d loss / d out_l on entry, delta = d loss / d pre-activation on return.  S: the layer's h.
template <int HP, bool TANH>
__global__ void __launch_bounds__(SCAN_TB) k_rnn_scan_bwd(const Rec *__restrict__ recs, int layer, int dirs, int H,
                                                          const float *__restrict__ S, float *__restrict__ G, long long N,
                                                          long long Npad, int T) {
    __shared__ __attribute__((aligned(16))) float Ws[HP * HP];
    __shared__ float Vs[HP > 8 ? HP * SCAN_TB : 1];
    const int d = blockIdx.y, C = dirs * H;
    stage_whh<HP>(Ws, recs[layer * dirs + d].w_hh, H, false);
    const long long n = (long long)blockIdx.x * SCAN_TB + threadIdx.x;
    if (n >= N) return;
    const long long off = (long long)d * H * Npad + n, tstride = (long long)C * Npad;
    const float *hb = S + off;
    float *gb = G + off;
    float dl[HP], g[HP], h[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) dl[j] = 0.f;
    int t = d ? 0 : T - 1;  // against the forward's order
    const int dt_ = d ? 1 : -1;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        g[j] = ldrow<HP>(gb + t * tstride, j, H, Npad);
        h[j] = ldrow<HP>(hb + t * tstride, j, H, Npad);
    }
    for (int s = 0; s < T; ++s, t += dt_) {
        float gn[HP], hn[HP];
        const int tn = s + 1 < T ? t + dt_ : t;
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            gn[j] = ldrow<HP>(gb + tn * tstride, j, H, Npad);
            hn[j] = ldrow<HP>(hb + tn * tstride, j, H, Npad);
        }
        float a[HP];
#pragma unroll
        for (int j = 0; j < HP; ++j) a[j] = g[j];
        matvec<HP>(Ws, Vs, dl, a);
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            dl[j] = TANH ? a[j] * (1.f - h[j] * h[j]) : (h[j] > 0.f ? a[j] : 0.f);
            if (j < H) gb[t * tstride + j * Npad] = dl[j];
            g[j] = gn[j];
            h[j] = hn[j];
        }
    }
}

// Parameter gradients of (layer, direction = blockIdx.y) as partial sums.  Rows: delta[j], j < H.  Columns: the IN inputs
// (times their dropout multipliers), the H previous hidden values h[t -+ 1], and a column of ones (the biases):
//   part[block][j][col] = sum over the block's positions (t, row) of delta[t][d H + j][row] V[col][t][row].
// Block b sums position tiles b, b + nblk, ...; inside a tile `groups` thread groups take interleaved positions and are
// added in group order at the end.
template <int CO>
__global__ void __launch_bounds__(DW_TB) k_rnn_dw(int layer, int dirs, int H, int IN, const float *__restrict__ D,
                                                  const float *__restrict__ X, const float *__restrict__ S, long long N,
                                                  long long Npad, int T, int nblk, float *__restrict__ part,
                                                  long long pstride, int drop_layer, float drop_p, const long long *__restrict__ seed_dev) {
    __shared__ float Ds[CO][DW_TP];
    // the staged tile [ncol][DW_TP]; at the end the groups' sums [groups][H][ncol] <= DW_TB x CO floats
    constexpr int VS = DW_MAXCOL * DW_TP > DW_TB * CO ? DW_MAXCOL * DW_TP : DW_TB * CO;
    __shared__ float Vs[VS];
    const int d = blockIdx.y, C = dirs * H, ncol = IN + H + 1;
    const int groups = DW_TB / ncol;  // ncol <= 97: at least two
    const Drop dr = make_drop(drop_layer >= 0 ? drop_p : 0.f, seed_dev);
    const long long P = (long long)T * Npad;
    for (int i = threadIdx.x; i < CO * DW_TP; i += DW_TB) (&Ds[0][0])[i] = 0.f;
    int grp = threadIdx.x / ncol;
    const int col = threadIdx.x - grp * ncol;
    if (grp >= groups) grp = -1;
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.f;
    for (long long tile = blockIdx.x; tile * DW_TP < P; tile += nblk) {
        const long long p0 = tile * DW_TP;  // Npad is a multiple of DW_TP: a tile lies in one t
        const int t = (int)(p0 / Npad);
        const long long n0 = p0 - (long long)t * Npad;
        __syncthreads();
        for (int e = threadIdx.x; e < H * DW_TP; e += DW_TB) {
            const int j = e / DW_TP, p = e - j * DW_TP;
            Ds[j][p] = n0 + p < N ? D[((long long)t * C + d * H + j) * Npad + n0 + p] : 0.f;
        }
        for (int e = threadIdx.x; e < ncol * DW_TP; e += DW_TB) {
            const int c = e / DW_TP, p = e - c * DW_TP;
            const long long n = n0 + p;
            float v = 0.f;
            if (n < N) {
                if (c < IN) {
                    v = X[((long long)t * IN + c) * Npad + n] * drop_mult(dr, n, drop_layer, c, t);
                } else if (c < IN + H) {
                    const int tp = d ? t + 1 : t - 1;
                    if (tp >= 0 && tp < T) v = S[((long long)tp * C + d * H + (c - IN)) * Npad + n];
                } else {
                    v = 1.f;
                }
            }
            Vs[e] = v;
        }
        __syncthreads();
        if (grp >= 0) {
            const float *vs = Vs + col * DW_TP;
            for (int p = grp; p < DW_TP; p += groups) {
                const float xv = vs[p];
#pragma unroll
                for (int c = 0; c < CO; ++c) acc[c] = fmaf(Ds[c][p], xv, acc[c]);
            }
        }
    }
    float *out = part + (layer * dirs + d) * pstride + (long long)blockIdx.x * H * ncol;
    __syncthreads();
    float *sums = Vs;
    if (grp >= 0) {
#pragma unroll
        for (int c = 0; c < CO; ++c)
            if (c < H) sums[(grp * H + c) * ncol + col] = acc[c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < H * ncol; e += DW_TB) {
        float v = 0.f;
        for (int gi = 0; gi < groups; ++gi) v += sums[gi * H * ncol + e];
        out[e] = v;
    }
}

struct LayerDims {
    int in[MAXLY];
};

// block (layer, direction): the dW blocks' partials added in block order (in double: a few thousand numbers per block),
// written into the gradient slots; db_ih = db_hh.
__global__ void __launch_bounds__(DW_TB) k_rnn_dw_final(const Rec *__restrict__ recs, LayerDims dims, int dirs, int H,
                                                        const float *__restrict__ part, long long pstride,
                                                        int nblk) {
    const int layer = blockIdx.x, d = blockIdx.y, IN = dims.in[layer], ncol = IN + H + 1;
    const Rec rc = recs[layer * dirs + d];
    const float *q0 = part + (layer * dirs + d) * pstride;
    for (int e = threadIdx.x; e < H * ncol; e += DW_TB) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += (double)q0[(long long)b * H * ncol + e];
        const int j = e / ncol, c = e - j * ncol;
        const float v = (float)s;
        if (c < IN) {
            if (rc.dw_ih) rc.dw_ih[j * IN + c] = v;
        } else if (c < IN + H) {
            if (rc.dw_hh) rc.dw_hh[j * H + (c - IN)] = v;
        } else {
            if (rc.db_ih) rc.db_ih[j] = v;
            if (rc.db_hh) rc.db_hh[j] = v;
        }
    }
}

long long pad64(long long N) { return (N + 63) / 64 * 64; }
int layer_in(int I, int H, int dirs, int l) { return l == 0 ? I : dirs * H; }
// floats of partial sums per (layer, direction): [nblk][H][ncol], sized by the widest layer
long long part_stride(int I, int H, int dirs, int nblk) {
    const int in_max = I > dirs * H ? I : dirs * H;
    return (long long)nblk * H * (in_max + H + 1);
}

int check_shape(int32_t I, int32_t H, int32_t layers, int32_t dirs, int32_t nonlin, int32_t T, int32_t dtype) {
    WFS_REQUIRE(I >= 1 && I <= MAXI, WFS_EINVAL, "RNN input size %d: 1 .. %d supported", I, MAXI);
    WFS_REQUIRE(H >= 1 && H <= MAXH, WFS_EINVAL, "RNN hidden size %d: 1 .. %d supported", H, MAXH);
    WFS_REQUIRE(layers >= 1 && layers <= MAXLY, WFS_EINVAL, "RNN of %d layers: 1 .. %d supported", layers, MAXLY);
    WFS_REQUIRE(dirs == 1 || dirs == 2, WFS_EINVAL, "RNN of %d directions", dirs);
    WFS_REQUIRE(nonlin == WFS_RNN_RELU || nonlin == WFS_RNN_TANH, WFS_EINVAL, "unknown RNN nonlinearity %d", nonlin);
    WFS_REQUIRE(T >= 1 && T <= WFS_RNN_MAX_T, WFS_EINVAL, "sequence length %d not in [1, %d]", T, WFS_RNN_MAX_T);
    WFS_REQUIRE(wfs_dtype_ok(dtype), WFS_EINVAL, "bad dtype %d", dtype);
    return WFS_OK;
}

int check_common(int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs, int32_t nonlin, int32_t dtype,
                 float dropout_p, const int64_t *seed_dev) {
    int rc = check_shape(I, H, layers, dirs, nonlin, T, dtype);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(N >= 0 && N <= (1ll << 40) / T, WFS_EINVAL, "%lld rows of %d samples", (long long)N, T);
    WFS_REQUIRE_DROPOUT(dropout_p, seed_dev);
    return WFS_OK;
}

dim3 t_grid(long long M, long long Npad) {
    const long long nt = Npad / TT;
    return dim3((unsigned)((M + TT - 1) / TT), (unsigned)(nt > 1024 ? 1024 : nt));
}

template <int HP>
void scan_fwd(bool tanh_, dim3 grid, hipStream_t st, const Rec *recs, int layer, int dirs, int H, float *S, long long N,
              long long Npad, int T, void *hidden, int dt) {
    if (tanh_)
        k_rnn_scan_fwd<HP, true><<<grid, dim3(SCAN_TB), 0, st>>>(recs, layer, dirs, H, S, N, Npad, T, hidden, dt);
    else
        k_rnn_scan_fwd<HP, false><<<grid, dim3(SCAN_TB), 0, st>>>(recs, layer, dirs, H, S, N, Npad, T, hidden, dt);
}
template <int HP>
void scan_bwd(bool tanh_, dim3 grid, hipStream_t st, const Rec *recs, int layer, int dirs, int H, const float *S, float *G,
              long long N, long long Npad, int T) {
    if (tanh_)
        k_rnn_scan_bwd<HP, true><<<grid, dim3(SCAN_TB), 0, st>>>(recs, layer, dirs, H, S, G, N, Npad, T);
    else
        k_rnn_scan_bwd<HP, false><<<grid, dim3(SCAN_TB), 0, st>>>(recs, layer, dirs, H, S, G, N, Npad, T);
}

}  // namespace

extern "C" int wfs_rnn_ok(int32_t I, int32_t H, int32_t layers, int32_t dirs, int32_t nonlinearity, int32_t T,
                          int32_t dtype) {
    return check_shape(I, H, layers, dirs, nonlinearity, T, dtype);
}

extern "C" int wfs_rnn_n_params(int32_t layers, int32_t dirs) {
    if (layers < 1 || layers > MAXLY || (dirs != 1 && dirs != 2)) return 0;
    return layers * dirs;
}

extern "C" size_t wfs_rnn_saved_floats(int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs) {
    if (check_shape(I, H, layers, dirs, WFS_RNN_RELU, T, WFS_F32) != WFS_OK || N < 0) return 0;
    return (size_t)pad64(N) * T * ((size_t)I + (size_t)layers * dirs * H);
}

extern "C" size_t wfs_rnn_bwd_workspace_floats(int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs) {
    if (check_shape(I, H, layers, dirs, WFS_RNN_RELU, T, WFS_F32) != WFS_OK || N < 0) return 0;
    const size_t Npad = (size_t)pad64(N), cm = (size_t)(I > dirs * H ? I : dirs * H);
    const int nblk = wfs_dw_blocks((long long)Npad * T, DW_TP, DW_MAXBLK);
    return 2 * cm * T * Npad + (size_t)layers * dirs * (size_t)part_stride(I, H, dirs, nblk);
}

extern "C" int wfs_rnn_fwd(const void *X, int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs,
                           int32_t nonlinearity, const void *param_ptrs, float *saved, void *Y, void *hidden,
                           int32_t dtype, float dropout_p, const int64_t *seed_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_common(N, T, I, H, layers, dirs, nonlinearity, dtype, dropout_p, seed_dev);
    if (rc != WFS_OK) return rc;
    if (N == 0) return WFS_OK;
    WFS_REQUIRE(X && param_ptrs && saved && Y, WFS_EINVAL, "NULL device pointer");
    const Rec *recs = (const Rec *)param_ptrs;
    const long long *seed = (const long long *)seed_dev;
    const long long Npad = pad64(N);
    const int C = dirs * H;
    const bool tanh_ = nonlinearity == WFS_RNN_TANH;
    float *in = saved;  // X transposed, then one slot per layer
    k_rnn_tin<<<t_grid((long long)T * I, Npad), dim3(TT, 8), 0, stream>>>(X, dtype, in, N, Npad, (long long)T * I);
    WFS_LAUNCH_CHECK();
    float *slot = saved + (long long)T * I * Npad;
    for (int l = 0; l < layers; ++l) {
        const int IN = layer_in(I, H, dirs, l);
        const dim3 mgrid((unsigned)((N + MIX_TB - 1) / MIX_TB), (unsigned)T, (unsigned)((C + MIX_CH - 1) / MIX_CH));
        k_rnn_mix<<<mgrid, dim3(MIX_TB), 0, stream>>>(recs, l, dirs, H, IN, 0, in, slot, N, Npad,
                                                      l > 0 && dropout_p > 0.f ? l - 1 : -1, dropout_p, seed);
        WFS_LAUNCH_CHECK();
        const dim3 sgrid((unsigned)(Npad / SCAN_TB), (unsigned)dirs);
        if (H <= 4)
            scan_fwd<4>(tanh_, sgrid, stream, recs, l, dirs, H, slot, N, Npad, T, hidden, dtype);
        else if (H <= 8)
            scan_fwd<8>(tanh_, sgrid, stream, recs, l, dirs, H, slot, N, Npad, T, hidden, dtype);
        else if (H <= 16)
            scan_fwd<16>(tanh_, sgrid, stream, recs, l, dirs, H, slot, N, Npad, T, hidden, dtype);
        else
            scan_fwd<32>(tanh_, sgrid, stream, recs, l, dirs, H, slot, N, Npad, T, hidden, dtype);
        WFS_LAUNCH_CHECK();
        in = slot;
        slot += (long long)T * C * Npad;
    }
    k_rnn_tout<<<t_grid((long long)T * C, Npad), dim3(TT, 8), 0, stream>>>(in, Y, dtype, N, Npad, (long long)T * C);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}

extern "C" int wfs_rnn_bwd(const void *dY, int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs,
                           int32_t nonlinearity, const void *param_ptrs, const float *saved, void *dX, float *workspace,
                           int32_t dtype, float dropout_p, const int64_t *seed_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_common(N, T, I, H, layers, dirs, nonlinearity, dtype, dropout_p, seed_dev);
    if (rc != WFS_OK) return rc;
    WFS_REQUIRE(N >= 1, WFS_EINVAL, "the backward needs at least one row (the gradients of an empty batch are zeros)");
    WFS_REQUIRE(dY && param_ptrs && saved && workspace, WFS_EINVAL, "NULL device pointer");
    const Rec *recs = (const Rec *)param_ptrs;
    const long long *seed = (const long long *)seed_dev;
    const long long Npad = pad64(N);
    const int C = dirs * H, cm = I > C ? I : C;
    const bool tanh_ = nonlinearity == WFS_RNN_TANH;
    const int nblk = wfs_dw_blocks(Npad * T, DW_TP, DW_MAXBLK);
    float *G = workspace, *Gn = G + (long long)cm * T * Npad, *part = Gn + (long long)cm * T * Npad;
    const long long pstride = part_stride(I, H, dirs, nblk);
    k_rnn_tin<<<t_grid((long long)T * C, Npad), dim3(TT, 8), 0, stream>>>(dY, dtype, G, N, Npad, (long long)T * C);
    WFS_LAUNCH_CHECK();
    LayerDims dims = {};
    for (int l = layers - 1; l >= 0; --l) {
        const int IN = layer_in(I, H, dirs, l);
        dims.in[l] = IN;
        const float *S = saved + (long long)T * Npad * (I + (long long)l * C);           // this layer's h
        const float *Xl = l == 0 ? saved : saved + (long long)T * Npad * (I + (long long)(l - 1) * C);  // its input
        const int drop_layer = l > 0 && dropout_p > 0.f ? l - 1 : -1;
        const dim3 sgrid((unsigned)(Npad / SCAN_TB), (unsigned)dirs);
        if (H <= 4)
            scan_bwd<4>(tanh_, sgrid, stream, recs, l, dirs, H, S, G, N, Npad, T);
        else if (H <= 8)
            scan_bwd<8>(tanh_, sgrid, stream, recs, l, dirs, H, S, G, N, Npad, T);
        else if (H <= 16)
            scan_bwd<16>(tanh_, sgrid, stream, recs, l, dirs, H, S, G, N, Npad, T);
        else
            scan_bwd<32>(tanh_, sgrid, stream, recs, l, dirs, H, S, G, N, Npad, T);
        WFS_LAUNCH_CHECK();
        const dim3 dgrid((unsigned)nblk, (unsigned)dirs);
        if (H <= 8)
            k_rnn_dw<8><<<dgrid, dim3(DW_TB), 0, stream>>>(l, dirs, H, IN, G, Xl, S, N, Npad, T, nblk, part, pstride, drop_layer,
                                                          dropout_p, seed);
        else if (H <= 16)
            k_rnn_dw<16><<<dgrid, dim3(DW_TB), 0, stream>>>(l, dirs, H, IN, G, Xl, S, N, Npad, T, nblk, part, pstride, drop_layer,
                                                           dropout_p, seed);
        else
            k_rnn_dw<32><<<dgrid, dim3(DW_TB), 0, stream>>>(l, dirs, H, IN, G, Xl, S, N, Npad, T, nblk, part, pstride, drop_layer,
                                                           dropout_p, seed);
        WFS_LAUNCH_CHECK();
        if (l > 0 || dX) {
            const dim3 mgrid((unsigned)((N + MIX_TB - 1) / MIX_TB), (unsigned)T, (unsigned)((IN + MIX_CH - 1) / MIX_CH));
            k_rnn_mix<<<mgrid, dim3(MIX_TB), 0, stream>>>(recs, l, dirs, H, IN, 1, G, Gn, N, Npad, drop_layer, dropout_p,
                                                          seed);
            WFS_LAUNCH_CHECK();
            float *tmp = G;
            G = Gn;
            Gn = tmp;
        }
    }
    if (dX) {
        k_rnn_tout<<<t_grid((long long)T * I, Npad), dim3(TT, 8), 0, stream>>>(G, dX, dtype, N, Npad, (long long)T * I);
        WFS_LAUNCH_CHECK();
    }
    k_rnn_dw_final<<<dim3(layers, dirs), dim3(DW_TB), 0, stream>>>(recs, dims, dirs, H, part, pstride, nblk);
    WFS_LAUNCH_CHECK();
    return WFS_OK;
}
