"""Plain float64 NumPy references, table builders and the case table for the 32-channel conv kernels of
csrc/conv_mfma.hip (32 -> 32, 2 -> 32 and the 32 x 2 dW), as they are reached through wfs_gather_conv, wfs_gather_dw and
wfs_conv_backward (csrc/gather_conv.hip).

NumPy only; the product is not imported.  tests/test_conv32_cases_host.py pins the references against the fp32 C oracle
and checks every case's structure on the CPU; tests/test_gpu_conv32_edges.py runs the table through the kernels and
holds every element to a bar on its own scale (ratio() below).

The references are the formulas of include/wfsparse.h, one offset at a time, on the table AS IT IS (no rulebook is
built).  Each returns, beside the value, the sum of the absolute terms of every output element: the element's own
scale, which the bars of a comparison are taken from.

Garbage beyond a device-side row count: table columns, stationary rows and gathered rows that no valid row may reach
hold NaN (values) or the row numbers of NaN rows (table entries) -- always in range, so that a wrong read shows as a
NaN and never as a fault.

Row counts (derived from the launchers at the end of csrc/conv_mfma.hip)
  16-row tiles (fp32 rows, k_gconv16_split / k_gconv16_f32) and 32-row tiles (16-bit rows, k_gconv32_bf16; every dW):
      1, 15, 16, 17, 31, 32, 33        one tile, a partly filled one, one row past a tile -- for both tile heights
  the valid tiles are cut into 8 XCD ranges of ceil(nt / 8) tiles:
      127, 128, 129                    nt = 8 and 9 sixteen-row tiles: at 8 every range holds one tile, at 9 the ranges
                                       hold 2 tiles and the last three are empty (as are ranges at every count below)
  waves per block w = ceil(expect / 256) clamped to 4 .. 12 (three-piece) / 16, in steps of 4; blocks = ceil(expect / w)
  rounded up to 8, at most 256; expect = the tiles, or 7/8 of them with a device-side count:
      16 385                           1025 sixteen-row tiles: w goes from 4 to 8 (fp32 rows).  Also 513 thirty-two-row
                                       tiles = 65 blocks of 8 waves of the 32 x 2 dW: more than 64 slabs, k_slab_reduce
                                       and k_slab_reduce_multi4 slice by 32 instead of 8
      20 000 with 19 990 valid         device count above 7/8 of the capacity: more valid tiles than the grid was sized for.
                                       Every grid stays below its 256-block cap here; waves take further tiles only
                                       because of the 7/8 sizing
      32 801                           1026 thirty-two-row tiles: w of gconv32_grid goes from 4 to 8 for 16-bit rows
                                       (16 385 gives them w = 4, 131 081 w = 16)
      65 552                           4097 sixteen-row tiles > 256 blocks x 16 waves (fp32 instructions; the three-piece
                                       grid of 256 x 12 is passed at 49 152): waves take further tiles off the counter
      131 081                          4097 thirty-two-row tiles > 256 x 16 (16-bit rows): waves stride to a second tile;
                                       also 4097 tiles > 512 blocks x 8 waves of the 32 x 2 dW
      46 112                           1441 thirty-two-row tiles > 36 x 40 = 72 x 20: dw32_blocks at its cap
  32 x 2 dW: one tile per wave, 8 waves per block (= slab):  255, 256, 257 = one slab, exactly one, two
  2 -> 32 forward: one tile per wave, 4 waves per block: 127, 128, 129; its 4096-block cap (524 288 rows) is not run
The two largest counts run sparse tables (25 % live, K = 27) so that their float64 reference takes about a second.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tail_cases import round_to

KINDS = ("f32", "bf16", "f16")
# one round to nearest of the stored value: the unit roundoff of 8 (bf16) and 11 (fp16) significant bits
U_ROUND = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
BAR32 = 1e-5                                                     # of the element's sum of absolute terms
GROUPS = (2, 3, 4, 6)               # SPLIT_GROUP, F16_GROUP, DW_KG / DWB_KG / DWS_KG, BF_GROUP
PACKED_KL = 3


# ------------------------------------------------------------------------------------------------------- references
def _f64(a):
    return np.asarray(a, np.float64)


def _sources(table, kmap, k, identity_k, valid):
    """(rows, source rows) of offset k among the valid rows: the row itself at identity_k, else the live entries of
    table column-map kmap[k]."""
    if k == identity_k:
        rows = np.arange(valid, dtype=np.int64)
        return rows, rows
    col = np.asarray(table[k if kmap is None else kmap[k], :valid], np.int64)
    rows = np.flatnonzero(col >= 0)
    return rows, col[rows]


def ref_gather_conv(table, kmap, K, identity_k, R, valid, X, W, transpose_w, bias):
    """Y[r] = bias + sum_k X[table[kmap[k], r]] . W[k]  (W[k]^T with transpose_w) for r < valid; rows beyond stay 0.
    Returns (Y, sum of |terms|) in float64."""
    X, W = _f64(X), _f64(W)
    Wk = W.transpose(0, 2, 1) if transpose_w else W
    assert X.shape[1] == Wk.shape[1], (X.shape, W.shape, transpose_w)
    Y = np.zeros((R, Wk.shape[2]))
    A = np.zeros_like(Y)
    if bias is not None:
        Y[:valid] = _f64(bias)
        A[:valid] = np.abs(_f64(bias))
    aX, aW = np.abs(X), np.abs(Wk)
    for k in range(K):
        rows, src = _sources(table, kmap, k, identity_k, valid)
        Y[rows] += X[src] @ Wk[k]
        A[rows] += aX[src] @ aW[k]
    return Y, A


def ref_gather_dw(table, kmap, K, identity_k, R, valid, S, G, swap):
    """dW[k, a, b] = sum_{r < valid} S[r, a] G[table[kmap[k], r], b]  (swap: dW[k, b, a]).  Returns (dW, sum |terms|)."""
    S, G = _f64(S), _f64(G)
    assert S.shape[0] == R
    dW = np.zeros((K, S.shape[1], G.shape[1]))
    A = np.zeros_like(dW)
    aS, aG = np.abs(S), np.abs(G)
    for k in range(K):
        rows, src = _sources(table, kmap, k, identity_k, valid)
        dW[k] = S[rows].T @ G[src]
        A[k] = aS[rows].T @ aG[src]
    if swap:
        dW, A = dW.transpose(0, 2, 1), A.transpose(0, 2, 1)
    return np.ascontiguousarray(dW), np.ascontiguousarray(A)


def ref_conv_backward(table, K, identity_k, R, valid, X, dY, W):
    """dX = sum_k dY[table[k]] . W[k]^T and dW[k] = X^T . dY[table[k]] through one by-input table.
    Returns (dX, |dX| terms, dW, |dW| terms)."""
    dX, aX = ref_gather_conv(table, None, K, identity_k, R, valid, dY, W, True, None)
    dW, aW = ref_gather_dw(table, None, K, identity_k, R, valid, X, dY, False)
    return dX, aX, dW, aW


def e32_gather_dw(table, kmap, K, identity_k, R, valid, S, G, swap, want, scale):
    """The error of a plain fp32 evaluation of ref_gather_dw against float64, in units of the element's own scale."""
    S, G = np.asarray(S, np.float32), np.asarray(G, np.float32)
    got = np.zeros((K, S.shape[1], G.shape[1]), np.float32)
    for k in range(K):
        rows, src = _sources(table, kmap, k, identity_k, valid)
        got[k] = S[rows].T @ G[src]
    if swap:
        got = got.transpose(0, 2, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, np.abs(got.astype(np.float64) - want) / scale, 0.0)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------ packed tables
def encode_packed(dense, kl=PACKED_KL):
    """The packed by-input table [K / kl, R] of include/wfsparse.h: entry = row << 3 | (k mod kl) in table row k / kl,
    -1 = none.  ``dense`` [K, R] must hold at most one live entry per (leading offset q = k / kl, row)."""
    dense = np.asarray(dense, np.int32)
    K, R = dense.shape
    assert K % kl == 0 and 1 <= kl <= 8
    packed = np.full((K // kl, R), -1, np.int32)
    for q in range(K // kl):
        block = dense[q * kl:(q + 1) * kl]
        live = block >= 0
        assert (live.sum(axis=0) <= 1).all(), "more than one entry per leading offset and row"
        o = live.argmax(axis=0)
        row = block[o, np.arange(R)]
        packed[q] = np.where(live.any(axis=0), (row << 3) | o, -1)
    return packed


def decode_packed(packed, K, kl=PACKED_KL):
    """The dense [K, R] table the packed one stands for: offset k = q * kl + (e & 7), row e >> 3."""
    packed = np.asarray(packed, np.int32)
    assert packed.shape[0] * kl == K
    dense = np.full((K, packed.shape[1]), -1, np.int32)
    for q in range(packed.shape[0]):
        e = packed[q]
        at = np.flatnonzero(e >= 0)
        dense[q * kl + (e[at] & 7), at] = e[at] >> 3
    return dense


# ------------------------------------------------------------------------------------------------------ table builders
def tile_active_counts(table, identity_k, valid, tile_rows):
    """Per tile of ``tile_rows`` valid rows: the number of offsets with at least one live entry (identity_k counts)."""
    K = table.shape[0]
    nt = -(-valid // tile_rows)
    out = np.zeros(nt, np.int64)
    for t in range(nt):
        live = (table[:, t * tile_rows:min(valid, (t + 1) * tile_rows)] >= 0).any(axis=1)
        if identity_k >= 0:
            live[identity_k] = True
        out[t] = int(live.sum())
    assert out.max(initial=0) <= K
    return out


def active_counts_wanted(K):
    """1, G - 1, G, G + 1 for every pipeline group size G, and K."""
    return sorted({n for n in {1, K} | {g + d for g in GROUPS for d in (-1, 0, 1)} if 1 <= n <= K})


DEAD32, DEAD16, DEAD_ROWS = 1, 6, (5, 70, 130)          # builder (c): tile indices and single rows without any entry
DENSITY = 0.25


def _fill(rng, table, k, rows, n_good):
    table[k, rows] = rng.integers(0, n_good, len(rows))


def build_table(rng, builder, K, R, valid, n_good, identity_k, packed):
    """The dense table [K, R] of one case and a dict of the facts its builder guarantees (checked by
    check_structure).  Entries of the valid columns are rows below ``n_good`` or -1."""
    t = np.full((K, R), -1, np.int32)
    facts = {}
    V = valid
    if builder in ("random", "subm", "single"):
        if packed:
            # at most one offset per leading offset q and row: draw the packed form first
            for q in range(K // PACKED_KL):
                live = np.flatnonzero(rng.random(V) < 0.5)
                o = rng.integers(0, PACKED_KL, len(live))
                t[q * PACKED_KL + o, live] = rng.integers(0, n_good, len(live))
        else:
            live = rng.random((K, V)) < DENSITY
            t[:, :V][live] = rng.integers(0, n_good, int(live.sum()))
        if V > 0 and not (t[:, :V] >= 0).any() and identity_k < 0:
            t[int(rng.integers(0, K)), int(rng.integers(0, V))] = int(rng.integers(0, n_good))     # tiny cases stay live
        if builder == "single" and V > 0:
            k0 = int((identity_k + 1) % K) if identity_k >= 0 else int(rng.integers(0, K))
            t[k0] = -1
            r0 = int(rng.integers(0, V))
            t[k0, r0] = int(rng.integers(0, n_good))
            facts["single"] = (k0, r0)
    elif builder == "dead":
        assert identity_k < 0 and not packed and V >= 160
        live = rng.random((K, V)) < DENSITY
        t[:, :V][live] = rng.integers(0, n_good, int(live.sum()))
        for r in np.flatnonzero(~(t[:, :V] >= 0).any(axis=0)):          # every other row has an entry
            t[int(rng.integers(0, K)), r] = int(rng.integers(0, n_good))
        t[:, DEAD32 * 32:DEAD32 * 32 + 32] = -1
        t[:, DEAD16 * 16:DEAD16 * 16 + 16] = -1
        t[:, list(DEAD_ROWS)] = -1
    elif builder == "active":
        assert not packed
        counts = active_counts_wanted(K)
        for tile in range(-(-V // 32)):
            n = counts[tile % len(counts)]
            pool = [k for k in range(K) if k != identity_k]
            ks = list(rng.choice(pool, n - (1 if identity_k >= 0 else 0), replace=False))
            for lo in (tile * 32, tile * 32 + 16):
                hi = min(V, lo + 16)
                for k in ks:
                    if lo >= hi:
                        continue
                    rows = lo + np.flatnonzero(rng.random(hi - lo) < 0.4)
                    if len(rows) == 0:
                        rows = np.array([int(rng.integers(lo, hi))])
                    _fill(rng, t, int(k), rows, n_good)
    else:
        raise ValueError(builder)
    if identity_k >= 0:
        t[identity_k, :] = -1          # the kernels must take the row itself, not the entry
    return t, facts


def check_structure(case, p):
    """The structure every builder promises, asserted on the CPU before anything runs."""
    t, V, K, ik = p.table, p.valid, case.K, case.identity_k
    assert t.shape == (K, case.R) and t.dtype == np.int32
    assert 0 <= V <= case.R and t.min() >= -1 and t.max(initial=-1) < p.src_rows
    assert (t[:, :V] < p.n_good).all(), "a valid column points at a garbage row"
    if ik >= 0:
        assert (t[ik] == -1).all() and p.src_rows >= case.R and p.n_good >= V
    if V < case.R:                     # garbage columns: in-range row numbers of NaN rows
        g = t[:, V:]
        assert (g >= 0).any() and (g[g >= 0] >= p.n_good).all() and np.isnan(p.B[p.n_good:]).all() and p.n_good < p.src_rows
        if p.A is not None:
            assert np.isnan(p.A[V:]).all()
    assert np.isfinite(p.B[:p.n_good]).all() and (p.A is None or np.isfinite(p.A[:V]).all())
    if case.builder == "random" and ik < 0:
        assert p.src_rows != case.R, "gathers from X_rows != R"
        if K * V >= 2000 and not case.packed:
            assert 0.2 < float((t[:, :V] >= 0).mean()) < 0.3
    if case.packed:
        assert K % PACKED_KL == 0 and ik < 0
        assert ((t.reshape(K // PACKED_KL, PACKED_KL, -1) >= 0).sum(axis=1) <= 1).all()
        assert np.array_equal(decode_packed(p.packed, K)[:, :V], t[:, :V])
    if case.builder == "subm":
        assert ik >= 0
    if case.builder == "dead":
        c16, c32 = tile_active_counts(t, ik, V, 16), tile_active_counts(t, ik, V, 32)
        assert c32[DEAD32] == 0 and c16[DEAD16] == 0 and c16[DEAD16 ^ 1] > 0 and c32[DEAD16 // 2] > 0
        for r in DEAD_ROWS:
            assert (t[:, r] == -1).all() and c16[r // 16] > 0
    if case.builder == "active":
        want = active_counts_wanted(K)
        c16, c32 = tile_active_counts(t, ik, V, 16), tile_active_counts(t, ik, V, 32)
        assert set(want) <= set(c32.tolist()) and set(want) <= set(c16.tolist()), (want, c16, c32)
        assert all(c16[i] == c32[i // 2] for i in range(len(c16)))
    if case.builder == "single" and V > 0:
        k0, r0 = p.facts["single"]
        assert (t[k0, :V] >= 0).sum() == 1 and t[k0, r0] >= 0


# ------------------------------------------------------------------------------------------------------------- cases
SHAPES = {"conv32": (32, 32), "c2c32": (2, 32), "dw32": (32, 32), "dw32x2": (32, 2), "bwd32": (32, 32)}
CASES = []


def _case(name, op, K=27, ik=-1, R=333, valid=None, src=301, kmap=None, builder="random", tr=False, bias=True,
          swap=False, packed=False, kinds=KINDS, long_sum=False, dead=False):
    assert op in SHAPES and kmap in (None, "ident", "mirror", "perm")
    if builder == "random" and ik >= 0:
        builder = "subm"
    CASES.append(SimpleNamespace(name="%s-%s" % (op, name), op=op, K=K, identity_k=ik, R=R, valid=valid, src=src, kmap=kmap,
                                 builder=builder, transpose_w=tr, bias=bias and not tr and op in ("conv32", "c2c32"),
                                 swap=swap, packed=packed, kinds=tuple(kinds), long_sum=long_sum,
                                 all_zero_ok=dead, seed=len(CASES)))


BIG32, MID16, BIG16 = 65552, 32801, 131081
H16 = ("bf16", "f16")

# row counts (the derivation is in the module docstring)
for _R in (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 16385):
    _case("R%d" % _R, "conv32", R=_R, src=_R + 29)
_case("R%d" % BIG32, "conv32", R=BIG32, src=BIG32 - 1000, kinds=("f32",))
_case("R%d" % MID16, "conv32", R=MID16, src=MID16 - 1000, kinds=H16)
_case("R%d" % BIG16, "conv32", R=BIG16, src=BIG16 - 1000, kinds=H16)
for _R in (1, 33, 16385):
    _case("R%d" % _R, "bwd32", R=_R, src=_R + 29, long_sum=_R > 10000)
_case("R%d" % BIG32, "bwd32", R=BIG32, src=BIG32 - 1000, kinds=("f32",), long_sum=True)
_case("R%d" % BIG16, "bwd32", R=BIG16, src=BIG16 - 1000, kinds=H16, long_sum=True)
_case("R33", "dw32", R=33, src=62)
_case("R16385", "dw32", R=16385, src=16414, long_sum=True)
_case("R46112", "dw32", R=46112, src=45000, long_sum=True)
for _R in (256, 257, 16385):
    _case("R%d" % _R, "dw32x2", R=_R, src=_R + 29, long_sum=_R > 10000)
_case("R%d" % BIG16, "dw32x2", R=BIG16, src=BIG16 + 29, kinds=("f32", "bf16"), long_sum=True)
_case("R129", "c2c32", R=129, src=158)
# K (27 is the plain value above); 28 and 32 leave the three-piece / 16-bit fast kernels
for _K in (1, 2, 3, 8, 9, 26, 28, 32):
    _case("K%d" % _K, "conv32", K=_K)
_case("K28", "dw32", K=28)
_case("K28", "bwd32", K=28)
# identity_k: 0, the SubM centre K / 2, K - 1 (the -1 of everything above); K = 1 with the table and without an entry
for _ik in (0, 13, 26):
    _case("ik%d" % _ik, "conv32", ik=_ik)
_case("K1_ik0", "conv32", K=1, ik=0)
_case("K1_ik0", "dw32x2", K=1, ik=0)
_case("ik13", "bwd32", ik=13)
_case("ik13", "dw32", ik=13)
# column maps
_case("ident", "conv32", kmap="ident")
_case("mirror_ik13", "conv32", kmap="mirror", ik=13)
_case("ident", "c2c32", kmap="ident")
_case("mirror_ik13", "c2c32", kmap="mirror", ik=13)
_case("perm", "c2c32", kmap="perm")
_case("ident", "dw32x2", kmap="ident")
_case("mirror_ik13_swap", "dw32x2", kmap="mirror", ik=13, swap=True)
# transposed filters, swapped dW
_case("tr", "conv32", tr=True)
_case("swap", "dw32", swap=True)
# device-side counts over a capacity of 333 rows (200 = 12 sixteen-row tiles + 8 rows = 6 thirty-two-row tiles + 8)
for _v in (0, 1, 200, 332, 333):
    _case("v%d" % _v, "conv32", valid=_v, dead=_v == 0)
for _v in (0, 200):
    _case("v%d" % _v, "bwd32", valid=_v, dead=_v == 0)
    _case("v%d" % _v, "dw32x2", valid=_v, dead=_v == 0)
_case("v0", "dw32", valid=0, dead=True)
_case("v200", "c2c32", valid=200)
_case("v200_ik13_mirror", "conv32", valid=200, ik=13, kmap="mirror")
_case("v200_ik13", "bwd32", valid=200, ik=13)
_case("R20000_v19990", "conv32", R=20000, valid=19990, src=19000)
# tiles without any entry; tiles with 1, G - 1, G, G + 1, K active offsets; one offset live in one row
for _op in ("conv32", "bwd32", "c2c32", "dw32x2"):
    _case("dead", _op, builder="dead")
_case("active", "conv32", builder="active", R=301)
_case("active_ik13", "conv32", builder="active", R=301, ik=13)
_case("active", "bwd32", builder="active", R=301)
_case("single", "conv32", builder="single")
_case("single", "bwd32", builder="single")
# packed by-input tables (kl = 3, K = 27): dX, dW and the one-launch backward
_case("packed", "conv32", tr=True, packed=True)
_case("packed", "dw32", packed=True)
_case("packed", "bwd32", packed=True)
_case("packed_v200", "bwd32", valid=200, packed=True)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases_for(kind, op=None):
    return [c for c in CASES if kind in c.kinds and (op is None or c.op == op)]


def make_kmap(case):
    K = case.K
    if case.kmap is None:
        return None
    if case.kmap == "ident":
        return list(range(K))
    if case.kmap == "mirror":
        return [K - 1 - k for k in range(K)]
    perm = [int(v) for v in np.random.default_rng(1000 + K).permutation(K)]
    assert perm != list(range(K)) and perm != [K - 1 - k for k in range(K)]
    return perm


@functools.lru_cache(maxsize=None)
def make_problem(name, kind):
    """One case in one row type: table (dense; ``packed`` beside it), column map, the stationary rows A [R, Ca] (dW and
    the backward), the gathered rows B [src_rows, Cb], filters and bias -- rows rounded to the row type, filters too for
    16-bit rows.  Read-only: shared between tests."""
    case = BY_NAME[name]
    rng = np.random.default_rng(77000 + case.seed)
    K, R, ik = case.K, case.R, case.identity_k
    V = R if case.valid is None else case.valid
    padded = V < R
    if ik >= 0:                          # the source of offset identity_k is the row itself: same row space
        src_rows = R
        n_good = V if padded else R
    else:
        src_rows = case.src
        n_good = src_rows - 3 if padded else src_rows
    table, facts = build_table(rng, case.builder, K, R, V, n_good, ik, case.packed)
    if padded:                           # garbage columns: row numbers of NaN rows, and no entry
        g = rng.integers(n_good, src_rows, (K, R - V)).astype(np.int32)
        g[rng.random((K, R - V)) < 0.3] = -1
        g[0, 0] = n_good
        if case.packed:                  # still one entry per leading offset
            keep = rng.integers(0, PACKED_KL, (K // PACKED_KL, R - V))
            g = np.where(np.arange(K)[:, None] % PACKED_KL == np.repeat(keep, PACKED_KL, axis=0), g, -1).astype(np.int32)
        if ik >= 0:
            g[ik] = -1
        table[:, V:] = g
    Ca, Cb = SHAPES[case.op]
    W = bias = A = None
    if case.op in ("conv32", "c2c32"):
        Cin, Cout = SHAPES[case.op]
        Cb = Cout if case.transpose_w else Cin
        W = (rng.standard_normal((K, Cin, Cout)) * 0.25).astype(np.float32)
        if case.bias:
            bias = rng.standard_normal(Cout).astype(np.float32)
    else:
        A = round_to(rng.standard_normal((R, Ca)), kind).copy()
        A[V:] = np.nan
        if case.op == "bwd32":
            W = (rng.standard_normal((K, 32, 32)) * 0.25).astype(np.float32)
    if W is not None and kind != "f32":
        W = round_to(W, kind)
    B = round_to(rng.standard_normal((src_rows, Cb)), kind).copy()
    B[n_good:] = np.nan
    p = SimpleNamespace(case=case, kind=kind, table=table, packed=encode_packed(table) if case.packed else None,
                        kmap=make_kmap(case), valid=V, padded=case.valid is not None, src_rows=src_rows, n_good=n_good,
                        A=A, B=B, W=W, bias=bias, facts=facts)
    for a in (table, p.packed, A, B, W, bias):
        if a is not None:
            a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """{tensor: (want float64, sum |terms|)} of one case, computed once.  Packed cases are computed from the PACKED table,
    decoded as include/wfsparse.h documents it."""
    p = make_problem(name, kind)
    c = p.case
    t = decode_packed(p.packed, c.K) if c.packed else p.table
    if c.op in ("conv32", "c2c32"):
        return {"Y": ref_gather_conv(t, p.kmap, c.K, c.identity_k, c.R, p.valid, p.B, p.W, c.transpose_w, p.bias)}
    if c.op in ("dw32", "dw32x2"):
        return {"dW": ref_gather_dw(t, p.kmap, c.K, c.identity_k, c.R, p.valid, p.A, p.B, c.swap)}
    dX, aX, dW, aW = ref_conv_backward(t, c.K, c.identity_k, c.R, p.valid, p.A, p.B, p.W)
    return {"dX": (dX, aX), "dW": (dW, aW)}


def e32_of(name, kind):
    """e32 of the dW of a long-sum case: what a plain fp32 sum of that length loses, for a bar of max(1e-5, 2 e32)."""
    p = make_problem(name, kind)
    c = p.case
    want, scale = reference(name, kind)["dW"]
    t = decode_packed(p.packed, c.K) if c.packed else p.table
    return e32_gather_dw(t, p.kmap, c.K, c.identity_k, c.R, p.valid, p.A, p.B, c.swap, want, scale)


def ratio(got, want, scale, u=0.0):
    """max over ALL elements of |got - want| / (u |want| + BAR32 scale); an element whose bar is 0 must be exact.
    Any non-finite ``got`` gives inf."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    bar = u * np.abs(want) + BAR32 * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(r.max())
