"""Case table, inputs and plain float64 NumPy references for the wide matrix-core products of csrc/wide.hip: the conv
forward / dX (wfs_wide_gather_conv), the conv dW (the wide arm of wfs_gather_dw) and the dense head layer
(wfs_wide_linear_fwd / _bwd).

NumPy only; the product is not imported.  tests/test_wide_cases_host.py pins the references, proves on the CPU that
every case reaches the planning arm it is there for (wfs_wide_plan: host only, nothing launched) and that its inputs
are well-posed; tests/test_gpu_wide_edges.py runs the table through the kernels.

The conv references are conv32_cases.ref_gather_conv / ref_gather_dw (the formulas of include/wfsparse.h on the table as
it is: by-output table with -1 entries, column map, identity offset, bias, transposed filter, valid count); each returns,
beside the value, the element's sum of absolute terms -- the scale its bar is taken from.

Two input sets per case
  exact   rows, dY and bias integers in [-3, 3], filters integers in [-2, 2]: every product and every partial sum is an
          integer below 2^24 (the longest sum of the table has 27 x 2050 terms of at most 6), exact in fp32 in any order
          and any split, so a result must equal float64 bit for bit (16-bit results: float64 rounded to the row type)
  gauss   standard-normal rows rounded to the row type, N(0, 0.05^2) filters (rounded too for 16-bit rows): both sides
          see the same operands

Planning constants restated here only to NAME the arms (the host test compares every claim with wfs_wide_plan): 128 x 128
output tiles, steps of 64 16-bit / 32 fp32 elements, offsets batched while tiles * nz < 384, the contraction cut when
blocks <= 128 and it is at least 16 (fp32: 2) steps long.
"""
import functools
from types import SimpleNamespace

import numpy as np

from conv32_cases import BAR32, U_ROUND, ratio, ref_gather_conv, ref_gather_dw          # noqa: F401  (re-exported)
from tail_cases import round_to

KINDS = ("f32", "bf16", "f16")
DT = {"f32": 0, "bf16": 1, "f16": 2}
SETS = ("exact", "gauss")
E32_MAX = 3e-6
PLAN_CONV, PLAN_DW, PLAN_LIN_FWD, PLAN_LIN_DW = 0, 1, 2, 3
PLAN_FIELDS = ("dense_first", "nz", "nseg", "ksplit", "kchunk", "slabs", "per_offset")


def h16(**kw):
    return dict(bf16=kw, f16=kw)


# ---------------------------------------------------------------------------------------------------------------- conv
# name -> K, R, X_rows, Cx, Cy, table?, column map, identity offset, the arm it is there for and the plan claimed per row type
CONV = {}


def _conv(name, K, R, XR, Cx, Cy, arm, plan, table=True, kmap=None, ik=-1, counts=()):
    assert name not in CONV and (table or (K == 1 and R == XR))
    CONV[name] = SimpleNamespace(name=name, K=K, R=R, XR=XR, Cx=Cx, Cy=Cy, table=table, kmap=kmap, ik=ik, arm=arm,
                                 plan=plan, counts=tuple(counts), seed=len(CONV))


def _p(dense_first, nz, nseg, ksplit, kchunk=None):
    d = dict(dense_first=dense_first, nz=nz, nseg=nseg, ksplit=ksplit)
    if kchunk is not None:
        d["kchunk"] = kchunk
    return d


def _all(**kw):
    return dict(f32=kw, bf16=kw, f16=kw)


def _counts(R):
    """0, 1, round a 128-row tile, the last row, all rows and one above (clamped by the kernels)."""
    return tuple(sorted({v for v in (0, 1, 127, 128, 129, R - 1, R, R + 1) if v >= 0}))


# direct store: one block batch, no split, bias in the epilogue, one partial step (40 < 64 and 40 = 32 + 8)
_conv("direct", 1, 130, 130, 40, 129, "direct", dict(f32=_p(0, 1, 1, 1, 64), **h16(**_p(0, 1, 1, 1, 64))), table=False, ik=0,
      counts=_counts(130))
# smallest R, Cx, Cy and the largest K: row and column clamps of g_load
_conv("R1", 9, 1, 1, 8, 128, "small", _all(**_p(0, 9, 1, 1)))
_conv("Cy8", 2, 127, 127, 128, 8, "small", dict(f32=_p(0, 2, 1, 2), **h16(**_p(0, 2, 1, 1))))
_conv("K128", 128, 40, 40, 8, 128, "small", _all(**_p(0, 128, 1, 1)))
# several offsets per block: 27 offsets over 14 batches of 2, the last batch holds 1; Cx = 72: 2 steps per segment for
# 16-bit rows, 3 for fp32, the last one partial (8 elements)
_conv("nseg2", 27, 640, 640, 72, 300, "nseg2", dict(f32=_p(0, 14, 2, 1, 96), **h16(**_p(0, 14, 2, 1, 128))),
      counts=_counts(640))
_conv("nseg2_subm", 27, 640, 640, 72, 300, "nseg2", dict(f32=_p(0, 14, 2, 1, 96), **h16(**_p(0, 14, 2, 1, 128))),
      kmap="mirror", ik=13, counts=(500,))
# 3 offsets per block, 9 batches, even; one step per segment for 16-bit rows: an odd number of steps
_conv("nseg3", 27, 1920, 1920, 40, 129, "nseg3", dict(f32=_p(0, 9, 3, 1, 64), **h16(**_p(0, 9, 3, 1, 64))))
# one row in the last row tile, 8 columns in the last column tile; 9 offsets over 5 batches, the last holds 1
_conv("tails", 9, 2049, 2049, 136, 264, "nseg2", dict(f32=_p(0, 5, 2, 1, 160), **h16(**_p(0, 5, 2, 1, 192))))
# contraction split, gather-first: last part of 76 elements / of 1 element / exact parts
_conv("split_1100", 1, 130, 130, 1100, 136, "split", dict(f32=_p(0, 1, 1, 18, 64), **h16(**_p(0, 1, 1, 9, 128))),
      table=False, ik=0)
_conv("split_1025", 1, 130, 130, 1025, 129, "split", dict(f32=_p(0, 1, 1, 17, 64), **h16(**_p(0, 1, 1, 9, 128))),
      table=False, ik=0)
_conv("split_1024", 3, 100, 100, 1024, 128, "split", dict(f32=_p(0, 3, 1, 16, 64), **h16(**_p(0, 3, 1, 8, 128))))
# dense-first (fewer source rows) with a split: k_sum_rows adds 17 / 9 slabs per offset (fp32: 33 / 17): its
# four-at-a-time loop and its tail
_conv("dense_2050", 3, 129, 100, 2050, 128, "dense_split", dict(f32=_p(1, 3, 1, 33, 64), **h16(**_p(1, 3, 1, 17, 128))))
_conv("dense_1030", 3, 200, 60, 1030, 130, "dense_split", dict(f32=_p(1, 3, 1, 17, 64), **h16(**_p(1, 3, 1, 9, 128))),
      counts=_counts(200))
_conv("dense_1030_map", 3, 200, 60, 1030, 130, "dense_split", dict(f32=_p(1, 3, 1, 17, 64), **h16(**_p(1, 3, 1, 9, 128))),
      kmap="mirror", counts=(150,))
# dense-first on fp32 rows and filters that need no copy (Cx and both filter widths multiples of 4)
_conv("dense_1028", 3, 129, 100, 1028, 128, "dense_split", dict(f32=_p(1, 3, 1, 17, 64), **h16(**_p(1, 3, 1, 9, 128))))

COUNT_CASES = ("direct", "nseg2", "dense_1030")          # gather-first direct, gather-first with slabs, dense-first


def conv_runs():
    """(case, valid count or None) of every conv product the GPU test runs."""
    out = []
    for c in CONV.values():
        out.append((c.name, None))
        out += [(c.name, v) for v in c.counts]
    return out


def kmap_of(c):
    return None if c.kmap is None else [c.K - 1 - k for k in range(c.K)]


def build_table(rng, K, R, XR, ik):
    """By-output table [K, R], about half of it live: it names source row 0 and the last source row, column 0 has every
    offset, the last column (and one in the middle) none."""
    t = rng.integers(0, XR, size=(K, R)).astype(np.int32)
    t[rng.random((K, R)) < 0.5] = -1
    t[:, 0] = rng.integers(0, XR, K)
    t[0, 0] = XR - 1
    if K > 1:
        t[K - 1, 0] = 0
    elif R > 2:
        t[0, 1] = 0
    if R > 1:
        t[:, R - 1] = -1
    if R > 4:
        t[:, R // 2] = -1
    if ik >= 0:
        t[ik] = -1                     # the kernels must take the row itself, not the entry
    return t


def _draw(rng, shape, which, kind, sigma=1.0, lim=3):
    if which == "exact":
        return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)
    a = rng.standard_normal(shape) * sigma
    return round_to(a, kind).astype(np.float64)


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def conv_problem(name, kind, which, transpose_w):
    """One conv case in one row type and orientation: table, column map, rows X [X_rows, Cx], fp32 filters W
    ([K, Cx, Cy], transposed: [K, Cy, Cx]) and bias (forward only).  Values of the row type (filters of fp32 rows: fp32).
    Read-only: shared between tests."""
    c = CONV[name]
    rng = np.random.default_rng(91000 + 10 * c.seed + (1 if transpose_w else 0))
    table = build_table(rng, c.K, c.R, c.XR, c.ik) if c.table else None
    X = _draw(rng, (c.XR, c.Cx), which, kind)
    Wshape = (c.K, c.Cy, c.Cx) if transpose_w else (c.K, c.Cx, c.Cy)
    W = _draw(rng, Wshape, which, kind, 0.05, 2)
    bias = None if transpose_w else _draw(rng, (c.Cy,), which, "f32")
    _freeze(table, X, W, bias)
    return SimpleNamespace(case=c, kind=kind, which=which, transpose_w=transpose_w, table=table, kmap=kmap_of(c), X=X, W=W,
                           bias=bias)


@functools.lru_cache(maxsize=None)
def conv_reference(name, kind, which, transpose_w):
    """(Y float64, sum |terms|) over ALL R rows: a row depends on its own table column only, so a device-side count v keeps
    rows [0, v) of this."""
    p = conv_problem(name, kind, which, transpose_w)
    c = p.case
    t = p.table if p.table is not None else np.full((c.K, c.R), -1, np.int32)
    Y, A = ref_gather_conv(t, p.kmap, c.K, c.ik, c.R, c.R, p.X, p.W, transpose_w, p.bias)
    _freeze(Y, A)
    return Y, A


def conv_rows_needed(p, valid):
    """Source rows the first ``valid`` output rows read: every other row may hold NaN."""
    c = p.case
    need = np.zeros(c.XR, bool)
    if c.ik >= 0:
        need[:valid] = True
    if p.table is not None:
        e = p.table[:, :valid]
        need[e[e >= 0]] = True
    return need


def conv_e32(name, kind, transpose_w):
    """Error of a plain fp32 evaluation of the gauss reference (offset after offset) against float64, of the scale."""
    p = conv_problem(name, kind, "gauss", transpose_w)
    c = p.case
    want, scale = conv_reference(name, kind, "gauss", transpose_w)
    X, W = p.X.astype(np.float32), p.W.astype(np.float32)
    Wk = W.transpose(0, 2, 1) if transpose_w else W
    Y = np.zeros((c.R, Wk.shape[2]), np.float32)
    if p.bias is not None:
        Y += p.bias.astype(np.float32)
    for k in range(c.K):
        if k == c.ik:
            rows = src = np.arange(c.R)
        else:
            col = p.table[k if p.kmap is None else p.kmap[k]]
            rows = np.flatnonzero(col >= 0)
            src = col[rows]
        Y[rows] += X[src] @ Wk[k]
    return _worst(Y, want, scale)


def _worst(got32, want, scale):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, np.abs(got32.astype(np.float64) - want) / scale, 0.0)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------ dW
DW = {}


def _dw(name, K, R, Cs, Cg, arm, plan, kmap=None, ik=-1, counts=(), table=True):
    DW[name] = SimpleNamespace(name=name, K=K, R=R, GR=R + 29 if (table and ik < 0) else R, Cs=Cs, Cg=Cg, arm=arm, plan=plan,
                               kmap=kmap, ik=ik, counts=tuple(counts), table=table, seed=len(DW))


def _s(ksplit, kchunk):
    return dict(ksplit=ksplit, kchunk=kchunk)


# the 16-bit split threshold: 16 steps of 64 rows
_dw("R1024", 1, 1024, 128, 8, "split", dict(f32=_s(16, 64), **h16(**_s(8, 128))))
_dw("R1023", 1, 1023, 128, 8, "whole", dict(f32=_s(16, 64), **h16(**_s(1, 1024))))
_dw("split_9", 1, 1100, 136, 129, "split", dict(f32=_s(18, 64), **h16(**_s(9, 128))),
    counts=("neg", 0, 1, "kchunk-1", "kchunk", "kchunk+1", 1099, 1100))
_dw("split_17", 1, 2049, 128, 128, "split", dict(f32=_s(33, 64), **h16(**_s(17, 128))), table=False, ik=0)
_dw("split_9_K3", 3, 1100, 40, 130, "split", dict(f32=_s(18, 64), **h16(**_s(9, 128))), ik=1)
# kchunk = 192: 3 steps per part for 16-bit rows, an odd count
_dw("odd_steps", 9, 1100, 130, 129, "split", dict(f32=_s(7, 160), **h16(**_s(6, 192))), kmap="mirror")
_dw("R63", 1, 63, 128, 8, "whole", dict(f32=_s(1, 64), **h16(**_s(1, 64))))
_dw("R64", 1, 64, 128, 8, "whole", dict(f32=_s(1, 64), **h16(**_s(1, 64))))


def dw_count(c, v, kchunk):
    """A count of the table as a number: 'neg' = -5, 'kchunk+-1' around the first part boundary of this row type."""
    if v == "neg":
        return -5
    if isinstance(v, str):
        return kchunk + {"kchunk-1": -1, "kchunk": 0, "kchunk+1": 1}[v]
    return v


def dw_runs():
    out = []
    for c in DW.values():
        out.append((c.name, None))
        out += [(c.name, v) for v in c.counts]
    return out


@functools.lru_cache(maxsize=None)
def dw_problem(name, kind, which):
    c = DW[name]
    rng = np.random.default_rng(93000 + c.seed)
    table = build_table(rng, c.K, c.R, c.GR, c.ik) if c.table else None
    S = _draw(rng, (c.R, c.Cs), which, kind)
    G = _draw(rng, (c.GR, c.Cg), which, kind)
    _freeze(table, S, G)
    return SimpleNamespace(case=c, kind=kind, which=which, table=table, kmap=kmap_of(c), S=S, G=G)


@functools.lru_cache(maxsize=None)
def dw_reference(name, kind, which, valid, swap):
    """(dW float64, sum |terms|) over the first ``valid`` rows (clamped to [0, R])."""
    p = dw_problem(name, kind, which)
    c = p.case
    v = min(max(valid, 0), c.R)
    t = p.table if p.table is not None else np.full((c.K, c.R), -1, np.int32)
    dW, A = ref_gather_dw(t, p.kmap, c.K, c.ik, c.R, v, p.S, p.G, swap)
    _freeze(dW, A)
    return dW, A


def dw_e32(name, kind):
    p = dw_problem(name, kind, "gauss")
    c = p.case
    want, scale = dw_reference(name, kind, "gauss", c.R, False)
    S, G = p.S.astype(np.float32), p.G.astype(np.float32)
    got = np.zeros((c.K, c.Cs, c.Cg), np.float32)
    for k in range(c.K):
        if k == c.ik:
            rows = src = np.arange(c.R)
        else:
            col = p.table[k if p.kmap is None else p.kmap[k]]
            rows = np.flatnonzero(col >= 0)
            src = col[rows]
        got[k] = S[rows].T @ G[src]
    return _worst(got, want, scale)


# -------------------------------------------------------------------------------------------------------------- linear
LIN = {}


def _lin(name, B, I, O, arm, plan):
    LIN[name] = SimpleNamespace(name=name, B=B, I=I, O=O, arm=arm, plan=plan, seed=len(LIN))


# plan: (forward ksplit, dW ksplit) per row type
_lin("smallest", 1, 256, 9, "small", dict(f32=(4, 1), bf16=(1, 1), f16=(1, 1)))
_lin("dw_split", 1100, 256, 9, "dw_split", dict(f32=(4, 18), bf16=(1, 9), f16=(1, 9)))
_lin("fwd_split", 129, 1030, 130, "fwd_split", dict(f32=(17, 3), bf16=(9, 1), f16=(9, 1)))
_lin("last_part_1", 2, 2049, 129, "fwd_split", dict(f32=(33, 1), bf16=(17, 1), f16=(17, 1)))
# dX contracts over O: 1100 terms, so that the exact set's dX leaves the integers bf16 holds (beyond 256)
_lin("long_dx", 130, 256, 1100, "long_dx", dict(f32=(4, 3), bf16=(1, 1), f16=(1, 1)))


@functools.lru_cache(maxsize=None)
def lin_problem(name, kind, which):
    """x [B, I] (row type), W [O, I] and b [O] (fp32; W of the row type's values for 16-bit rows), dY [B, O] (fp32 holding
    values of the row type: the backward rounds it to the row type as an operand)."""
    c = LIN[name]
    rng = np.random.default_rng(95000 + c.seed)
    x = _draw(rng, (c.B, c.I), which, kind)
    W = _draw(rng, (c.O, c.I), which, kind, 0.05, 2)
    b = _draw(rng, (c.O,), which, "f32")
    g = _draw(rng, (c.B, c.O), which, kind)
    _freeze(x, W, b, g)
    return SimpleNamespace(case=c, kind=kind, which=which, x=x, W=W, b=b, g=g)


def ref_linear(x, W, b, g):
    """{tensor: (value, sum |terms|)} of y = x W^T + b, dX = g W, dW = g^T x, db = sum_rows g in float64."""
    x, W, b, g = (np.asarray(a, np.float64) for a in (x, W, b, g))
    ax, aW, ag = np.abs(x), np.abs(W), np.abs(g)
    return {"y": (x @ W.T + b, ax @ aW.T + np.abs(b)), "dX": (g @ W, ag @ aW), "dW": (g.T @ x, ag.T @ ax),
            "db": (g.sum(0), ag.sum(0))}


@functools.lru_cache(maxsize=None)
def lin_reference(name, kind, which):
    p = lin_problem(name, kind, which)
    ref = ref_linear(p.x, p.W, p.b, p.g)
    for v, a in ref.values():
        _freeze(v, a)
    return ref


def lin_e32(name, kind):
    """{tensor: e32} of the gauss set."""
    p = lin_problem(name, kind, "gauss")
    ref = lin_reference(name, kind, "gauss")
    x, W, b, g = (a.astype(np.float32) for a in (p.x, p.W, p.b, p.g))
    db = np.zeros(g.shape[1], np.float32)
    for r in range(g.shape[0]):                        # index order: row after row
        db += g[r]
    got = {"y": x @ W.T + b, "dX": g @ W, "dW": g.T @ x, "db": db}
    return {k: _worst(got[k], *ref[k]) for k in got}


def plan_of(lib, which, kind, K, R, XR, Ca, Cb, has_table=1):
    """wfs_wide_plan as a (taken, dict) pair."""
    import ctypes
    out = (ctypes.c_int32 * 7)(*([-7] * 7))
    rc = lib.wfs_wide_plan(which, K, R, XR, Ca, Cb, has_table, DT[kind], out)
    return rc, dict(zip(PLAN_FIELDS, [int(v) for v in out]))
