"""Plain float64 NumPy references and case tables for the classifier tail: the streaming head (csrc/head.hip), the sparse
head (csrc/shead.hip), the mapped dense() (csrc/dense.hip) and the fused cross-entropy (k_xent_mean).

NumPy only; the product is not imported.  tests/test_tail_cases_host.py pins the references against each other and
against torch in float64 on the CPU; tests/test_gpu_tail_edges.py compares the kernels with them.

ref_sparse_head is written as loops over the active cells of the map, straight from the formulas of include/wfsparse.h.
It is deliberately NOT ref_linear on a densified tensor: the host test holds the two against each other.
"""
import numpy as np

EMPTY = 0xFFFFFFFF                   # an unset ticket (include/wfsparse.h, wfs_rulebook_cell_map)
KINDS = ("f32", "bf16", "f16")       # row storage types of the kernels
# one round-to-nearest of an fp32 value to the storage type, twice the half-ulp bound (bf16: 2^-9, fp16: 2^-12)
ROUND_REL = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
F16_MIN_NORMAL, F16_MAX = 2.0 ** -14, 65504.0


# ------------------------------------------------------------------------------------------------ rounding, comparing
def round_to(x, kind):
    """x rounded once (to nearest even) to the storage type, returned as float32 holding exactly representable values."""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "f32":
        return x
    if kind == "f16":
        return x.astype(np.float16).astype(np.float32)
    assert kind == "bf16"
    bits = x.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000          # finite inputs only
    return bits.astype(np.uint32).view(np.float32).reshape(x.shape)


def err_ratio(got, want, rel, rel_of_scale=None):
    """max over the elements of |got - want| / (rel * |want| + rel_of_scale * max|want|): <= 1 passes.  Elements where
    ``want`` is not finite must hold the same non-finite value (NaN matches NaN); the scale is taken over the finite
    ones.  A bar of 0 (want all zero) asks for exact equality."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    rel_of_scale = rel if rel_of_scale is None else rel_of_scale
    fin = np.isfinite(want)
    same = np.where(np.isnan(want), np.isnan(got), got == want)
    if not same[~fin].all():
        return float("inf")
    if not fin.any():
        return 0.0
    g, w = got[fin], want[fin]
    if not np.isfinite(g).all():
        return float("inf")
    err = np.abs(g - w)
    bar = rel * np.abs(w) + rel_of_scale * np.abs(w).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bar)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------- references
def ref_linear(x, W, b, g):
    """y = x W^T + b and the gradients of sum(y * g): returns y, dx, dW, db in float64 (b may be None)."""
    x, W, g = np.asarray(x, np.float64), np.asarray(W, np.float64), np.asarray(g, np.float64)
    y = x @ W.T
    if b is not None:
        y = y + np.asarray(b, np.float64)[None, :]
    return y, g @ W, g.T @ x, g.sum(axis=0)


def live_rows(row_of_cell, valid):
    """The map with rows >= valid (and anything negative) turned into -1."""
    r = np.asarray(row_of_cell, np.int64)
    return np.where((r >= 0) & (r < valid), r, -1)


def ref_sparse_head(X, row_of_cell, valid, B, V, C, W, b, G):
    """Y[b][o] = b[o] + sum X[r][c] W[o][c V + cell];  dX[r][c] = sum_o G[b][o] W[o][c V + cell];
    dW[o][c V + cell] = sum_b G[b][o] X[r][c];  dB = sum_b G.  Returns Y, dX, dW, dB and the mask of the rows of dX that
    some live cell references (the other rows are nobody's to write)."""
    X, W, G = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(G, np.float64)
    O = W.shape[0]
    assert W.shape == (O, C * V) and G.shape == (B, O) and X.shape[1] == C
    rows = live_rows(row_of_cell, valid)
    assert rows.shape == (B * V,)
    Y = np.zeros((B, O)) if b is None else np.tile(np.asarray(b, np.float64), (B, 1))
    dX = np.zeros(X.shape)
    dW = np.zeros((O, C * V))
    touched = np.zeros(X.shape[0], bool)
    for at in np.flatnonzero(rows >= 0):
        ev, cell, r = at // V, at % V, rows[at]
        for o in range(O):
            w = W[o, cell::V]                               # the C weights of this cell, V apart
            Y[ev, o] += np.dot(X[r], w)
            dX[r] += G[ev, o] * w
            dW[o, cell::V] += G[ev, o] * X[r]
        touched[r] = True
    return Y, dX, dW, G.sum(axis=0), touched


def ref_dense_mapped(X, row_of_cell, valid, B, V, C):
    """dense() through the map: Y[b][c][cell] = X[row][c] or 0.  Pure data movement: any dtype, returned as it is."""
    X = np.asarray(X)
    rows = live_rows(row_of_cell, valid).reshape(B, V)
    Y = np.zeros((B, C, V), X.dtype)
    for ev, cell in zip(*np.nonzero(rows >= 0)):
        Y[ev, :, cell] = X[rows[ev, cell]]
    return Y


def ref_dense_mapped_bwd(dY, row_of_cell, valid, B, V, C, dX_before):
    """dX[row][c] = dY[b][c][cell of row]; rows that no live cell references keep what ``dX_before`` holds."""
    dY = np.asarray(dY).reshape(B, C, V)
    rows = live_rows(row_of_cell, valid).reshape(B, V)
    dX = np.array(dX_before, copy=True)
    for ev, cell in zip(*np.nonzero(rows >= 0)):
        dX[rows[ev, cell]] = dY[ev, :, cell]
    return dX


def ref_xent_mean(z, t, ignore_index=-100):
    """CrossEntropyLoss(reduction='mean'): max-shifted log-sum-exp in float64.  Returns (loss, dz); NaN and zeros when
    no row counts."""
    z, t = np.asarray(z, np.float64), np.asarray(t, np.int64)
    B, C = z.shape
    counted = (t != ignore_index) & (t >= 0) & (t < C)
    n = int(counted.sum())
    dz = np.zeros((B, C))
    if n == 0:
        return float("nan"), dz
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    se = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(se))[:, 0]
    idx = np.flatnonzero(counted)
    loss = float((lse[idx] - z[idx, t[idx]]).sum() / n)
    dz[idx] = e[idx] / se[idx]
    dz[idx, t[idx]] -= 1.0
    return loss, dz / n


# --------------------------------------------------------------------------------------------------------- cell maps
class CellMap:
    """row_of_cell int64 [B * V] (-1 = empty) and its device form: ``ticket`` uint32 / ``slot`` int32 [B * V].  In the
    "cell_row" form both are views of ONE int32 array (-1 = empty), passed as both pointers."""

    def __init__(self, row_of_cell, ticket, slot, form):
        self.row_of_cell, self.ticket, self.slot, self.form = row_of_cell, ticket, slot, form


def decode_cell_map(ticket, slot):
    """What the kernels read out of (ticket, slot): the row of every cell, -1 where the ticket is unset or the id < 0."""
    ticket, slot = np.asarray(ticket).view(np.uint32), np.asarray(slot, np.int64)
    return np.where((ticket != EMPTY) & (slot >= 0), slot, -1)


def make_cell_map(rng, B, V, M, fill, form):
    """A random injective cell -> row map over B events of V cells and M rows, about ``fill`` of the cells active.

    Always active: the first and the last cell of the first and of the last event (so the tail tile of a V that is no
    multiple of 64 has an active cell).  Always empty: one whole event (B >= 3: with fewer events the corner cells leave
    none), and one cell of the tail tile when it has room (not at B = V = 1).  Row 0 is always referenced (M >= 1); with
    fewer active cells than rows some rows stay unreferenced.

    form="ticket": arbitrary tickets (0 and values with the top bit set among them) and a separate slot array whose
    EMPTY cells hold in-range row ids, so a kernel that ignores the ticket reads a wrong row.
    form="cell_row": one int32 array, -1 = empty, serving as ticket and slot (ops._event_local_conv's map)."""
    assert form in ("ticket", "cell_row") and B >= 1 and V >= 1 and M >= 1
    N = B * V
    forced_on = {0, V - 1, (B - 1) * V, N - 1}
    forced_off = set()
    if B >= 3:
        ev = 1 + int(rng.integers(0, B - 2))
        forced_off |= set(range(ev * V, (ev + 1) * V))
    if V % 64 != 0:          # the tail tile holds cell V - 1 of the first event (active); keep one of its cells empty
        free = [b * V + c for b in range(B) for c in range((V // 64) * 64, V) if (b * V + c) not in forced_on]
        if free and not forced_off.intersection(free):
            forced_off.add(free[int(rng.integers(0, len(free)))])
    forced_on = sorted(forced_on)
    assert len(forced_on) <= M, "M too small for the corner cells"
    others = np.array([c for c in range(N) if c not in forced_off and c not in set(forced_on)], np.int64)
    n_more = int(np.clip(round(fill * N) - len(forced_on), 0, min(len(others), M - len(forced_on))))
    active = np.concatenate([np.array(forced_on, np.int64), rng.choice(others, n_more, replace=False)]).astype(np.int64)
    ids = rng.choice(np.arange(1, M), len(active) - 1, replace=False) if len(active) > 1 else np.zeros(0, np.int64)
    ids = rng.permutation(np.concatenate([[0], ids]).astype(np.int64))          # row 0 referenced, anywhere
    row_of_cell = np.full(N, -1, np.int64)
    row_of_cell[active] = ids
    if form == "cell_row":
        cell_row = row_of_cell.astype(np.int32)
        return CellMap(row_of_cell, cell_row.view(np.uint32), cell_row, form)
    ticket = rng.integers(0, EMPTY, N, dtype=np.uint64).astype(np.uint32)          # never EMPTY itself
    ticket[active[:2]] = np.array([0, 0x80000000], np.uint32)[:len(active[:2])]
    ticket[row_of_cell < 0] = EMPTY
    slot = rng.integers(0, M, N).astype(np.int32)                                   # empty cells: an in-range row id
    slot[active] = ids
    return CellMap(row_of_cell, ticket, slot, form)


# ----------------------------------------------------------------------------------------------------------- values
def make_linear_values(rng, B, I, O, kind):
    """X [B, I] rounded to ``kind``, W [O, I], bias [O], G [B, O] as float32.  For fp16 rows G is positive and the O
    weights of one input share a sign, so |dX| = |sum_o G W| >= 0.5 * 0.05 * O stays in fp16's normal range (no
    cancellation to a subnormal); the other types draw everything from a normal distribution."""
    X = round_to(rng.standard_normal((B, I)), kind)
    if kind == "f16":
        G = rng.uniform(0.5, 1.5, (B, O)).astype(np.float32)
        W = (rng.choice([-1.0, 1.0], (1, I)) * rng.uniform(0.05, 0.25, (O, I))).astype(np.float32)
    else:
        G = rng.standard_normal((B, O)).astype(np.float32)
        W = (rng.standard_normal((O, I)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(O).astype(np.float32)
    return X, W, bias, G


def make_shead_values(rng, M, B, V, C, O, kind):
    """Rows X [M, C] rounded to ``kind`` and the head's W [O, C * V], bias, G [B, O] (make_linear_values' rules)."""
    _x, W, bias, G = make_linear_values(rng, B, C * V, O, kind)
    return round_to(rng.standard_normal((M, C)), kind), W, bias, G


def shead_rows(B, V, fill=0.4, spare=5):
    """Row count of a sparse-head case: the active cells and a few rows no cell references."""
    return max(4, int(round(fill * B * V))) + spare


def make_shead_problem(B, V, C, O, kind, form="ticket", M=None, fill=0.4):
    """One sparse-head case, seeded by its shape: (cell map, M, X, W, bias, G)."""
    rng = np.random.default_rng(7 + 1000003 * B + 1009 * V + 17 * C + O + (0 if form == "ticket" else 500))
    M = shead_rows(B, V, fill) if M is None else M
    cmap = make_cell_map(rng, B, V, M, fill, form)
    X, W, bias, G = make_shead_values(rng, M, B, V, C, O, kind)
    return cmap, M, X, W, bias, G


def make_xent_values(rng, B, C, scale):
    """Logits [B, C] at ``scale``, targets with every 11th row (from row 3) ignored; for B > 1 and C >= 2 one row holds
    [+88, -88, 0, ...]: exp(88) overflows fp32 unless the maximum is subtracted first."""
    z = (rng.standard_normal((B, C)) * scale).astype(np.float32)
    t = rng.integers(0, C, B).astype(np.int64)
    t[3::11] = -100
    if B > 1 and C >= 2:
        r = min(B - 1, 5)
        z[r] = 0.0
        z[r, 0], z[r, 1] = 88.0, -88.0
        t[r] = C - 1
    return z, t


# ------------------------------------------------------------------------------------------------------ case tables
# sparse head.  Grid A: every O x every wave count, 2 tiles (6-cell tail) x 2 slices (1-event tail)
SHEAD_GRID_A = [(O, C, 17, 70) for O in (1, 2, 3, 4) for C in (8, 16, 32, 64)]
SHEAD_GRID_A_IDS = ["O%d_C%d" % (O, C) for (O, C, _B, _V) in SHEAD_GRID_A]
# Grid B at O = 3, C = 32: one cell; V < 64; exact tile and slice; one past both; 3 slices x 2 full tiles; 5 tiles
SHEAD_GRID_B = [(1, 1), (1, 63), (16, 64), (17, 65), (33, 128), (5, 280)]
SHEAD_GRID_B_IDS = ["B%d_V%d" % bv for bv in SHEAD_GRID_B]
SHEAD_B_OC = (3, 32)
SHEAD_VALID = dict(B=17, V=70, C=16, O=2, spare=37)
SHEAD_VALID_CASES = ["all_valid", "partial", "none_valid_nan_rows", "row0_inf"]
# (B, V, C, O) wfs_sparse_head_ok must refuse, and neighbours it must take
SHEAD_REJECTED = [("C4", 2, 8, 4, 3), ("C72", 2, 8, 72, 3), ("C12", 2, 8, 12, 3), ("O0", 2, 8, 32, 0), ("O5", 2, 8, 32, 5),
                  ("V_2p24", 1, 1 << 24, 8, 1), ("OCV_2p31", 1, 1 << 23, 64, 4)]
SHEAD_ACCEPTED = [("C8", 2, 8, 8, 3), ("C64", 2, 8, 64, 3), ("O1", 2, 8, 32, 1), ("O4", 2, 8, 32, 4),
                  ("V_2p24m1", 1, (1 << 24) - 1, 8, 1), ("OCV_2p31m", 1, (1 << 23) - 1, 64, 4)]

# streaming head: scalar kernels below 1024 or I % 8 != 0; 256 threads in [1024, 8192); 1024 threads from 8192
HEAD_I_F32 = [1, 7, 15, 16, 17, 1016, 1024, 1032, 2048, 2056, 4093, 4096, 8184, 8192]
HEAD_I_16BIT = [15, 1024, 2056, 8192]
HEAD_O = list(range(1, 9))
HEAD_O_I = [269, 2056]
HEAD_B = [1, 16, 17, 32, 33, 512, 513]          # head_chunks: ceil(B / 32) clamped to 1 .. 16
HEAD_MODE_I = [269, 2056]
HEAD_DEFAULT = dict(B=37, O=3)


def head_chunks(B):
    return int(min(16, max(1, -(-B // 32))))


def head_is_scalar(I):
    return I % 8 != 0 or I < 1024


# mapped dense
DENSE_CASES = [(C, V) for C in (4, 128) for V in (2, 64, 66)]
DENSE_IDS = ["C%d_V%d" % cv for cv in DENSE_CASES]
DENSE_B = 3

# cross-entropy: the single block strides the rows by 1024
XENT_SHAPES = [(1, 3), (1024, 3), (1025, 2), (7, 1), (5, 4096), (2049, 4)]
XENT_IDS = ["B%d_C%d" % bc for bc in XENT_SHAPES]
XENT_SCALES = [4.0, 60.0]
