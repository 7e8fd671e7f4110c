"""Cases and a float64 NumPy restatement for ClassificationMetrics (csrc/classmetrics.hip, psd/class_metrics.py).

The builder (``make_case``) draws gaussian logits (sigma = 2), rounds them to the row type and forms fp64 probabilities
from the ROUNDED values.  A row that has a probability within ``P_MARGIN`` = 1e-5 of a threshold, or whose two largest
logits lie within ``X_MARGIN`` = 1e-4 of each other, is drawn again, so every drawn row satisfies the margin
(``margin_ok``): on such a row any correct softmax -- fp64 here, fp32 in torch -- gives the same bins and the same
argmax, no row has to be left out of a comparison, and every integer table is compared whole and exactly.

Crafted rows are appended as they are, without the margin; they are exact in any correct arithmetic:
  * all logits equal: exp(0) = 1, the sum is C, p = 1 / C; for C = 2, 4, 5, 10 and T = 100 it lies exactly ON a threshold
    (the same rational, rounded the same way) and counts as ``>=``; the argmax is index 0;
  * one logit 200 above the rest: exp(-200) vanishes against 1 in fp64, so p = 1 meets the last threshold and the others
    round to fp32 zero, below the first;
  * (C >= 3) a tie of the largest logit at indices 1 and C - 1, the rest 200 below: the FIRST index wins, p = 1 / 2 each.

``host_tables`` is the restatement: head (rows counted, correct, loss rows, ignored), confusion [C, C], roc [C, 2, T + 1]
as int64, and the float64 loss mean.  ``naive_tables`` says the same with loops, for the host test of the restatement.

tests/golden/class_metrics_cases.npz (tests/golden/make_class_metrics_goldens.py) holds, for each name in ``RECORDED``,
the builder's logits and labels as they were when the reference ran (``<name>_logits``, ``<name>_labels``) and what the
reference's own ``ROCCurve.update`` / ``compute`` returned for class indices 0 and C - 1 on torch's fp32 CPU softmax of
those logits (``<name>_roc0``, ``<name>_rocl``, float32 [2, T]).
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_metrics_cases.npz")
P_MARGIN, X_MARGIN = 1e-5, 1e-4
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)
# name -> (rows drawn, classes, thresholds, row type, seed)
RECORDED = {"c2_f32": (300, 2, 100, "f32", 11), "c5_f32": (300, 5, 100, "f32", 12), "c5_bf16": (200, 5, 100, "bf16", 13),
            "c4_f16": (200, 4, 100, "f16", 14), "c10_f32": (120, 10, 100, "f32", 15)}


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def thresholds(T):
    return np.array([np.float32((i + 1.0) / T) for i in range(T)], np.float32)


def round_to(x, dtype):
    """float32 array -> the float32 values it takes when stored in ``dtype``."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TORCH_DTYPE[dtype]).float().numpy()


def probabilities(x):
    """fp64 softmax of the stored logits; also the row maximum and the sum of exponentials."""
    x = np.asarray(x, np.float64)
    m = x.max(axis=1, keepdims=True) if x.shape[0] else np.zeros((0, 1))
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, m[:, 0], s[:, 0]


def margin_ok(x, thr):
    """Per row: no probability within P_MARGIN of a threshold, the two largest logits more than X_MARGIN apart."""
    p = probabilities(x)[0]
    near = np.abs(p[:, :, None] - thr.astype(np.float64)[None, None, :]).min(axis=2).min(axis=1) <= P_MARGIN
    top = np.sort(np.asarray(x, np.float64), axis=1)
    return ~near & (top[:, -1] - top[:, -2] > X_MARGIN)


def crafted_rows(C):
    rows = [np.zeros(C, np.float32), np.full(C, -1.5, np.float32)]
    for hot in (0, C - 1):
        r = np.full(C, -3.0, np.float32)
        r[hot] = 197.0                        # 200 above the rest
        rows.append(r)
    if C >= 3:
        r = np.full(C, -198.0, np.float32)
        r[1] = r[C - 1] = 2.0
        rows.append(r)
    return np.stack(rows)


def make_case(n, C, T=100, dtype="f32", seed=0, crafted=True):
    """(logits float32 [N, C] holding ``dtype`` values, labels int64 [N], drawn rows): ``n`` drawn rows that satisfy the
    margin, then the crafted rows once per label 0 and C - 1."""
    rng = np.random.default_rng(seed)
    thr = thresholds(T)
    x = round_to(rng.normal(0.0, 2.0, (n, C)), dtype)
    redrawn = 0
    for _ in range(200):
        bad = np.nonzero(~margin_ok(x, thr))[0] if n else []
        if len(bad) == 0:
            break
        redrawn += len(bad)
        x[bad] = round_to(rng.normal(0.0, 2.0, (len(bad), C)), dtype)
    else:
        raise AssertionError("rows still inside the margin after 200 draws")
    labels = rng.integers(0, C, n).astype(np.int64)
    if crafted:
        cr = round_to(crafted_rows(C), dtype)
        assert np.array_equal(cr, crafted_rows(C))            # every crafted value is exact in all three row types
        x = np.concatenate([x, cr, cr])
        labels = np.concatenate([labels, np.zeros(len(cr), np.int64), np.full(len(cr), C - 1, np.int64)])
    return np.ascontiguousarray(x, np.float32), labels, n, redrawn


def recorded_case(name):
    n, C, T, dtype, seed = RECORDED[name]
    x, labels, _n, _r = make_case(n, C, T, dtype, seed)
    return x, labels, C, T, dtype


def host_tables(x, labels, C, thr, ignore=-100, mask=None, n_valid=None, skip=None):
    """The restatement.  ``x`` float32 [N, C] stored logits, ``mask`` the loss mask, ``n_valid`` the valid count, ``skip``
    a boolean [N] of rows left out of everything (the flagged rows of the flag tests).  Returns a dict: ``head`` = (rows
    counted, correct, loss rows, ignored), ``confusion``, ``roc`` (int64) and ``loss`` (float64 mean, NaN with no row)."""
    N, T = len(labels), len(thr)
    nv = N if n_valid is None else max(0, min(N, int(n_valid)))
    live = np.arange(N) < nv
    if skip is not None:
        live &= ~np.asarray(skip, bool)
    ignored = int((live & (labels == ignore)).sum())
    rows = np.nonzero(live & (labels != ignore))[0]
    xs, lab = np.asarray(x, np.float32)[rows], labels[rows]
    p, m, s = probabilities(xs)
    pred = xs.argmax(axis=1) if len(rows) else np.zeros(0, np.int64)            # the first index of the maximum
    bins = np.searchsorted(thr, p.astype(np.float32), side="right")             # #{i : thr[i] <= p}
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (lab, pred), 1)
    roc = np.zeros((C, 2, T + 1), np.int64)
    for k in range(C):
        np.add.at(roc[k], ((lab == k).astype(np.int64), bins[:, k]), 1)
    nll = m + np.log(s) - xs.astype(np.float64)[np.arange(len(rows)), lab]
    in_loss = np.ones(len(rows), bool) if mask is None else np.asarray(mask)[rows] != 0
    return dict(head=(len(rows), int((pred == lab).sum()), int(in_loss.sum()), ignored), confusion=confusion, roc=roc,
                loss=float(nll[in_loss].sum() / in_loss.sum()) if in_loss.any() else float("nan"))


def naive_tables(x, labels, C, thr, ignore=-100, mask=None, n_valid=None):
    """``host_tables`` with loops and ``math``: one row, one class, one threshold at a time."""
    N, T = len(labels), len(thr)
    nv = N if n_valid is None else max(0, min(N, int(n_valid)))
    n = correct = loss_rows = ignored = 0
    total = 0.0
    confusion, roc = np.zeros((C, C), np.int64), np.zeros((C, 2, T + 1), np.int64)
    for r in range(nv):
        lab = int(labels[r])
        if lab == ignore:
            ignored += 1
            continue
        row = [float(v) for v in x[r]]
        m = max(row)
        pred = row.index(m)
        e = [math.exp(v - m) for v in row]
        s = sum(e)
        n += 1
        correct += pred == lab
        confusion[lab, pred] += 1
        for k in range(C):
            p = np.float32(e[k] / s)
            roc[k, int(lab == k), sum(1 for t in thr if p >= t)] += 1
        if mask is None or mask[r]:
            loss_rows += 1
            total += m + math.log(s) - row[lab]
    return dict(head=(n, correct, loss_rows, ignored), confusion=confusion, roc=roc,
                loss=total / loss_rows if loss_rows else float("nan"))


def rates(roc_k):
    """int64 [2, T + 1] -> (tn, fp, fn, tp), each int64 [T], by counting: positive at threshold i when the bin is above i."""
    T = roc_k.shape[1] - 1
    fp = np.array([roc_k[0, i + 1:].sum() for i in range(T)], np.int64)
    tp = np.array([roc_k[1, i + 1:].sum() for i in range(T)], np.int64)
    return roc_k[0].sum() - fp, fp, roc_k[1].sum() - tp, tp


def reference_curve(roc_k):
    """The reference's ``ROCCurve.compute()`` formula on torchmetrics 0.2's float32 [true, predicted] matrices."""
    tn, fp, fn, tp = (a.astype(np.float32) for a in rates(roc_k))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([tn / (tn + fp), fn / (fn + tp)])
