"""Inputs and a vectorised NumPy restatement of the tables behind the reference's PIDEvaluator.add and
MetricPairAggregator.add / add_normalized (src/evaluation/PIDEvaluator.py, MetricAggregator.py and the row walks they call
in src/utils/SparseUtils.py), written from their behaviour.  tests/test_pid_evaluator_host.py holds it against the values
recorded in tests/golden/pid_evaluator_cases.npz; the GPU tests compare the kernels with the RECORDED values, and use this
file only where the issue asks for a host restatement (the LitSegClassifier loop).  tools/bench_pid_evaluator.py uses it
as the host arm.

The npz (made by tests/golden/make_pid_evaluator_goldens.py) holds, per case ``<name>``:
  <name>_kind        "pid" or "pairs"
  <name>_nb          number of batches; per batch k the inputs <name>_b<k>_{coords, pred, targ, phys, n_valid} (pid) or
                     <name>_b<k>_{params, result, category, n_valid} (pairs); n_valid = -1 means "not given"
  <name>_dtype       "f32" / "bf16" / "f16": what the phys rows are handed to the GPU as (their values are already rounded)
  <name>_nbins, <name>_ranges, <name>_C   (pairs) the metrics and the class count
  expected           <name>_m<i>_{mean, n, dev}, <name>_p<i>_<j>_{val, n}; pid also <name>_{SE_confusion, confusion_SE,
                     confusion_energy}
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pid_evaluator_cases.npz")
N_CLASSES, N_CONFUSION, N_SE_MAX = 5, 10, 6
E_INDEX, Z_INDEX, PSD_INDEX = 0, 4, 5


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def case_names(gold, kind=None):
    names = [str(n) for n in gold["case_names"]]
    return [n for n in names if kind is None or str(gold[n + "_kind"]) == kind]


def batches_of(gold, name):
    kind = str(gold[name + "_kind"])
    keys = ("coords", "pred", "targ", "phys", "n_valid") if kind == "pid" else ("params", "result", "category", "n_valid")
    return [{k: gold["%s_b%d_%s" % (name, b, k)] for k in keys} for b in range(int(gold[name + "_nb"]))]


def bin_index(v, low, high, nb):
    """get_bin_index over an array: 0 below low, nb + 1 from high, else the first j in 1 .. nb with
    j * ((high - low) / nb) + low > v, 0 if there is none."""
    v = np.asarray(v, np.float64)
    w = (high - low) / nb
    edges = np.arange(1, nb + 1) * w + low
    above = edges[None, :] > v[:, None]
    walk = np.where(above.any(axis=1), above.argmax(axis=1) + 1, 0)
    return np.where(v < low, 0, np.where(v >= high, nb + 1, walk))


def bin_confusion(v, low, high, nb):
    """confusion_accumulate_1d's bin: -1 (dropped) below low or above high, else the first j with edge j above v, minus
    one; 0 if there is none (a value exactly at high)."""
    v = np.asarray(v, np.float64)
    w = (high - low) / nb
    edges = np.arange(1, nb + 1) * w + low
    above = edges[None, :] > v[:, None]
    walk = np.where(above.any(axis=1), above.argmax(axis=1), 0)
    return np.where((v < low) | (v > high), -1, walk)


def table_ints(nbins, C):
    """wfs_metric_pairs_table_ints from the layout of include/wfsparse.h."""
    P = len(nbins)
    n = sum(2 * C * (nbins[i] + 2) for i in range(P))
    return n + sum(2 * C * (nbins[i] + 2) * (nbins[j] + 2) for i in range(P - 1) for j in range(i + 1, P))


class HostPairTables:
    """Count and match-sum tables of MetricPairAggregator over 0/1 results."""

    def __init__(self, nbins, ranges, C):
        self.nbins, self.ranges, self.C = [int(n) for n in nbins], [tuple(r) for r in ranges], int(C)
        P = len(self.nbins)
        self.n1 = [np.zeros((C, nb + 2), np.int64) for nb in self.nbins]
        self.m1 = [np.zeros((C, nb + 2), np.int64) for nb in self.nbins]
        self.n2 = {(i, j): np.zeros((C, self.nbins[i] + 2, self.nbins[j] + 2), np.int64)
                   for i in range(P - 1) for j in range(i + 1, P)}
        self.m2 = {k: np.zeros_like(v) for k, v in self.n2.items()}

    def add(self, params, result, category):
        keep = category >= 0
        cat, res = category[keep].astype(np.int64), result[keep].astype(np.int64)
        b = [bin_index(params[i][keep], *self.ranges[i], self.nbins[i]) for i in range(len(self.nbins))]
        for i in range(len(self.nbins)):
            np.add.at(self.n1[i], (cat, b[i]), 1)
            np.add.at(self.m1[i], (cat, b[i]), res)
        for (i, j) in self.n2:
            np.add.at(self.n2[(i, j)], (cat, b[i], b[j]), 1)
            np.add.at(self.m2[(i, j)], (cat, b[i], b[j]), res)


def pid_rows(coords, pred, targ, phys, seg_status, n_valid=-1):
    """Per-row outputs of PIDEvaluator.add's walks over the valid rows: accuracy, multiplicity, SE mask, n_SE, the [4, N]
    parameters and the category (target on a single-ended row, else -1).  The lookahead ends with the valid rows."""
    n = len(coords) if n_valid < 0 else int(n_valid)
    c, p, t = coords[:n], pred[:n], targ[:n]
    ev = c[:, 2]
    start = np.flatnonzero(np.r_[True, ev[1:] != ev[:-1]]) if n else np.zeros(0, np.int64)
    run = np.repeat(np.arange(len(start)), np.diff(np.r_[start, n]))
    mult = np.diff(np.r_[start, n])[run] if n else np.zeros(0, np.int64)
    se = seg_status[c[:, 0], c[:, 1]] == 0.5
    n_se = np.bincount(run, weights=se, minlength=len(start)).astype(np.int64)[run] if n else np.zeros(0, np.int64)
    ph = np.asarray(phys[:n], np.float32)
    params = np.stack([ph[:, E_INDEX], ph[:, PSD_INDEX], mult.astype(np.float32), ph[:, Z_INDEX]]).astype(np.float32)
    return dict(accuracy=(p == t).astype(np.int32), mult=mult.astype(np.int32), se=se.astype(np.int32),
                n_se=n_se.astype(np.int32), params=params, category=np.where(se, t, -1).astype(np.int32))


class HostPIDTables:
    """PIDEvaluator's tables on the host: add() per batch, results() in the evaluator's form (integer tables only)."""

    def __init__(self, seg_status, nbins, ranges, e_scale=12.0):
        self.seg = np.asarray(seg_status, np.float32)
        self.pairs = HostPairTables(nbins, ranges, N_CLASSES)
        self.e_high = N_CONFUSION / e_scale
        self.SE_confusion = np.zeros((N_CLASSES, N_CLASSES), np.int64)
        self.confusion_SE = np.zeros((N_SE_MAX + 2, N_CLASSES, N_CLASSES), np.int64)
        self.confusion_energy = np.zeros((N_CONFUSION + 1, N_CLASSES, N_CLASSES), np.int64)

    def add(self, coords, pred, targ, phys, n_valid=-1):
        r = pid_rows(coords, pred, targ, phys, self.seg, n_valid)
        n = len(r["accuracy"])
        p, t = pred[:n], targ[:n]
        self.pairs.add(r["params"], r["accuracy"], r["category"])
        se = r["se"] == 1
        np.add.at(self.SE_confusion, (t[se], p[se]), 1)
        k = bin_confusion(r["n_se"], -0.5, N_SE_MAX + 0.5, N_SE_MAX + 1)
        np.add.at(self.confusion_SE, (k[k >= 0], t[k >= 0], p[k >= 0]), 1)
        k = bin_confusion(r["params"][0], 0.0, self.e_high, N_CONFUSION)
        np.add.at(self.confusion_energy, (k[k >= 0], t[k >= 0], p[k >= 0]), 1)
