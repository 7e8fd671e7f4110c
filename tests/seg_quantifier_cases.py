"""Inputs and a vectorised NumPy restatement of the tables behind the reference's SegEvaluator.add
(src/evaluation/SegEvaluator.py over MetricPairAggregator.add_normalized and StatsUtils.ErrorAggregator.add_norm), written
from their behaviour.  tests/test_seg_quantifier_host.py holds it against the values recorded in
tests/golden/seg_quantifier_cases.npz; the GPU tests compare the kernels with the RECORDED values, and use this file only
for the LitSegQuantifier loop.  tools/bench_seg_quantifier.py uses it as the host arm.

The npz (made by tests/golden/make_seg_quantifier_goldens.py) holds, per case ``<name>``:
  <name>_meta          int64 [batches, has_pid, target_index, raises, fixed_edges, nan_rows]; raises = 1: the reference fails
                       on the case (a first subset whose largest |error| is 0 or NaN) and no tables are recorded; nan_rows = 1:
                       a counted row has a NaN error, which makes the reference's metric tables NaN: only the error tables
                       are compared
  <name>_dtype         "f32" / "bf16" / "f16": what results and target are handed to the GPU as (values already rounded)
  <name>_ov            [k, 4] rows (key, low, high, n_bins): bin_overrides
  <name>_fixed         [2]: error_edges fixed in advance (when fixed_edges = 1)
  <name>_b<k>_*        per batch the inputs {coords, results, target, pid, n_valid}; n_valid = -1 means "not given"
  <name>_b<k>_rows     [4, n] per valid row: multiplicity, single-ended flag, category, PID slot
  <name>_one           [3, cells] rows (mean, n, dev) over the 1-D cells [C, n_bins + 2] of the four metrics in order
  <name>_two           [2, cells] rows (sum, n) over the cells of all pairs, 0_1, 0_2, ..
  <name>_error_hist, <name>_error_2d, <name>_error_edges [C, 2], <name>_error_edges_set [C]
"""
import os

import numpy as np

from pid_evaluator_cases import bin_index
from tensor_evaluator_cases import HostRealPairTables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_quantifier_cases.npz")
TOL = 1e-5          # the project's bar for evaluator float tables, of the output's largest magnitude in the golden
E_INDEX, Z_INDEX, PSD_INDEX = 0, 4, 5
CLASS_PIDS = [[1], [4], [6, 258], [256], [512]]
SLOT_PIDS = [1, 4, 6, 258, 256, 512]
SLOT_CLASS = [0, 1, 2, 2, 3, 4]
TORCH_DTYPES = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def case_names(gold):
    return [str(n) for n in gold["case_names"]]


def meta_of(gold, name):
    nb, has_pid, ti, raises, fixed, nan_rows = (int(v) for v in gold[name + "_meta"])
    return dict(batches=nb, has_pid=bool(has_pid), target_index=ti, raises=bool(raises), nan_rows=bool(nan_rows),
                fixed=tuple(float(v) for v in gold[name + "_fixed"]) if fixed else None,
                dtype=str(gold[name + "_dtype"]),
                bin_overrides={int(v[0]): [float(v[1]), float(v[2]), int(v[3])] for v in gold[name + "_ov"]})


def batches_of(gold, name):
    return [{k: gold["%s_b%d_%s" % (name, b, k)] for k in ("coords", "results", "target", "pid", "n_valid")}
            for b in range(int(gold[name + "_meta"][0]))]


def constructor_kwargs(gold, name):
    m = meta_of(gold, name)
    kw = dict(target_index=m["target_index"], bin_overrides=m["bin_overrides"] or None,
              additional_field_names=["PID"] if m["has_pid"] else None)
    if m["fixed"] is not None:
        kw["error_edges"] = m["fixed"]
    return kw


def metric_setup(bin_overrides=None, e_scale=12.0, z_scale=1200.0):
    """(n_bins, normalised ranges) of the four metrics energy / psd / multiplicity / z, and all eight default bins."""
    bins = [[0.0, e_scale, 100], [-15., 15., 100], [0.0, 5000., 100], [0.0, 5000., 100], [-z_scale / 2., z_scale / 2., 100],
            [0.0, 0.6, 100], [0.0, 30., 100], [0.0, 1176., 100]]
    for k, v in (bin_overrides or {}).items():
        bins[int(k)] = list(v)
    params = [bins[0], bins[5], [0.5, 6.5, 6], bins[4]]
    ranges = []
    for (lo, hi, nb), norm in zip(params, [e_scale, 1.0, 1.0, z_scale]):
        w = (hi - lo) / nb
        e = np.arange(lo, hi + w / 2, w)
        lo2, hi2 = float(e[0]), float(e[-1])
        ranges.append((lo2 / norm + 0.5, hi2 / norm + 0.5) if lo2 < 0 else (lo2 / norm, hi2 / norm))
    return [int(p[2]) for p in params], ranges, bins


def error_edge_range(max_abs, nb):
    """(edges[0], edges[-1]) of get_bins(-1.1 max, 1.1 max, nb)."""
    lo, hi = -1.1 * max_abs, 1.1 * max_abs
    w = (hi - lo) / nb
    e = np.arange(lo, hi + w / 2, w)
    return float(e[0]), float(e[-1])


def seg_rows(coords, pid, seg_status, n_valid=-1, has_pid=True):
    """Per valid row: multiplicity, single-ended flag, category and PID slot.  The lookahead ends with the valid rows."""
    n = len(coords) if n_valid < 0 else int(n_valid)
    c = np.asarray(coords)[:n]
    ev = c[:, 2]
    start = np.flatnonzero(np.r_[True, ev[1:] != ev[:-1]]) if n else np.zeros(0, np.int64)
    run = np.repeat(np.arange(len(start)), np.diff(np.r_[start, n]))
    mult = np.diff(np.r_[start, n])[run] if n else np.zeros(0, np.int64)
    se = seg_status[c[:, 0], c[:, 1]] == 0.5
    if has_pid:
        p = np.asarray(pid)[:n].astype(np.int64)
        slot = np.full(n, -1, np.int64)
        for s, v in enumerate(SLOT_PIDS):
            slot[p == v] = s
        slot = np.where(se, slot, -1)
        cat = np.where(slot >= 0, np.asarray(SLOT_CLASS)[np.maximum(slot, 0)], -1)
    else:
        slot, cat = np.zeros(n, np.int64), np.zeros(n, np.int64)
    return dict(mult=mult.astype(np.int32), se=se.astype(np.int32), category=cat.astype(np.int32), slot=slot.astype(np.int32))


class HostSegTables:
    """SegEvaluator's tables on the host: add() per batch, results() in the evaluator's form."""

    def __init__(self, seg_status, target_index=4, bin_overrides=None, has_pid=True, error_edges=None):
        self.seg, self.ti, self.has_pid = np.asarray(seg_status, np.float32), int(target_index), bool(has_pid)
        self.nbins, self.ranges, bins = metric_setup(bin_overrides)
        self.C = 5 if has_pid else 1
        self.names = ["energy", "psd", "multiplicity", "z"]
        self.pairs = HostRealPairTables(self.nbins, self.ranges, self.C)
        self.nb = nb = int(bins[self.ti][2])
        self.error_hist = np.zeros((self.C, nb + 2), np.int64)
        self.error_2d = np.zeros((self.C, nb + 2, nb + 2), np.int64)
        self.edges, self.edges_set = np.zeros((self.C, 2)), np.zeros(self.C, np.int32)
        if error_edges is not None:
            self.edges[:], self.edges_set[:] = error_edges, 1

    def add(self, results, target, coords, pid=None, n_valid=-1):
        r = seg_rows(coords, pid, self.seg, n_valid, self.has_pid)
        n = len(r["mult"])
        res, tg = np.asarray(results, np.float64)[:n], np.asarray(target, np.float64)[:n]
        err = res - tg[:, self.ti]
        params = np.stack([tg[:, E_INDEX], tg[:, PSD_INDEX], r["mult"].astype(np.float64), tg[:, Z_INDEX]])
        self.pairs.add(params, np.abs(err), r["category"])
        slots = range(6) if self.has_pid else [0]
        for s in slots:                       # add_norm once per (class, pid), in class_PIDs order
            sel = r["slot"] == s
            if not sel.any():
                continue
            c = SLOT_CLASS[s] if self.has_pid else 0
            if not self.edges_set[c]:
                m = float(np.abs(err[sel]).max())
                if not (m > 0 and np.isfinite(m)):
                    raise ValueError("a first subset whose largest |error| is 0 or not finite")
                self.edges[c], self.edges_set[c] = error_edge_range(m, self.nb), 1
            np.add.at(self.error_hist[c], bin_index(err[sel], self.edges[c, 0], self.edges[c, 1], self.nb), 1)
            np.add.at(self.error_2d[c], (bin_index(tg[sel, self.ti], 0.0, 1.0, self.nb),
                                         bin_index(res[sel], 0.0, 1.0, self.nb)), 1)

    def results(self):
        return {"metric_pairs": self.pairs.results(self.names), "error_hist": self.error_hist.copy(),
                "error_2d": self.error_2d.copy(), "error_edges": self.edges.copy(),
                "error_edges_set": self.edges_set.copy()}


def expected(gold, name):
    """The recorded tables of a case in the form ``compare`` takes."""
    m = meta_of(gold, name)
    nbins, _ranges, _bins = metric_setup(m["bin_overrides"])
    C = 5 if m["has_pid"] else 1
    one, two, out, at = gold[name + "_one"], gold[name + "_two"], {}, 0
    for i, nb in enumerate(nbins):
        size = C * (nb + 2)
        out["m%d_mean" % i], out["m%d_dev" % i] = one[0, at:at + size].reshape(C, -1), one[2, at:at + size].reshape(C, -1)
        out["m%d_n" % i] = one[1, at:at + size].reshape(C, -1).astype(np.int64)
        at += size
    at = 0
    for i in range(len(nbins) - 1):
        for j in range(i + 1, len(nbins)):
            shape = (C, nbins[i] + 2, nbins[j] + 2)
            size = int(np.prod(shape))
            out["p%d_%d_val" % (i, j)] = two[0, at:at + size].reshape(shape)
            out["p%d_%d_n" % (i, j)] = two[1, at:at + size].reshape(shape).astype(np.int64)
            at += size
    for k in ("error_hist", "error_2d", "error_edges", "error_edges_set"):
        out[k] = gold["%s_%s" % (name, k)]
    return out


def as_expected(res):
    """Results in the evaluator's form (this file's restatement) as the dict ``compare`` takes."""
    from tensor_evaluator_cases import as_expected as pairs_expected
    out = pairs_expected(res["metric_pairs"], ["energy", "psd", "multiplicity", "z"])
    for k in ("error_hist", "error_2d", "error_edges", "error_edges_set"):
        out[k] = res[k]
    return out


def compare(exp, name, res, worst=None, errors_only=False):
    """Counts exactly, ``error_edges`` bit for bit, the real-valued tables within TOL of the recorded output's largest
    magnitude (tensor_evaluator_cases.compare).  ``errors_only``: the error tables and edges alone."""
    from tensor_evaluator_cases import compare as compare_pairs
    if not errors_only:
        compare_pairs(exp, name, res["metric_pairs"], ["energy", "psd", "multiplicity", "z"], worst=worst)
    assert res["error_hist"].dtype == np.int64 and res["error_2d"].dtype == np.int64
    assert np.array_equal(res["error_edges_set"], exp["error_edges_set"]), (name, res["error_edges_set"])
    assert np.array_equal(np.asarray(res["error_edges"], np.float64).view(np.int64),
                          np.asarray(exp["error_edges"], np.float64).view(np.int64)), (name, res["error_edges"], exp["error_edges"])
    assert np.array_equal(res["error_hist"], exp["error_hist"]), (name, "error_hist")
    assert np.array_equal(res["error_2d"], exp["error_2d"]), (name, "error_2d")
