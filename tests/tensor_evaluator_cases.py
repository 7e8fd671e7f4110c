"""Inputs and a vectorised NumPy restatement of the tables behind the reference's TensorEvaluator.add
(src/evaluation/TensorEvaluator.py:70-91 over MetricAggregator.add_normalized, MetricPairAggregator.add_normalized and
StatsAggregator.increment_metric), written from their behaviour.  tests/test_tensor_evaluator_host.py holds it against the
values recorded in tests/golden/tensor_evaluator_cases.npz; the GPU tests compare the kernels with the RECORDED values, and
use this file only for the LitWaveform loop.  tools/bench_tensor_evaluator.py uses it as the host arm.

The restatement is float64 throughout and does not use the kernels' fixed-point image: per batch and cell a two-pass mean
and M2, merged into the running (n, mean, M2) by Chan's pairwise update.

The npz (made by tests/golden/make_tensor_evaluator_goldens.py) holds, per case ``<name>`` (packed into few arrays, to
keep the archive's per-array overhead down):
  <name>_strs          [kind, dtype, metric_name]: kind "tensor" (a TensorEvaluator) or "pairs" (RealMetricPairTables on
                       its own); dtype "f32" / "bf16" / "f16" / "i64", what the target is handed to the GPU as (values
                       already rounded)
  <name>_meta          int64 [batches, n_classes, target_has_phys, target_index (-1: None)]
  <name>_ov            [k, 4] rows (key, low, high, n_bins): bin_overrides (tensor)
  <name>_b<k>_*        per batch the inputs {c, target, results, n_valid} (tensor) or {params, results, category,
                       n_valid} (pairs); n_valid = -1 means "not given"
  <name>_metric_names, <name>_metric_table [P, 6] rows (low, high, n_bins, range low, range high, scale_factor): what the
                       reference's constructor makes; the range is add_normalized's
  <name>_one           [3, cells] rows (mean, n, dev) over the 1-D cells [C, n_bins + 2] of all metrics in order
  <name>_two           [2, cells] rows (sum, n) over the cells [C, n_bins_i + 2, n_bins_j + 2] of all pairs, 0_1, 0_2, ..
  <name>_det           [2, 14, 11, 2]: the per-PMT sum and count (tensor)
"""
import os

import numpy as np

from pid_evaluator_cases import bin_index

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tensor_evaluator_cases.npz")
NX, NY = 14, 11
TOL = 1e-5          # the project's bar for evaluator float tables, of the output's largest magnitude in the golden


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def kind_of(gold, name):
    return str(gold[name + "_strs"][0])


def dtype_of(gold, name):
    return str(gold[name + "_strs"][1])


def case_names(gold, kind=None):
    names = [str(n) for n in gold["case_names"]]
    return [n for n in names if kind is None or kind_of(gold, n) == kind]


def batches_of(gold, name):
    keys = ("c", "target", "results", "n_valid") if kind_of(gold, name) == "tensor" else \
        ("params", "results", "category", "n_valid")
    return [{k: gold["%s_b%d_%s" % (name, b, k)] for k in keys} for b in range(int(gold[name + "_meta"][0]))]


def metrics_of(gold, name):
    """(names, n_bins, ranges, n_classes) as recorded from the reference's constructor."""
    t = gold[name + "_metric_table"]
    return [str(n) for n in gold[name + "_metric_names"]], [int(v) for v in t[:, 2]], [(float(r[3]), float(r[4])) for r in t], \
        int(gold[name + "_meta"][1])


def constructor_kwargs(gold, name):
    """The TensorEvaluator keyword arguments of a "tensor" case."""
    _nb, C, has_phys, ti = (int(v) for v in gold[name + "_meta"])
    kw = dict(target_has_phys=bool(has_phys), target_index=None if ti < 0 else ti,
              metric_name=str(gold[name + "_strs"][2]) or None)
    if len(gold[name + "_ov"]):
        kw["bin_overrides"] = {int(v[0]): [float(v[1]), float(v[2]), int(v[3])] for v in gold[name + "_ov"]}
    if C > 1:
        kw["class_names"] = ["c%d" % i for i in range(C)]
    return kw


def expected(gold, name):
    """The recorded tables of a case: "m<i>_mean" / "_n" / "_dev", "p<i>_<j>_val" / "_n", "det_sum" / "det_n"."""
    _names, nbins, _ranges, C = metrics_of(gold, name)
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
    if name + "_det" in gold:
        out["det_sum"], out["det_n"] = gold[name + "_det"][0], gold[name + "_det"][1].astype(np.int64)
    return out


def _fold(state, cells, values, shape):
    """Chan's update of (n, mean, M2) over ``shape`` with one batch's values at the flat cell indices ``cells``."""
    n, mean, M2 = state
    size = int(np.prod(shape))
    nb = np.bincount(cells, minlength=size).astype(np.int64)
    sb = np.bincount(cells, weights=values, minlength=size)
    mb = np.where(nb > 0, sb / np.maximum(nb, 1), 0.0)
    M2b = np.bincount(cells, weights=(values - mb[cells]) ** 2, minlength=size)
    tot = n.reshape(-1) + nb
    delta = mb - mean.reshape(-1)
    safe = np.maximum(tot, 1)
    mean.reshape(-1)[:] = np.where(nb > 0, mean.reshape(-1) + delta * nb / safe, mean.reshape(-1))
    M2.reshape(-1)[:] += M2b + delta * delta * n.reshape(-1) * nb / safe
    n.reshape(-1)[:] = tot


class HostRealPairTables:
    """(mean, n, dev) per metric and (sum, n) per pair of MetricPairAggregator over real-valued results."""

    def __init__(self, nbins, ranges, C=1):
        self.nbins, self.ranges, self.C = [int(n) for n in nbins], [tuple(r) for r in ranges], int(C)
        P = len(self.nbins)
        self.one = [tuple(np.zeros((C, nb + 2), t) for t in (np.int64, np.float64, np.float64)) for nb in self.nbins]
        self.n2 = {(i, j): np.zeros((C, self.nbins[i] + 2, self.nbins[j] + 2), np.int64)
                   for i in range(P - 1) for j in range(i + 1, P)}
        self.s2 = {k: np.zeros(v.shape, np.float64) for k, v in self.n2.items()}

    def add(self, params, results, category):
        keep = category >= 0
        cat, res = category[keep].astype(np.int64), np.asarray(results, np.float64)[keep]
        b = [bin_index(np.asarray(params[i], np.float64)[keep], *self.ranges[i], self.nbins[i])
             for i in range(len(self.nbins))]
        for i, st in enumerate(self.one):
            _fold(st, cat * (self.nbins[i] + 2) + b[i], res, st[0].shape)
        for (i, j) in self.n2:
            np.add.at(self.n2[(i, j)], (cat, b[i], b[j]), 1)
            np.add.at(self.s2[(i, j)], (cat, b[i], b[j]), res)

    def results(self, names):
        out = {"metrics": {}, "pairs": {}}
        for name, (n, mean, M2) in zip(names, self.one):
            dev = np.where(n > 2, np.sqrt(M2 / np.maximum(n - 1, 1)), 0.0)          # finalize2d
            out["metrics"][name] = (mean.copy(), n.copy(), dev)
        for (i, j), n in self.n2.items():
            out["pairs"]["%d_%d" % (i, j)] = (self.s2[(i, j)].copy(), n.copy())
        return out


def pmt_of(c):
    """(x, y, side, inside) of every row: a detector number [N] decodes as the reference compares it,
    det == 2 * (14 * y + x) + side; rows [N, 3] are (x, y, side).  ``inside``: the reference's loop selects the row."""
    c = np.asarray(c).astype(np.int64)
    if c.ndim == 1:
        x, y, side = (c // 2) % 14, (c // 2) // 14, c % 2
        inside = (c >= 0) & (y < NY)
    else:
        x, y, side = c[:, 0], c[:, 1], c[:, 2]
        inside = (x >= 0) & (x < NX) & (y >= 0) & (y < NY) & (side >= 0) & (side < 2)
    return x, y, side, inside


class HostTensorTables:
    """TensorEvaluator's tables on the host: add() per batch, results() in the evaluator's form."""

    def __init__(self, nbins, ranges, metric_names, metric_name, C=1):
        self.pairs = HostRealPairTables(nbins, ranges, C)
        self.names, self.det_name = list(metric_names), "det_{}".format(metric_name)
        self.det_sum, self.det_n = np.zeros((NX, NY, 2), np.float64), np.zeros((NX, NY, 2), np.int64)

    def add(self, c, target, results, n_valid=-1):
        n = len(results) if n_valid < 0 else int(n_valid)
        c, target, results = np.asarray(c)[:n], np.asarray(target)[:n], np.asarray(results, np.float64)[:n]
        if c.ndim == 2 and c.shape[1] == 1:
            c = c.reshape(-1)
        params = target.T if target.ndim == 2 else target[None, :]
        self.pairs.add(params.astype(np.float64), results, np.zeros(n, np.int32))
        x, y, side, inside = pmt_of(c)
        np.add.at(self.det_n, (x[inside], y[inside], side[inside]), 1)
        np.add.at(self.det_sum, (x[inside], y[inside], side[inside]), results[inside])

    def results(self):
        out = self.pairs.results(self.names)
        out[self.det_name] = (self.det_sum.copy(), self.det_n.copy())
        return out


def compare(exp, name, res, names, det_name=None, scale=1, worst=None):
    """``exp``: ``expected(gold, name)``.  Counts exactly; mean, dev, pair sums and per-PMT sums within TOL of the recorded output's largest magnitude.
    ``scale``: the case was fed ``scale`` times (counts and sums scale, mean does not; dev is then not compared).
    ``worst``: a dict that collects the largest error / scale seen per kind of output."""
    def close(kind, got, want):
        bound = TOL * float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        if worst is not None and np.abs(want).max() > 0:
            worst[kind] = max(worst.get(kind, 0.0), err / float(np.abs(want).max()))
        assert err <= bound, (name, kind, err, bound)

    assert list(res["metrics"]) == list(names)
    for i, mname in enumerate(names):
        mean, n, dev = res["metrics"][mname]
        assert n.dtype == np.int64 and np.array_equal(n, scale * exp["m%d_n" % i]), (name, mname)
        close("mean", mean, exp["m%d_mean" % i])
        if scale == 1:
            close("dev", dev, exp["m%d_dev" % i])
    P = len(names)
    assert sorted(res["pairs"]) == sorted("%d_%d" % (i, j) for i in range(P - 1) for j in range(i + 1, P))
    for key, (val, n) in res["pairs"].items():
        assert val.dtype == np.float64 and n.dtype == np.int64
        assert np.array_equal(n, scale * exp["p%s_n" % key]), (name, key)
        close("pair sum", val, scale * exp["p%s_val" % key])
    if det_name is not None:
        s, n = res[det_name]
        assert s.shape == (NX, NY, 2) and n.dtype == np.int64 and np.array_equal(n, scale * exp["det_n"]), name
        close("per-PMT sum", s, scale * exp["det_sum"])


def as_expected(res, names, det_name=None):
    """Results in the evaluator's form (this file's restatement) as the dict ``compare`` takes."""
    out = {}
    for i, n in enumerate(names):
        out["m%d_mean" % i], out["m%d_n" % i], out["m%d_dev" % i] = res["metrics"][n]
    for key, (val, n) in res["pairs"].items():
        out["p%s_val" % key], out["p%s_n" % key] = val, n
    if det_name is not None:
        out["det_sum"], out["det_n"] = res[det_name]
    return out
