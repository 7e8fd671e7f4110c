"""``MetricPairTables``: the reference's ``MetricPairAggregator`` (src/evaluation/MetricAggregator.py:339-366, over its
``MetricAggregator`` / ``Metric2DAggregator``) on the GPU: a 0/1 result of every element binned by each of P parameters
and by every pair of them, per class.

``add`` is one HIP launch on the current stream (csrc/metricpairs.hip); nothing is read back until ``results()``.  Both
reference callers feed the aggregator a 0/1 result (``find_matches``, ``calculate_class_accuracy``), so every table is an
exact int64 count -- a count table and a match-sum table -- bit-identical from run to run, and N ranks combine them with
one integer SUM.  The running mean / M2 that ``metric_accumulate_1d`` keeps follow from the two counts in closed form
(``triple_1d``).  Results that are not 0/1 are rejected here; ``RealMetricPairTables`` below takes them (a per-element
loss, the reference's ``TensorEvaluator``).
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .eval_common import FIX_BITS, FIXED_ONE, TableCursor, check_n_valid, raise_flags, read_back, require_gpu

MAX_METRICS = 16                # WFS_METRIC_PAIRS_MAX, include/wfsparse.h
FLAG_TEXT = {4: "a category lay outside class_names",
             8: "a result was neither 0 nor 1"}


def triple_1d(matches, n):
    """(mean, n, dev) of ``metric_accumulate_1d``'s sequential Welford update over 0/1 results, in closed form from the
    sum of matches and the count, after ``finalize`` / ``finalize2d`` (dev = sqrt(M2 / (n - 1)) when n > 2, else 0)."""
    m, c = matches.astype(np.float64), n.astype(np.float64)
    safe = np.where(n > 0, c, 1.0)
    mean = np.where(n > 0, m / safe, 0.0)
    M2 = np.where(n > 0, m * (c - m) / safe, 0.0)
    dev = np.where(n > 2, np.sqrt(M2 / np.where(n > 2, c - 1.0, 1.0)), 0.0)
    return mean, n.copy(), dev


def bin_edge_range(low, high, n_bins):
    """First and last entry of the reference's ``get_bins(low, high, n_bins)`` (src/utils/util.py): what
    ``MetricAggregator`` keeps as ``bin_edges[0]`` / ``bin_edges[-1]`` and bins by."""
    width = (high - low) / n_bins
    edges = np.arange(low, high + width / 2, width)
    return float(edges[0]), float(edges[-1])


def normalized_range(low, high, norm_factor):
    """The range ``MetricAggregator.add_normalized`` bins a parameter normalised to [0, 1] by."""
    if norm_factor is None:
        return 0.0, 1.0
    if low < 0:
        return low / norm_factor + 0.5, high / norm_factor + 0.5
    return low / norm_factor, high / norm_factor


def table_layout(n_bins, n_classes):
    """(key, shape) of every table in the order of include/wfsparse.h; each stands for a count table followed by a
    match-sum table of that shape.  Keys: the metric's index, or ``"i_j"`` for a pair."""
    P, C = len(n_bins), int(n_classes)
    layout = [(i, (C, n_bins[i] + 2)) for i in range(P)]
    for i in range(P - 1):
        for j in range(i + 1, P):
            layout.append(("%d_%d" % (i, j), (C, n_bins[i] + 2, n_bins[j] + 2)))
    return layout


class MetricPairTables:
    # what RealMetricPairTables changes: the entry points, the layout, the result's check and the texts
    _table_ints, _accumulate = "wfs_metric_pairs_table_ints", "wfs_metric_pairs_accumulate"
    _layout_of = staticmethod(table_layout)
    _result_text = "result (0 / 1) and category must be int32 [%(M)d]; real-valued results are not supported"
    _flag_text = FLAG_TEXT

    def __init__(self, device, metrics, class_names):
        """``metrics``: a list of ``(name, low, high, n_bins)``, ``MetricAggregator``'s leading arguments."""
        self._name = name = type(self).__name__
        self.device = require_gpu(device, name)
        self.class_names = list(class_names)
        self.n_classes = len(self.class_names)
        self.names = [str(m[0]) for m in metrics]
        self.n_bins = [int(m[3]) for m in metrics]
        self.P = len(self.names)
        if not 1 <= self.P <= MAX_METRICS or self.n_classes < 1 or min(self.n_bins) < 1:
            raise ValueError("%s: 1 to %d metrics with at least one bin each and at least one class" % (name, MAX_METRICS))
        self.ranges = [bin_edge_range(float(m[1]), float(m[2]), int(m[3])) for m in metrics]
        self._nb = _lib.i32_array(self.n_bins)
        self._layout = self._layout_of(self.n_bins, self.n_classes)
        lib = _lib.load()
        self._accumulate_fn = getattr(lib, self._accumulate)
        n = int(getattr(lib, self._table_ints)(self.P, self._nb, self.n_classes))
        assert n == sum((e[2] if len(e) > 2 else 2) * int(np.prod(e[1])) for e in self._layout)
        self.tables = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, params, result, category, n_valid=None, ranges=None):
        """``params`` float32 [P, M]; ``result`` [M], int32 of 0 / 1 (``RealMetricPairTables``: float32); ``category``
        int32 [M], the class index of every element or -1 to leave it out; ``n_valid`` a device int64 count of the valid
        elements.  ``ranges``: one ``(low, high)`` per metric; the default bins by the metrics' own edges (the
        reference's ``add``), a caller passes ``add_normalized``'s ranges.  One launch on the current stream; no
        read-back."""
        name, M = self._name, int(result.shape[0])
        if params.dtype != torch.float32 or tuple(params.shape) != (self.P, M):
            raise RuntimeError("%s.add: params must be float32 [%d, %d], got %s %s"
                               % (name, self.P, M, params.dtype, tuple(params.shape)))
        if not self._result_ok(result, category, M):
            raise RuntimeError("%s.add: %s" % (name, self._result_text % {"M": M}))
        check_n_valid(n_valid, name + ".add")
        ranges = self.ranges if ranges is None else ranges
        if len(ranges) != self.P:
            raise ValueError("%s.add: one (low, high) per metric" % name)
        lo = (ctypes.c_double * self.P)(*[float(r[0]) for r in ranges])
        hi = (ctypes.c_double * self.P)(*[float(r[1]) for r in ranges])
        p = _lib.ptr
        _lib.check(self._accumulate_fn(
            p(params), p(result), p(category), M, p(n_valid), self.P, lo, hi, self._nb, self.n_classes, p(self.tables),
            p(self.flags), _lib.stream_ptr()))

    @staticmethod
    def _result_ok(result, category, M):
        return result.dtype == torch.int32 and category.dtype == torch.int32 and category.shape[0] == M

    def reset(self):
        self.tables.zero_()
        self.flags.zero_()

    def state_tensors(self):
        """The persistent accumulator: integer sums over batches, so N ranks combine it with one SUM all-reduce."""
        return [self.tables]

    def _check_flags(self):
        raise_flags(self._name, int(self.flags.item()), self._flag_text)

    def split(self, host):
        """``results()`` from the host copy of ``tables``."""
        return split_results(host, self._layout, self.names)

    def results(self):
        """One read-back: ``{"metrics": {name: (mean, n, dev)}, "pairs": {"i_j": (sum of matches, n)}}`` (real-valued:
        the sum of results) with the reference's shapes [C, nb + 2] and [C, nb_i + 2, nb_j + 2]."""
        self._check_flags()
        return self.split(read_back(self.tables).rest())


def split_results(host, layout, names):
    out, cur = {"metrics": {}, "pairs": {}}, TableCursor(host)
    for key, shape in layout:
        n, m = cur.take_pair(shape)
        if isinstance(key, int):
            out["metrics"][names[key]] = triple_1d(m, n)
        else:
            out["pairs"][key] = (m.astype(np.float64), n.copy())
    return out


# ---- real-valued results ---------------------------------------------------------------------------------------------
REAL_TABS = 5                   # per 1-D cell: n, S, Q0, Q1, Q2 (include/wfsparse.h)
REAL_LIMIT = float(1 << 15)     # |result| < 2^15
REAL_FLAG_TEXT = {4: "a category lay outside class_names",
                  8: "a result had no fixed-point image (not finite, or |result| >= 2^15)",
                  16: "the fixed-point sum of a cell left int64"}


def real_triple_1d(n, S, Q0, Q1, Q2):
    """(mean, n, dev) of ``metric_accumulate_1d``'s Welford update after ``finalize2d``, from the integer tables of the
    real-valued accumulate: mean = S / (n 2^32), M2 = (n Q - S^2) / (n 2^64) with Q = Q0 + Q1 2^32 + Q2 2^64, dev =
    sqrt(M2 / (n - 1)) when n > 2, else 0.  Python integers: n Q - S^2 is exact, so a loss that is nearly constant within
    a bin keeps its spread; every quotient is rounded once."""
    mean, dev = np.zeros(n.shape, np.float64), np.zeros(n.shape, np.float64)
    for idx in zip(*np.nonzero(n)):
        k, s = int(n[idx]), int(S[idx])
        mean[idx] = s / (k << FIX_BITS)
        if k > 2:
            q = int(Q0[idx]) + (int(Q1[idx]) << 32) + (int(Q2[idx]) << 64)
            dev[idx] = math.sqrt((k * q - s * s) / ((k * (k - 1)) << (2 * FIX_BITS)))
    return mean, n.copy(), dev


def real_table_layout(n_bins, n_classes):
    """(key, shape, tables) of every group of tables in the order of include/wfsparse.h: five per metric, two per pair."""
    return [(key, shape, REAL_TABS if isinstance(key, int) else 2) for key, shape in table_layout(n_bins, n_classes)]


def raw_real_tables(host, layout):
    """{key: [int64 tables]} of a ``RealMetricPairTables`` buffer: n, S, Q0, Q1, Q2 per metric, n, S per pair."""
    cur = TableCursor(host)
    return {key: [cur.take(shape) for _k in range(tabs)] for key, shape, tabs in layout}


def finish_real_tables(raw, names, last_metric_factor=1):
    """``{"metrics": {name: (mean, n, dev)}, "pairs": {"i_j": (sum, n)}}`` from integer tables; ``last_metric_factor``
    multiplies n, S and Q of the last metric's 1-D table (every row entered that many times)."""
    out = {"metrics": {}, "pairs": {}}
    last = len(names) - 1
    for key, t in raw.items():
        if isinstance(key, int):
            f = last_metric_factor if key == last else 1
            out["metrics"][names[key]] = real_triple_1d(*[a * f for a in t])
        else:
            out["pairs"][key] = (t[1].astype(np.float64) / FIXED_ONE, t[0].copy())
    return out


def split_real_results(host, layout, names):
    return finish_real_tables(raw_real_tables(host, layout), names)


class RealMetricPairTables(MetricPairTables):
    """``MetricPairTables`` for a result that is a real number (a per-element loss): ``MetricPairAggregator`` as the
    reference's ``TensorEvaluator`` feeds it.  Per 1-D cell the count, S = sum v and Q = sum v^2 of the fixed-point images
    v = round(result * 2^32), per pair cell the count and S -- all int64, changed by integer atomics only, so the tables
    are independent of the order of the elements, bit-identical from run to run, and N ranks combine them with one
    integer SUM.  Everything but the attributes below is the base class's."""
    _table_ints, _accumulate = "wfs_metric_pairs_real_table_ints", "wfs_metric_pairs_accumulate_real"
    _layout_of = staticmethod(real_table_layout)
    _result_text = "result must be float32 [%(M)d] and category int32 [%(M)d]"
    _flag_text = REAL_FLAG_TEXT

    @staticmethod
    def _result_ok(result, category, M):
        return result.dtype == torch.float32 and result.dim() == 1 and category.dtype == torch.int32 and \
            tuple(category.shape) == (M,)

    def split(self, host, last_metric_factor=1):
        return finish_real_tables(raw_real_tables(host, self._layout), self.names, last_metric_factor)
