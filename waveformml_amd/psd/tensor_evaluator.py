"""``TensorEvaluator``: the reference's evaluator of the per-pulse module (src/evaluation/TensorEvaluator.py on
AD1Evaluator / StatsAggregator) on the GPU: the per-row loss of a ``LitWaveform`` test batch summed per PMT, binned by
every physics quantity of the target and by every pair of them.

The reference's ``add`` copies four tensors to the host, builds 308 boolean masks over the batch (one per (x, y, side))
and walks the rows 8 + 28 times.  Here ``add`` is two HIP launches on the current stream (csrc/metricpairs.hip: one thread
per row, then the real-valued pairwise accumulate); nothing is read back until ``results()``.  Every table is int64 and
changes through integer atomics only -- counts, and sums of the fixed-point image round(loss * 2^32) of every row's loss
and of its square (psd/metric_pairs.RealMetricPairTables) -- so the tables do not depend on the order of the rows, are
bit-identical from run to run, and N ranks combine them with one integer SUM.

What is mirrored: the constructor arithmetic (``E_scale``, ``default_bins`` with ``bin_overrides``, ``scale_factor``, the
metrics of ``_init_results`` in its three modes and their ``norm_factor``) and the tables of ``add``.  Not mirrored: plots
and TensorBoard, the calibration database (``calgroup`` raises), ``metric_unit`` (kept, it only labels plots).

Where this departs from a reference run:

* A loss that is not finite, or whose magnitude reaches 2^15, has no fixed-point image: ``results()`` raises, where the
  reference carries the NaN into every bin the row touches.
* The per-PMT tables are float64 sums and int64 counts (the reference keeps float32 and int32).
* ``c`` of shape [N, 1] is read as detector numbers [N]; the reference compares such a column with (i, j, k) by
  broadcasting, which selects rows only where i = j = k.
"""
import numpy as np
import torch

from .. import _lib
from .eval_common import (FIXED_ONE, check_n_valid, raise_flags, read_back, require_device_tensors, require_gpu,
                          reserve_rows)
from .metric_pairs import REAL_FLAG_TEXT, RealMetricPairTables, normalized_range
from .pid_evaluator import CELL_LENGTH, E_NORMALIZATION_FACTOR, Z_NORMALIZATION_FACTOR, default_bins

PHYS_NAMES = ["Energy", "dt", "PE0", "PE1", "z", "PSD", "t offset", "distance to PMT"]
PHYS_UNITS = ["MeV", "ns", "", "", "mm", "", "ns", "mm"]
_TARGET_CODES = {torch.float32: _lib.WFS_F32, torch.bfloat16: _lib.WFS_BF16, torch.float16: _lib.WFS_F16,
                 torch.int64: _lib.WFS_TENSOR_TARGET_I64}


def metric_setup(e_scale=None, target_has_phys=False, target_index=None, metric_name=None, metric_unit=None,
                 bin_overrides=None):
    """The constructor arithmetic of the reference (AD1Evaluator.__init__, TensorEvaluator.__init__ / _init_results,
    MetricAggregator): the metrics ``(name, low, high, n_bins)``, their ``norm_factor`` and the ranges ``add_normalized``
    bins by, the metric's ``scale_factor`` and the scale of the per-PMT tables."""
    E_scale, E_adjust = E_NORMALIZATION_FACTOR, 1.0
    if e_scale:
        E_adjust = E_scale / e_scale
        E_scale = e_scale
    PE_scale = 5000. / E_adjust
    scales = [E_scale, 30., PE_scale, PE_scale, Z_NORMALIZATION_FACTOR, 1.0, 30., CELL_LENGTH]    # scale_factor(index)
    bins = default_bins(E_scale, Z_NORMALIZATION_FACTOR, E_adjust, bin_overrides)
    if target_index is not None:
        if metric_name is None:
            metric_name = "mean absolute error"
        if metric_unit is None:
            metric_unit = PHYS_UNITS[target_index]
            if "squared" in metric_name:
                metric_unit += "^2"
    if target_has_phys:
        if target_index is None:
            raise RuntimeError("target is tensor of phys quantities, must pass the target index to the evaluator")
        metrics = [(name, *bins[i]) for i, name in enumerate(PHYS_NAMES)]
        norm = list(scales)
        scale = det_scale = scales[target_index]
    elif target_index is not None:
        metrics, norm = [(PHYS_NAMES[target_index], *bins[target_index])], [None]
        scale, det_scale = scales[target_index], 1
    else:
        metrics, norm = [("unknown" if metric_name is None else metric_name, 0., 1., 40)], [None]
        scale, det_scale = 1., 1
    return dict(E_scale=E_scale, E_adjust=E_adjust, default_bins=bins, metrics=metrics, norm_factors=norm,
                metric_name=metric_name, metric_unit=metric_unit, scale_factor=scale, det_scale_factor=det_scale)


class TensorEvaluator:
    def __init__(self, device, calgroup=None, e_scale=None, target_has_phys=False, target_index=None, metric_name=None,
                 metric_unit=None, class_names=None, bin_overrides=None):
        self.device = require_gpu(device, "TensorEvaluator")
        if calgroup is not None:
            raise RuntimeError("TensorEvaluator: calgroup (the PROSPECT_CALDB calibration database) is not supported; the segment "
                               "evaluators take the curves as calibration= (psd/calibration.py)")
        self.nx, self.ny = 14, 11
        setup = metric_setup(e_scale, target_has_phys, target_index, metric_name, metric_unit, bin_overrides)
        self.E_scale, self.E_adjust, self.z_scale = setup["E_scale"], setup["E_adjust"], Z_NORMALIZATION_FACTOR
        self.default_bins = setup["default_bins"]
        self.target_has_phys, self.target_index = bool(target_has_phys), target_index
        self.metric_name, self.metric_unit = setup["metric_name"], setup["metric_unit"]
        self.class_names = list(class_names) if class_names else ["Single"]
        self.metrics, self.norm_factors = setup["metrics"], setup["norm_factors"]
        self.scale_factor, self.det_scale_factor = setup["scale_factor"], setup["det_scale_factor"]
        self.metric_pairs = RealMetricPairTables(self.device, self.metrics, self.class_names)
        self.metric_names = self.metric_pairs.names
        self.P = self.metric_pairs.P
        # MetricAggregator.add_normalized's ranges
        self.normalized_ranges = [normalized_range(lo, hi, nf)
                                  for (lo, hi), nf in zip(self.metric_pairs.ranges, self.norm_factors)]
        self.det_name = "det_{}".format(self.metric_name)
        self.det_tables = torch.zeros(2 * self.nx * self.ny * 2, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._rows_cap = -1

    def add(self, c, f, target, results, n_valid=None):
        """The reference's signature (TensorEvaluator.add): ``c`` int32 / int64 detector numbers [N] or (x, y, side) rows
        [N, 3]; ``f`` the rows (not used, as in the reference); ``target`` [N, 8] fp32 / bf16 / fp16 with
        ``target_has_phys``, else [N] of those types or of int64 class indices; ``results`` the per-row loss [N].
        ``n_valid``: device-side row count of a capacity-padded batch.  Two launches on the current stream; no
        read-back, the caller's tensors are only read."""
        require_device_tensors(c, target, results)
        if c.dim() == 2 and c.shape[1] == 1:
            c = c.reshape(-1)
        rows = int(c.shape[0])
        if c.dtype not in (torch.int32, torch.int64) or not (c.dim() == 1 or (c.dim() == 2 and c.shape[1] == 3)):
            raise RuntimeError("TensorEvaluator.add: c must be int32 / int64 detector numbers [N] or (x, y, side) rows "
                               "[N, 3], got %s %s" % (c.dtype, tuple(c.shape)))
        want = (rows, self.P) if self.target_has_phys else (rows,)
        if tuple(target.shape) != want:
            raise RuntimeError("TensorEvaluator.add: target must be %s, got %s" % (list(want), tuple(target.shape)))
        if tuple(results.shape) != (rows,):
            raise RuntimeError("TensorEvaluator.add: results must be the per-row loss [%d], got %s"
                               % (rows, tuple(results.shape)))
        check_n_valid(n_valid, "TensorEvaluator.add")
        if rows == 0:
            return
        if target.dtype not in _TARGET_CODES:
            target = target.to(torch.float32)
        results = results.detach().to(torch.float32).contiguous()
        c, target = c.contiguous(), target.detach().contiguous()
        reserve_rows(self, rows, [("parameters", torch.float32, (self.P, -1)), ("category", torch.int32, (-1,))])
        p = _lib.ptr
        _lib.check(_lib.load().wfs_tensor_rows(
            p(c), int(c.dtype == torch.int64), 1 if c.dim() == 1 else 3, p(target), _TARGET_CODES[target.dtype], self.P,
            p(results), rows, p(n_valid), self.nx, self.ny, p(self.parameters), p(self.category), p(self.det_tables),
            p(self.flags), _lib.stream_ptr()))
        self.metric_pairs.add(self.parameters, results, self.category, n_valid, ranges=self.normalized_ranges)

    def reset(self):
        self.det_tables.zero_()
        self.flags.zero_()
        self.metric_pairs.reset()

    def state_tensors(self):
        """The persistent accumulators: integer sums over batches, so N ranks combine them with one SUM all-reduce each."""
        return [self.det_tables] + self.metric_pairs.state_tensors()

    def results(self):
        """One read-back.  ``metrics`` = {name: (mean, n, dev)} and ``pairs`` = {"i_j": (sum, n)} as
        ``RealMetricPairTables.results()`` (``pairs`` is empty for a single metric), ``det_<metric_name>`` = (loss sum
        [14, 11, 2] float64, n [14, 11, 2] int64), ``scale_factor`` what the reference scales the metric by in its
        plots."""
        mp = self.metric_pairs
        cur = read_back(self.flags, mp.flags, self.det_tables, mp.tables)
        raise_flags("TensorEvaluator", int(cur.take(1)[0]) | int(cur.take(1)[0]), REAL_FLAG_TEXT)
        n, s = cur.take_pair((self.nx, self.ny, 2))
        res = mp.split(cur.rest())
        res[self.det_name] = (s.astype(np.float64) / FIXED_ONE, n.copy())
        res["scale_factor"] = self.scale_factor
        return res
