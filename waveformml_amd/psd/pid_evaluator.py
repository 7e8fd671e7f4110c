"""``PIDEvaluator``: the per-batch half of the reference's evaluator of the per-segment classifier
(src/evaluation/PIDEvaluator.py on SingleEndedEvaluator / AD1Evaluator) on the GPU.

The reference's ``add`` copies five tensors to the host and walks the rows several times (``calculate_class_accuracy``,
``gen_multiplicity_list``, ``gen_SE_mask``, ``retrieve_n_SE``, ``confusion_accumulate``, ``confusion_accumulate_1d``), then
runs 5 classes x (4 + 6) binned accumulations through ``MetricPairAggregator.add_normalized``.  Here ``add`` is three HIP
launches on the current stream (csrc/metricpairs.hip: event offsets, one thread per row, the pairwise tables); nothing is
read back until ``results()``.  Every table is an exact int64 count.

What is mirrored: the constructor arithmetic (``E_scale``, ``z_scale``, ``default_bins`` with ``bin_overrides``, the four
metrics energy / psd / multiplicity / z and their ``norm_factor``), the tables of ``add``.  Not mirrored: plots, the
calibration database.  ``ROCCurve`` is psd/class_metrics.ClassificationMetrics (``LitSegClassifier.metrics``).

Where this departs from a reference run, because the reference's code and its intent part:

* ``gen_multiplicity_list`` and ``retrieve_n_SE`` look ahead with ``coo[cur_mult + i]`` without a bound and read one past
  the end on the batch's last event.  Here the lookahead ends with the batch (or at ``n_valid``).
* ``add`` passes ``phys[0]`` -- the first ROW -- as the metric of ``confusion_energy``, so ``confusion_accumulate_1d``
  fills the table from the first ``n_phys`` rows only, binned by row 0's physics values.  The table here holds what the
  call means: every row, binned by ``phys[:, E_index]``.  ``confusion_energy`` therefore does NOT agree with a reference
  run; every other table does.
* ``additional_field_names=None`` raises in the reference's constructor (``"phys" in None``); the default here is
  ``("phys",)``.
* The confusion tables are int64 (the reference keeps int32).
"""
import numpy as np
import torch

from .. import _lib
from .eval_common import (check_coords, check_n_valid, raise_flags, read_back, require_device_tensors, require_gpu,
                          reserve_rows, seg_status_tensor)
from .metric_pairs import MetricPairTables, bin_edge_range, normalized_range
from .segments import SE_DEAD_PMTS

FLAG_TEXT = {1: "the event column of a batch was not sorted or held an event outside the batch",
             2: "a segment coordinate lay outside the detector grid",
             4: "a prediction or label lay outside the five PID classes"}
PID_MAPPED_NAMES = {0: "Ionization", 1: "Recoil", 2: "Neutron Capture", 3: "Ingress", 4: "Muon"}
E_NORMALIZATION_FACTOR, Z_NORMALIZATION_FACTOR, CELL_LENGTH = 12., 1200., 1176.
E_INDEX, DT_INDEX, PE0_INDEX, PE1_INDEX, Z_INDEX, PSD_INDEX, TOFFSET_INDEX, DP_INDEX = range(8)


def default_bins(E_scale, z_scale=Z_NORMALIZATION_FACTOR, E_adjust=1.0, bin_overrides=None):
    """``AD1Evaluator.default_bins`` (src/evaluation/AD1Evaluator.py:60-66) with ``override_default_bins``."""
    dt_scale, toffset_scale, PE_scale = 30., 30., 5000. / E_adjust
    bins = [[0.0, E_scale, 100], [-dt_scale / 2., dt_scale / 2., 100], [0.0, PE_scale, 100], [0.0, PE_scale, 100],
            [-z_scale / 2., z_scale / 2., 100], [0.0, 0.6, 100], [0.0, toffset_scale, 100], [0.0, CELL_LENGTH, 100]]
    for key, v in (bin_overrides or {}).items():
        try:
            bins[int(key)] = list(v)
        except ValueError:
            raise IOError("Keys for 'evaluation_config.bin_overrides' dictionary must be integers")
    return bins


def metric_setup(e_scale=None, bin_overrides=None):
    """The constructor arithmetic of the reference (AD1Evaluator.__init__, PIDEvaluator.initialize, MetricAggregator):
    scales, ``default_bins``, the four metrics, their ``norm_factor`` and the ranges ``add_normalized`` bins by."""
    E_scale, E_adjust = E_NORMALIZATION_FACTOR, 1.0
    if e_scale:
        E_adjust = E_scale / e_scale
        E_scale = float(e_scale)
    bins = default_bins(E_scale, Z_NORMALIZATION_FACTOR, E_adjust, bin_overrides)
    params = [bins[0], bins[5], [0.5, 6.5, 6], bins[4]]
    norm = [E_scale, 1.0, 1.0, Z_NORMALIZATION_FACTOR]
    edges = [bin_edge_range(float(p[0]), float(p[1]), int(p[2])) for p in params]
    return dict(E_scale=E_scale, z_scale=Z_NORMALIZATION_FACTOR, E_adjust=E_adjust, default_bins=bins,
                metric_names=["energy", "psd", "multiplicity", "z"], metric_params=params, norm_factors=norm,
                normalized_ranges=[normalized_range(lo, hi, nf) for (lo, hi), nf in zip(edges, norm)])


def set_metric_attributes(ev, setup):
    """The attributes every evaluator built on ``metric_setup`` carries, under the reference's names."""
    ev.z_scale, ev.E_scale, ev.E_adjust = setup["z_scale"], setup["E_scale"], setup["E_adjust"]
    ev.E_index, ev.PSD_index, ev.z_index = E_INDEX, PSD_INDEX, Z_INDEX
    ev.default_bins = setup["default_bins"]
    ev.metric_names, ev.metric_params = setup["metric_names"], setup["metric_params"]
    ev.normalized_ranges = setup["normalized_ranges"]         # MetricAggregator.add_normalized's


class PIDEvaluator:
    # the zero-filled per-row buffers of ``add``
    _ROW_BUFFERS = [(n, torch.int32, (-1,)) for n in ("accuracy", "multiplicity", "se_mask", "n_SE", "category")] + \
                   [("parameters", torch.float32, (4, -1))]

    def __init__(self, device, additional_field_names=("phys",), e_scale=None, seg_status=None,
                 dead_pmts=SE_DEAD_PMTS, n_confusion=10, n_SE_max=6, bin_overrides=None):
        self.device = require_gpu(device, "PIDEvaluator")
        self.nx, self.ny = 14, 11
        setup = metric_setup(e_scale, bin_overrides)
        set_metric_attributes(self, setup)
        self.norm_factors = setup["norm_factors"]
        self.additional_field_names = list(additional_field_names) if additional_field_names is not None else ["phys"]
        self.phys_index = self.additional_field_names.index("phys") if "phys" in self.additional_field_names else 0
        self.n_confusion, self.n_SE_max = int(n_confusion), int(n_SE_max)
        self.class_names = [PID_MAPPED_NAMES[i] for i in range(5)]
        self.n_classes = len(self.class_names)
        self.seg_status = seg_status_tensor(self.device, seg_status, dead_pmts, self.nx, self.ny)
        self.metric_pairs = MetricPairTables(self.device, [(n, *p) for n, p in zip(self.metric_names, self.metric_params)],
                                             self.class_names)
        self.confusion_energy_high = self.n_confusion / self.E_scale
        C = self.n_classes
        self._layout = [("SE_confusion", (C, C)), ("confusion_SE", (self.n_SE_max + 2, C, C)),
                        ("confusion_energy", (self.n_confusion + 1, C, C))]
        n = int(_lib.load().wfs_pid_table_ints(self.n_confusion, self.n_SE_max))
        assert n == sum(int(np.prod(s)) for _k, s in self._layout)
        self.tables = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._rows_cap, self._offsets = -1, None

    def add(self, pred, target, c, additional_fields=None, n_valid=None, n_events=None):
        """The reference's signature (PIDEvaluator.add): ``pred`` and ``target`` int64 class indices [N], ``c`` int32
        [N, 3] = (x, y, event), ``additional_fields`` the list of extra per-row tensors, of which the one at ``"phys"``'s
        place in ``additional_field_names`` is used ([N, n_phys], fp32 / bf16 / fp16; a one-element list is unwrapped).
        ``n_valid``: device-side row count of a capacity-padded batch.  ``n_events``: the batch's event count; without it
        the row count bounds the event indices (every event that has an index has at least one row).  Launches on the
        current stream; no read-back, the caller's tensors are only read."""
        if additional_fields is None:
            return
        phys = additional_fields[self.phys_index]
        if isinstance(phys, (list, tuple)):
            phys = phys[0]
        rows = int(c.shape[0])
        require_device_tensors(pred, target, c, phys)
        check_coords(c, None, "PIDEvaluator.add")
        if pred.dtype != torch.int64 or target.dtype != torch.int64 or tuple(pred.shape) != (rows,) or \
                tuple(target.shape) != (rows,):
            raise RuntimeError("PIDEvaluator.add: predictions and targets must be int64 [N] class indices")
        if phys.dim() != 2 or phys.shape[0] != rows or phys.shape[1] <= max(self.E_index, self.PSD_index, self.z_index):
            raise RuntimeError("PIDEvaluator.add: phys must be [N, n_phys > %d], got %s"
                               % (max(self.E_index, self.PSD_index, self.z_index), tuple(phys.shape)))
        check_n_valid(n_valid, "PIDEvaluator.add")
        if rows == 0:
            return
        E = int(n_events) if n_events is not None else rows
        reserve_rows(self, rows, self._ROW_BUFFERS, E)
        p = _lib.ptr
        _lib.check(_lib.load().wfs_pid_row_stats(
            p(c), p(pred), p(target), p(phys), int(phys.shape[1]), _lib.dtype_code(phys), rows, p(n_valid), E,
            p(self.seg_status), self.nx, self.ny, self.E_index, self.PSD_index, self.z_index, self.n_confusion,
            self.n_SE_max, self.confusion_energy_high, p(self._offsets), p(self.accuracy), p(self.multiplicity),
            p(self.se_mask), p(self.n_SE), p(self.parameters), p(self.category), p(self.tables), p(self.flags),
            _lib.stream_ptr()))
        self.metric_pairs.add(self.parameters, self.accuracy, self.category, n_valid, ranges=self.normalized_ranges)

    def reset(self):
        self.tables.zero_()
        self.flags.zero_()
        self.metric_pairs.reset()

    def state_tensors(self):
        """The persistent accumulators: integer sums over batches, so N ranks combine them with one SUM all-reduce each."""
        return [self.tables] + self.metric_pairs.state_tensors()

    def results(self):
        """One read-back.  ``SE_confusion`` [5, 5], ``confusion_SE`` [n_SE_max + 2, 5, 5], ``confusion_energy``
        [n_confusion + 1, 5, 5] as int64 (label-major), and ``metric_pairs`` = ``MetricPairTables.results()``."""
        mp = self.metric_pairs
        cur = read_back(self.flags, mp.flags, self.tables, mp.tables)
        raise_flags("PIDEvaluator", int(cur.take(1)[0]) | int(cur.take(1)[0]), FLAG_TEXT)
        res = {name: cur.take(shape).copy() for name, shape in self._layout}
        res["metric_pairs"] = mp.split(cur.rest())
        return res
