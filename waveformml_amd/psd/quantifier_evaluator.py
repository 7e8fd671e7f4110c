"""``SegEvaluator``: the per-batch half of the reference's evaluator of the per-segment regression module
(src/evaluation/SegEvaluator.py on SingleEndedEvaluator / AD1Evaluator, with src/utils/StatsUtils.ErrorAggregator) on the
GPU.

The reference's ``add`` copies four tensors to the host, walks the rows (``gen_multiplicity_list``, ``gen_SE_mask``) and
then, per class and PID, bins the absolute error through ``MetricPairAggregator.add_normalized`` and the signed error
through ``ErrorAggregator.add_norm``.  Here ``add`` is five HIP launches on the current stream (csrc/segquant.hip: event
offsets, one thread per row, the edge fix-up, the error bins; csrc/metricpairs.hip: the real-valued pair tables);
nothing is read back until ``results()``.  Five while the row count stays what it was: the seven per-row buffers are
allocated zero-filled for a row count and again whenever it changes (as ``PIDEvaluator``'s), so a batch of another size
adds seven fill launches.

What is mirrored: the constructor arithmetic (``pid_evaluator.metric_setup``: ``E_scale``, ``default_bins`` with
``bin_overrides``, the four metrics energy / psd / multiplicity / z and their normalised ranges, ``target_index``,
``scale_factor``), the tables of ``add``.  Not mirrored: plots and TensorBoard, and everything behind the calibration
database (``calgroup`` raises).

``ErrorAggregator``: per class ``error_hist`` [C, nb + 2] over the class's ``error_edges`` and ``error_2d``
[C, nb + 2, nb + 2] (x = actual, y = predicted, both over [0, 1]), nb = ``default_bins[target_index][2]``, as int64
counts (the reference keeps doubles that hold counts).  The reference fixes a class's ``error_edges`` on the FIRST
``add_norm`` call that reaches the class -- ``add_norm`` is called once per (class, pid) in ``class_PIDs`` order, so for
"Neutron Capture" the pid-6 rows of the first batch that has any decide, the pid-258 rows only when that batch has no
pid-6 row -- as ``get_bins(-1.1 max|error|, 1.1 max|error|, nb)``, whose last entry is not ``high``
(csrc/wfs_erroredges.h).  The device reproduces this without a read-back: the row launch folds per PID slot the row
count and max |error|, a one-workgroup launch sets the edges of every class that has none from its first slot with
rows, the bin launch bins by them.  ``error_edges`` and ``error_edges_set`` persist across ``add`` calls; ``reset()``
clears them.  A first subset whose max |error| is 0 or not finite leaves the class unset and makes ``results()`` raise
(``np.arange`` fails there in the reference).  ``error_edges=(low, high)`` fixes every class's range in advance.

Where this departs from a reference run:

* ``gen_multiplicity_list`` looks ahead without a bound and reads one past the end on the batch's last event.  Here the
  lookahead ends with the batch (or at ``n_valid``).
* Without ``"PID"`` among ``additional_field_names`` the reference means one class, ``"all"``, over every row with NO
  single-ended mask (the ``else`` branch of ``add``) -- but can never get there: its constructor reads ``self.has_PID``,
  which only the PID branch sets, and ``add`` indexes ``additional_fields[None]`` first.  Here that form works as its
  ``else`` branch reads.
* ``error = results - target`` is formed in fp64 from the stored values (the reference subtracts in float32).
* A row whose error is NaN (a NaN prediction or target) is binned by the error tables as the reference's walk leaves
  it -- bin 0 of ``error_hist`` and of the NaN axis of ``error_2d`` -- but its |error| has no fixed-point image: the
  metric tables leave the row out and ``results()`` raises (``RealMetricPairTables``' flag), where the reference carries
  the NaN into every bin the row touches.  In a class's FIRST subset a NaN makes the largest |error| NaN: the edges
  stay unset and ``results()`` raises, as ``np.arange`` does in the reference.
* ``state_tensors()`` returns the metric tables and ``error_2d``, and ``error_hist`` only with edges fixed in advance:
  data-dependent edges differ from rank to rank, so that table cannot be summed.  Under several ranks ``results()``
  reports the local ``error_hist`` and ``error_edges``.
"""
import numpy as np
import torch

from .. import _lib
from .eval_common import (check_coords, check_n_valid, pid_field, raise_flags, read_back, require_device_tensors,
                          require_gpu, reserve_rows, seg_status_tensor)
from .metric_pairs import REAL_FLAG_TEXT, RealMetricPairTables
from .pid_evaluator import PID_MAPPED_NAMES, metric_setup, set_metric_attributes
from .segments import SE_DEAD_PMTS

FLAG_TEXT = {1: "the event column of a batch was not sorted or held an event outside the batch",
             2: "a segment coordinate lay outside the detector grid"}
CLASS_PIDS = [[1], [4], [6, 258], [256], [512]]      # retrieve_class_names_PIDS(): PID_MAP inverted, in its order
N_SLOTS = 6


class SegEvaluator:
    # the zero-filled per-row buffers of ``add``
    _ROW_BUFFERS = [("mae", torch.float32, (-1,)), ("error", torch.float64, (-1,))] + \
                   [(n, torch.int32, (-1,)) for n in ("multiplicity", "se_mask", "category", "slot")] + \
                   [("parameters", torch.float32, (4, -1))]

    def __init__(self, device, additional_field_names=None, e_scale=None, seg_status=None, dead_pmts=SE_DEAD_PMTS,
                 bin_overrides=None, target_index=4, error_edges=None, calgroup=None):
        self.device = require_gpu(device, "SegEvaluator")
        if calgroup is not None:
            raise RuntimeError("SegEvaluator: the calibration database (calgroup) is not mirrored; ZEvaluator takes the "
                               "curves as calibration= (psd/calibration.py)")
        self.nx, self.ny = 14, 11
        setup = metric_setup(e_scale, bin_overrides)
        set_metric_attributes(self, setup)
        self.norm_factors = setup["norm_factors"]
        self.target_index = int(target_index)
        if not 0 <= self.target_index < len(self.default_bins):
            raise ValueError("SegEvaluator: target_index must name one of the %d phys columns" % len(self.default_bins))
        self.metric_name = "mean absolute error"
        # AD1Evaluator.scale_factor
        self.scaling = {0: self.E_scale, 1: 30., 2: 5000. / self.E_adjust, 3: 5000. / self.E_adjust, 4: self.z_scale,
                        5: 1.0}.get(self.target_index)
        self.additional_field_names = list(additional_field_names) if additional_field_names is not None else None
        self.has_PID = self.additional_field_names is not None and "PID" in self.additional_field_names
        self.PID_index = self.additional_field_names.index("PID") if self.has_PID else None
        if self.has_PID:
            self.class_names, self.class_PIDs = [PID_MAPPED_NAMES[i] for i in range(5)], [list(p) for p in CLASS_PIDS]
        else:
            self.class_names, self.class_PIDs = ["all"], None
        self.n_classes = len(self.class_names)
        self.seg_status = seg_status_tensor(self.device, seg_status, dead_pmts, self.nx, self.ny)
        self.metric_pairs = RealMetricPairTables(
            self.device, [(n, *p) for n, p in zip(self.metric_names, self.metric_params)], self.class_names)
        self.n_bins = int(self.default_bins[self.target_index][2])
        C, nb = self.n_classes, self.n_bins
        self.fixed_edges = None
        if error_edges is not None:
            lo, hi = float(error_edges[0]), float(error_edges[1])
            if not hi > lo:
                raise ValueError("SegEvaluator: error_edges must be (low, high) with high > low")
            self.fixed_edges = (lo, hi)
        # the persistent state: two int64 count tables, the edges and their flags (results() packs them into one read-back)
        self.error_hist = torch.zeros((C, nb + 2), dtype=torch.int64, device=self.device)
        self.error_2d = torch.zeros((C, nb + 2, nb + 2), dtype=torch.int64, device=self.device)
        self.error_edges = torch.zeros((C, 2), dtype=torch.float64, device=self.device)
        self.error_edges_set = torch.zeros(C, dtype=torch.int32, device=self.device)
        self.error_flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._slot_scratch = torch.zeros(2 * N_SLOTS, dtype=torch.int64, device=self.device)
        self._rows_cap, self._offsets = -1, None
        self._init_edges()

    def _init_edges(self):
        self.error_edges.zero_()
        self.error_edges_set.zero_()
        if self.fixed_edges is not None:
            self.error_edges[:, 0] = self.fixed_edges[0]
            self.error_edges[:, 1] = self.fixed_edges[1]
            self.error_edges_set.fill_(1)

    def add(self, results, target, c, additional_fields=None, n_valid=None, n_events=None):
        """The reference's signature (SegEvaluator.add): ``results`` [N] fp32 / bf16 / fp16 predictions, ``target``
        [N, n_phys >= 6] of the same kinds, ``c`` int32 [N, 3] = (x, y, event), ``additional_fields`` the list of extra
        per-row tensors, of which the one at ``"PID"``'s place in ``additional_field_names`` is used (int32 or int64 [N]).
        ``n_valid``: device-side row count of a capacity-padded batch.  ``n_events``: the batch's event count; without it
        the row count bounds the event indices.  Launches on the current stream; no read-back, the caller's tensors are
        only read."""
        pid = pid_field(additional_fields, self.PID_index, "SegEvaluator.add") if self.has_PID else None
        rows = int(c.shape[0])
        require_device_tensors(results, target, c, pid)
        check_coords(c, None, "SegEvaluator.add")
        if tuple(results.shape) != (rows,):
            raise RuntimeError("SegEvaluator.add: results must be [N], got %s" % (tuple(results.shape),))
        need = max(self.E_index, self.PSD_index, self.z_index, self.target_index)
        if target.dim() != 2 or target.shape[0] != rows or target.shape[1] <= need:
            raise RuntimeError("SegEvaluator.add: target must be [N, n_phys > %d], got %s" % (need, tuple(target.shape)))
        if pid is not None and (pid.dtype not in (torch.int32, torch.int64) or tuple(pid.shape) != (rows,)):
            raise RuntimeError("SegEvaluator.add: PID must be int32 or int64 [N]")
        check_n_valid(n_valid, "SegEvaluator.add")
        if rows == 0:
            return
        results, target = results.contiguous(), target.contiguous()
        E = int(n_events) if n_events is not None else rows
        reserve_rows(self, rows, self._ROW_BUFFERS, E)
        p, lib = _lib.ptr, _lib.load()
        rd, td, n_phys = _lib.dtype_code(results), _lib.dtype_code(target), int(target.shape[1])
        _lib.check(lib.wfs_segq_row_stats(
            p(c), p(results), rd, p(target), td, n_phys, p(pid), int(pid is not None and pid.dtype == torch.int64), rows,
            p(n_valid), E, p(self.seg_status), self.nx, self.ny, self.E_index, self.PSD_index, self.z_index,
            self.target_index, p(self._offsets), p(self.mae), p(self.error), p(self.multiplicity), p(self.se_mask),
            p(self.parameters), p(self.category), p(self.slot), p(self._slot_scratch), p(self.flags), _lib.stream_ptr()))
        self.metric_pairs.add(self.parameters, self.mae, self.category, n_valid, ranges=self.normalized_ranges)
        _lib.check(lib.wfs_segq_error_accumulate(
            p(results), rd, p(target), td, n_phys, self.target_index, p(self.error), p(self.category), rows, p(n_valid),
            self.n_classes, int(self.has_PID), self.n_bins, p(self._slot_scratch), p(self.error_edges),
            p(self.error_edges_set), p(self.error_flags), p(self.error_hist), p(self.error_2d), _lib.stream_ptr()))

    def reset(self):
        self.error_hist.zero_()
        self.error_2d.zero_()
        self.error_flags.zero_()
        self.flags.zero_()
        self._slot_scratch.zero_()
        self._init_edges()
        self.metric_pairs.reset()

    def state_tensors(self):
        """The accumulators N ranks combine with one SUM all-reduce each: the metric tables and ``error_2d``, and
        ``error_hist`` only when the edges were fixed in advance (data-dependent edges differ from rank to rank)."""
        out = self.metric_pairs.state_tensors() + [self.error_2d]
        if self.fixed_edges is not None:
            out.append(self.error_hist)
        return out

    def results(self):
        """One read-back.  ``metric_pairs`` = ``RealMetricPairTables.results()``; ``error_hist`` [C, nb + 2] and
        ``error_2d`` [C, nb + 2, nb + 2] as int64; ``error_edges`` [C, 2] = (edges[0], edges[-1]) per class (zeros where
        ``error_edges_set`` [C] is 0); ``scale_factor``."""
        mp = self.metric_pairs
        C, nb = self.n_classes, self.n_bins
        edge_bits = self.error_edges.reshape(-1).view(torch.int64)
        cur = read_back(self.flags, mp.flags, self.error_flags, self.error_edges_set, edge_bits, self.error_hist,
                        self.error_2d, mp.tables)
        f, f_pairs, f_edges = (int(v) for v in cur.take(3))
        raise_flags("SegEvaluator", f, FLAG_TEXT)
        if f_edges:
            bad = [self.class_names[k] for k in range(C) if f_edges >> k & 1]
            raise RuntimeError("SegEvaluator: the first rows of class %s had a largest |error| of 0 or one that is not "
                               "finite: no error histogram range follows from it" % ", ".join(bad))
        raise_flags("SegEvaluator", f_pairs, REAL_FLAG_TEXT)
        res = {"error_edges_set": cur.take(C).astype(np.int32)}
        res["error_edges"] = cur.take(2 * C).copy().view(np.float64).reshape(C, 2)
        res["error_hist"] = cur.take((C, nb + 2)).copy()
        res["error_2d"] = cur.take((C, nb + 2, nb + 2)).copy()
        res["metric_pairs"] = mp.split(cur.rest())
        res["scale_factor"] = self.scaling
        return res
