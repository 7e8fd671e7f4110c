"""``ZEvaluatorRealWFNorm``: the per-batch half of the reference's z evaluator for real detector data
(src/evaluation/ZEvaluator.py ``ZEvaluatorRealWFNorm`` on ``RealDataEvaluator`` and ``WaveformEvaluator``) on the GPU: what
``LitZ`` feeds when its test targets are the seven phys planes.

The reference's ``add`` copies five tensors to the host, aligns both PMT pulses of every row (``align_wfs``), runs
13 x 2 pairwise accumulations over the five aligned samples (``analyze_wf_z``), one dense per-class pairwise accumulation
(``RealDataEvaluator.add``), and twice the seven-table walk ``z_deviation_with_E_full_correlation`` -- once for the
network, once for the neighbour-average baseline ``z_basic_prediction_dense`` builds in between.  Here ``add`` is nine HIP
launches on the current stream (csrc/zreal.hip: event offsets, rows, pulse alignment, baseline, two table walks;
csrc/metricpairs.hip: the class tables and one launch per PMT side of the sample tables), whatever the number of slices
and classes; nothing is read back until ``results()``.  Every table is int64, changed by integer atomics only: exact,
independent of row order and launch shape, and N ranks combine them with one integer SUM.

The twelve z-sliced sample aggregators share metrics and bins, so they are ONE ``RealMetricPairTables`` whose categories
are ``slice * C + class`` plus one leftover category (index ``12 * C``) for the rows in no (slice, class) cell; the
reference's thirteenth, all-z aggregator is the integer sum over the categories, formed in ``results()``.

Where the reference's code and its intent part:

* The PID field is mapped ONCE and the caller's tensor is not modified (the reference maps it in place in
  ``RealDataEvaluator.add`` and again in ``analyze_wf_z`` whenever no row of the batch mapped to class 3).
* ``MetricPairAggregator.add_dense_normalized_with_categories`` adds the last metric inside its loop: z's 1-D class table
  receives every row ``len(names) - 1 = 3`` times.  ``results()`` applies that as a factor on n, S and Q
  (``count_last_metric_once=True`` gives the single count instead).
* The multiplicity the class tables see is the number of single-ended rows of the event, and only single-ended rows enter
  them (``coo[SE_inds]``); both are kept.  A batch without a single-ended row is skipped (the reference indexes row 0 of an
  empty list there).
* A PID that ``PID_MAP`` does not name stays as it is: 2 counts as class 2, 7 matches no class.  A class index outside
  ``[0, C)`` goes to the leftover category of the sample tables; on a single-ended row the class tables leave it out and
  ``results()["class_out_of_range"]`` is True (the reference indexes past its arrays there).
* A NaN prediction or target has no fixed-point image: the row is left out and ``results()`` raises.
* ``align_wfs`` reads ``data[k + start]`` without a bound; here samples beyond the row are 0.
* The lookaheads end at the valid rows; events are identified by their index (``swap_sparse_from_dense`` counts changes
  of the event column instead, which is the same for batches whose events all have rows).

Not mirrored: plots, TensorBoard, the ``EnergyEvaluator`` branch under ``hasattr(self, "calibrator")``, ``fft_pulses``,
``z_E_from_cal``; ``calgroup`` raises.
"""
import numpy as np
import torch

from .. import _lib
from .eval_common import (FIXED_ONE, check_coords, pid_field, raise_flags, read_back, require_gpu, reserve_rows,
                          seg_status_tensor)
from .metric_pairs import REAL_FLAG_TEXT, RealMetricPairTables, finish_real_tables, raw_real_tables  # noqa: F401
from .pid_evaluator import (CELL_LENGTH, E_INDEX, PID_MAPPED_NAMES, PSD_INDEX, Z_INDEX, metric_setup,  # noqa: F401
                            set_metric_attributes)
from .segment_evaluator import _plane_args
from .segments import SE_DEAD_PMTS, blind_left

FLAG_TEXT = {1: "the event column of a batch was not sorted or held an event outside the batch",
             2: "a segment coordinate lay outside the detector grid",
             8: "a deviation was not finite or too large for the fixed-point sums, or a sum overflowed"}
CLASS_RANGE_FLAG = 4            # a single-ended row's class index outside the class tables: reported, not raised
PID_MAP = {1: 0, 4: 1, 6: 2, 256: 3, 258: 2, 512: 4}
PULSE_ANALYSIS_SAMPLES, NUM_Z_BINS = 5, 10
N_SLICES = NUM_Z_BINS + 2
_UNSET = object()


def table_shapes(nx=14, ny=11, n_mult=6, n_z=100, n_E=100):
    """(name, shape) of the seven tables of one ``z_deviation_with_E_full_correlation`` run, in the order of
    include/wfsparse.h; the reference's ``register_duplicates`` shapes."""
    nm1 = n_mult + 1
    return [("seg_mult_zmae", (nx, ny, nm1)), ("z_mult_single", (n_z + 2, nm1)), ("z_mult_dual", (n_z + 2, nm1)),
            ("z_E_single", (n_z + 2, n_E + 2)), ("z_E_dual", (n_z + 2, n_E + 2)), ("E_mult_single", (n_E + 2, nm1)),
            ("E_mult_dual", (n_E + 2, nm1))]


def z_real_setup(e_scale=None, bin_overrides=None):
    """The constructor arithmetic of the reference (AD1Evaluator, RealDataEvaluator, WaveformEvaluator.init_sample_metrics,
    ZEvaluatorRealWFNorm.__init__) without a device: ``metric_setup`` plus the table bounds and the sample metrics."""
    s = metric_setup(e_scale, bin_overrides)
    bins = s["default_bins"]
    s["E_bounds"] = [float(bins[0][0]), float(bins[0][1])]
    s["n_E"], s["n_mult"], s["n_z"] = int(bins[0][-1]), 6, 100
    s["mult_bounds"], s["z_bounds"] = [0.5, 6.5], [0., CELL_LENGTH]
    s["E_low"], s["E_high"] = s["E_bounds"][0] / s["E_scale"], s["E_bounds"][1] / s["E_scale"]
    s["sample_names"] = ["sample {}".format(i) for i in range(PULSE_ANALYSIS_SAMPLES)]
    s["sample_params"] = [[1.0E-6, 0.01 * (i + 1), 100] for i in range(PULSE_ANALYSIS_SAMPLES)]
    return s


def map_pid(pid):
    """``convert_PID(pid, PID_MAP)`` on a copy: a PID the map does not name stays as it is."""
    pid = np.asarray(pid)
    out = pid.copy()
    for key, val in PID_MAP.items():
        out[pid == key] = val
    return out


def z_slice(z):
    """The slice of ``analyze_wf_z`` every z (mm) falls in, -1 for none (NaN): 0: z <= -600; i = 1 .. 9:
    -600 + (i - 1) 120 < z <= -600 + i 120; 10: 480 < z < 600; 11: z >= 600."""
    z = np.asarray(z, np.float64)
    inc = 1200 / NUM_Z_BINS
    out = np.full(z.shape, -1, np.int32)
    for i in range(N_SLICES):
        if i == 0:
            inds = z <= -600
        elif i == 11:
            inds = z >= 600
        elif i == 10:
            inds = (z > -600 + (i - 1) * inc) & (z < 600)
        else:
            inds = (z > -600 + (i - 1) * inc) & (z <= -600 + i * inc)
        out[inds] = i
    return out


def sample_category(z, cls, n_classes):
    """``slice * C + class``, or the leftover category ``12 * C`` for a row in no (slice, class) cell."""
    sl, cls = z_slice(z), np.asarray(cls, np.int64)
    ok = (sl >= 0) & (cls >= 0) & (cls < n_classes)
    return np.where(ok, sl * n_classes + np.where(ok, cls, 0), N_SLICES * n_classes).astype(np.int32)


def split_sample_tables(raw, names, n_classes):
    """The reference's 13 sample aggregators from the category-encoded tables: a list of 12 per-slice results with
    [C, ...] tables and, last, the all-z aggregator (class "any", [1, ...]) as the integer sum over every category,
    the leftover one included.  Also returns the leftover category's own tables."""
    C = n_classes
    per_slice = []
    for i in range(N_SLICES):
        per_slice.append(finish_real_tables({k: [a[i * C:(i + 1) * C] for a in t] for k, t in raw.items()}, names))
    allz = finish_real_tables({k: [a.sum(axis=0, keepdims=True) for a in t] for k, t in raw.items()}, names)
    left = finish_real_tables({k: [a[N_SLICES * C:] for a in t] for k, t in raw.items()}, names)
    return per_slice + [allz], left


class ZEvaluatorRealWFNorm:
    name = "ZEvaluatorRealWFNorm"
    # the zero-filled per-row buffers of ``add``
    _ROW_BUFFERS = [(n, torch.float32, (-1,)) for n in ("z_pred", "z_true", "energy", "mae", "dev_mm", "baseline")] + \
                   [(n, torch.int32, (-1,)) for n in ("class_category", "sample_category", "se_mask")] + \
                   [("parameters", torch.float32, (4, -1)), ("samples", torch.float32, (2, PULSE_ANALYSIS_SAMPLES, -1)),
                    ("start", torch.int32, (-1, 2))]

    def __init__(self, device, e_scale=None, additional_field_names=None, wf_analysis=_UNSET, bin_overrides=None,
                 excludes=None, seg_status=None, blind_detl=None, dead_pmts=SE_DEAD_PMTS, namespace=None, calgroup=None,
                 count_last_metric_once=False):
        """``excludes``: the reference's keyword for the list of dead PMTs (SingleEndedEvaluator); ``dead_pmts`` is this
        project's name for it.  ``wf_analysis``: present (whatever its value) switches the waveform analysis on."""
        self.device = require_gpu(device, "ZEvaluatorRealWFNorm")
        if calgroup is not None:
            raise RuntimeError("ZEvaluatorRealWFNorm: the calibration database (calgroup) is not mirrored; ZEvaluator takes "
                               "the curves as calibration= (psd/calibration.py)")
        self.nx, self.ny = 14, 11
        dead_pmts = dead_pmts if excludes is None else tuple(excludes)
        s = z_real_setup(e_scale, bin_overrides)
        set_metric_attributes(self, s)
        self.E_bounds, self.mult_bounds, self.z_bounds = s["E_bounds"], s["mult_bounds"], s["z_bounds"]
        self.n_mult, self.n_E, self.n_z = s["n_mult"], s["n_E"], s["n_z"]
        self.E_low, self.E_high = s["E_low"], s["E_high"]
        self.metric_name, self.metric_unit, self.scaling = "mean absolute error", "mm", self.z_scale
        self.namespace = "evaluation/{}_".format(namespace) if namespace else "evaluation/"
        # the reference switches the waveform analysis on by the PRESENCE of the keyword (WaveformEvaluator.__init__)
        self.analyze_waveforms = wf_analysis is not _UNSET
        self.additional_field_names = list(additional_field_names) if additional_field_names is not None else None
        self.has_PID = self.additional_field_names is not None and "PID" in self.additional_field_names
        self.PID_index = self.additional_field_names.index("PID") if self.has_PID else None
        self.class_names = [PID_MAPPED_NAMES[i] for i in range(5)] if self.has_PID else None
        self.sample_class_names = self.class_names if self.has_PID else ["any"]
        self.n_sample_classes = len(self.sample_class_names)
        self.last_metric_factor = 1 if count_last_metric_once else len(s["metric_names"]) - 1
        both = "seg_status and blind_detl must be [%d, %d]"
        self.seg_status = seg_status_tensor(self.device, seg_status, dead_pmts, self.nx, self.ny, both)
        bl = blind_left(dead_pmts, self.nx, self.ny) if blind_detl is None else np.asarray(blind_detl, np.int32)
        if bl.shape != (self.nx, self.ny):
            raise ValueError(both % (self.nx, self.ny))
        self.blind_detl = torch.from_numpy(np.ascontiguousarray(bl)).to(self.device)
        self.sample_names, self.sample_params = s["sample_names"], s["sample_params"]
        self.metric_pairs = self.sample_pairs = None
        if self.has_PID:
            self.metric_pairs = RealMetricPairTables(
                self.device, [(n, *p) for n, p in zip(self.metric_names, self.metric_params)], self.class_names)
        if self.analyze_waveforms:
            self.sample_pairs = RealMetricPairTables(
                self.device, [(n, *p) for n, p in zip(self.sample_names, self.sample_params)],
                ["%d/%s" % (i, c) for i in range(N_SLICES) for c in self.sample_class_names] + ["unbinned"])
        self._layout = table_shapes(self.nx, self.ny, self.n_mult, self.n_z, self.n_E)
        self.table_names = [n for n, _s in self._layout] + [n + "_cal" for n, _s in self._layout]
        n = int(_lib.load().wfs_zreal_table_ints(self.nx, self.ny, self.n_mult, self.n_z, self.n_E))
        assert n == sum(2 * int(np.prod(sh)) for _n, sh in self._layout)
        self.tables = torch.zeros((2, n), dtype=torch.int64, device=self.device)       # the network's, the baseline's
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._rows_cap, self._offsets = -1, None

    def add(self, predictions, target, c, f, additional_fields=None, n_valid=None, n_events=None):
        """The reference's signature: ``predictions`` a dense [B, 1, 14, 11] map (plane 0 is scored), ``target`` the
        dense [B, >= 6, 14, 11] map of normalised phys planes, ``c`` int32 [N, 3] = (x, y, event), ``f`` the feature
        rows [N, 2 L] (left PMT's L samples, then the right PMT's; fp32 / bf16 / fp16; read only with ``wf_analysis``),
        ``additional_fields`` the list of extra per-row tensors, of which the one at ``"PID"``'s place in
        ``additional_field_names`` is used (int32 or int64 [N]).  ``n_valid``: device-side row count of a
        capacity-padded batch.  ``n_events``: the batch's event count when it is below B.  Launches on the current
        stream; no read-back, the caller's tensors are only read."""
        check_coords(c, n_valid, "ZEvaluatorRealWFNorm.add")
        rows, B = int(c.shape[0]), int(predictions.shape[0])
        pid = None
        if self.has_PID:
            pid = pid_field(additional_fields, self.PID_index, "ZEvaluatorRealWFNorm.add")
            if not pid.is_cuda or pid.dtype not in (torch.int32, torch.int64) or tuple(pid.shape) != (rows,):
                raise RuntimeError("ZEvaluatorRealWFNorm.add: PID must be a device int32 or int64 [N]")
            pid = pid.contiguous()
        E = B if n_events is None else int(n_events)
        if not 1 <= E <= B:
            raise RuntimeError("ZEvaluatorRealWFNorm.add: n_events must lie in [1, %d]" % B)
        need = max(self.E_index, self.PSD_index, self.z_index)
        pa = _plane_args(predictions, 0, B, self.nx, self.ny, "predictions")
        ta = _plane_args(target, need, B, self.nx, self.ny, "target")
        if rows == 0:
            return
        L = 0
        if self.analyze_waveforms:
            if not f.is_cuda or f.dim() != 2 or f.shape[0] != rows or f.shape[1] % 2 or f.shape[1] < 2:
                raise RuntimeError("ZEvaluatorRealWFNorm.add: f must be device rows [N, 2 L], got %s" % (tuple(f.shape),))
            f, L = f.contiguous(), int(f.shape[1]) // 2
        reserve_rows(self, rows, self._ROW_BUFFERS, E)
        p, lib, stream = _lib.ptr, _lib.load(), _lib.stream_ptr()
        _lib.check(lib.wfs_zreal_row_stats(
            p(c), *pa, ta[0], ta[1], ta[2], ta[3], self.z_index, self.E_index, self.PSD_index, p(pid),
            int(pid is not None and pid.dtype == torch.int64), rows, p(n_valid), E, p(self.seg_status), self.nx, self.ny,
            self.n_sample_classes, self.z_scale, p(self._offsets), p(self.z_pred), p(self.z_true), p(self.energy),
            p(self.mae), p(self.dev_mm), p(self.parameters), p(self.class_category), p(self.sample_category),
            p(self.se_mask), p(self.flags), stream))
        if self.metric_pairs is not None:
            self.metric_pairs.add(self.parameters, self.mae, self.class_category, n_valid, ranges=self.normalized_ranges)
        if self.sample_pairs is not None:
            _lib.check(lib.wfs_align_pulses(p(f), _lib.dtype_code(f), rows, p(n_valid), L, PULSE_ANALYSIS_SAMPLES,
                                            p(self.samples), p(self.start), stream))
            for side in range(2):
                self.sample_pairs.add(self.samples[side], self.dev_mm, self.sample_category, n_valid)
        for k, pred_rows in enumerate((self.z_pred, self.baseline)):
            if k == 1:
                _lib.check(lib.wfs_zreal_baseline(p(c), rows, p(n_valid), E, p(self._offsets), p(self.z_true),
                                                  p(self.seg_status), self.nx, self.ny, p(self.baseline), stream))
            _lib.check(lib.wfs_zreal_accumulate(
                p(c), rows, p(n_valid), E, p(self._offsets), p(pred_rows), p(self.z_true), p(self.energy),
                p(self.seg_status), p(self.blind_detl), self.nx, self.ny, self.n_mult, self.n_z, self.z_scale, self.E_low,
                self.E_high, self.n_E, p(self.tables[k]), p(self.flags), stream))

    def reset(self):
        self.tables.zero_()
        self.flags.zero_()
        for t in (self.metric_pairs, self.sample_pairs):
            if t is not None:
                t.reset()

    def state_tensors(self):
        """The persistent accumulators: integer sums over batches, so N ranks combine them with one SUM all-reduce each."""
        out = [self.tables]
        for t in (self.metric_pairs, self.sample_pairs):
            if t is not None:
                out += t.state_tensors()
        return out

    def results(self):
        """One read-back.  The fourteen tables under the reference's names as (float64 sums, int64 counts);
        ``"metric_pairs"`` (with PID): the class tables ``{"metrics": {name: (mean, n, dev)}, "pairs": {"i_j": (sum, n)}}``
        with [5, ...] shapes; ``"z_binned_metric_pairs"`` (with ``wf_analysis``): the 13 sample aggregators in the
        reference's order, twelve slices with [C, ...] tables and the all-z one with [1, ...];
        ``"unbinned_sample_pairs"``: the leftover category's own tables; ``"class_out_of_range"``."""
        parts = [self.flags]
        for t in (self.metric_pairs, self.sample_pairs):
            parts.append(t.flags if t is not None else torch.zeros_like(self.flags))
        parts.append(self.tables)
        for t in (self.metric_pairs, self.sample_pairs):
            if t is not None:
                parts.append(t.tables)
        cur = read_back(*parts)
        f, f_class, f_sample = (int(v) for v in cur.take(3))
        raise_flags(self.name, f & ~CLASS_RANGE_FLAG, FLAG_TEXT)
        raise_flags(self.name + ", class tables", f_class, REAL_FLAG_TEXT)
        raise_flags(self.name + ", sample tables", f_sample, REAL_FLAG_TEXT)
        res = {"class_out_of_range": bool(f & CLASS_RANGE_FLAG)}
        for cal in ("", "_cal"):
            for name, shape in self._layout:
                n, s = cur.take_pair(shape)
                res[name + cal] = (s.astype(np.float64) / FIXED_ONE, n.copy())
        if self.metric_pairs is not None:
            mp = self.metric_pairs
            res["metric_pairs"] = mp.split(cur.take(mp.tables.shape[0]), self.last_metric_factor)
        if self.sample_pairs is not None:
            sp = self.sample_pairs
            res["z_binned_metric_pairs"], res["unbinned_sample_pairs"] = split_sample_tables(
                raw_real_tables(cur.take(sp.tables.shape[0]), sp._layout), sp.names, self.n_sample_classes)
        return res

    def retrieve_error_metrics(self, results=None):
        """The four curves ``retrieve_error_metrics`` logs, in mm over the energy bins 1 .. n_E, as a dict under the
        reference's tags; an energy bin without rows gives 0."""
        res = self.results() if results is None else results
        out = {}
        for tag, key in (("single_z_MAE_vs_E", "E_mult_single"), ("dual_z_MAE_vs_E", "E_mult_dual"),
                         ("single_z_MAE_cal_vs_E", "E_mult_single_cal"), ("dual_z_MAE_cal_vs_E", "E_mult_dual_cal")):
            s, n = res[key]
            out[self.namespace + tag] = [float(self.z_scale * np.sum(s[i, :]) / np.sum(n[i, :])) if np.sum(n[i, :]) > 0
                                         else 0 for i in range(1, self.n_E + 1)]
        return out
