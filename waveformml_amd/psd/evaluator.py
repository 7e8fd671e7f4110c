"""``PSDEvaluator``: the per-batch statistics of the reference's evaluator (src/evaluation/PSDEvaluator.py) on the GPU.

The reference's ``LitPSD.test_step`` hands every batch to ``PSDEvaluator.add`` (:101-198), which copies the batch to the
host and walks it sample by sample (``average_pulse``, src/utils/SparseUtils.py:405-487).  Here ``add`` is three HIP
launches on the current stream (csrc/evalstats.hip: event offsets, per-event pulse statistics, table accumulation); nothing
is read back until ``results()``.

What is mirrored: the constructor defaults, the accumulators of ``add`` (``mult_acc``, ``ene_psd_acc``, ``pos_acc``,
``confusion_energy``, ``confusion_SE``, the summed pulses and their counts) and ``finalize()``; with ``metric_pairs=True``
also ``MetricPairAggregator``'s per-class tables over the nine metrics of ``_init_results`` (psd/metric_pairs.py, two more
launches per ``add``; their input is ``self.features``, the ``[9, E]`` feature matrix of the batch).  What is not:
TensorBoard histograms, plots and the calibration database -- a caller that has gains passes them as an array.
``PhysEvaluator`` is psd/phys_evaluator.py.

Two things of the reference that matter for comparing numbers:

* ``average_pulse`` never stores ``n_SE`` of a batch's last event (it stays 0).  The default does the same so that the
  tables agree with a reference run; ``fix_last_event_n_SE=True`` stores the real count.
* ``metric_accumulate_2d`` takes two arrays, the reference's result triples hold three; the tables here are what the call
  means: the first array is the sum of matches, the second the count, the third stays zero.
"""
import numpy as np
import torch

from .. import _lib
from .eval_common import check_coords, raise_flags, read_back, require_device_tensors, require_gpu
from .metric_pairs import MetricPairTables, triple_1d

FLAG_TEXT = {1: "the event column of a batch was not sorted or held an event outside the batch",
             2: "a segment coordinate lay outside the detector grid",
             4: "a prediction or label lay outside class_names"}


def result_shapes(class_names, n_bins=100, n_mult=10, n_confusion=10, n_SE_max=4, nx=14, ny=11):
    """Keys of the reference's ``results`` dict (PSDEvaluator._init_results) and the shape of each entry's arrays."""
    C = len(class_names)
    shapes = {"mult_acc": (n_mult + 2,), "ene_acc": (n_bins + 2,), "pos_acc": (nx + 2, ny + 2),
              "ene_psd_acc": (n_bins + 2, n_bins + 2), "confusion_energy": (n_confusion + 1, C, C),
              "confusion_SE": (n_SE_max + 2, C, C)}
    for name in class_names:
        shapes["ene_psd_prec_{}".format(name)] = (n_bins + 2, n_bins + 2)
        shapes["ene_prec_{}".format(name)] = (n_bins + 2,)
        shapes["mult_prec_{}".format(name)] = (n_mult + 2,)
    return shapes


class PSDEvaluator:
    def __init__(self, class_names, device, gains=None, seg_status=None, n_samples=150, n_bins=100, n_mult=10,
                 n_confusion=10, n_SE_max=4, emin=0.0, emax=5.0, psd_min=0.0, psd_max=0.6, nx=14, ny=11,
                 fix_last_event_n_SE=False, metric_pairs=False):
        self.device = require_gpu(device, "PSDEvaluator")
        self.class_names = list(class_names)
        self.n_classes = len(self.class_names)
        self.n_samples, self.n_bins, self.n_mult = int(n_samples), int(n_bins), int(n_mult)
        self.n_confusion, self.n_SE_max, self.nx, self.ny = int(n_confusion), int(n_SE_max), int(nx), int(ny)
        self.emin, self.emax, self.psd_min, self.psd_max = float(emin), float(emax), float(psd_min), float(psd_max)
        self.fix_last_event_n_SE = bool(fix_last_event_n_SE)
        self.calibrated = gains is not None
        g = np.ones((self.nx, self.ny, 2)) if gains is None else np.asarray(gains, dtype=np.float64)
        s = np.zeros((self.nx, self.ny), np.float32) if seg_status is None else np.asarray(seg_status, dtype=np.float32)
        if g.shape != (self.nx, self.ny, 2) or s.shape != (self.nx, self.ny):
            raise ValueError("gains must be [%d, %d, 2] and seg_status [%d, %d]" % (self.nx, self.ny, self.nx, self.ny))
        self.gain_factor = torch.from_numpy(np.ascontiguousarray(g)).to(self.device)
        self.seg_status = torch.from_numpy(np.ascontiguousarray(s)).to(self.device)
        lib = _lib.load()
        W, C = 2 * self.n_samples, self.n_classes
        n = int(lib.wfs_eval_table_ints(self.n_bins, self.n_mult, self.n_confusion, self.n_SE_max, self.nx, self.ny, C))
        # (name, shape) in the order of include/wfsparse.h
        nm, ne, px, py = self.n_mult + 2, self.n_bins + 2, self.nx + 2, self.ny + 2
        self._layout = [("mult_n", (nm,)), ("mult_m", (nm,)), ("ene_psd_n", (ne, ne)), ("ene_psd_m", (ne, ne)),
                        ("pos_n", (px, py)), ("pos_m", (px, py)), ("confusion_energy", (self.n_confusion + 1, C, C)),
                        ("confusion_SE", (self.n_SE_max + 2, C, C)), ("n_wfs", (C + 1,)), ("n_labelled_wfs", (C,))]
        assert sum(int(np.prod(s)) for _n, s in self._layout) == n
        self.tables = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.sum_wf = torch.zeros((C + 1, W), dtype=torch.float64, device=self.device)
        self.sum_labelled = torch.zeros((C, W), dtype=torch.float64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._rows_cap, self._events_cap = 0, 0
        # MetricPairAggregator over _init_results' nine metrics; energy, psd and multiplicity follow this evaluator's ranges
        self.metric_pairs = None
        if metric_pairs:
            self.metric_pairs = MetricPairTables(self.device, [
                ("energy", self.emin, self.emax, self.n_bins), ("psd", self.psd_min, self.psd_max, self.n_bins),
                ("multiplicity", 0.5, self.n_mult + 0.5, self.n_mult), ("x_dev", 0., 4., 20), ("y_dev", 0., 3., 20),
                ("$\\Delta$t_dev", 0., 10., 20), ("E_dev", 0., 2., 40), ("t_variance", 0., 1000.0, 40),
                ("n_variance", 0.0, 0.25, 40)], self.class_names)

    def _reserve(self, rows, events):
        """Per-batch buffers; allocated on the first call and again only when a batch exceeds them."""
        dev, W = self.device, 2 * self.n_samples
        if rows > self._rows_cap:
            self._rowstats = torch.empty((rows, 4), dtype=torch.float64, device=dev)
            self._rows_cap = rows
        if events != self._events_cap:
            E = events
            self._offsets = torch.zeros(E + 1, dtype=torch.int32, device=dev)
            self.avg_coo = torch.zeros((E, 2), dtype=torch.float64, device=dev)
            self.summed_pulses = torch.zeros((E, W), dtype=torch.float32, device=dev)
            self.output_stats = torch.zeros((6, E), dtype=torch.float32, device=dev)
            self.multiplicity = torch.zeros(E, dtype=torch.int32, device=dev)
            self.n_SE = torch.zeros(E, dtype=torch.int32, device=dev)
            self.psdl = torch.zeros(E, dtype=torch.float32, device=dev)
            self.psdr = torch.zeros(E, dtype=torch.float32, device=dev)
            self.energy = torch.zeros(E, dtype=torch.float32, device=dev)
            self.features = torch.zeros((9, E), dtype=torch.float32, device=dev)
            if self.metric_pairs is not None:
                self._match = torch.zeros(E, dtype=torch.int32, device=dev)
                self._category = torch.zeros(E, dtype=torch.int32, device=dev)
            self._events_cap = E

    def add(self, batch, output, predictions):
        """``batch`` = ``([coords, feats], labels)`` or, capacity-padded, ``([coords, feats, n_valid], labels)`` with a
        device-side row count; ``output`` are the logits (kept for the reference's signature), ``predictions`` their
        argmax.  Launches on the current stream; no read-back, the caller's tensors are only read."""
        inputs, labels = batch
        coords, feats = inputs[0], inputs[1]
        n_valid = inputs[2] if len(inputs) > 2 else None
        require_device_tensors(coords, feats, labels, predictions)
        W = 2 * self.n_samples
        rows = int(coords.shape[0])
        check_coords(coords, None, "PSDEvaluator.add")
        if feats.shape[0] != rows or feats.numel() != rows * W:
            raise RuntimeError("PSDEvaluator.add: waveforms must be [N, %d] (n_samples = %d), got %s"
                               % (W, self.n_samples, tuple(feats.shape)))
        E = int(labels.shape[0])
        if predictions.shape[0] != E or labels.dtype != torch.int64 or predictions.dtype != torch.int64:
            raise RuntimeError("PSDEvaluator.add: labels and predictions must be int64 [E]")
        if n_valid is not None and n_valid.dtype != torch.int64:      # its device is not tested here, unlike check_n_valid
            raise RuntimeError("PSDEvaluator.add: n_valid must be a device int64")
        self._reserve(rows, E)
        lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
        _lib.check(lib.wfs_event_pulse_stats(
            p(coords), p(feats), rows, self.n_samples, _lib.dtype_code(feats), p(n_valid), E, p(self.gain_factor),
            p(self.seg_status), self.nx, self.ny, int(self.fix_last_event_n_SE), p(self._offsets), p(self._rowstats),
            p(self.avg_coo), p(self.summed_pulses), p(self.output_stats), p(self.multiplicity), p(self.n_SE),
            p(self.psdl), p(self.psdr), p(self.energy), p(self.features), p(self.flags), st))
        _lib.check(lib.wfs_eval_accumulate(
            E, self.n_samples, self.n_classes, p(self.avg_coo), p(self.summed_pulses), p(self.multiplicity), p(self.n_SE),
            p(self.psdl), p(self.psdr), p(self.energy), p(predictions), p(labels), self.n_bins, self.n_mult,
            self.n_confusion, self.n_SE_max, self.nx, self.ny, self.emin, self.emax, self.psd_min, self.psd_max,
            p(self.tables), p(self.sum_wf), p(self.sum_labelled), p(self.flags), st))
        if self.metric_pairs is not None:
            # the reference's class loop (results[label_class_inds], skipping empty classes) is category = label; the
            # rows of self.features are in its concatenate order: energy, psdl, multiplicity, the six output_stats
            _lib.check(lib.wfs_match_categories(p(predictions), p(labels), E, p(self._match), p(self._category), st))
            self.metric_pairs.add(self.features, self._match, self._category)

    def reset(self):
        self.tables.zero_()
        self.sum_wf.zero_()
        self.sum_labelled.zero_()
        self.flags.zero_()
        if self.metric_pairs is not None:
            self.metric_pairs.reset()

    def state_tensors(self):
        """The persistent accumulators; all are sums over batches, so N ranks combine them with one SUM all-reduce each
        (psd/evaluate.test_loop)."""
        own = [self.tables, self.sum_wf, self.sum_labelled]
        return own if self.metric_pairs is None else own + self.metric_pairs.state_tensors()

    def _check_flags(self):
        f = int(self.flags.item())
        if self.metric_pairs is not None:
            f |= int(self.metric_pairs.flags.item()) & 4
        raise_flags("PSDEvaluator", f, FLAG_TEXT)

    def results(self):
        """One read-back.  The reference's ``results`` dict after ``finalize()`` -- (mean, n, M2) triples where
        ``metric_accumulate_1d`` fills them, (sum of matches, n, zeros) where ``metric_accumulate_2d`` does, the
        never-filled ``ene_acc`` / ``*_prec_*`` entries as zeros of the reference's shapes -- plus the pulse sums."""
        self._check_flags()
        cur = read_back(self.tables)
        t = {name: cur.take(shape).copy() for name, shape in self._layout}
        nb, nm = self.n_bins + 2, self.n_mult + 2

        def empty_1d(k):
            return np.zeros(k), np.zeros(k, np.int64), np.zeros(k)

        def empty_2d(a, b):
            return np.zeros((a, b)), np.zeros((a, b), np.int64), np.zeros((a, b))

        res = {"mult_acc": triple_1d(t["mult_m"], t["mult_n"]),
               "ene_acc": empty_1d(nb),
               "pos_acc": (t["pos_m"].astype(np.float64), t["pos_n"], np.zeros(t["pos_n"].shape)),
               "ene_psd_acc": (t["ene_psd_m"].astype(np.float64), t["ene_psd_n"], np.zeros((nb, nb))),
               "confusion_energy": t["confusion_energy"],
               "confusion_SE": t["confusion_SE"]}
        for name in self.class_names:
            res["ene_psd_prec_{}".format(name)] = empty_2d(nb, nb)
            res["ene_prec_{}".format(name)] = empty_1d(nb)
            res["mult_prec_{}".format(name)] = empty_1d(nm)
        res["summed_waveforms"] = self.sum_wf.cpu().numpy().astype(np.float32)
        res["n_wfs"] = t["n_wfs"]
        res["summed_labelled_waveforms"] = self.sum_labelled.cpu().numpy().astype(np.float32)
        res["n_labelled_wfs"] = t["n_labelled_wfs"]
        if self.metric_pairs is not None:
            res["metric_pairs"] = self.metric_pairs.split(read_back(self.metric_pairs.tables).rest())
        return res
