"""``PhysEvaluator``: the reference's evaluator for extracted-feature batches (src/evaluation/PSDEvaluator.py:301-397) on
the GPU.

The reference's ``LitPSD`` builds it for ``PulseDatasetDet`` (src/engineering/LitPSD.py:35-46): every row of a batch holds
seven extracted physics quantities of one segment instead of a waveform.  ``add`` is three HIP launches on the current
stream (csrc/physstats.hip: event offsets, the per-event weighted averages, table accumulation); nothing is read back until
``results()``.

What is mirrored: ``PSDEvaluator``'s constructor defaults with ``emax = 10``; the derived columns of ``add`` (fp32, as the
code forms them, not as its docstring says); ``weighted_average_quantities`` with numba's accumulator types; the
accumulators ``mult_acc``, ``ene_psd_acc``, ``pos_acc``, ``confusion_energy`` and, per TRUE class, ``ene_psd_prec_<c>``,
``ene_prec_<c>`` and ``mult_prec_<c>``; ``finalize()``.  What is not: TensorBoard histograms, plots, the calibration
database.  With ``spectra=True`` (this project's addition) the feature histograms the reference only sends to TensorBoard
are kept as int64 tables in ``hist_add_1d``'s convention.

Quirks of the reference that are kept, because they decide the numbers:

* ``out_coords += coord[0:2] * ene_current`` weighs a row by the RUNNING energy sum of its event, not by its own energy.
* An event whose energy sum is not above zero keeps its un-normalised sums, energy 0 and multiplicity 0.
* ``confusion_SE`` is never filled by ``PhysEvaluator.add``: zeros.  ``ene_acc`` likewise.
* ``metric_accumulate_2d`` takes two arrays, the reference's result triples hold three; the tables here are what the call
  means: the first array is the sum of matches, the second the count, the third stays zero.

(The class loop's ``if len(label_class_inds) == 0: continue`` tests the length of ``np.nonzero``'s TUPLE, which is 1: it
never skips a class, so a class without events simply adds nothing, here as there.)
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .config import DictionaryUtility
from .eval_common import check_coords, raise_flags, read_back, require_device_tensors, require_gpu, reserve_offsets
from .evaluator import result_shapes
from .metric_pairs import triple_1d

FLAG_TEXT = {1: "the event column of a batch was not sorted or held an event outside the batch",
             4: "a prediction or label lay outside class_names"}

N_QUANTITIES = 7
FEATURE_NAMES = ["energy", "psd", "rise_time", "PEL", "PER", "z", "start_time", "multiplicity"]
# AD1Evaluator.default_bins (src/evaluation/AD1Evaluator.py:60-63) by its own index: E, dt, PE0, PE1, z, PSD, t offset
DEFAULT_BINS = [[0.0, 12.0, 100], [-15.0, 15.0, 100], [0.0, 5000.0, 100], [0.0, 5000.0, 100], [-600.0, 600.0, 100],
                [0.0, 0.6, 100], [0.0, 30.0, 100]]
# the default_bins index behind each of the first seven features (PhysEvaluator.add:322-348: ene, psd, dt, PE, PE, z, t0)
FEATURE_BIN_INDEX = [0, 5, 1, 2, 2, 4, 6]
MULT_BINS = [-0.5, 20.5, 21]


def spectrum_bins(bin_overrides=None):
    """``(low, high, bins)`` of the eight spectra: ``AD1Evaluator.default_bins`` after ``override_default_bins`` for the
    seven averages (PE0's entry serves both PE columns, as in the reference), then the multiplicity's."""
    bins = [list(b) for b in DEFAULT_BINS]
    if bin_overrides:
        if not isinstance(bin_overrides, dict):
            bin_overrides = DictionaryUtility.to_dict(bin_overrides)
        for key, value in bin_overrides.items():
            try:
                bins[int(key)] = list(value)
            except ValueError:
                raise IOError("Keys for 'evaluation_config.bin_overrides' dictionary must be integers")
    out = [bins[i] for i in FEATURE_BIN_INDEX] + [MULT_BINS]
    return [(float(lo), float(hi), int(nb)) for lo, hi, nb in out]


class PhysEvaluator:
    def __init__(self, class_names, device, n_bins=100, n_mult=10, n_confusion=10, n_SE_max=4, emin=0.0, emax=10.0,
                 psd_min=0.0, psd_max=0.6, nx=14, ny=11, spectra=False, bin_overrides=None, **ignored):
        """``ignored``: the other keys of a config's ``evaluation_config`` (the reference hands that whole section to its
        evaluators as keywords)."""
        self.device = require_gpu(device, "PhysEvaluator")
        self.class_names = list(class_names)
        self.n_classes = len(self.class_names)
        self.n_bins, self.n_mult, self.n_confusion = int(n_bins), int(n_mult), int(n_confusion)
        self.n_SE_max, self.nx, self.ny = int(n_SE_max), int(nx), int(ny)
        self.emin, self.emax, self.psd_min, self.psd_max = float(emin), float(emax), float(psd_min), float(psd_max)
        lib = _lib.load()
        C = self.n_classes
        n = int(lib.wfs_phys_table_ints(self.n_bins, self.n_mult, self.n_confusion, self.nx, self.ny, C))
        # (name, shape) in the order of include/wfsparse.h
        nm, ne, px, py = self.n_mult + 2, self.n_bins + 2, self.nx + 2, self.ny + 2
        self._layout = [("mult_n", (nm,)), ("mult_m", (nm,)), ("ene_psd_n", (ne, ne)), ("ene_psd_m", (ne, ne)),
                        ("pos_n", (px, py)), ("pos_m", (px, py)), ("confusion_energy", (self.n_confusion + 1, C, C)),
                        ("ene_psd_prec", (C, 2, ne, ne)), ("ene_prec", (C, 2, ne)), ("mult_prec", (C, 2, nm))]
        assert sum(int(np.prod(s)) for _n, s in self._layout) == n
        self.tables = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.spectrum_bins = spectrum_bins(bin_overrides)
        self.spectra = None
        self._spec_ranges = self._spec_bins = None
        if spectra:
            self._spec_bins = _lib.i32_array([nb for _lo, _hi, nb in self.spectrum_bins])
            self._spec_ranges = (ctypes.c_double * 16)(*[v for lo, hi, _nb in self.spectrum_bins for v in (lo, hi)])
            ns = int(lib.wfs_phys_spectra_ints(C, self._spec_bins))
            assert ns == 2 * C * sum(nb + 2 for _lo, _hi, nb in self.spectrum_bins)
            self.spectra = torch.zeros(ns, dtype=torch.int64, device=self.device)
        self._offsets, self._events_cap = None, 0
        self._seen = False                    # a batch has been added since the last reset()

    def _reserve(self, events):
        """Per-batch buffers; allocated on the first call and again only when the event count changes."""
        reserve_offsets(self, events)
        if events != self._events_cap:
            dev = self.device
            self.avg_coo = torch.zeros((events, 2), dtype=torch.float64, device=dev)
            self.features = torch.zeros((N_QUANTITIES + 1, events), dtype=torch.float32, device=dev)
            self.multiplicity = torch.zeros(events, dtype=torch.int32, device=dev)
            self._events_cap = events

    def add(self, batch, output, predictions):
        """``batch`` = ``([coords, feats], labels)`` or, capacity-padded, ``([coords, feats, n_valid], labels)`` with a
        device-side row count; ``feats`` is ``[N, 7]``; ``output`` are the logits (kept for the reference's signature),
        ``predictions`` their argmax.  Launches on the current stream; no read-back, the caller's tensors are only read."""
        inputs, labels = batch
        coords, feats = inputs[0], inputs[1]
        n_valid = inputs[2] if len(inputs) > 2 else None
        require_device_tensors(coords, feats, labels, predictions)
        check_coords(coords, n_valid, "PhysEvaluator.add")
        rows = int(coords.shape[0])
        if feats.dim() != 2 or feats.shape[0] != rows or feats.shape[1] != N_QUANTITIES:
            raise RuntimeError("PhysEvaluator.add: features must be [N, %d] (E, dt, PE0, PE1, z, PSD, t offset), got %s"
                               % (N_QUANTITIES, tuple(feats.shape)))
        E = int(labels.shape[0])
        if predictions.shape[0] != E or labels.dtype != torch.int64 or predictions.dtype != torch.int64:
            raise RuntimeError("PhysEvaluator.add: labels and predictions must be int64 [E]")
        self._reserve(E)
        lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()
        _lib.check(lib.wfs_phys_event_stats(p(coords), p(feats), rows, _lib.dtype_code(feats), p(n_valid), E,
                                            p(self._offsets), p(self.avg_coo), p(self.features), p(self.multiplicity),
                                            p(self.flags), st))
        _lib.check(lib.wfs_phys_accumulate(E, self.n_classes, p(self.avg_coo), p(self.features), p(self.multiplicity),
                                           p(predictions), p(labels), self.n_bins, self.n_mult, self.n_confusion, self.nx,
                                           self.ny, self.emin, self.emax, self.psd_min, self.psd_max, p(self.tables),
                                           self._spec_ranges, self._spec_bins, p(self.spectra), p(self.flags), st))
        self._seen = True

    def reset(self):
        self.tables.zero_()
        self.flags.zero_()
        self._seen = False
        if self.spectra is not None:
            self.spectra.zero_()

    def state_tensors(self):
        """The persistent accumulators; all are integer sums over batches, so N ranks combine them with one SUM
        all-reduce each (psd/evaluate.test_loop)."""
        return [self.tables] if self.spectra is None else [self.tables, self.spectra]

    def results(self):
        """One read-back.  The reference's ``results`` dict after ``finalize()``: (mean, n, M2-after-finalize) triples
        where ``metric_accumulate_1d`` fills them, (sum of matches, n, zeros) where ``metric_accumulate_2d`` does,
        ``ene_acc`` and ``confusion_SE`` as zeros; plus ``features``, the ``[8, E]`` float32 feature matrix of the LAST
        batch (``feature_names`` names its rows; ``[8, 0]`` when no batch came since ``reset()``), and, when asked for,
        ``spectra``."""
        last = [self.features.view(torch.int32)] if self._seen else []        # float32 bits travel in the one copy
        cur = read_back(*([self.flags, self.tables] + ([] if self.spectra is None else [self.spectra]) + last))
        raise_flags("PhysEvaluator", int(cur.take((1,))[0]), FLAG_TEXT)
        t = {name: cur.take(shape).copy() for name, shape in self._layout}
        nb, C = self.n_bins + 2, self.n_classes

        def pair_2d(m, n):
            return m.astype(np.float64), n, np.zeros(n.shape)

        res = {"mult_acc": triple_1d(t["mult_m"], t["mult_n"]),
               "ene_acc": (np.zeros(nb), np.zeros(nb, np.int64), np.zeros(nb)),
               "pos_acc": pair_2d(t["pos_m"], t["pos_n"]),
               "ene_psd_acc": pair_2d(t["ene_psd_m"], t["ene_psd_n"]),
               "confusion_energy": t["confusion_energy"],
               "confusion_SE": np.zeros((self.n_SE_max + 2, C, C), np.int64)}
        for c, name in enumerate(self.class_names):
            res["ene_psd_prec_{}".format(name)] = pair_2d(t["ene_psd_prec"][c, 1], t["ene_psd_prec"][c, 0])
            res["ene_prec_{}".format(name)] = triple_1d(t["ene_prec"][c, 1], t["ene_prec"][c, 0])
            res["mult_prec_{}".format(name)] = triple_1d(t["mult_prec"][c, 1], t["mult_prec"][c, 0])
        assert sorted(res) == sorted(result_shapes(self.class_names, self.n_bins, self.n_mult, self.n_confusion,
                                                   self.n_SE_max, self.nx, self.ny))
        res["feature_names"] = list(FEATURE_NAMES)
        if self.spectra is not None:
            spec = {"by_truth": {}, "by_prediction": {}}
            for side in ("by_truth", "by_prediction"):
                for name in self.class_names:
                    spec[side][name] = {f: cur.take((b[2] + 2,)).copy() for f, b in zip(FEATURE_NAMES,
                                                                                         self.spectrum_bins)}
            res["spectra"] = spec
        bits = cur.rest().astype(np.int32)
        res["features"] = bits.view(np.float32).reshape(N_QUANTITIES + 1, -1)
        return res
