"""``ZEvaluator``, ``EnergyEvaluator``, ``EZEvaluator``: the per-batch half of the reference's per-segment evaluators
(src/evaluation/ZEvaluator.py ``ZEvaluatorBase`` / ``ZEvaluatorWF``, EnergyEvaluator.py ``EnergyEvaluatorWF``,
EZEvaluator.py ``EZEvaluatorBase``) on the GPU.  The calibration database itself is not read; a caller that has the
curves a ``Calibrator`` carries passes them as ``calibration=`` (calibration.py).

The reference's ``add`` copies predictions, targets and coordinates to the host and walks the rows one by one
(``z_deviation``, ``z_deviation_with_E``, ``z_error``, ``E_deviation``, src/utils/SparseUtils.py).  Here ``add`` is two HIP
launches per evaluator on the current stream (csrc/segstats.hip: event offsets, one thread per row); nothing is read back
until ``results()``.  Deviation sums are kept as exact fixed-point integers (2^-32 units), so the tables are bit-identical
from run to run and N ranks combine them with an integer SUM.

What is mirrored: the constructor defaults, the tables of ``add`` with their keys, shapes and dtypes, and the scalars
of ``retrieve_error_metrics`` (returned as a dict instead of TensorBoard calls).  Without a calibration the ``*_cal``
and ``E_z_*`` entries exist and stay zero.  With one, ``add`` first runs the reference's classical reconstruction
``calc_calib_z_E`` on the waveform rows ``f`` (csrc/calibz.hip, one wavefront per row, results stay on the device) and
the accumulate launch scores the prediction and the calibrated value side by side, as the reference's ``hascal`` branches
do (``ZEvaluatorWF.add`` / ``z_from_cal``, ``EnergyEvaluatorWF.add`` / ``calc_deviation_with_z``).  Not mirrored:
``ZEvaluatorPhys``, ``EZEvaluatorPhys``, the sqlite reader behind ``calgroup``, plots.

Two things of the reference that matter for comparing numbers:

* Without a calibration group ``ZEvaluatorWF.add`` uses ``E`` only to switch the energy axis to the true-energy range
  (``set_true_E``): the ``E_mult_mae_*`` tables stay empty.  ``use_energy=True`` is an addition of this project: the
  tables are filled through the ``z_deviation_with_E`` arithmetic from the ``E`` the caller passes (times ``E_scale``).
* ``EZEvaluatorBase.add`` scores plane 0 as energy and plane 1 as z, while ``LitEZ`` concatenates (z, E): the reference
  scores the planes crosswise.  ``EZEvaluator`` keeps that by default; ``planes="lit"`` scores what ``LitEZ`` produces.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .calibration import CalibratedReconstruction
from .eval_common import (FIXED_ONE, check_coords, raise_flags, read_back, require_device_tensors, require_gpu,
                          reserve_offsets, seg_status_tensor)
from .segments import SE_DEAD_PMTS

FLAG_TEXT = {1: "the event column of a batch was not sorted or held an event outside the batch",
             2: "a segment coordinate lay outside the detector grid",
             4: "an energy target was zero (the relative error divides by it)",
             8: "a deviation was not finite or too large for the fixed-point sums, or a sum overflowed",
             16: "a waveform sample or the calibrated z / E of a row was not finite (the reference raises there)"}


def z_result_shapes(nmult=6, n_bins=20, n_err_bins=50, n_sample=3, nx=14, ny=11):
    """Keys of ``ZEvaluatorBase._init_results`` and the shape of each entry's arrays."""
    shapes = {}
    for cal in ("", "_cal"):
        shapes["seg_mult_mae" + cal] = (nx, ny, nmult + 1)
        for k in ("z_mult_mae_single", "z_mult_mae_dual", "E_mult_mae_single", "E_mult_mae_dual"):
            shapes[k + cal] = (n_bins + 2, nmult + 1)
        shapes["seg_sample_error" + cal] = (n_sample, nmult + 1, n_err_bins + 2)
    return shapes


def energy_result_shapes(n_mult=10, n_E=20, n_z=20, nx=14, ny=11):
    """Keys registered by ``EnergyEvaluatorBase.initialize`` and the shape of each entry's arrays."""
    shapes = {}
    for cal in ("", "_cal"):
        shapes["seg_mult_Emape" + cal] = (nx, ny, n_mult + 1)
        for k in ("E_mult_single", "E_mult_dual"):
            shapes[k + cal] = (n_E + 2, n_mult + 1)
        for k in ("E_z_single", "E_z_dual"):
            shapes[k + cal] = (n_E + 2, n_z + 2)
    return shapes


def _plane_args(t, plane, B, nx, ny, what):
    """(pointer, dtype code, batch stride, plane stride, plane) of plane ``plane`` of a [B, P, nx, ny] map; a
    [B, nx, ny] map counts as P = 1."""
    require_device_tensors(t)
    if t.dim() == 3:
        t = t.unsqueeze(1)
    if t.dim() != 4 or t.shape[0] != B or t.shape[2] != nx or t.shape[3] != ny or not 0 <= plane < t.shape[1]:
        raise RuntimeError("%s must be [%d, P > %d, %d, %d], got %s" % (what, B, plane, nx, ny, tuple(t.shape)))
    if t.stride(3) != 1 or t.stride(2) != ny or t.stride(0) < 0 or t.stride(1) < 0:
        raise RuntimeError("%s: the [%d, %d] planes must be contiguous" % (what, nx, ny))
    return ctypes.c_void_p(t.data_ptr()), _lib.dtype_code(t), t.stride(0), t.stride(1), plane


class _SegmentTables:
    """What the two evaluators share: the int64 table buffer, flags, offsets scratch, the split into named tables."""
    name = "segment evaluator"

    def _init_tables(self, n_ints, layout):
        self._layout = layout                     # (name, shape, is_pair) in the order of include/wfsparse.h
        assert sum(int(np.prod(s)) * (2 if pair else 1) for _n, s, pair in layout) == n_ints
        self.tables = torch.zeros(n_ints, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._offsets = None

    def reset(self):
        self.tables.zero_()
        self.flags.zero_()

    def state_tensors(self):
        """The persistent accumulators: integer sums over batches, so N ranks combine them with one SUM all-reduce."""
        return [self.tables]

    def _check_flags(self):
        raise_flags(self.name, int(self.flags.item()), FLAG_TEXT)

    def _read_tables(self):
        """One read-back: {name: (float32 sums, int32 counts)} or {name: int32 counts}."""
        self._check_flags()
        cur, out = read_back(self.tables), {}
        for name, shape, pair in self._layout:
            if pair:
                n, s = cur.take_pair(shape)
                out[name] = ((s.astype(np.float64) / FIXED_ONE).astype(np.float32), n.astype(np.int32))
            else:
                out[name] = cur.take(shape).astype(np.int32)
        return out


class ZEvaluator(_SegmentTables):
    name = "ZEvaluator"

    def __init__(self, device, seg_status=None, use_energy=False, nmult=6, n_bins=20, n_err_bins=50, error_low=-1000.,
                 error_high=1000., z_scale=1200., E_low=0.0, E_high=10.0, true_E_high=9.0, E_scale=12.,
                 sample_segs=((5, 4), (10, 3), (7, 5)), nx=14, ny=11, calibration=None, n_samples=150, sample_width=4):
        self.device = require_gpu(device, "ZEvaluator")
        self.use_energy = bool(use_energy)
        self.nmult, self.n_bins, self.n_err_bins, self.nx, self.ny = int(nmult), int(n_bins), int(n_err_bins), int(nx), int(ny)
        self.error_low, self.error_high, self.z_scale = float(error_low), float(error_high), float(z_scale)
        self.E_low, self.E_high, self.true_E_high, self.E_scale = float(E_low), float(E_high), float(true_E_high), float(E_scale)
        self.has_true_E = False
        self.seg_status = seg_status_tensor(self.device, seg_status, SE_DEAD_PMTS, self.nx, self.ny)
        self.sample_segs = np.asarray(sample_segs, dtype=np.int32).reshape(-1, 2)
        self._sample_segs = torch.from_numpy(np.ascontiguousarray(self.sample_segs)).to(self.device)
        ns, nm1, nb = len(self.sample_segs), self.nmult + 1, self.n_bins + 2
        n = int(_lib.load().wfs_seg_z_table_ints(self.nx, self.ny, self.nmult, self.n_bins, self.n_err_bins, ns))
        layout = [("seg_mult_mae", (self.nx, self.ny, nm1), True), ("z_mult_mae_single", (nb, nm1), True),
                  ("z_mult_mae_dual", (nb, nm1), True), ("E_mult_mae_single", (nb, nm1), True),
                  ("E_mult_mae_dual", (nb, nm1), True), ("seg_sample_error", (ns, nm1, self.n_err_bins + 2), False)]
        self.calibration, self._recon, self._row_scratch = calibration, None, None
        if calibration is not None:
            # ZEvaluatorWF with a calibrator: a second table set of the same layout behind the first
            self._recon = CalibratedReconstruction(self.device, calibration, n_samples, sample_width, self.z_scale,
                                                   self.nx, self.ny)
            layout = layout + [(k + "_cal", shape, pair) for k, shape, pair in layout]
            n *= 2
        self._init_tables(n, layout)

    def set_true_E(self):
        if not self.has_true_E:
            self.has_true_E = True
            self.E_high = self.true_E_high

    def add(self, predictions, target, c, f, E=None, target_is_cal=False, additional_fields=None, n_valid=None):
        """The reference's signature (ZEvaluatorWF.add): ``predictions`` and ``target`` are dense [B, 1, 14, 11] maps
        (plane 0 is scored), ``c`` int32 [N, 3] = (x, y, event), ``E`` an optional dense [B, 14, 11] true-energy map.
        Without a calibration ``f``, ``target_is_cal`` and ``additional_fields`` are ignored.  With one, ``f`` holds
        the waveform rows [N, 2 * n_samples] the calibrated z and E are reconstructed from, and ``target_is_cal=True``
        scores z_from_cal's neighbour-average map (z_basic_prediction_dense) in place of the calibrated z.
        ``n_valid``: device-side row count of a capacity-padded ``c``."""
        self.add_planes(predictions, 0, target, 0, c, E, 0, n_valid, f=f, target_is_cal=target_is_cal)

    def add_planes(self, predictions, pred_plane, target, target_plane, c, E=None, E_plane=0, n_valid=None, f=None,
                   cal=None, target_is_cal=False):
        """``add`` on chosen planes of [B, P, 14, 11] maps, without slicing them.  Launches on the current stream; no
        read-back, the caller's tensors are only read.  ``cal``: (z_cal, E_cal) of these rows when the caller has run the
        reconstruction already (EZEvaluator runs it once for both evaluators)."""
        check_coords(c, n_valid, "ZEvaluator.add")
        B = int(predictions.shape[0])
        if E is not None:
            self.set_true_E()
        pa = _plane_args(predictions, pred_plane, B, self.nx, self.ny, "predictions")
        ta = _plane_args(target, target_plane, B, self.nx, self.ny, "target")
        if self._recon is not None:
            # the reference's hascal branch: z_deviation_with_E for the prediction and for the calibrated z, on the true
            # energy when there is one, else on the calibrated energy
            zc, Ec = cal if cal is not None else self._recon.run(f, c, self.flags, n_valid)
            ea = _plane_args(E, E_plane, B, self.nx, self.ny, "E") if E is not None else (None, _lib.WFS_F32, 0, 0, 0)
            p = _lib.ptr
            scratch = None
            if target_is_cal:
                if self._row_scratch is None or self._row_scratch.shape[1] != c.shape[0]:
                    self._row_scratch = torch.zeros((2, int(c.shape[0])), dtype=torch.float32, device=self.device)
                scratch = self._row_scratch
            _lib.check(_lib.load().wfs_seg_z_accumulate_cal(
                p(c), int(c.shape[0]), p(n_valid), B, *pa, *ta, *ea, p(zc), p(Ec), 1 if target_is_cal else 0, p(scratch),
                p(self.seg_status), self.nx, self.ny,
                p(self._sample_segs), len(self.sample_segs), self.nmult, self.n_bins, self.z_scale, self.n_err_bins,
                self.error_low, self.error_high, self.E_low, self.E_high, self.E_scale, p(reserve_offsets(self, B)),
                p(self.tables), p(self.flags), _lib.stream_ptr()))
            return
        if E is not None and self.use_energy:
            ea = _plane_args(E, E_plane, B, self.nx, self.ny, "E")
        else:
            ea = (None, _lib.WFS_F32, 0, 0, 0)
        p = _lib.ptr
        _lib.check(_lib.load().wfs_seg_z_accumulate(
            p(c), int(c.shape[0]), p(n_valid), B, *pa, *ta, *ea, p(self.seg_status), self.nx, self.ny,
            p(self._sample_segs), len(self.sample_segs), self.nmult, self.n_bins, self.z_scale, self.n_err_bins,
            self.error_low, self.error_high, self.E_low, self.E_high, self.E_scale, p(reserve_offsets(self, B)),
            p(self.tables), p(self.flags), _lib.stream_ptr()))

    def results(self):
        """One read-back.  The reference's ``results`` dict: (float32 sums, int32 counts) pairs, int32 histograms; without
        a calibration the never-filled ``*_cal`` entries as zeros."""
        res = self._read_tables()
        if self._recon is None:
            for k, v in list(res.items()):
                res[k + "_cal"] = tuple(np.zeros_like(a) for a in v) if isinstance(v, tuple) else np.zeros_like(v)
        return res

    def retrieve_error_metrics(self, results=None):
        """The scalars ``ZEvaluatorBase.retrieve_error_metrics`` logs (in mm), under the reference's tag names; the
        per-multiplicity ones as lists over multiplicity 1 .. nmult.  An empty table gives nan, as in the reference."""
        res = self.results() if results is None else results
        out = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for kind in ("single", "dual"):
                s, n = res["z_mult_mae_%s" % kind]
                out["evaluation/%s_mae" % kind] = float(np.sum(s) / np.sum(n) * self.z_scale)
                if self._recon is None:
                    out["evaluation/%s_mae_cal" % kind] = 0.0
                else:
                    sc, nc = res["z_mult_mae_%s_cal" % kind]
                    out["evaluation/%s_mae_cal" % kind] = float(np.sum(sc) / np.sum(nc) * self.z_scale)
                out["evaluation/%s_mae_mult" % kind] = [float(self.z_scale * np.sum(s[:, i]) / np.sum(n[:, i]))
                                                        for i in range(self.nmult)]
        return out


class EnergyEvaluator(_SegmentTables):
    name = "EnergyEvaluator"

    def __init__(self, device, seg_status=None, n_mult=10, n_E=20, E_bounds=(0., 9.), E_scale=12., n_z=20, nx=14, ny=11,
                 calibration=None, z_scale=1200., n_samples=150, sample_width=4):
        self.device = require_gpu(device, "EnergyEvaluator")
        self.n_mult, self.n_E, self.n_z, self.nx, self.ny = int(n_mult), int(n_E), int(n_z), int(nx), int(ny)
        self.E_bounds, self.E_scale = [float(E_bounds[0]), float(E_bounds[1])], float(E_scale)
        self.seg_status = seg_status_tensor(self.device, seg_status, SE_DEAD_PMTS, self.nx, self.ny)
        nm1, nb = self.n_mult + 1, self.n_E + 2
        n = int(_lib.load().wfs_seg_energy_table_ints(self.nx, self.ny, self.n_mult, self.n_E))
        layout = [("seg_mult_Emape", (self.nx, self.ny, nm1), True), ("E_mult_single", (nb, nm1), True),
                  ("E_mult_dual", (nb, nm1), True)]
        self.calibration, self._recon, self.z_scale = calibration, None, float(z_scale)
        if calibration is not None:
            # EnergyEvaluatorWF with a calibrator: the E_z tables, and a second table set for the calibrated energy
            if self.n_z < self.n_E:
                raise ValueError("EnergyEvaluator: with a calibration n_z >= n_E (E_deviation_with_z bins z in n_E bins)")
            self._recon = CalibratedReconstruction(self.device, calibration, n_samples, sample_width, self.z_scale,
                                                   self.nx, self.ny)
            layout = layout + [("E_z_single", (nb, self.n_z + 2), True), ("E_z_dual", (nb, self.n_z + 2), True)]
            layout = layout + [(k + "_cal", shape, pair) for k, shape, pair in layout]
            n = int(_lib.load().wfs_seg_energy_cal_table_ints(self.nx, self.ny, self.n_mult, self.n_E, self.n_z))
        self._init_tables(n, layout)

    def add(self, predictions, target, c, f, n_valid=None):
        """The reference's signature (EnergyEvaluatorWF.add): plane 0 of dense [B, 1, 14, 11] maps.  ``f`` is ignored
        without a calibration; with one it holds the waveform rows [N, 2 * n_samples]."""
        self.add_planes(predictions, 0, target, 0, c, n_valid, f=f)

    def add_planes(self, predictions, pred_plane, target, target_plane, c, n_valid=None, f=None, cal=None):
        check_coords(c, n_valid, "EnergyEvaluator.add")
        B = int(predictions.shape[0])
        pa = _plane_args(predictions, pred_plane, B, self.nx, self.ny, "predictions")
        ta = _plane_args(target, target_plane, B, self.nx, self.ny, "target")
        p = _lib.ptr
        if self._recon is not None:
            # calc_deviation_with_z: the prediction and the calibrated E, both binned by the calibrated z
            zc, Ec = cal if cal is not None else self._recon.run(f, c, self.flags, n_valid)
            _lib.check(_lib.load().wfs_seg_energy_accumulate_cal(
                p(c), int(c.shape[0]), p(n_valid), B, *pa, *ta, p(zc), p(Ec), p(self.seg_status), self.nx, self.ny,
                self.n_mult, self.n_E, self.n_z, self.E_bounds[0], self.E_bounds[1], self.E_scale, self.z_scale,
                p(reserve_offsets(self, B)), p(self.tables), p(self.flags), _lib.stream_ptr()))
            return
        _lib.check(_lib.load().wfs_seg_energy_accumulate(
            p(c), int(c.shape[0]), p(n_valid), B, *pa, *ta, p(self.seg_status), self.nx, self.ny, self.n_mult, self.n_E,
            self.E_bounds[0], self.E_bounds[1], self.E_scale, p(reserve_offsets(self, B)), p(self.tables), p(self.flags),
            _lib.stream_ptr()))

    def results(self):
        """One read-back.  The reference's ``results`` dict; without a calibration ``*_cal`` and the ``E_z_*`` tables are
        zeros of the reference's shapes."""
        res = self._read_tables()
        for k, shape in energy_result_shapes(self.n_mult, self.n_E, self.n_z, self.nx, self.ny).items():
            if k not in res:
                res[k] = (np.zeros(shape, np.float32), np.zeros(shape, np.int32))
        return res

    def retrieve_error_metrics(self, results=None):
        """``EnergyEvaluatorBase.retrieve_error_metrics``: percent errors per energy bin 1 .. n_E."""
        res = self.results() if results is None else results
        out = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for kind in ("single", "dual"):
                s, n = res["E_mult_%s" % kind]
                out["evaluation/%s_E_MAPE" % kind] = [float(100. * np.sum(s[i, :]) / np.sum(n[i, :]))
                                                     for i in range(1, self.n_E + 1)]
                if self._recon is not None:
                    s, n = res["E_mult_%s_cal" % kind]
                    out["evaluation/%s_E_MAPE_cal" % kind] = [float(100. * np.sum(s[i, :]) / np.sum(n[i, :]))
                                                             for i in range(1, self.n_E + 1)]
        return out


class EZEvaluator:
    """``EZEvaluatorBase``: an EnergyEvaluator and a ZEvaluator on the two planes of a [B, 2, 14, 11] map.

    ``planes="reference"`` (default) is the reference's ``add`` literally: plane 0 goes to the energy evaluator, plane 1
    to the z evaluator with target plane 0 as ``E``.  ``LitEZ`` produces (z, E), so the reference scores the planes
    crosswise; ``planes="lit"`` scores plane 0 as z and plane 1 as energy."""

    def __init__(self, device, planes="reference", seg_status=None, use_energy=False, E_scale=12., z_params=None,
                 energy_params=None, calibration=None, n_samples=150, sample_width=4):
        if planes not in ("reference", "lit"):
            raise ValueError("planes must be 'reference' or 'lit', got %r" % (planes,))
        self.device = require_gpu(device, "EZEvaluator")
        self.planes = planes
        self.energy_plane, self.z_plane = (0, 1) if planes == "reference" else (1, 0)
        self.calibration = calibration
        wf = dict(calibration=calibration, n_samples=n_samples, sample_width=sample_width)
        self.EnergyEvaluator = EnergyEvaluator(device, seg_status=seg_status, E_scale=E_scale, **wf, **(energy_params or {}))
        self.ZEvaluator = ZEvaluator(device, seg_status=seg_status, use_energy=use_energy, E_scale=E_scale, **wf,
                                     **(z_params or {}))
        if calibration is not None:
            ra, rb = self.EnergyEvaluator._recon, self.ZEvaluator._recon
            if (ra.n_samples, ra.sample_width, ra.z_scale) != (rb.n_samples, rb.sample_width, rb.z_scale):
                raise ValueError("EZEvaluator: the two evaluators must agree on n_samples, sample_width and z_scale")

    def add(self, predictions, target, c, f, n_valid=None):
        cal = None
        if self.calibration is not None:
            # one reconstruction serves both; its flag lands in the energy evaluator's word, which results() reads
            cal = self.EnergyEvaluator._recon.run(f, c, self.EnergyEvaluator.flags, n_valid)
        self.EnergyEvaluator.add_planes(predictions, self.energy_plane, target, self.energy_plane, c, n_valid, cal=cal)
        self.ZEvaluator.add_planes(predictions, self.z_plane, target, self.z_plane, c, target, self.energy_plane, n_valid,
                                   cal=cal)

    def reset(self):
        self.EnergyEvaluator.reset()
        self.ZEvaluator.reset()

    def state_tensors(self):
        return self.EnergyEvaluator.state_tensors() + self.ZEvaluator.state_tensors()

    def results(self):
        return {"EnergyEvaluator": self.EnergyEvaluator.results(), "ZEvaluator": self.ZEvaluator.results()}

    def retrieve_error_metrics(self):
        out = self.EnergyEvaluator.retrieve_error_metrics()
        out.update(self.ZEvaluator.retrieve_error_metrics())
        return out
