"""``CalibrationCurves``: the arrays a reference ``Calibrator`` carries (src/evaluation/Calibrator.py:34-56), handed over
as arrays.  The reference fills them from its sqlite calibration database (``PROSPECT_CALDB`` / ``calgroup``); that reader
is not part of this project, so a caller that has the curves passes them in, as ``PredictionWriter(gains=...)`` takes its
gains.  Everything downstream of them, the classical reconstruction ``calc_calib_z_E``, runs on the GPU
(csrc/calibz.hip) and fills the ``*_cal`` and ``E_z_*`` tables of the segment evaluators (segment_evaluator.py).

The file format is an ``.npz`` with exactly the keys of ``SHAPES``.  The arrays are stored as float32, the reference's
dtype; ``to(device)`` uploads fp64 copies of those values once, with ``gain_factor = MAX_RANGE / gains`` formed on the
host in float64 as ``ZEvaluatorWF.__init__`` forms it (src/evaluation/ZEvaluator.py:497-498).
"""
import numpy as np
import torch

from .. import _lib

MAX_RANGE = 2 ** 14 - 1                      # reference src/datasets/HDF5Dataset.py:14-16
NX, NY = 14, 11
T_POINTS, TIME_POINTS, LIGHT_POINTS, SUM_POINTS = 50, 50, 51, 50       # include/wfsparse.h WFS_CALIB_*_POINTS
SHAPES = {"gains": (NX, NY, 2), "eres": (NX, NY, 2), "rel_times": (NX, NY), "sampletime": (NX, NY, 2),
          "t_interp_curves": (NX, NY, 2, T_POINTS, 2), "time_pos_curves": (NX, NY, TIME_POINTS, 2),
          "light_pos_curves": (NX, NY, LIGHT_POINTS, 2), "light_sum_curves": (NX, NY, SUM_POINTS, 2)}
CALGROUP_MESSAGE = ("calgroup= names a group of the reference's sqlite calibration database (PROSPECT_CALDB), which this "
                    "project does not read; pass the curves as calibration=CalibrationCurves.load(path) "
                    "(dataset_config.calibration_file in a config)")


class CalibrationCurves:
    """A plain holder of the eight arrays, validated: shapes as in the reference, every value finite, no zero gain."""

    def __init__(self, **arrays):
        missing, extra = sorted(set(SHAPES) - set(arrays)), sorted(set(arrays) - set(SHAPES))
        if missing or extra:
            raise ValueError("CalibrationCurves: missing %s, unknown %s; the arrays are %s" % (missing, extra, sorted(SHAPES)))
        for name, shape in SHAPES.items():
            a = np.asarray(arrays[name])
            if a.shape != shape:
                raise ValueError("CalibrationCurves: %s must have shape %s, got %s" % (name, shape, a.shape))
            if not np.issubdtype(a.dtype, np.floating) and not np.issubdtype(a.dtype, np.integer):
                raise ValueError("CalibrationCurves: %s must be numeric, got %s" % (name, a.dtype))
            a = np.ascontiguousarray(a, dtype=np.float32)
            if not np.isfinite(a).all():
                raise ValueError("CalibrationCurves: %s holds a value that is not finite" % name)
            setattr(self, name, a)
        if (self.gains == 0).any():
            raise ValueError("CalibrationCurves: gains holds a zero (gain_factor = MAX_RANGE / gains)")
        self._device = {}

    @property
    def gain_factor(self):
        """``np.divide(np.full((nx, ny, 2), MAX_RANGE), gains)``: float64."""
        return np.divide(np.full(SHAPES["gains"], MAX_RANGE), self.gains.astype(np.float64))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if sorted(z.files) != sorted(SHAPES):
                raise ValueError("%s: a calibration file holds exactly %s, got %s" % (path, sorted(SHAPES), sorted(z.files)))
            return cls(**{k: z[k] for k in SHAPES})

    def save(self, path):
        np.savez_compressed(path, **{k: getattr(self, k) for k in SHAPES})

    def to(self, device):
        """The device copies, uploaded once per device: fp64 tensors named as wfs_calib_z_E's arguments."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("CalibrationCurves.to: the reconstruction runs on the GPU only, got %s" % device)
        if device not in self._device:
            host = {"gain_factor": self.gain_factor}
            host.update({k: getattr(self, k).astype(np.float64) for k in SHAPES if k != "gains"})
            self._device[device] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items()}
        return self._device[device]


CURVE_ARGS = ("gain_factor", "eres", "rel_times", "sampletime", "t_interp_curves", "time_pos_curves", "light_pos_curves",
              "light_sum_curves")


class CalibratedReconstruction:
    """``calc_calib_z_E`` on the device rows of a batch: one launch of wfs_calib_z_E into buffers that grow with the
    batch's capacity.  ``run`` returns (z_cal, E_cal) as fp64 [n_cap] tensors; ``state`` and ``peaks`` stay readable until
    the next call."""

    def __init__(self, device, calibration, n_samples=150, sample_width=4, z_scale=1200., nx=NX, ny=NY):
        if not isinstance(calibration, CalibrationCurves):
            raise TypeError("calibration must be a CalibrationCurves, got %s" % type(calibration).__name__)
        if (nx, ny) != (NX, NY):
            raise ValueError("a calibration covers the %d x %d detector, got %d x %d" % (NX, NY, nx, ny))
        self.device = torch.device(device)
        self.calibration, self.curves = calibration, calibration.to(self.device)
        self.n_samples, self.sample_width, self.z_scale = int(n_samples), int(sample_width), float(z_scale)
        self.z = self.E = self.state = self.peaks = None

    def run(self, f, c, flags, n_valid=None):
        n = int(c.shape[0])
        if f.dim() != 2 or f.shape[0] != n or f.shape[1] != 2 * self.n_samples:
            raise RuntimeError("calibration: f must be [%d, %d] (two sides of n_samples = %d), got %s"
                               % (n, 2 * self.n_samples, self.n_samples, tuple(f.shape)))
        if self.z is None or self.z.shape[0] < n:
            self.z = torch.zeros(n, dtype=torch.float64, device=self.device)
            self.E = torch.zeros(n, dtype=torch.float64, device=self.device)
            self.state = torch.zeros(n, dtype=torch.int32, device=self.device)
            self.peaks = torch.full((n, 2, 5), -1, dtype=torch.int32, device=self.device)
        p = _lib.ptr
        _lib.check(_lib.load().wfs_calib_z_E(
            p(f), _lib.dtype_code(f), p(c), n, p(n_valid), self.n_samples, NX, NY, *[p(self.curves[k]) for k in CURVE_ARGS],
            self.sample_width, self.z_scale, p(self.z), p(self.E), p(self.state), p(self.peaks), p(flags),
            _lib.stream_ptr()))
        return self.z, self.E
