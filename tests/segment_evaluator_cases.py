"""Float64 NumPy restatement of the row walks behind the reference's ZEvaluatorWF.add / EnergyEvaluatorWF.add without a
calibration group (z_deviation, z_deviation_with_E, z_error, E_deviation, src/utils/SparseUtils.py:1190-1455), written
from their behaviour and vectorised over rows.  tests/test_segment_evaluator_host.py and the golden generator hold it
against the tables recorded in tests/golden/segment_evaluator_cases.npz; the GPU tests compare the kernels with the
RECORDED values, not with this file.  tools/bench_segment_evaluator.py uses it as the host arm.

It differs from the reference in one thing: the reference adds every deviation into float32 tables as it goes, here the
sums are float64 and cast once.  Integer tables agree exactly, float tables to fp32 rounding of the running sums.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment_evaluator_cases.npz")
DTYPES = ("f32", "bf16", "f16")
Z_DEFAULTS = dict(nmult=6, n_bins=20, n_err_bins=50, error_low=-1000., error_high=1000., z_scale=1200., E_low=0.0,
                  E_high=10.0, true_E_high=9.0, E_scale=12., nx=14, ny=11)
E_DEFAULTS = dict(n_mult=10, n_E=20, n_z=20, E_low=0.0, E_high=9.0, E_scale=12., nx=14, ny=11)
SAMPLE_SEGS = ((5, 4), (10, 3), (7, 5))
Z_PAIRS = ("seg_mult_mae", "z_mult_mae_single", "z_mult_mae_dual", "E_mult_mae_single", "E_mult_mae_dual")
E_PAIRS = ("seg_mult_Emape", "E_mult_single", "E_mult_dual")


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def multiplicity(event):
    """Per row: the length of the run of equal event ids the row belongs to (what the reference's look-ahead finds)."""
    event = np.asarray(event)
    start = np.flatnonzero(np.concatenate([[True], event[1:] != event[:-1]]))
    length = np.diff(np.concatenate([start, [len(event)]]))
    return np.repeat(length, length)


def mult_column(mult, nmult):
    return np.where((mult > 0) & (mult <= nmult), mult - 1, nmult)


def walk_bin(v, low, high, width, nb):
    """get_bin_index: 0 below low, nb + 1 from high, else the first j with j * width + low > v."""
    v = np.asarray(v, np.float64)
    edges = np.arange(1, nb + 1) * width + low
    above = edges[None, :] > v[:, None]
    b = np.where(above.any(axis=1), above.argmax(axis=1) + 1, 0)
    return np.where(v < low, 0, np.where(v >= high, nb + 1, b))


def z_bin(true_z, zrange, nz):
    """z_deviation's walk: the first k with k * (zrange / nz) - zrange / 2 > true_z."""
    true_z = np.asarray(true_z, np.float64)
    edges = np.arange(1, nz + 1) * (zrange / nz) - zrange / 2.
    above = edges[None, :] > true_z[:, None]
    b = np.where(above.any(axis=1), above.argmax(axis=1) + 1, 0)
    return np.where(true_z < -zrange / 2., 0, np.where(true_z >= zrange / 2., nz + 1, b))


def _pair(shape):
    return [np.zeros(shape, np.float64), np.zeros(shape, np.int64)]


def _add(pair, idx, dev):
    np.add.at(pair[0], idx, dev)
    np.add.at(pair[1], idx, 1)


def _rows(coords, maps):
    coords = np.asarray(coords)
    x, y, e = coords[:, 0], coords[:, 1], coords[:, 2]
    return (x, y, e) + tuple(np.asarray(m)[e, x, y].astype(np.float32).astype(np.float64) for m in maps)


class HostZTables:
    """ZEvaluatorWF.add without a calibration group; ``use_energy``: z_deviation_with_E from the E the caller passes."""

    def __init__(self, seg_status, use_energy=False, sample_segs=SAMPLE_SEGS, **params):
        self.p = dict(Z_DEFAULTS, **params)
        self.seg_status, self.use_energy, self.sample_segs = np.asarray(seg_status), use_energy, np.asarray(sample_segs)
        p = self.p
        nm1, nb = p["nmult"] + 1, p["n_bins"] + 2
        self.t = {"seg_mult_mae": _pair((p["nx"], p["ny"], nm1))}
        for k in Z_PAIRS[1:]:
            self.t[k] = _pair((nb, nm1))
        self.t["seg_sample_error"] = np.zeros((len(self.sample_segs), nm1, p["n_err_bins"] + 2), np.int64)
        self.E_high = p["E_high"]

    def add(self, coords, pred, targ, E=None):
        """pred, targ, E: dense [B, nx, ny] maps."""
        p = self.p
        if E is not None:
            self.E_high = p["true_E_high"]                                  # set_true_E
        x, y, e, pv, tv = _rows(coords, (pred, targ))
        col = mult_column(multiplicity(e), p["nmult"])
        dev = np.abs(pv - tv)
        zb = z_bin((tv - 0.5) * p["z_scale"], p["z_scale"], p["n_bins"])
        single = self.seg_status[x, y] > 0
        _add(self.t["seg_mult_mae"], (x, y, col), dev)
        _add(self.t["z_mult_mae_single"], (zb[single], col[single]), dev[single])
        _add(self.t["z_mult_mae_dual"], (zb[~single], col[~single]), dev[~single])
        if E is not None and self.use_energy:
            ev = np.asarray(E)[e, x, y].astype(np.float32) * np.float32(p["E_scale"])   # the host-side float32 product
            eb = walk_bin(ev.astype(np.float64), p["E_low"], self.E_high, (self.E_high - p["E_low"]) / p["n_bins"],
                          p["n_bins"])
            _add(self.t["E_mult_mae_single"], (eb[single], col[single]), dev[single])
            _add(self.t["E_mult_mae_dual"], (eb[~single], col[~single]), dev[~single])
        err = (pv - tv) * p["z_scale"]
        bw = (p["error_high"] - p["error_low"]) / p["n_err_bins"]
        hb = walk_bin(err, p["error_low"], p["error_high"], bw, p["n_err_bins"])
        for s, (sx, sy) in enumerate(self.sample_segs):
            # sample_index takes the first segment that matches
            first = np.ones(len(x), bool)
            for (px, py) in self.sample_segs[:s]:
                first &= ~((x == px) & (y == py))
            on = (x == sx) & (y == sy) & first
            np.add.at(self.t["seg_sample_error"], (np.full(on.sum(), s), col[on], hb[on]), 1)

    def results(self):
        out = {}
        for k, v in self.t.items():
            out[k] = (v[0].astype(np.float32), v[1].astype(np.int32)) if isinstance(v, list) else v.astype(np.int32)
        return out


class HostEnergyTables:
    """EnergyEvaluatorWF.add without a calibration group (E_deviation)."""

    def __init__(self, seg_status, **params):
        self.p = dict(E_DEFAULTS, **params)
        self.seg_status = np.asarray(seg_status)
        p = self.p
        nm1, nb = p["n_mult"] + 1, p["n_E"] + 2
        self.t = {"seg_mult_Emape": _pair((p["nx"], p["ny"], nm1)), "E_mult_single": _pair((nb, nm1)),
                  "E_mult_dual": _pair((nb, nm1))}

    def add(self, coords, pred, targ):
        p = self.p
        x, y, e, pv, tv = _rows(coords, (pred, targ))
        col = mult_column(multiplicity(e), p["n_mult"])
        dev = np.abs(pv - tv) / tv
        eb = walk_bin(tv * p["E_scale"], p["E_low"], p["E_high"], (p["E_high"] - p["E_low"]) / p["n_E"], p["n_E"])
        single = self.seg_status[x, y] > 0
        _add(self.t["seg_mult_Emape"], (x, y, col), dev)
        _add(self.t["E_mult_single"], (eb[single], col[single]), dev[single])
        _add(self.t["E_mult_dual"], (eb[~single], col[~single]), dev[~single])

    def results(self):
        return {k: (v[0].astype(np.float32), v[1].astype(np.int32)) for k, v in self.t.items()}


def assert_tables_match(got, gold, tag, keys, what=""):
    """Integer tables exactly; float tables within 1e-5 of the recorded table's largest absolute entry.  Returns the worst
    ratio seen (error / scale) for printing."""
    worst = 0.0
    for k in keys:
        g = got[k]
        if isinstance(g, tuple):
            ref_s, ref_n = gold[tag + k + "_sum"], gold[tag + k + "_n"]
            assert np.array_equal(np.asarray(g[1], np.int64), ref_n.astype(np.int64)), (what, tag, k, "counts")
            scale = float(np.abs(ref_s).max())
            err = float(np.abs(np.asarray(g[0], np.float64) - ref_s.astype(np.float64)).max())
            assert err <= 1e-5 * scale, (what, tag, k, err, scale)
            if scale > 0:
                worst = max(worst, err / scale)
        else:
            assert np.array_equal(np.asarray(g, np.int64), gold[tag + k].astype(np.int64)), (what, tag, k)
    return worst
