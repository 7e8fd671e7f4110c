"""NumPy restatement of the arithmetic behind the reference's PhysEvaluator.add (src/evaluation/PSDEvaluator.py:319-397) and
weighted_average_quantities (src/utils/SparseUtils.py:490-529), written from their behaviour with the accumulator types
numba gives them: the energy and the coordinate sums float64, the six weighted quantities float32, every product and sum
rounded on its own, rows in order.  tests/test_phys_evaluator_host.py holds it against the values recorded in
tests/golden/phys_evaluator_cases.npz; the GPU tests compare the kernels with the RECORDED values and use this file only
where no recording exists (the block-boundary batches).  tools/bench_phys_evaluator.py has its own, vectorised host arm.
"""
import os

import numpy as np

from evaluator_cases import confusion_bin, metric_bin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phys_evaluator_cases.npz")
FEATURES = ["energy", "psd", "rise_time", "PEL", "PER", "z", "start_time", "multiplicity"]
# (low, high, bins) of the spectra: AD1Evaluator.default_bins for E, PSD, dt, PE0, PE0, z, t offset; then the multiplicity
SPECTRUM_BINS = [(0.0, 12.0, 100), (0.0, 0.6, 100), (-15.0, 15.0, 100), (0.0, 5000.0, 100), (0.0, 5000.0, 100),
                 (-600.0, 600.0, 100), (0.0, 30.0, 100), (-0.5, 20.5, 21)]
DEFAULTS = dict(n_bins=100, n_mult=10, n_confusion=10, n_SE_max=4, emin=0.0, emax=10.0, psd_min=0.0, psd_max=0.6, nx=14,
                ny=11)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def derived(f):
    """The stack (energy, psd, dt, PEL, PER, z, t0) [7, N] of PhysEvaluator.add:328-338, in float32 as NumPy forms it."""
    f = np.asarray(f, np.float32)
    h, c = np.float32(0.5), np.float32
    return np.stack((f[:, 0] * c(12.), f[:, 5], (f[:, 1] - h) * c(30.), f[:, 2] * c(5000.), f[:, 3] * c(5000.),
                     (f[:, 4] - h) * c(1200.), f[:, 6] * c(30.)), axis=0)


def event_averages(coords, f, n_events):
    """avg_coo float64 [E, 2], features float32 [8, E] (the seven averages and the multiplicity), multiplicity int32 [E],
    for rows grouped by event number 0 .. n_events - 1."""
    coords = np.asarray(coords)
    q = derived(f)
    avg = np.zeros((n_events, 2))
    feat = np.zeros((8, n_events), np.float32)
    mult = np.zeros(n_events, np.int32)
    for e in range(n_events):
        rows = np.nonzero(coords[:, 2] == e)[0]
        ene, coo, acc = np.float64(0.0), np.zeros(2), np.zeros(7, np.float32)
        for r in rows:
            ene = ene + np.float64(q[0, r])
            coo = coo + coords[r, :2].astype(np.float64) * ene        # the RUNNING sum: the reference's quirk
            acc[1:] = acc[1:] + q[1:, r] * q[0, r]                    # float32 product, float32 sum
        if ene > 0:
            coo = coo / ene
            acc[1:] = (acc[1:].astype(np.float64) / ene).astype(np.float32)
            acc[0] = np.float32(ene)
            mult[e] = len(rows)
        avg[e], feat[:7, e] = coo, acc
    feat[7] = mult
    return avg, feat, mult


class HostTables:
    """The accumulators PhysEvaluator.add fills, from event_averages()'s output, as (count, sum of matches) pairs."""

    def __init__(self, n_classes, spectra=False, **kw):
        self.p = dict(DEFAULTS, C=n_classes, **kw)
        p, C = self.p, n_classes
        nm, ne = p["n_mult"] + 2, p["n_bins"] + 2
        z = lambda *s: np.zeros(s, np.int64)                                   # noqa: E731
        self.t = dict(mult_n=z(nm), mult_m=z(nm), ene_psd_n=z(ne, ne), ene_psd_m=z(ne, ne),
                      pos_n=z(p["nx"] + 2, p["ny"] + 2), pos_m=z(p["nx"] + 2, p["ny"] + 2),
                      confusion_energy=z(p["n_confusion"] + 1, C, C), ene_psd_prec=z(C, 2, ne, ne), ene_prec=z(C, 2, ne),
                      mult_prec=z(C, 2, nm))
        self.spectra = [[[z(nb + 2) for _lo, _hi, nb in SPECTRUM_BINS] for _c in range(C)] for _s in range(2)] \
            if spectra else None

    def add(self, avg_coo, feat, mult, predictions, labels):
        p, t = self.p, self.t
        ok = (predictions >= 0) & (predictions < p["C"]) & (labels >= 0) & (labels < p["C"])
        avg_coo, feat, mult, predictions, labels = avg_coo[ok], feat[:, ok], mult[ok], predictions[ok], labels[ok]
        hit = (predictions == labels).astype(np.int64)
        km = metric_bin(mult.astype(np.float64), 0.5, p["n_mult"] + 0.5, p["n_mult"])
        bx = metric_bin(feat[0], p["emin"], p["emax"], p["n_bins"])
        by = metric_bin(feat[1], p["psd_min"], p["psd_max"], p["n_bins"])
        qx = metric_bin(avg_coo[:, 0], 0.0, float(p["nx"]), p["nx"])
        qy = metric_bin(avg_coo[:, 1], 0.0, float(p["ny"]), p["ny"])
        np.add.at(t["mult_n"], km, 1)
        np.add.at(t["mult_m"], km, hit)
        np.add.at(t["ene_psd_n"], (bx, by), 1)
        np.add.at(t["ene_psd_m"], (bx, by), hit)
        np.add.at(t["pos_n"], (qx, qy), 1)
        np.add.at(t["pos_m"], (qx, qy), hit)
        k = confusion_bin(feat[0], 0.0, p["emax"], p["n_confusion"])
        np.add.at(t["confusion_energy"], (k[k >= 0], labels[k >= 0], predictions[k >= 0]), 1)
        zero = np.zeros_like(labels)
        np.add.at(t["ene_psd_prec"], (labels, zero, bx, by), 1)
        np.add.at(t["ene_psd_prec"], (labels, zero + 1, bx, by), hit)
        np.add.at(t["ene_prec"], (labels, zero, bx), 1)
        np.add.at(t["ene_prec"], (labels, zero + 1, bx), hit)
        np.add.at(t["mult_prec"], (labels, zero, km), 1)
        np.add.at(t["mult_prec"], (labels, zero + 1, km), hit)
        if self.spectra is not None:
            for f, (lo, hi, nb) in enumerate(SPECTRUM_BINS):
                k = metric_bin(feat[f].astype(np.float64), lo, hi, nb)
                for side, key in ((0, labels), (1, predictions)):
                    for c in range(p["C"]):
                        np.add.at(self.spectra[side][c][f], k[key == c], 1)
