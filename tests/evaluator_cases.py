"""Float64 NumPy restatement of the arithmetic behind the reference's PSDEvaluator.add (src/evaluation/PSDEvaluator.py:101-198
and the helpers it calls in src/utils/SparseUtils.py), written from their behaviour and vectorised over samples and rows.
tests/test_evaluator_host.py holds it against the helper outputs recorded in tests/golden/evaluator_cases.npz; the GPU tests
compare the kernels with the RECORDED values, not with this file.  tools/bench_evaluator.py uses it as the host arm.

It differs from the reference in what is rounded to fp32 on the way (the reference accumulates ``psdl``, ``psdr`` and the
summed pulses in fp32 arrays; here only the results are cast), so whole-batch results agree to fp32 rounding, helper
results to fp64 rounding.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_cases.npz")
PSD_LO, PSD_DIV, PSD_HI = -3, 11, 50
METRIC_NAMES = ["energy", "psd", "multiplicity", "x_dev", "y_dev", "dt_dev", "E_dev", "t_variance", "n_variance"]


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def calc_arrival(v):
    """Half-peak arrival of every row of v [R, T]."""
    v = np.asarray(v, np.float64)
    thresh = 0.5 * np.maximum(v.max(axis=1), 0.0)
    above = v > thresh[:, None]
    has = above.any(axis=1)
    first = np.where(has, above.argmax(axis=1), 0)
    r = np.arange(v.shape[0])
    d = v[r, first]
    dp = v[r, np.maximum(first - 1, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        at0 = thresh / d
        mid = first + (thresh - dp) / (d - dp)
    return np.where(has, np.where(first == 0, at0, mid), 0.0)


def integrate_lininterp_range(v, r0, r1):
    """Rows of v [R, T] integrated from r0 [R] to r1 [R] with linear interpolation at the ends, clamped to the pulse."""
    v = np.asarray(v, np.float64)
    R, T = v.shape
    r0, r1 = np.asarray(r0, np.float64), np.asarray(r1, np.float64)
    i0, i1 = np.ceil(r0).astype(np.int64), np.floor(r1).astype(np.int64)
    d0, d1 = i0 - r0, r1 - i1
    j = np.arange(T)[None, :]
    inside = (j >= np.maximum(i0, 0)[:, None]) & (j <= np.minimum(i1, T - 1)[:, None]) & (i0 <= i1)[:, None]
    s = np.where(inside, v, 0.0).sum(axis=1)
    r = np.arange(R)

    def at(i):
        return v[r, np.clip(i, 0, T - 1)]
    s = s - np.where((0 <= i0) & (i0 < T), (1 - d0) * (1 - d0) / 2 * at(i0), 0.0)
    s = s + np.where((1 <= i0) & (i0 <= T), d0 * d0 / 2 * at(i0 - 1), 0.0)
    s = s - np.where((0 <= i1) & (i1 < T), (1 - d1) * (1 - d1) / 2 * at(i1), 0.0)
    s = s + np.where((-1 <= i1) & (i1 < T - 1), d1 * d1 / 2 * at(i1 + 1), 0.0)
    return s


def calc_psd(v, arrival):
    fast = integrate_lininterp_range(v, arrival + PSD_LO, arrival + PSD_DIV)
    slow = integrate_lininterp_range(v, arrival + PSD_DIV, arrival + PSD_HI)
    tot = slow + fast
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot == 0, 0.0, slow / np.where(tot == 0, 1.0, tot))


def calc_time(v):
    v = np.asarray(v, np.float64)
    t = (v * (np.arange(v.shape[1]) + 0.5)).sum(axis=1)
    s = v.sum(axis=1)
    return np.where(s != 0, t / np.where(s != 0, s, 1.0), 0.0)


def normalize_coords(coord, tot_l, tot_r, psdl, psdr, dt):
    coord = np.array(coord, np.float64)
    if tot_l > 0 or tot_r > 0:
        dt = dt / (tot_l + tot_r)
        coord = coord / (tot_l + tot_r)
    if tot_l > 0:
        psdl = psdl / tot_l
    if tot_r > 0:
        psdr = psdr / tot_r
    return coord, psdl, psdr, dt


def calc_spread(coords, pulses, nsamp, x, y, dt, E):
    """(dx, dy, ddt, dE) of one event: coords [m, >= 2], pulses [m, 2 nsamp] already gain-scaled."""
    m = pulses.shape[0]
    if m < 2:
        return 0.0, 0.0, 0.0, 0.0
    p = np.asarray(pulses, np.float64)
    w = np.arange(nsamp) + 0.5
    totl, totr = p[:, :nsamp].sum(axis=1), p[:, nsamp:].sum(axis=1)
    timel, timer = (p[:, :nsamp] * w).sum(axis=1), (p[:, nsamp:] * w).sum(axis=1)
    both, left, right = (totl > 0) & (totr > 0), (totl > 0) & ~(totr > 0), ~(totl > 0) & (totr > 0)
    sl, sr = np.where(totl > 0, totl, 1.0), np.where(totr > 0, totr, 1.0)
    ddt = np.where(both, np.abs((timer / sr - timel / sl) - dt) * (totl + totr), 0.0)
    ddt = ddt + np.where(left, np.abs(-1.0 * timel / sl - dt) * totl, 0.0)
    ddt = ddt + np.where(right, np.abs(timer / sr - dt) * totr, 0.0)
    dE = np.where(both, np.abs(E - (totl + totr)), 0.0) + np.where(left, np.abs(E - totl), 0.0) \
        + np.where(right, np.abs(E - totr), 0.0)
    t = totl + totr
    tot = t.sum()
    if not tot > 0:
        return 0.0, 0.0, 0.0, 0.0
    dx = (np.abs(coords[:, 0] - x) * t).sum()
    dy = (np.abs(coords[:, 1] - y) * t).sum()
    return dx / tot, dy / tot, ddt.sum() / tot, dE.sum() / m


def moment_variance(data, n, weights=None):
    """First return value (svar) of the reference's moment()."""
    if n <= 1:
        return 0.0
    d = np.asarray(data, np.float64)[:n]
    if weights is None:
        ave = d.sum() / n
        return (((d - ave) ** 2) * (d != 0)).sum() / (n - 1)
    w = np.asarray(weights, np.float64)[:n]
    pos = w > 0
    s, ws = (d * w)[pos].sum(), w[pos].sum()
    ave = s / ws if ws > 0 else s / n
    dev2 = ((d - ave) ** 2) * (d != 0)
    if ws > 0:
        return (dev2 * w).sum() / (ws - 1) if ws > 1 else 0.0
    return dev2.sum() / (n - 1)


def metric_bin(v, low, high, nbins):
    """get_bin_index: underflow 0, >= high -> nbins + 1, else the first j with j * width + low > v."""
    v = np.asarray(v, np.float64)
    width = (high - low) / nbins
    edges = np.arange(1, nbins + 1) * width + low
    gt = edges[None, :] > v[:, None]
    j = np.where(gt.any(axis=1), gt.argmax(axis=1) + 1, 0)
    return np.where(v < low, 0, np.where(v >= high, nbins + 1, j))


def confusion_bin(v, low, high, nbins):
    """confusion_accumulate_1d: -1 = not counted (below low or above high), else (first j with edge > v) - 1, 0 if none."""
    v = np.asarray(v, np.float64)
    width = (high - low) / nbins
    edges = np.arange(1, nbins + 1) * width + low
    gt = edges[None, :] > v[:, None]
    j = np.where(gt.any(axis=1), gt.argmax(axis=1), 0)
    return np.where((v < low) | (v > high), -1, j)


def bin_edges(low, high, nbins):
    return np.arange(0, nbins + 1) * ((high - low) / nbins) + low


def average_pulse(coords, pulses, gains, seg_status, n_events, fix_last_event_n_SE=False):
    """What the reference's average_pulse leaves in its output arrays, for rows grouped by event id 0 .. n_events - 1."""
    coords = np.asarray(coords)
    T = pulses.shape[1] // 2
    g = np.asarray(gains, np.float64)[coords[:, 0], coords[:, 1]]
    left = np.asarray(pulses[:, :T], np.float64) * g[:, :1]
    right = np.asarray(pulses[:, T:], np.float64) * g[:, 1:]
    tot_l, tot_r = left.sum(axis=1), right.sum(axis=1)
    psd_l, psd_r = calc_psd(left, calc_arrival(left)), calc_psd(right, calc_arrival(right))
    dtr = (calc_time(right) - calc_time(left)) * (tot_l + tot_r)
    scaled = np.concatenate([left, right], axis=1).astype(np.float32)          # the reference's in-place fp32 store
    se = np.asarray(seg_status)[coords[:, 0], coords[:, 1]] == 0.5
    out = dict(avg_coo=np.zeros((n_events, 2)), summed=np.zeros((n_events, 2 * T), np.float32),
               stats=np.zeros((6, n_events), np.float32), multiplicity=np.zeros(n_events, np.int32),
               psdl=np.zeros(n_events, np.float32), psdr=np.zeros(n_events, np.float32),
               n_SE=np.zeros(n_events, np.int32))
    times = np.arange(T) + 0.5
    for e in range(n_events):
        rows = np.nonzero(coords[:, 2] == e)[0]
        if len(rows) == 0:
            continue
        tl, tr, t = tot_l[rows].sum(), tot_r[rows].sum(), tot_l[rows] + tot_r[rows]
        coo, pl, pr, dt = normalize_coords((coords[rows, :2] * t[:, None]).sum(axis=0), tl, tr,
                                           (psd_l[rows] * tot_l[rows]).sum(), (psd_r[rows] * tot_r[rows]).sum(),
                                           dtr[rows].sum())
        out["avg_coo"][e], out["psdl"][e], out["psdr"][e] = coo, pl, pr
        out["stats"][:4, e] = calc_spread(coords[rows], scaled[rows], T, coo[0], coo[1], dt, t.sum() / len(rows))
        out["summed"][e] = scaled[rows].astype(np.float64).sum(axis=0)
        pulse = out["summed"][e, :T] + out["summed"][e, T:]
        out["stats"][4, e] = moment_variance(times, T, pulse)
        out["stats"][5, e] = moment_variance(pulse, T)
        out["multiplicity"][e] = len(rows)
        if fix_last_event_n_SE or e != n_events - 1:
            out["n_SE"][e] = se[rows].sum()
    out["energy"] = (out["summed"].astype(np.float64).sum(axis=1) * 0.5).astype(np.float32)
    return out


class HostTables:
    """The accumulators PSDEvaluator.add fills, from average_pulse()'s output."""

    def __init__(self, n_classes, T, n_bins=100, n_mult=10, n_confusion=10, n_SE_max=4, emin=0.0, emax=5.0, psd_min=0.0,
                 psd_max=0.6, nx=14, ny=11):
        self.p = dict(C=n_classes, n_bins=n_bins, n_mult=n_mult, n_confusion=n_confusion, n_SE_max=n_SE_max, emin=emin,
                      emax=emax, psd_min=psd_min, psd_max=psd_max, nx=nx, ny=ny)
        C = n_classes
        z = lambda *s: np.zeros(s, np.int64)                                   # noqa: E731
        self.t = dict(mult_n=z(n_mult + 2), mult_m=z(n_mult + 2), ene_psd_n=z(n_bins + 2, n_bins + 2),
                      ene_psd_m=z(n_bins + 2, n_bins + 2), pos_n=z(nx + 2, ny + 2), pos_m=z(nx + 2, ny + 2),
                      confusion_energy=z(n_confusion + 1, C, C), confusion_SE=z(n_SE_max + 2, C, C), n_wfs=z(C + 1),
                      n_labelled_wfs=z(C))
        self.summed_waveforms = np.zeros((C + 1, 2 * T))
        self.summed_labelled_waveforms = np.zeros((C, 2 * T))

    def add(self, s, predictions, labels):
        p, t = self.p, self.t
        hit = (predictions == labels).astype(np.int64)
        m = s["multiplicity"].astype(np.int64)
        k = metric_bin(m, 0.5, p["n_mult"] + 0.5, p["n_mult"])
        np.add.at(t["mult_n"], k, 1)
        np.add.at(t["mult_m"], k, hit)
        bx = metric_bin(s["energy"], p["emin"], p["emax"], p["n_bins"])
        for psd in (s["psdl"], s["psdr"]):
            by = metric_bin(psd, p["psd_min"], p["psd_max"], p["n_bins"])
            np.add.at(t["ene_psd_n"], (bx, by), 1)
            np.add.at(t["ene_psd_m"], (bx, by), hit)
        qx = metric_bin(s["avg_coo"][:, 0], 0.0, float(p["nx"]), p["nx"])
        qy = metric_bin(s["avg_coo"][:, 1], 0.0, float(p["ny"]), p["ny"])
        np.add.at(t["pos_n"], (qx, qy), 1)
        np.add.at(t["pos_m"], (qx, qy), hit)
        k = confusion_bin(s["energy"], 0.0, p["emax"], p["n_confusion"])
        np.add.at(t["confusion_energy"], (k[k >= 0], labels[k >= 0], predictions[k >= 0]), 1)
        k = confusion_bin(s["n_SE"], -0.5, p["n_SE_max"] + 0.5, p["n_SE_max"] + 1)
        np.add.at(t["confusion_SE"], (k[k >= 0], labels[k >= 0], predictions[k >= 0]), 1)
        t["n_wfs"][0] += m.sum()
        np.add.at(t["n_wfs"], labels + 1, m)
        np.add.at(t["n_labelled_wfs"], predictions, m)
        sm = s["summed"].astype(np.float64)
        self.summed_waveforms[0] += sm.sum(axis=0)
        np.add.at(self.summed_waveforms, labels + 1, sm)
        np.add.at(self.summed_labelled_waveforms, predictions, sm)
