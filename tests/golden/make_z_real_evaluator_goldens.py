"""Generates tests/golden/z_real_evaluator_cases.npz from the REFERENCE's own arithmetic (the reference tree, this container
only): inputs and what its functions give for them.  No reference text is written anywhere; the npz holds arrays only.
The layout of the file is described in tests/z_real_evaluator_cases.py.

How the reference is run (the method and the helpers of make_pid_evaluator_goldens.py)
  * numba is not installed here, so the functions are taken from the syntax trees IN MEMORY, their ``@nb.jit`` decorators
    dropped, and executed unmodified: align_wfs, find_peak, calc_crossing, find_edge_crossing (src/utils/WaveformUtils.py);
    z_deviation_with_E_full_correlation, increment_metric_mult_SE, increment_metric_SE_2d, z_basic_prediction_dense,
    mean_absolute_error_dense, metric_accumulate_dense_1d_with_categories, metric_accumulate_dense_2d_with_categories,
    metric_accumulate_1d, metric_accumulate_2d, get_bin_index, finalize2d, swap_sparse_from_dense
    (src/utils/SparseUtils.py); get_bins (src/utils/util.py).
  * Constructor constants are read from the classes' trees (AD1Evaluator, SingleEndedEvaluator.set_SE_segs with blind_detl,
    RealDataEvaluator, WaveformEvaluator.init_sample_metrics, ZEvaluatorRealWFNorm.__init__, PID_MAP).  The bodies of
    ZEvaluatorRealWFNorm.add, RealDataEvaluator.add, WaveformEvaluator.analyze_wf_z / _align_wfs,
    MetricPairAggregator.add / add_dense_normalized_with_categories and the MetricAggregator / Metric2DAggregator methods
    under them are repeated here call for call.
  * Float widths: numba types ``float32 element (op) float literal`` as float64; the functions get float64 arrays holding
    the fp32 (or bf16 / f16 rounded) values.  The exception is the baseline map, float32 as in the reference.
  * The PID is mapped ONCE (the reference maps it again in analyze_wf_z when no row of the batch mapped to class 3).  A
    batch without a single-ended row skips the class tables (the reference indexes row 0 of an empty list).
  * The generator FAILS rather than records a case in which a ``maxloc + tx`` lies within 1e-6 of a half-integer, a binned
    value lies within 1e-6 of its range of an interior edge without being exactly on it, or a peak lies within 4 samples
    of a row's end (the unmodified align_wfs would index past the row).

Run:  python tests/golden/make_z_real_evaluator_goldens.py
"""
import ast
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_pid_evaluator_goldens as mp                                   # noqa: E402

SPARSE = ["get_bin_index", "metric_accumulate_1d", "metric_accumulate_2d", "finalize2d", "mean_absolute_error_dense",
          "metric_accumulate_dense_1d_with_categories", "metric_accumulate_dense_2d_with_categories",
          "z_basic_prediction_dense", "z_deviation_with_E_full_correlation", "increment_metric_mult_SE",
          "increment_metric_SE_2d", "swap_sparse_from_dense"]
WAVE = ["align_wfs", "find_peak", "calc_crossing", "find_edge_crossing"]
NX, NY = 14, 11


def _module_constants(tree):
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            try:
                out[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    return out


def _last_assigned(fn, attr=None, name=None):
    hits = []
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1:
            t = node.targets[0]
            if (attr and isinstance(t, ast.Attribute) and t.attr == attr) or (name and isinstance(t, ast.Name) and t.id == name):
                hits.append(node.value)
    return hits[-1]


def reference():
    raw = mp._functions(mp._tree("src", "utils", "SparseUtils.py"), SPARSE, dict(sqrt=math.sqrt))
    raw.update(mp._functions(mp._tree("src", "utils", "util.py"), ["get_bins"], dict(np=np)))
    wave = mp._functions(mp._tree("src", "utils", "WaveformUtils.py"), WAVE, {})
    _r, me, seg = mp.reference()
    consts = _module_constants(mp._tree("src", "evaluation", "AD1Evaluator.py"))
    se = mp._tree("src", "evaluation", "SingleEndedEvaluator.py")
    dead = mp._eval(mp._assigned(mp._method(se, "SingleEndedEvaluator", "__init__"), name="SE_dead_pmts", kind=ast.List))
    blindl = np.zeros((NX, NY), np.int8)
    for pmt in dead:                                     # set_SE_segs
        r = pmt % 2
        s = int((pmt - r) / 2)
        if r == 0:
            blindl[s % 14, math.floor(s / 14)] = 1
    me.blindl = blindl
    real = mp._method(mp._tree("src", "evaluation", "RealDataEvaluator.py"), "RealDataEvaluator", "__init__")
    me.real_names = mp._eval(_last_assigned(real, attr="metric_names"))
    me.real_params = mp._eval(_last_assigned(real, name="metric_params"), self=me)
    me.real_scales = mp._eval(_last_assigned(real, name="scales"), self=me)
    assert me.real_names == me.metric_names
    wtree = mp._tree("src", "evaluation", "WaveformEvaluator.py")
    wc = _module_constants(wtree)
    me.n_samples, me.n_zbins = wc["PULSE_ANALYSIS_SAMPLES"], wc["NUM_Z_BINS"]
    me.sample_params = mp._eval(_last_assigned(mp._method(wtree, "WaveformEvaluator", "init_sample_metrics"),
                                               name="metric_params"), range=range, **wc)
    zinit = mp._method(mp._tree("src", "evaluation", "ZEvaluator.py"), "ZEvaluatorRealWFNorm", "__init__")
    me.n_mult, me.n_z = mp._eval(_last_assigned(zinit, attr="n_mult")), mp._eval(_last_assigned(zinit, attr="n_z"))
    me.mult_bounds = mp._eval(_last_assigned(zinit, attr="mult_bounds"))
    me.z_bounds = mp._eval(_last_assigned(zinit, attr="z_bounds"), **consts)
    me.E_bounds = mp._eval(_last_assigned(zinit, attr="E_bounds"), self=me)
    me.n_E = mp._eval(_last_assigned(zinit, attr="n_E"), self=me)
    me.pid_map = _module_constants(mp._tree("src", "evaluation", "PIDEvaluator.py"))["PID_MAP"]
    return raw, wave, me, seg


class RefDensePairs:
    """MetricPairAggregator.add_dense_normalized_with_categories over MetricAggregator / Metric2DAggregator arrays."""

    def __init__(self, raw, names, nbins, ranges, C):
        self.raw, self.names, self.nbins, self.ranges, self.C = raw, names, nbins, ranges, C
        P = len(nbins)
        self.is_mult = [n == "multiplicity" for n in names]
        self.val = [np.zeros((C, nb + 2)) for nb in nbins]
        self.num = [np.zeros((C, nb + 2), np.int64) for nb in nbins]
        self.M2 = [np.zeros((C, nb + 2)) for nb in nbins]
        self.val2 = {(i, j): np.zeros((C, nbins[i] + 2, nbins[j] + 2)) for i in range(P - 1) for j in range(i + 1, P)}
        self.num2 = {k: np.zeros(v.shape, np.int64) for k, v in self.val2.items()}

    def _add1(self, i, results, parameter, categories, c):                # MetricAggregator.add_dense_normalized_...
        self.raw["metric_accumulate_dense_1d_with_categories"](
            results, parameter, self.val[i], self.num[i], self.M2[i], categories, list(self.ranges[i]), self.nbins[i], c,
            use_multiplicity=self.is_mult[i])

    def _add2(self, i, j, results, p1, p2, categories, c):                # Metric2DAggregator.add_dense_normalized_...
        mi = 0 if self.is_mult[i] else (1 if self.is_mult[j] else -1)
        self.raw["metric_accumulate_dense_2d_with_categories"](
            results, np.stack((p1, p2), axis=1), self.val2[(i, j)], self.num2[(i, j)], categories, list(self.ranges[i]),
            list(self.ranges[j]), self.nbins[i], self.nbins[j], c, multiplicity_index=mi)

    def add(self, results, parameters, parameter_names, categories, c):
        idx = self.names.index
        for i in range(len(parameter_names) - 1):
            ind1 = idx(parameter_names[i])
            self._add1(ind1, results, parameters[:, i], categories, c)
            for j in range(i + 1, len(parameter_names)):
                ind2 = idx(parameter_names[j])
                if ind2 < ind1:
                    self._add2(ind2, ind1, results, parameters[:, j], parameters[:, i], categories, c)
                else:
                    self._add2(ind1, ind2, results, parameters[:, i], parameters[:, j], categories, c)
            ind = idx(parameter_names[-1])                                # inside the loop, as in the reference
            self._add1(ind, results, parameters[:, -1], categories, c)


def sparse(out, key, val, num):
    idx = np.flatnonzero(num)
    out[key + "_idx"], out[key + "_n"], out[key + "_val"] = idx.astype(np.int64), num.ravel()[idx], val.ravel()[idx]
    assert not np.any(val.ravel()[num.ravel() == 0])


def store_pairs(raw, out, name, vals, nums, M2s, val2, num2):
    """1-D tables dense (after finalize2d), pair tables sparse over their flattened shape."""
    for i in range(len(vals)):
        raw["finalize2d"](vals[i], nums[i], M2s[i])
        out["%s_m%d_mean" % (name, i)], out["%s_m%d_n" % (name, i)], out["%s_m%d_dev" % (name, i)] = vals[i], nums[i], M2s[i]
    for (i, j), v in val2.items():
        sparse(out, "%s_p%d_%d" % (name, i, j), v, num2[(i, j)])


def near_edge(values, lo, hi, nb, width=None):
    """Which values lie within 1e-6 of the range of an edge without being exactly on it."""
    w = (hi - lo) / nb if width is None else width
    v = np.asarray(values, np.float64).ravel()
    v = v[np.isfinite(v)]
    edges = np.arange(1, nb + 1) * w + lo
    edges = np.concatenate([[lo, hi], edges])
    d = np.abs(v[:, None] - edges[None, :])
    return v[((d < 1e-6 * (hi - lo)) & (d != 0)).any(axis=1)]


def check_clear(what, values, lo, hi, nb, width=None):
    """Every value further than 1e-6 of the range from an interior edge, or exactly on it."""
    bad = near_edge(values, lo, hi, nb, width)
    assert not len(bad), "%s: a value within 1e-6 of an edge: %r" % (what, bad)


def pulse_rows(rng, wave, N, L, peak_max, dtype, sample_bins):
    """Noisy pulses: a rising edge, a peak at a random sample <= peak_max, a decaying tail; amplitudes 0.002 .. 0.08.
    A pulse whose values, once rounded to the dtype, put the arrival sample within 1e-3 of a half-integer (16-bit
    values do that now and then), the peak beyond peak_max, or an aligned sample within 1e-6 of its range of a bin edge
    (sample_bins: (low, high, n) per sample) is drawn again."""
    rows = np.zeros((N, 2 * L), np.float32)
    t = np.arange(L)
    for i in range(N):
        for s in range(2):
            while True:
                pk = rng.integers(1, peak_max + 1)
                amp = rng.uniform(0.002, 0.08)
                rise = np.exp(-0.5 * ((t - pk) / rng.uniform(0.6, 1.6)) ** 2)
                tail = np.exp(-(t - pk) / rng.uniform(1.5, 6.0))
                v = (np.where(t <= pk, rise, tail) * amp + rng.uniform(0, 0.02 * amp, L)).astype(np.float32)
                d = mp.rounded(v, dtype).astype(np.float64)
                maxloc = wave["find_peak"](d)
                with np.errstate(all="ignore"):
                    arrival = maxloc + wave["calc_crossing"](d, -0.5, maxloc)
                if maxloc > peak_max or abs(arrival - math.floor(arrival) - 0.5) <= 1e-3:
                    continue
                wfs = np.zeros((1, 2, len(sample_bins)))
                with np.errstate(all="ignore"):
                    wave["align_wfs"](np.stack([d, d])[None], wfs)
                if not any(len(near_edge(wfs[0, 0, k], lo, hi, nb)) for k, (lo, hi, nb) in enumerate(sample_bins)):
                    break
            rows[i, s * L:(s + 1) * L] = v
    return rows


def pattern_rows(L):
    """The alignment edge cases, one per side: every pattern keeps its peak at most L - 5."""
    f = np.float32
    pats = {}
    base = np.zeros(L, f)
    v = base.copy(); v[:4] = [0.01, 0.2, 1.0, 0.3]; v[4:] = 0.05; pats["clean"] = v
    v = base.copy(); v[:5] = [0.0, 0.3, 0.9, 0.9, 0.2]; pats["flat_top_2"] = v
    if L >= 10:
        v = base.copy(); v[:7] = [0.0, 0.1, 0.7, 0.7, 0.7, 0.4, 0.1]; pats["flat_top_3"] = v
        v = base.copy(); v[:8] = [0.0, 0.3, 0.8, 0.4, 0.8, 0.2, 0.1, 0.0]; pats["two_equal"] = v
        v = base.copy(); v[:8] = [0.0, 0.2, 0.6, 0.3, 0.9, 0.2, 0.0, 0.0]; pats["second_higher"] = v
        v = base.copy(); v[:8] = [0.0, 0.2, 0.9, 0.3, 0.6, 0.2, 0.0, 0.0]; pats["first_higher"] = v
        v = base.copy(); v[:9] = [0.0, 0.2, 0.5, 0.5, 0.3, 0.3, 0.6, 0.1, 0.0]; pats["flat_then_fall"] = v
    else:
        v = base.copy(); v[:6] = [0.0, 0.8, 0.4, 0.8, 0.2, 0.1]; pats["two_equal"] = v
    pats["monotone_up"] = np.linspace(0.1, 1.0, L).astype(f)
    pats["monotone_down"] = np.linspace(1.0, 0.1, L).astype(f)
    pats["all_zero"] = base.copy()
    pats["constant"] = np.full(L, 0.25, f)
    v = base.copy(); v[:4] = [1.0, 0.6, 0.3, 0.1]; pats["peak_at_0"] = v
    v = base.copy(); v[:4] = [0.1, 1.0, 0.5, 0.2]; pats["peak_at_1"] = v
    v = base.copy(); v[:5] = [0.0, 0.45, 1.0, 0.5, 0.2]; pats["start_zero"] = v
    v = base.copy(); v[:5] = [0.8, 0.9, 1.0, 0.5, 0.2]; pats["off_start"] = v
    v = np.full(L, -1.0, f); v[:4] = [-1.0, -0.5, -0.8, -0.9]; pats["negative_peak"] = v       # tx = 0
    v = base.copy(); v[:5] = [0.3, 0.1, 0.25, 0.1, 0.0]; pats["below_first"] = v             # no candidate beats v[0]
    if L > 64:                                   # the kernel's 64-sample chunks
        v = base.copy(); v[2:L - 6] = 0.5; v[1] = 0.2; v[L - 6] = 0.1; pats["long_plateau"] = v
        v = base.copy(); v[40:64] = 0.5; v[39] = 0.2; v[64] = 0.1; pats["fall_in_next_chunk"] = v
    if L >= 80:
        v = base.copy(); v[60:68] = [0.0, 0.1, 0.4, 0.9, 0.9, 0.9, 0.3, 0.0]; pats["plateau_across_chunks"] = v
    names = sorted(pats)
    rows = np.zeros((len(names), 2 * L), f)
    for i, n in enumerate(names):
        rows[i, :L], rows[i, L:] = pats[n], pats[names[(i + 1) % len(names)]]
    return rows, names


def run_align(wave, rows, L, P):
    """_align_wfs, and the start index align_wfs forms on the way (its own lines, repeated)."""
    N = rows.shape[0]
    f = rows.astype(np.float64).reshape((N, 2, L))
    start, arrival = np.zeros((N, 2), np.int32), np.zeros((N, 2))
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(2):
                maxloc = wave["find_peak"](f[i, j])
                assert maxloc <= L - 5, "a peak within 4 samples of the row's end"
                arrival[i, j] = maxloc + wave["calc_crossing"](f[i, j], -0.5, maxloc)
                start[i, j] = int(round(arrival[i, j])) - 1
        frac = np.abs(arrival - np.floor(arrival) - 0.5)
        assert (frac > 1e-6).all(), "an arrival sample within 1e-6 of a half-integer"
        wfs = np.zeros((N, 2, P))
        wave["align_wfs"](f, wfs)
    return wfs, start


def main():
    raw, wave, me, seg = reference()
    rng = np.random.default_rng(20241019)
    E_i, PSD_i, z_i = me.E_index, me.PSD_index, me.z_index
    P = me.n_samples
    out = {"seg_status": seg, "blind_detl": me.blindl.astype(np.int32), "E_scale": np.float64(me.E_scale),
           "z_scale": np.float64(me.z_scale), "phys_indices": np.array([E_i, PSD_i, z_i]),
           "n_mult": np.int64(me.n_mult), "n_z": np.int64(me.n_z), "n_E": np.int64(me.n_E),
           "E_bounds": np.array(me.E_bounds, np.float64), "mult_bounds": np.array(me.mult_bounds, np.float64),
           "z_bounds": np.array(me.z_bounds, np.float64), "default_bins": np.array(me.default_bins, np.float64),
           "n_samples": np.int64(P), "n_zbins": np.int64(me.n_zbins),
           "pid_map": np.array(sorted(me.pid_map.items()), np.int64), "metric_names": np.array(me.real_names)}
    nbins = [int(p[2]) for p in me.real_params]
    edges = [mp.edges_of(raw, *p) for p in me.real_params]
    ranges = [mp.normalized(lo, hi, s) for (lo, hi), s in zip(edges, me.real_scales)]
    out["class_nbins"], out["class_ranges"] = np.array(nbins), np.array(ranges)
    s_nb = [int(p[2]) for p in me.sample_params]
    s_ranges = [mp.edges_of(raw, *p) for p in me.sample_params]
    out["sample_params"], out["sample_nbins"] = np.array(me.sample_params, np.float64), np.array(s_nb)
    out["sample_ranges"] = np.array(s_ranges)
    s_bins = [(r[0], r[1], n) for r, n in zip(s_ranges, s_nb)]
    E_low, E_high = me.E_bounds[0] / me.E_scale, me.E_bounds[1] / me.E_scale
    out["E_range"] = np.array([E_low, E_high])
    tshape = {"seg_mult_zmae": (NX, NY, me.n_mult + 1), "z_mult_single": (me.n_z + 2, me.n_mult + 1),
              "z_mult_dual": (me.n_z + 2, me.n_mult + 1), "z_E_single": (me.n_z + 2, me.n_E + 2),
              "z_E_dual": (me.n_z + 2, me.n_E + 2), "E_mult_single": (me.n_E + 2, me.n_mult + 1),
              "E_mult_dual": (me.n_E + 2, me.n_mult + 1)}
    out["table_names"] = np.array(list(tshape))
    for k, v in tshape.items():
        out["shape_" + k] = np.array(v)

    # ---- alignment alone
    al_names = []
    for L, dts in ((8, ("f32", "bf16", "f16")), (65, ("f32", "bf16", "f16")), (150, ("f32",))):
        pat, pnames = pattern_rows(L)
        out["al_patterns_L%d" % L] = np.array(pnames)
        for dt in dts:
            rows = np.concatenate([pat, pulse_rows(rng, wave, 20, L, L - 5, dt, s_bins)])
            rows = mp.rounded(rows, dt).astype(np.float64)
            wfs, start = run_align(wave, rows, L, P)
            n = "al_L%d_%s" % (L, dt)
            out[n + "_rows"], out[n + "_samples"], out[n + "_start"] = rows, wfs, start
            out[n + "_L"], out[n + "_dtype"] = np.int64(L), np.array(dt)
            al_names.append(n)
    out["align_names"] = np.array(al_names)

    se_cells, de_cells, dead_cells = np.argwhere(seg == 0.5), np.argwhere(seg == 0.0), np.argwhere(seg == 1.0)
    assert len(dead_cells) and (me.blindl[seg == 0.5] == 1).any() and (me.blindl[seg == 0.5] == 0).any()
    pids = np.array(sorted(me.pid_map), np.int64)

    def diag(a, b):
        return abs(a[0] - b[0]) == 1 and abs(a[1] - b[1]) == 1

    def chain():
        """SE a, SE b, DE d with d diagonal to a and b diagonal to a: rows (a, b, d) average a from d, then b from a."""
        for a in se_cells[rng.permutation(len(se_cells))]:
            for b in se_cells:
                for d in de_cells:
                    if diag(a, d) and diag(a, b) and not diag(b, d):
                        return [a, b, d]
        raise AssertionError("no chain")

    def cells(n, n_se, n_dead=0):
        pick = np.concatenate([se_cells[rng.choice(len(se_cells), n_se, replace=False)],
                               dead_cells[rng.choice(len(dead_cells), n_dead, replace=False)],
                               de_cells[rng.choice(len(de_cells), n - n_se - n_dead, replace=False)]])
        return pick[rng.permutation(n)]

    def make_batch(events, L, dtype, pid_pool=pids, pad=0):
        """events: a list of cell arrays [n, 2].  Per-row values, then the dense maps the module hands over."""
        co = np.concatenate([np.column_stack([c, np.full(len(c), e)]) for e, c in enumerate(events)]).astype(np.int32)
        N, B = len(co), len(events)
        phys = rng.random((N, 7)).astype(np.float32)
        phys[:, E_i] = rng.random(N) * 1.1 - 0.02
        phys[:, PSD_i] = rng.random(N) * 0.7 - 0.03
        phys[:, z_i] = rng.random(N) * 0.98 + 0.01
        pr = (phys[:, z_i] + rng.normal(0, 0.05, N)).astype(np.float32)
        return dict(coords=co, phys=phys, pr=pr, pid=pid_pool[rng.integers(0, len(pid_pool), N)].astype(np.int64),
                    feats=pulse_rows(rng, wave, N, L, L - 5, dtype, s_bins), B=B, dtype=dtype, n_valid=np.int64(-1), pad=pad)

    def finish(bt):
        """Round to the dtype, scatter to dense maps, append padding rows."""
        dt, co, N, B = bt["dtype"], bt["coords"], len(bt["coords"]), bt["B"]
        phys, pr, feats = mp.rounded(bt["phys"], dt), mp.rounded(bt["pr"], dt), mp.rounded(bt["feats"], dt)
        pred, targ = np.zeros((B, 1, NX, NY)), np.zeros((B, 7, NX, NY))
        pred[co[:, 2], 0, co[:, 0], co[:, 1]] = pr
        targ[co[:, 2], :, co[:, 0], co[:, 1]] = phys
        pid = bt["pid"]
        if bt["pad"]:
            k = bt["pad"]
            co = np.concatenate([co, np.tile(np.array([[-5, 40, 999]], np.int32), (k, 1))])
            feats = np.concatenate([feats, np.full((k, feats.shape[1]), np.nan, np.float32)])
            pid = np.concatenate([pid, np.full(k, 77, np.int64)])
            bt["n_valid"] = np.int64(N)
        return dict(coords=co, pred=pred, targ=targ, feats=feats.astype(np.float64), pid=pid, n_valid=bt["n_valid"])

    ev_names = []

    def ev_case(name, batches, has_pid=True, wf=True):
        C = 5 if has_pid else 1
        res = {k + cal: (np.zeros(s), np.zeros(s, np.int64)) for cal in ("", "_cal") for k, s in tshape.items()}
        dense = RefDensePairs(raw, me.real_names, nbins, ranges, 5)
        aggs = [mp.RefPairs(raw, s_nb, C) for _ in range(me.n_zbins + 2)] + [mp.RefPairs(raw, s_nb, 1)]
        for b, bt in enumerate(batches):
            bt = finish(bt)
            for k, v in bt.items():
                out["%s_b%d_%s" % (name, b, k)] = v
            nv = len(bt["coords"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            coo, pred, targ, f = bt["coords"][:nv], bt["pred"], bt["targ"], bt["feats"][:nv]
            L = f.shape[1] // 2
            # ZEvaluatorRealWFNorm.add, call for call
            class_indices = bt["pid"][:nv].copy()
            if has_pid:
                results = np.zeros_like(pred[:, 0, :, :])
                raw["mean_absolute_error_dense"](pred[:, 0, :, :], targ[:, z_i, :, :], results)
                # RealDataEvaluator.add
                for key, val in me.pid_map.items():                       # convert_PID
                    class_indices[class_indices == key] = val
                cls_dense = np.zeros((pred.shape[0], NX, NY), np.int64)   # get_dense_matrix
                cls_dense[coo[:, 2], coo[:, 0], coo[:, 1]] = class_indices
                mult_inds = np.zeros((pred.shape[0], NX, NY))
                mult_inds[coo[:, 2], coo[:, 0], coo[:, 1]] = 1
                parameters = np.stack((targ[:, E_i, :], targ[:, PSD_i], mult_inds, targ[:, z_i]), axis=1)
                SE_inds = seg[coo[:, 0], coo[:, 1]] == 0.5                  # retrieve_SE_inds
                if SE_inds.any():
                    dense.add(results, parameters, me.real_names, cls_dense, coo[SE_inds])
                for i, (r, n) in enumerate(zip(ranges, nbins)):
                    if i != 2:
                        check_clear("%s class metric %d" % (name, i), parameters[:, i][mult_inds == 1], r[0], r[1], n)
            if wf:
                z_pred = (pred[:, 0, :, :] - 0.5) * me.z_scale
                z_real = (targ[:, z_i, :, :] - 0.5) * me.z_scale
                z_list, z_pred_list = np.zeros(coo.shape[0]), np.zeros(coo.shape[0])
                raw["swap_sparse_from_dense"](z_pred_list, z_pred, coo)
                raw["swap_sparse_from_dense"](z_list, z_real, coo)
                # analyze_wf_z on the once-mapped classes
                ci = class_indices if has_pid else np.zeros((coo.shape[0]))
                wfs, start = run_align(wave, f, L, P)                     # _align_wfs
                out["%s_b%d_samples" % (name, b)], out["%s_b%d_start" % (name, b)] = wfs, start
                for i, (r, n) in enumerate(zip(s_ranges, s_nb)):
                    check_clear("%s sample %d" % (name, i), wfs[:, :, i], r[0], r[1], n)
                wfs = np.transpose(wfs, (2, 1, 0))
                inc = 1200 / me.n_zbins
                z = z_list
                results_mm = np.abs(z - z_pred_list)
                aggs[-1].add(results_mm, wfs[:, 0], 0, s_ranges)
                aggs[-1].add(results_mm, wfs[:, 1], 0, s_ranges)
                for i in range(me.n_zbins + 2):
                    for j in range(C):
                        cm = (ci == j) if has_pid else np.ones(len(z), bool)
                        if i == 0:
                            inds = cm & (z <= -600)
                        elif i == 11:
                            inds = cm & (z >= 600)
                        elif i == 10:
                            inds = cm & (z > -600 + (i - 1) * inc) & (z < 600)
                        else:
                            inds = cm & (z > -600 + (i - 1) * inc) & (z <= -600 + i * inc)
                        inds = inds == 1
                        aggs[i].add(results_mm[inds], wfs[:, 0, inds], j, s_ranges)
                        aggs[i].add(results_mm[inds], wfs[:, 1, inds], j, s_ranges)
            args = (seg, me.blindl, NX, NY, me.n_mult, me.n_z, me.z_scale, targ[:, E_i, :, :], E_low, E_high, me.n_E)

            def walk(p, cal):
                r = lambda k: res[k + cal]
                raw["z_deviation_with_E_full_correlation"](
                    coo, p, targ[:, z_i, :, :], r("seg_mult_zmae")[0], r("seg_mult_zmae")[1], r("z_mult_dual")[0],
                    r("z_mult_dual")[1], r("z_mult_single")[0], r("z_mult_single")[1], r("z_E_single")[0],
                    r("z_E_single")[1], r("z_E_dual")[0], r("z_E_dual")[1], r("E_mult_single")[0], r("E_mult_single")[1],
                    r("E_mult_dual")[0], r("E_mult_dual")[1], *args)
            walk(pred[:, 0, :, :], "")
            cal_pred = np.zeros((pred.shape[0], NX, NY), np.float32)      # get_dense_matrix(torch.full(.., 0.5), c)
            cal_pred[coo[:, 2], coo[:, 0], coo[:, 1]] = 0.5
            cal_pred[:, seg != 0.5] = targ[:, z_i, seg != 0.5]
            raw["z_basic_prediction_dense"](coo, cal_pred, targ[:, z_i, :, :], truth_is_cal=True)
            out["%s_b%d_baseline" % (name, b)] = cal_pred[coo[:, 2], coo[:, 0], coo[:, 1]].copy()
            assert out["%s_b%d_baseline" % (name, b)].dtype == np.float32
            walk(cal_pred, "_cal")
            tz = targ[coo[:, 2], z_i, coo[:, 0], coo[:, 1]]
            true_z = (tz - 0.5) * me.z_scale
            check_clear(name + " dist", np.concatenate([588. - true_z, 588. + true_z]), 0., 1176., me.n_z,
                        me.z_scale / me.n_z)
            check_clear(name + " E", targ[coo[:, 2], E_i, coo[:, 0], coo[:, 1]], E_low, E_high, me.n_E)
        out[name + "_nb"], out[name + "_has_pid"], out[name + "_wf"] = np.int64(len(batches)), np.int64(has_pid), np.int64(wf)
        out[name + "_dtype"] = np.array(batches[0]["dtype"])
        for k, (s, n) in res.items():
            out["%s_%s_sum" % (name, k)], out["%s_%s_n" % (name, k)] = s, n
        if has_pid:
            store_pairs(raw, out, name + "_class", dense.val, dense.num, dense.M2, dense.val2, dense.num2)
        if wf:
            cat = lambda arrs: np.concatenate(arrs, axis=0)              # [12 C, ...]: category = slice * C + class
            sl = aggs[:-1]
            store_pairs(raw, out, name + "_smp", [cat([a.val[i] for a in sl]) for i in range(P)],
                        [cat([a.num[i] for a in sl]) for i in range(P)], [cat([a.M2[i] for a in sl]) for i in range(P)],
                        {k: cat([a.val2[k] for a in sl]) for k in sl[0].val2},
                        {k: cat([a.num2[k] for a in sl]) for k in sl[0].num2})
            a = aggs[-1]
            store_pairs(raw, out, name + "_allz", a.val, a.num, a.M2, a.val2, a.num2)
        ev_names.append(name)
        print("case %s done" % name)

    def rand_events(counts, n_se, n_dead=None):
        n_dead = n_dead or [0] * len(counts)
        return [cells(n, k, d) for n, k, d in zip(counts, n_se, n_dead)]

    # two adds per dtype; L = 65 for fp32, 8 for the 16-bit rows
    for dt, L in (("f32", 65), ("bf16", 8), ("f16", 8)):
        ev_case("two_adds_" + dt, [make_batch(rand_events([8, 1, 12, 6, 9, 7], [5, 1, 6, 2, 4, 3], [1, 0, 2, 0, 1, 0]), L, dt),
                                   make_batch(rand_events([10, 7, 3, 14], [4, 7, 0, 6], [0, 0, 1, 2]), L, dt)])
    ev_case("L150", [make_batch(rand_events([5, 9, 4, 6], [3, 4, 2, 3]), 150, "f32")])
    # the baseline's walk: chains in event 0 (row 0 of the batch is never a source) and in event 2; an event with only
    # single-ended rows; a double-ended truth of exactly 0.5; z at -600 (a target of exactly 0), 600 and the slice edge 0;
    # E under and over range; multiplicities n_mult and n_mult + 1
    ch0, ch2 = chain(), chain()
    extra = de_cells[[i for i in range(len(de_cells)) if not any((de_cells[i] == c).all() for c in ch2)][:3]]
    bt = make_batch([np.array(ch0), cells(4, 4), np.concatenate([np.array(ch2), extra]), cells(6, 3, 1), cells(7, 3, 1)],
                    8, "f32")
    co = bt["coords"]
    ev2 = np.flatnonzero(co[:, 2] == 2)
    bt["phys"][ev2[3], z_i] = 0.5                                          # double-ended, exactly 0.5
    ev3, ev4 = np.flatnonzero(co[:, 2] == 3), np.flatnonzero(co[:, 2] == 4)
    bt["phys"][ev3[0], z_i], bt["phys"][ev3[1], z_i], bt["phys"][ev3[2], z_i] = 0.0, 1.0, 0.5
    bt["phys"][ev4[0], z_i], bt["phys"][ev4[1], z_i], bt["phys"][ev4[2], z_i] = 0.0, 1.0, 0.5
    bt["phys"][ev3[3], E_i], bt["phys"][ev3[4], E_i] = -0.01, 1.2
    bt["phys"][ev4[3], E_i], bt["phys"][ev4[4], E_i] = -0.01, 1.2
    ev_case("special", [bt])
    # PID absent
    ev_case("no_pid", [make_batch(rand_events([6, 5, 8], [3, 2, 5], [1, 0, 1]), 8, "f32")], has_pid=False)
    # a batch without class 3 (PID 256), with an unmapped PID 2 anywhere and 7 on double-ended rows only
    bt = make_batch(rand_events([7, 6, 9], [4, 3, 5], [0, 1, 0]), 8, "f32", pid_pool=np.array([1, 4, 6, 258, 512, 2], np.int64))
    de_rows = np.flatnonzero(seg[bt["coords"][:, 0], bt["coords"][:, 1]] != 0.5)
    bt["pid"][de_rows[:3]] = 7
    assert (bt["pid"] == 2).any()
    ev_case("no_class3", [bt])
    # n_valid below the row count, NaN in the padding
    ev_case("padded", [make_batch(rand_events([5, 8, 4], [2, 5, 2], [0, 1, 0]), 8, "f32", pad=11)])
    # waveform analysis off
    ev_case("no_wf", [make_batch(rand_events([6, 7], [3, 4]), 8, "f32")], wf=False)

    out["case_names"] = np.array(ev_names)
    path = os.path.join(HERE, "z_real_evaluator_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote z_real_evaluator_cases.npz: %d arrays, %d cases, %d bytes" % (len(out), len(ev_names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
