"""Generates tests/golden/pid_evaluator_cases.npz from the REFERENCE's own evaluation arithmetic (the reference tree, this
container only): inputs and the tables its functions give for them.  No reference text is written anywhere; the npz holds
arrays only.  The layout of the file is described in tests/pid_evaluator_cases.py.

How the reference is run (the method of make_evaluator_goldens.py)
  * numba is not installed here, so the functions are taken from src/utils/SparseUtils.py's syntax tree IN MEMORY, their
    ``@nb.jit`` decorators dropped, and executed unmodified: get_bin_index, metric_accumulate_1d, metric_accumulate_2d,
    finalize2d, confusion_accumulate, confusion_accumulate_1d, gen_multiplicity_list, retrieve_n_SE, gen_SE_mask,
    calculate_class_accuracy, find_matches; get_bins from src/utils/util.py the same way.
  * Constructor constants are read from the classes' trees: the normalisation factors and ``default_bins`` of
    AD1Evaluator, the dead-PMT list and ``set_SE_segs`` arithmetic of SingleEndedEvaluator, ``metric_params``, ``scales``,
    ``n_confusion``, ``n_SE_max`` of PIDEvaluator.initialize, the metric names and parameters of
    PSDEvaluator._init_results.  The bodies of PIDEvaluator.add, MetricPairAggregator.add / add_normalized,
    MetricAggregator.add / add_normalized and Metric2DAggregator.add / add_normalized are repeated here call for call.
  * Float widths: the parameter comparisons are float32 elements against float64 edges, which numba computes in float64;
    the functions get float64 arrays holding the fp32 (or bf16 / f16 rounded) values.
  * gen_multiplicity_list and retrieve_n_SE look ahead past the end of the batch.  They are run on the case with ONE
    sentinel row appended whose event index is -1, through a view that reports the case's own row count as its shape: the
    walk is defined, the functions are untouched, the sentinel has no output.
  * confusion_energy: the reference's add passes phys[0] (the first ROW).  The golden is the unmodified
    confusion_accumulate_1d called with the column phys[:, E_index] -- what the call means.
  * PSDEvaluator(metric_pairs=True): the two table batches of evaluator_cases.npz (read only) go through average_pulse
    as in make_evaluator_goldens.py; the metric ranges of energy / psd / multiplicity follow emin / emax / psd_min /
    psd_max / n_mult as the rest of this project's PSDEvaluator does.

Run:  python tests/golden/make_pid_evaluator_goldens.py
"""
import ast
import math
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

WANTED = ["get_bin_index", "metric_accumulate_1d", "metric_accumulate_2d", "finalize2d", "confusion_accumulate",
          "confusion_accumulate_1d", "gen_multiplicity_list", "retrieve_n_SE", "gen_SE_mask", "calculate_class_accuracy",
          "find_matches"]


def _tree(*path):
    return ast.parse(open(os.path.join(REF, *path)).read())


def _functions(tree, wanted, ns):
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(n.name for n in keep) == sorted(wanted)
    for n in keep:
        n.decorator_list = []
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "<reference, in memory>", "exec"), ns)
    return ns


def _method(tree, cls, name):
    c = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
    return [n for n in c.body if isinstance(n, ast.FunctionDef) and n.name == name][0]


def _assigned(fn, attr=None, name=None, kind=ast.expr):
    """The right-hand side of the first ``self.<attr> = ...`` / ``<name> = ...`` in a function, as an expression tree."""
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1:
            t = node.targets[0]
            hit = (attr and isinstance(t, ast.Attribute) and t.attr == attr) or \
                (name and isinstance(t, ast.Name) and t.id == name)
            if hit and isinstance(node.value, kind):
                return node.value
    raise KeyError(attr or name)


def _eval(expr, **ns):
    e = ast.Expression(expr)
    ast.fix_missing_locations(e)
    return eval(compile(e, "<reference expression, in memory>", "eval"), ns)


def reference():
    raw = _functions(_tree("src", "utils", "SparseUtils.py"), WANTED, dict(sqrt=math.sqrt))
    raw.update(_functions(_tree("src", "utils", "util.py"), ["get_bins"], dict(np=np)))
    ad1 = _tree("src", "evaluation", "AD1Evaluator.py")
    consts = {}
    for node in ad1.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            try:
                consts[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    init = _method(ad1, "AD1Evaluator", "__init__")
    me = types.SimpleNamespace(E_scale=consts["E_NORMALIZATION_FACTOR"], z_scale=consts["Z_NORMALIZATION_FACTOR"],
                               E_adjust=1.0)
    for k in ("dt_scale", "toffset_scale", "PE_scale", "E_index", "z_index", "PSD_index"):
        exprs = [n.value for n in ast.walk(init) if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Attribute)
                 and n.targets[0].attr == k]
        setattr(me, k, _eval(exprs[-1], self=me, **consts))
    me.default_bins = _eval(_assigned(init, attr="default_bins"), self=me, **consts)
    se = _tree("src", "evaluation", "SingleEndedEvaluator.py")
    dead = _eval(_assigned(_method(se, "SingleEndedEvaluator", "__init__"), name="SE_dead_pmts", kind=ast.List))
    seg = np.zeros((14, 11), np.float32)
    for pmt in dead:                                     # set_SE_segs
        r = pmt % 2
        s = int((pmt - r) / 2)
        seg[s % 14, math.floor(s / 14)] += 0.5
    pid = _method(_tree("src", "evaluation", "PIDEvaluator.py"), "PIDEvaluator", "initialize")
    me.metric_names = _eval(_assigned(pid, attr="metric_names"))
    me.metric_params = _eval(_assigned(pid, name="metric_params"), self=me)
    me.scales = _eval(_assigned(pid, name="scales"), self=me)
    me.n_confusion, me.n_SE_max = _eval(_assigned(pid, attr="n_confusion")), _eval(_assigned(pid, attr="n_SE_max"))
    psd = _method(_tree("src", "evaluation", "PSDEvaluator.py"), "PSDEvaluator", "_init_results")
    me.psd_names = _eval(_assigned(psd, name="metric_names"))
    stub = types.SimpleNamespace(default_bins=[[0, 0, 1]] * 8, E_index=0, PSD_index=5)
    me.psd_params = _eval(_assigned(psd, name="metric_params"), self=stub)
    return raw, me, seg


class Lookahead:
    """An array with one sentinel row behind it, reporting the length without the sentinel."""

    def __init__(self, rows, sentinel):
        self.ext = np.concatenate([rows, sentinel[None]])
        self.shape = (len(rows),) + rows.shape[1:]

    def __getitem__(self, i):
        return self.ext[i]


def edges_of(raw, low, high, nb):
    e = raw["get_bins"](low, high, nb)                   # MetricAggregator.bin_edges
    return float(e[0]), float(e[-1])


def normalized(lo, hi, norm):                            # MetricAggregator.add_normalized / Metric2DAggregator.get_ranges
    if norm is None:
        return [0.0, 1.0]
    if lo < 0:
        return [lo / norm + 0.5, hi / norm + 0.5]
    return [lo / norm, hi / norm]


class RefPairs:
    """MetricPairAggregator over MetricAggregator / Metric2DAggregator arrays, on the reference's functions."""

    def __init__(self, raw, nbins, C):
        self.raw, self.nbins, self.C = raw, nbins, C
        P = len(nbins)
        self.val = [np.zeros((C, nb + 2)) for nb in nbins]
        self.num = [np.zeros((C, nb + 2), np.int64) for nb in nbins]
        self.M2 = [np.zeros((C, nb + 2)) for nb in nbins]
        self.val2 = {(i, j): np.zeros((C, nbins[i] + 2, nbins[j] + 2)) for i in range(P - 1) for j in range(i + 1, P)}
        self.num2 = {k: np.zeros(v.shape, np.int64) for k, v in self.val2.items()}

    def add(self, results, parameters, c, ranges):       # MetricPairAggregator.add / add_normalized, call for call
        raw, nb = self.raw, self.nbins
        P = parameters.shape[0]
        for i in range(P - 1):
            raw["metric_accumulate_1d"](results, parameters[i, :], self.val[i][c], self.num[i][c], self.M2[i][c],
                                        list(ranges[i]), nb[i])
            for j in range(i + 1, P):
                raw["metric_accumulate_2d"](results, np.stack((parameters[i, :], parameters[j, :]), axis=1),
                                            self.val2[(i, j)][c], self.num2[(i, j)][c], list(ranges[i]), list(ranges[j]),
                                            nb[i], nb[j])
        raw["metric_accumulate_1d"](results, parameters[-1, :], self.val[-1][c], self.num[-1][c], self.M2[-1][c],
                                    list(ranges[-1]), nb[-1])

    def store(self, out, name):
        for i in range(len(self.nbins)):
            self.raw["finalize2d"](self.val[i], self.num[i], self.M2[i])      # MetricAggregator.finalize
            out["%s_m%d_mean" % (name, i)], out["%s_m%d_n" % (name, i)] = self.val[i], self.num[i]
            out["%s_m%d_dev" % (name, i)] = self.M2[i]
        for (i, j), v in self.val2.items():
            assert np.array_equal(v, np.round(v))
            out["%s_p%d_%d_val" % (name, i, j)] = v.astype(np.int64)
            out["%s_p%d_%d_n" % (name, i, j)] = self.num2[(i, j)]


def rounded(a, dtype):
    import torch
    t = torch.from_numpy(np.asarray(a, np.float32)).to(dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[dtype])
    return t.float().numpy()


def edge_values(lo, hi, nb, fall):
    """fp32 probes of one range: around low, around one interior edge, below / at high, +inf, NaN (+ a fall-through)."""
    f = np.float32
    w = (hi - lo) / nb
    k = nb // 3 + 1
    mid = f(k * w + lo)
    vals = [np.nextafter(f(lo), f(-np.inf)), f(lo), np.nextafter(f(lo), f(np.inf)), np.nextafter(mid, f(-np.inf)), mid,
            np.nextafter(mid, f(np.inf)), f(lo + (k + 0.5) * w), np.nextafter(f(hi), f(-np.inf)), f(hi),
            np.nextafter(f(hi), f(np.inf)), f(np.inf), f(np.nan), f(-np.inf)]
    if np.nextafter(f(hi), f(-np.inf)) >= hi:             # fp32(high) lies above high: step down to below it
        vals.append(np.nextafter(np.nextafter(f(hi), f(-np.inf)), f(-np.inf)))
    if fall is not None:
        vals.append(fall)
    return np.array(vals, np.float32)


def find_fall_through(raw, lo, hi, nb):
    """An fp32 value in [low, high) that the reference's walk leaves in bin 0, among the 4096 fp32 values below high and
    the 64 around every interior edge; None if there is none."""
    f = np.float32
    w = (hi - lo) / nb
    v = f(hi)
    for _ in range(4096):
        v = np.nextafter(v, f(-np.inf))
        if lo <= float(v) < hi and raw["get_bin_index"](float(v), lo, hi, w, nb) == 0:
            return v
    for j in range(1, nb + 1):
        v = np.nextafter(f(j * w + lo), f(np.inf))
        for _ in range(4):
            v = np.nextafter(v, f(np.inf))
        for _ in range(8):
            v = np.nextafter(v, f(-np.inf))
            if lo <= float(v) < hi and raw["get_bin_index"](float(v), lo, hi, w, nb) == 0:
                return v
    return None


def main():
    import pid_evaluator_cases as pc
    raw, me, seg = reference()
    rng = np.random.default_rng(20240917)
    out = {"seg_status": seg, "E_scale": np.float64(me.E_scale), "z_scale": np.float64(me.z_scale),
           "metric_names": np.array(me.metric_names), "n_confusion": np.int64(me.n_confusion),
           "n_SE_max": np.int64(me.n_SE_max), "phys_indices": np.array([me.E_index, me.PSD_index, me.z_index])}
    nbins = [int(p[2]) for p in me.metric_params]
    pid_edges = [edges_of(raw, *p) for p in me.metric_params]
    pid_ranges = [normalized(lo, hi, s) for (lo, hi), s in zip(pid_edges, me.scales)]
    out["pid_nbins"], out["pid_edges"], out["pid_ranges"] = np.array(nbins), np.array(pid_edges), np.array(pid_ranges)
    out["pid_metric_params"] = np.array(me.metric_params, np.float64)
    out["pid_confusion_energy_range"] = np.array([0.0, me.n_confusion / me.E_scale])
    # an e_scale / bin_overrides constructor, for the range arithmetic alone
    alt = types.SimpleNamespace(E_scale=8.0, z_scale=me.z_scale)
    alt_bins = [list(b) for b in me.default_bins]
    alt_bins[0][1] = 8.0
    alt_bins[4] = [-500.0, 500.0, 40]
    alt_params = [alt_bins[0], alt_bins[5], [0.5, 6.5, 6], alt_bins[4]]
    alt_edges = [edges_of(raw, *p) for p in alt_params]
    out["alt_ranges"] = np.array([normalized(lo, hi, s) for (lo, hi), s in zip(alt_edges, [8.0, 1.0, 1.0, me.z_scale])])
    out["alt_nbins"] = np.array([int(p[2]) for p in alt_params])

    se_cells = np.argwhere(seg == 0.5)
    de_cells = np.argwhere(seg == 0.0)
    names = []

    def cells(n, n_se):
        pick = np.concatenate([se_cells[rng.choice(len(se_cells), n_se, replace=False)],
                               de_cells[rng.choice(len(de_cells), n - n_se, replace=False)]])
        return pick[rng.permutation(n)]

    def make_phys(n, dtype):
        ph = rng.random((n, 8)).astype(np.float32)
        ph[:, me.E_index] = rng.random(n) * 1.1 - 0.02              # some below 0, some above 10 / 12 and above 1
        ph[:, me.PSD_index] = rng.random(n) * 0.7 - 0.03
        ph[:, me.z_index] = rng.random(n) * 1.1 - 0.05
        return rounded(ph, dtype)

    def make_batch(counts, n_se, dtype, wrong=None, one_class=None):
        co = np.concatenate([np.column_stack([cells(n, k), np.full(n, e)]) for e, (n, k) in enumerate(zip(counts, n_se))])
        N = len(co)
        targ = rng.integers(0, 5, N) if one_class is None else np.full(N, one_class)
        pred = np.where(rng.random(N) < 0.6, targ, rng.integers(0, 5, N))
        if wrong:
            pred = (targ + 1 + rng.integers(0, 4, N)) % 5
        return dict(coords=co.astype(np.int32), pred=pred.astype(np.int64), targ=targ.astype(np.int64),
                    phys=make_phys(N, dtype), n_valid=np.int64(-1))

    def pid_case(name, batches, dtype="f32"):
        pairs = RefPairs(raw, nbins, 5)
        res = {"confusion_energy": np.zeros((me.n_confusion + 1, 5, 5), np.int64),
               "confusion_SE": np.zeros((me.n_SE_max + 2, 5, 5), np.int64), "SE_confusion": np.zeros((5, 5), np.int64)}
        host = pc.HostPIDTables(seg, nbins, pid_ranges, me.E_scale)
        for b, bt in enumerate(batches):
            nv = len(bt["coords"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            coo, results, targ = bt["coords"][:nv], bt["pred"][:nv], bt["targ"][:nv]
            phys = bt["phys"][:nv].astype(np.float64)
            # PIDEvaluator.add, call for call
            accuracy = np.zeros((results.shape[0],), np.int32)
            raw["calculate_class_accuracy"](results, targ, accuracy)
            mult = np.zeros((phys.shape[0],))
            sentinel = np.array([0, 0, -1], coo.dtype)
            raw["gen_multiplicity_list"](Lookahead(coo[:, 2], sentinel[2]), mult)
            parameters = np.stack((phys[:, me.E_index], phys[:, me.PSD_index], mult, phys[:, me.z_index]), axis=1)
            parameters = np.swapaxes(parameters, 0, 1)
            se_mask = np.zeros((coo.shape[0],), dtype=bool)
            raw["gen_SE_mask"](coo, seg, se_mask)
            for i in range(5):
                ind_match = targ == i
                ind_match = ind_match * se_mask
                pairs.add(accuracy[ind_match], parameters[:, ind_match], i, pid_ranges)
            n_SE = np.zeros((results.shape[0],), dtype=np.int32)
            raw["retrieve_n_SE"](Lookahead(coo, sentinel), seg, n_SE)
            raw["confusion_accumulate"](results[se_mask], targ[se_mask], res["SE_confusion"])
            raw["confusion_accumulate_1d"](results, targ, phys[:, me.E_index], res["confusion_energy"],
                                           [0.0, me.n_confusion / me.E_scale], me.n_confusion)
            raw["confusion_accumulate_1d"](results, targ, n_SE, res["confusion_SE"], [-0.5, me.n_SE_max + 0.5],
                                           me.n_SE_max + 1)
            for k, v in bt.items():
                out["%s_b%d_%s" % (name, b, k)] = v
            out["%s_b%d_rows" % (name, b)] = np.stack([accuracy, mult.astype(np.int32), se_mask.astype(np.int32), n_SE])
            host.add(bt["coords"], bt["pred"], bt["targ"], bt["phys"], int(bt["n_valid"]))
        out[name + "_kind"], out[name + "_nb"], out[name + "_dtype"] = np.array("pid"), np.int64(len(batches)), np.array(dtype)
        for k, v in res.items():
            out["%s_%s" % (name, k)] = v
            assert np.array_equal(getattr(host, k), v), (name, k)       # the restatement agrees with the reference
        pairs.store(out, name)
        for i in range(4):
            assert np.array_equal(host.pairs.n1[i], pairs.num[i]), (name, i)
        for k in pairs.val2:
            assert np.array_equal(host.pairs.n2[k], pairs.num2[k]) and np.array_equal(host.pairs.m2[k], pairs.val2[k])
        names.append(name)

    def pairs_case(name, nb, ranges, C, batches, skip_empty):
        pairs = RefPairs(raw, nb, C)
        host = pc.HostPairTables(nb, ranges, C)
        for b, bt in enumerate(batches):
            nv = len(bt["result"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            par, res, cat = bt["params"][:, :nv].astype(np.float64), bt["result"][:nv].astype(np.float64), bt["category"][:nv]
            for i in range(C):
                inds = np.asarray(cat == i).nonzero()[0]
                if skip_empty and len(inds) == 0:               # PSDEvaluator.add:143-147
                    continue
                pairs.add(res[inds], par[:, inds], i, ranges)
            for k, v in bt.items():
                out["%s_b%d_%s" % (name, b, k)] = v
            host.add(bt["params"][:, :nv], bt["result"][:nv], bt["category"][:nv])
        out[name + "_kind"], out[name + "_nb"], out[name + "_dtype"] = np.array("pairs"), np.int64(len(batches)), np.array("f32")
        out[name + "_nbins"], out[name + "_ranges"], out[name + "_C"] = np.array(nb), np.array(ranges, np.float64), np.int64(C)
        pairs.store(out, name)
        for k in pairs.val2:
            assert np.array_equal(host.n2[k], pairs.num2[k]) and np.array_equal(host.m2[k], pairs.val2[k]), (name, k)
        names.append(name)

    # (a) event structure
    pid_case("one_row", [make_batch([1], [1], "f32")])
    pid_case("last_event_se", [make_batch([1, 5, 2], [0, 0, 2], "f32")])
    pid_case("seven_se", [make_batch([3, 9, 2], [1, 7, 0], "f32")])
    b = make_batch([4, 6, 3, 5], [2, 3, 1, 2], "f32")
    b["n_valid"] = np.int64(12)                                          # ends inside event 2
    b["coords"][12:] = [[-5, 40, 999]] * (len(b["coords"]) - 12)
    b["pred"][12:], b["targ"][12:], b["phys"][12:] = 77, -3, np.nan
    pid_case("padded", [b])
    # (c) classes
    b = make_batch([5, 7, 4], [3, 4, 2], "f32")
    b["targ"] = np.where(b["targ"] == 3, 1, b["targ"])
    b["pred"] = np.where(b["pred"] == 3, 0, b["pred"])
    pid_case("empty_class", [b])
    pid_case("one_class", [make_batch([6, 6], [4, 3], "f32", one_class=2)])
    pid_case("all_wrong", [make_batch([6, 5, 4], [4, 3, 2], "f32", wrong=True)])
    # (d) two adds, and the three dtypes of the phys rows (a batch that is more than one workgroup's slice of rows would
    # need > 1024 rows; 64 rows with several events is what the goldens hold, the GPU tests tile them for more blocks)
    for dt in ("f32", "bf16", "f16"):
        pid_case("two_adds_" + dt, [make_batch([8, 1, 12, 6, 9], [5, 1, 6, 2, 4], dt),
                                    make_batch([10, 7, 3, 14], [4, 7, 0, 6], dt)], dt)
    # (b) bin edges of the four PID ranges, per dtype the values that dtype can hold
    fall = {}
    for i, (r, n) in enumerate(zip(pid_ranges, nbins)):
        fall[i] = find_fall_through(raw, r[0], r[1], n)
        print("PID range %d [%r, %r] / %d: fall-through value %s" % (
            i, r[0], r[1], n, "none exists among the fp32 values searched" if fall[i] is None else repr(fall[i])))
    out["pid_fall_through_found"] = np.array([fall[i] is not None for i in range(4)])
    for dt in ("f32", "bf16", "f16"):
        probes = [rounded(edge_values(r[0], r[1], n, fall[i]), dt) for i, (r, n) in enumerate(zip(pid_ranges, nbins))]
        N = max(len(p) for p in probes)
        counts = [1, 2, 3, 4, 5, 6, 7][:]
        while sum(counts) < N:
            counts.append(1)
        counts[-1] -= sum(counts) - N
        counts = [c for c in counts if c > 0]
        b = make_batch(counts, counts, dt)                               # every row single-ended: every row is scored
        for col, p in ((me.E_index, probes[0]), (me.PSD_index, probes[1]), (me.z_index, probes[3])):
            b["phys"][:len(p), col] = p
        pid_case("edges_" + dt, [b], dt)

    # ---- MetricPairTables on its own: the PSD evaluator's nine metrics, C = 2
    ev = np.load(os.path.join(HERE, "evaluator_cases.npz"), allow_pickle=False)
    d = {k: float(ev["default_" + k]) for k in ("n_bins", "n_mult", "emin", "emax", "psd_min", "psd_max")}
    psd_params = [list(p) for p in me.psd_params]
    psd_params[0] = [d["emin"], d["emax"], int(d["n_bins"])]
    psd_params[1] = [d["psd_min"], d["psd_max"], int(d["n_bins"])]
    psd_params[2] = [0.5, d["n_mult"] + 0.5, int(d["n_mult"])]
    psd_nb = [int(p[2]) for p in psd_params]
    psd_ranges = [edges_of(raw, *p) for p in psd_params]
    out["psd_metric_names"], out["psd_nbins"], out["psd_ranges"] = np.array(me.psd_names), np.array(psd_nb), np.array(psd_ranges)
    out["psd_metric_params"] = np.array(psd_params, np.float64)
    pfall = {}
    for i, (r, n) in enumerate(zip(psd_ranges, psd_nb)):
        pfall[i] = find_fall_through(raw, r[0], r[1], n)
        print("PSD range %d [%r, %r] / %d: fall-through value %s" % (
            i, r[0], r[1], n, "none exists among the fp32 values searched" if pfall[i] is None else repr(pfall[i])))
    out["psd_fall_through_found"] = np.array([pfall[i] is not None for i in range(9)])
    probes = [edge_values(r[0], r[1], n, pfall[i]) for i, (r, n) in enumerate(zip(psd_ranges, psd_nb))]
    M = max(len(p) for p in probes)
    par = np.stack([np.resize(p, M) for p in probes]).astype(np.float32)
    par = np.concatenate([par, np.stack([rng.permutation(row) for row in par])], axis=1)      # edges against edges
    M = par.shape[1]
    pairs_case("psd_edges", psd_nb, psd_ranges, 2,
               [dict(params=par, result=rng.integers(0, 2, M).astype(np.int32), category=rng.integers(0, 2, M).astype(np.int32),
                     n_valid=np.int64(-1))], True)

    def rand_params(M):
        return np.stack([(rng.random(M) * 1.3 - 0.1) * (r[1] - r[0]) + r[0] for r in psd_ranges]).astype(np.float32)

    M = 48
    skip = rng.integers(-1, 2, M).astype(np.int32)
    pairs_case("psd_skipped", psd_nb, psd_ranges, 2,
               [dict(params=rand_params(M), result=rng.integers(0, 2, M).astype(np.int32), category=skip, n_valid=np.int64(-1)),
                dict(params=rand_params(M), result=np.zeros(M, np.int32), category=np.ones(M, np.int32), n_valid=np.int64(30))],
               True)
    pairs_case("psd_empty_class", psd_nb, psd_ranges, 2,
               [dict(params=rand_params(M), result=rng.integers(0, 2, M).astype(np.int32), category=np.zeros(M, np.int32),
                     n_valid=np.int64(-1))], True)

    # (f) the kernel keeps the 1-D tables in an LDS image of at most 4096 cells and goes to global atomics above it:
    # 2 metrics of 2040 + 4 bins are 4096 cells with 2 classes and 6144 with 3; the third class stays empty, so the
    # tables of the first two are the same on both sides
    M = 64
    dpar = np.stack([np.r_[edge_values(0.0, 1.0, 2040, None), rng.random(M).astype(np.float32)][:M],
                     (rng.random(M) * 1.2 - 0.1).astype(np.float32)])
    dbatch = dict(params=dpar, result=rng.integers(0, 2, M).astype(np.int32), category=rng.integers(-1, 2, M).astype(np.int32),
                  n_valid=np.int64(-1))
    for C in (2, 3):
        pairs_case("dispatch_C%d" % C, [2040, 4], [(0.0, 1.0), (0.0, 1.0)], C, [dbatch], False)

    # ---- PSDEvaluator(metric_pairs=True) on the two table batches of evaluator_cases.npz
    import make_evaluator_goldens as meg
    _raw, ns = meg.reference_functions()
    pairs = RefPairs(raw, psd_nb, 3)
    feats = []
    for b in range(2):
        labels, predictions = ev["tab%d_labels" % b], ev["tab%d_predictions" % b]
        o = meg.run_average_pulse(ns, ev["tab%d_coords" % b], ev["tab%d_pulses" % b], ev["gains"], ev["seg_status"], len(labels))
        results = raw["find_matches"](predictions, labels, np.zeros((predictions.shape[0],)))
        f = np.concatenate((np.expand_dims(o["energy"], 0), np.expand_dims(o["psdl"], 0),
                            np.expand_dims(o["multiplicity"], 0), o["stats"]), axis=0).astype(np.float64)
        feats.append(f)
        for i in range(3):
            inds = np.asarray(labels == i).nonzero()[0]
            if len(inds) == 0:
                continue
            pairs.add(results[inds], f[:, inds], i, psd_ranges)
    # how far every recorded feature is from its nearest bin edge, relative to the bin width: the GPU's own features
    # agree with the recorded ones to 1e-5 of their scale (tests/test_gpu_evaluator.py), so a clearance above that keeps
    # every event in its bin
    clear = []
    for i, (r, n) in enumerate(zip(psd_ranges, psd_nb)):
        w = (r[1] - r[0]) / n
        v = np.concatenate([f[i] for f in feats])
        e = np.arange(n + 1) * w + r[0]
        dist = np.abs(v[:, None] - e[None, :]).min(axis=1)
        exact = np.isin(v, e)                                           # a value exactly on an edge is exact on both sides
        clear.append(float((dist[~exact] / max(np.abs(v).max(), 1e-30)).min()) if (~exact).any() else np.inf)
    out["psd_tab_clearance"] = np.array(clear)
    print("PSD table batches: smallest distance of a feature to a bin edge, relative to the feature's scale:", clear)
    out["psd_tab_kind"] = np.array("psd_tab")
    pairs.store(out, "psd_tab")

    out["case_names"] = np.array(names)
    path = os.path.join(HERE, "pid_evaluator_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote pid_evaluator_cases.npz: %d arrays, %d cases, %d bytes" % (len(out), len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
