"""Generates tests/golden/evaluator_cases.npz from the REFERENCE's own evaluation arithmetic (the reference tree, this
container only): inputs and the outputs its functions give for them.  No reference text is written anywhere; the npz holds
arrays only.

How the reference is run
  * numba is not installed here, so src/utils/SparseUtils.py cannot be imported.  Its functions are taken from the file's
    syntax tree IN MEMORY, their ``@nb.jit`` decorators dropped (an identity jit), and executed unmodified:
    calc_arrival, calc_psd, integrate_lininterp_range, sum_range, calc_time, calc_spread, normalize_coords, moment,
    find_max, vec_sum, get_residual, get_bin_index, metric_accumulate_1d, metric_accumulate_2d, confusion_accumulate_1d,
    find_matches, finalize.
  * ``average_pulse`` AS A WHOLE is run from that in-memory copy with its one division ``pulses.shape[1] / 2`` made
    integral (plain Python refuses the float slice bound; nothing else of it is touched, nothing of it goes to disk).
  * numba would type the accumulators of calc_spread and moment as float64 (an int or float literal unified with a
    float32 element); plain Python keeps a float32 running sum instead.  To record what the reference computes under
    numba, average_pulse sees calc_spread and moment through wrappers that hand the same float32 VALUES over as float64
    arrays.  The helpers recorded on their own get float64 inputs directly.
  * PSDEvaluator.add itself is not executed (TensorBoard, torchmetrics, plotting); its accumulation calls are repeated
    here, argument for argument, on the reference's helpers.  Where add() passes a three-array result tuple to
    metric_accumulate_2d (which takes two arrays) the first two are passed.  The constructor defaults and the
    metric names are read from the class's syntax tree (literal assignments in __init__, the list in _init_results); the
    result keys and shapes are those of _init_results for these defaults.

Run:  python tests/golden/make_evaluator_goldens.py
"""
import ast
import math
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

WANTED = ["moment", "find_matches", "vec_sum", "confusion_accumulate_1d", "get_bin_index", "metric_accumulate_1d",
          "metric_accumulate_2d", "normalize_coords", "calc_spread", "calc_time", "find_max", "average_pulse",
          "calc_arrival", "calc_psd", "integrate_lininterp_range", "sum_range", "get_residual", "finalize"]


def reference_functions():
    tree = ast.parse(open(os.path.join(REF, "src", "utils", "SparseUtils.py")).read())
    keep = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in WANTED:
            node.decorator_list = []
            if node.name == "average_pulse":
                n_div = 0
                for sub in ast.walk(node):
                    if isinstance(sub, ast.BinOp) and isinstance(sub.op, ast.Div) and \
                            isinstance(sub.right, ast.Constant) and sub.right.value == 2 and \
                            isinstance(sub.left, ast.Subscript):
                        sub.op = ast.FloorDiv()
                        n_div += 1
                assert n_div == 1
            keep.append(node)
    assert sorted(n.name for n in keep) == sorted(WANTED)
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = dict(ceil=math.ceil, floor=math.floor, sqrt=math.sqrt, log=math.log, exp=math.exp, zeros=np.zeros,
              int32=np.int32, float32=np.float32)
    exec(compile(mod, "<reference SparseUtils, in memory>", "exec"), ns)
    raw = dict(ns)
    # what average_pulse sees: numba's float64 accumulators (see the docstring)
    ns["calc_spread"] = lambda coords, pulses, *a: raw["calc_spread"](coords, pulses.astype(np.float64), *a)
    ns["moment"] = lambda data, n, weights=None: raw["moment"](
        np.asarray(data, np.float64), n, None if weights is None else np.asarray(weights, np.float64))
    return raw, ns


def reference_defaults():
    tree = ast.parse(open(os.path.join(REF, "src", "evaluation", "PSDEvaluator.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PSDEvaluator"][0]
    init = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
    out = {}
    for node in ast.walk(init):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Attribute):
            try:
                v = ast.literal_eval(node.value)
            except ValueError:
                continue
            if isinstance(v, (int, float)) and not isinstance(v, bool):
                out.setdefault(node.targets[0].attr, float(v))
    res = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_init_results"][0]
    names = None
    for node in ast.walk(res):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "metric_names":
            names = [e.value for e in node.value.elts]
    return out, names


def make_rows(rng, n, T, dtype):
    """n plausible PMT pulse pairs [n, 2T] in [0, 1]: a fast rise, a two-component decay, a little positive noise."""
    import torch
    t = np.arange(T)[None, :]
    rows = np.zeros((n, 2 * T))
    for h in range(2):
        t0 = rng.uniform(2, max(3.0, T * 0.3), (n, 1))
        amp = rng.uniform(0.05, 1.0, (n, 1))
        slow = rng.uniform(0.05, 0.5, (n, 1))
        x = np.maximum(t - t0, 0.0)
        shape = (1 - np.exp(-x / 1.5)) * ((1 - slow) * np.exp(-x / 4.0) + slow * np.exp(-x / 25.0))
        rows[:, h * T:(h + 1) * T] = amp * shape + np.abs(rng.normal(0, 0.002, (n, T)))
    r = torch.from_numpy(rows).to(dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[dtype])
    return r.float().numpy()                                                   # the rounded values, as float32


def run_average_pulse(ns, coords, pulses, gains, seg_status, E):
    T = pulses.shape[1] // 2
    o = dict(avg_coo=np.zeros((E, 2)), summed=np.zeros((E, 2 * T), np.float32), stats=np.zeros((6, E), np.float32),
             multiplicity=np.zeros(E, np.int32), psdl=np.zeros(E, np.float32), psdr=np.zeros(E, np.float32),
             n_SE=np.zeros(E, np.int32))
    with np.errstate(all="ignore"):
        ns["average_pulse"](coords, pulses.copy(), gains, np.arange(0.5, T - 0.49, 1.0), o["avg_coo"], o["summed"],
                            o["stats"], o["multiplicity"], o["psdl"], o["psdr"], o["n_SE"], seg_status)
    o["energy"] = np.sum(o["summed"], axis=1) * 0.5                            # PSDEvaluator.add:130
    return o


def coords_for(rng, counts, nx=14, ny=11):
    rows = []
    for e, n in enumerate(counts):
        cells = rng.choice(nx * ny, size=n, replace=False)
        rows += [(c // ny, c % ny, e) for c in cells]
    return np.array(rows, np.int32)


def main():
    raw, ns = reference_functions()
    defaults, metric_names = reference_defaults()
    out = {}
    for k in ["n_bins", "n_mult", "emin", "emax", "psd_min", "psd_max", "nx", "ny", "n_samples", "n_confusion", "n_SE_max"]:
        out["default_" + k] = np.float64(defaults[k])
    out["metric_names"] = np.array(metric_names)
    rng = np.random.default_rng(20240611)
    gains = rng.uniform(0.8, 1.25, (14, 11, 2))
    gains[2, 3], gains[5, 6] = 1.0, 1.0
    seg = np.zeros((14, 11), np.float32)
    seg.flat[rng.choice(14 * 11, 30, replace=False)] = 0.5
    seg[0, 0], seg[13, 10] = 1.0, 0.5
    out["gains"], out["seg_status"] = gains, seg

    # ---- per-event statistics: 7 events of 1, 2, 3, 5, 1, 17, 64 rows
    counts = [1, 2, 3, 5, 1, 17, 64]
    first = np.concatenate([[0], np.cumsum(counts)])
    for T in (20, 150):
        for dtype in ("f32", "bf16", "f16"):
            c = coords_for(rng, counts)
            c[first[5]], c[first[5] + 1] = (13, 10, 5), (0, 0, 5)            # a 0.5 and a 1.0 cell for certain
            c[first[6]] = (13, 10, 6)
            p = make_rows(rng, len(c), T, dtype)
            p[first[1]:first[2]] = 0                                           # event 1: no charge at all, two rows
            p[first[2]] = 0                                                    # an all-zero row inside an event
            p[first[3], T:] = 0                                                # right half all zeros
            p[first[3] + 1, :T] = 0                                            # left half all zeros
            p[first[3] + 2, 0] = 2 * p[first[3] + 2, :T].max()                 # left peak at sample 0
            p[first[3] + 3, 2 * T - 1] = 2 * p[first[3] + 3, T:].max()         # right peak at the last sample
            p[first[3] + 3, T - 1] = 2 * p[first[3] + 3, :T].max()             # left peak at the last sample
            o = run_average_pulse(ns, c, p, gains, seg, len(counts))
            tag = "stats_T%d_%s_" % (T, dtype)
            out[tag + "coords"], out[tag + "pulses"] = c, p
            for k, v in o.items():
                out[tag + k] = v

    # ---- helpers on their own (float64 inputs), for the NumPy restatement
    T = 20
    hp = make_rows(rng, 12, T, "f32")[:, :T].astype(np.float64)
    hp[0] = 0
    hp[1, 0] = 3.0
    hp[2, T - 1] = 3.0
    hp[3, 5:] = 0
    arr = np.array([raw["calc_arrival"](r) for r in hp])
    out["h_pulses"], out["h_arrival"] = hp, arr
    out["h_psd"] = np.array([raw["calc_psd"](r, a, -3, 50, 11, 0) for r, a in zip(hp, arr)], np.float64)
    out["h_time"] = np.array([raw["calc_time"](r, T) for r in hp], np.float64)
    rr = np.array([[-3.5, 2.25], [0.0, 19.0], [4.75, 4.9], [18.5, 70.0], [-9.0, -2.0], [25.0, 30.0], [3.0, 3.0],
                   [19.5, 20.5], [-1.0, 0.5], [6.5, 5.5]])
    out["h_ranges"] = rr
    out["h_integ"] = np.array([[raw["integrate_lininterp_range"](r, a, b) for a, b in rr] for r in hp], np.float64)
    sc = coords_for(rng, [6])
    sp = make_rows(rng, 6, T, "f32").astype(np.float64)
    sp[1, T:] = 0
    sp[2, :T] = 0
    sp[3] = 0
    out["h_spread_coords"], out["h_spread_pulses"] = sc, sp
    out["h_spread_args"] = np.array([5.3, 4.1, 0.7, 2.9])
    out["h_spread"] = np.array(raw["calc_spread"](sc, sp, T, 6, 5.3, 4.1, 0.7, 2.9), np.float64)
    out["h_spread_one"] = np.array(raw["calc_spread"](sc[:1], sp[:1], T, 1, 5.3, 4.1, 0.7, 2.9), np.float64)
    out["h_spread_zero"] = np.array(raw["calc_spread"](sc[:2], sp[:2] * 0, T, 2, 5.3, 4.1, 0.7, 2.9), np.float64)
    times = np.arange(0.5, T - 0.49, 1.0)
    mo = []
    for w in (hp[4], hp[0], hp[5] * 0.01, hp[6] - 0.1):                        # usual, no weight, weight sum < 1, some < 0
        mo.append([raw["moment"](times, T, weights=w)[0], raw["moment"](w, T)[0]])
    out["h_moment_weights"] = np.array([hp[4], hp[0], hp[5] * 0.01, hp[6] - 0.1])
    out["h_moment"] = np.array(mo, np.float64)
    nc = []
    for tl, tr in [(2.0, 3.0), (0.0, 3.0), (2.0, 0.0), (0.0, 0.0)]:
        coo, a, b, d = raw["normalize_coords"](np.array([7.0, 9.0]), tl, tr, 1.5, 0.6, 4.0)
        nc.append([coo[0], coo[1], a, b, d])
    out["h_normalize"] = np.array(nc, np.float64)
    vals = np.array([-0.2, 0.0, 0.05, 0.1, 0.15, 0.3, 2.5, 4.95, 4.999999, 5.0, 5.000001, 7.0, 0.6, 0.006, 0.012])
    out["h_bin_values"] = vals
    for name, (lo, hi, nb) in dict(e=(0.0, 5.0, 100), p=(0.0, 0.6, 100), c=(0.0, 5.0, 10), s=(-0.5, 4.5, 5)).items():
        out["h_metric_bin_" + name] = np.array([raw["get_bin_index"](v, lo, hi, (hi - lo) / nb, nb) for v in vals])
        cb = []
        for v in vals:
            t = np.zeros((nb + 1, 1, 1), np.int64)
            raw["confusion_accumulate_1d"](np.array([0]), np.array([0]), np.array([v]), t, [lo, hi], nb)
            cb.append(int(np.argmax(t[:, 0, 0])) if t.sum() else -1)
        out["h_confusion_bin_" + name] = np.array(cb)

    # ---- tables: two batches, T = 20, three class names of which class 2 never occurs
    T, C = 20, 3
    P = {k: defaults[k] for k in ["n_bins", "n_mult", "emin", "emax", "psd_min", "psd_max", "nx", "ny", "n_confusion",
                                  "n_SE_max"]}
    nb, nm, ncf, nse, nx, ny = (int(P[k]) for k in ["n_bins", "n_mult", "n_confusion", "n_SE_max", "nx", "ny"])
    edges = dict(e=np.arange(nb + 1) * ((P["emax"] - P["emin"]) / nb) + P["emin"],
                 c=np.arange(ncf + 1) * (P["emax"] / ncf),
                 p=np.arange(nb + 1) * ((P["psd_max"] - P["psd_min"]) / nb) + P["psd_min"],
                 x=np.arange(nx + 1.0), y=np.arange(ny + 1.0))

    def clear(v, e):
        return np.abs(np.asarray(v, np.float64)[..., None] - e).min() > 1e-4

    def candidate(n_rows, scale):
        c = coords_for(rng, [n_rows])
        p = make_rows(rng, n_rows, T, "f32") * np.float32(scale)
        return c, p

    def crafted_at_high():
        # energy exactly emax = 5: two rows on unit-gain cells, every number a small dyadic -> exact in any order
        c = np.array([(2, 3, 0), (5, 6, 0)], np.int32)
        p = np.zeros((2, 2 * T), np.float32)
        for r in range(2):
            for h in range(2):
                p[r, h * T], p[r, h * T + 15] = 2.0, 0.5
        return c, p

    results = {"mult_acc": (np.zeros(nm + 2), np.zeros(nm + 2, np.int64), np.zeros(nm + 2)),
               "pos_acc": (np.zeros((nx + 2, ny + 2)), np.zeros((nx + 2, ny + 2), np.int64)),
               "ene_psd_acc": (np.zeros((nb + 2, nb + 2)), np.zeros((nb + 2, nb + 2), np.int64)),
               "confusion_energy": np.zeros((ncf + 1, C, C), np.int64),
               "confusion_SE": np.zeros((nse + 2, C, C), np.int64)}
    summed_wf, summed_lab = np.zeros((C + 1, 2 * T), np.float32), np.zeros((C, 2 * T), np.float32)
    n_wfs, n_lab = np.zeros(C + 1, np.int64), np.zeros(C, np.int64)
    for b, n_events in enumerate((37, 24)):
        events = []
        plan = [("craft", 0)] if b == 0 else []
        plan += [("neg", 3), ("big", 4), ("big", 12), ("rand", 11), ("rand", 12), ("rand", 2)]
        while len(events) < n_events:
            kind, n_rows = plan.pop(0) if plan else ("rand", int(rng.integers(2, 11)))
            if kind == "craft":
                c, p = crafted_at_high()
            else:
                c, p = candidate(n_rows, dict(neg=-0.3, big=rng.uniform(3.0, 6.0), rand=rng.uniform(0.02, 1.2))[kind])
            o = run_average_pulse(ns, c, p, gains, seg, 1)
            ok = clear(o["psdl"], edges["p"]) and clear(o["psdr"], edges["p"]) and clear(o["avg_coo"][:, 0], edges["x"]) \
                and clear(o["avg_coo"][:, 1], edges["y"])
            if kind == "craft":
                assert o["energy"][0] == P["emax"]
            else:
                ok = ok and clear(o["energy"], edges["e"]) and clear(o["energy"], edges["c"])
            if ok:
                events.append((c, p, kind == "craft"))
        coords = np.concatenate([np.column_stack([c[:, :2], np.full(len(c), e, np.int32)]) for e, (c, _p, _k) in
                                 enumerate(events)]).astype(np.int32)
        pulses = np.concatenate([p for _c, p, _k in events])
        exact = np.array([k for _c, _p, k in events])
        labels = rng.integers(0, 2, n_events).astype(np.int64)
        predictions = np.where(rng.random(n_events) < 0.7, labels, 1 - labels).astype(np.int64)
        o = run_average_pulse(ns, coords, pulses, gains, seg, n_events)
        # PSDEvaluator.add:141-198 on the reference's helpers
        res = raw["find_matches"](predictions, labels, np.zeros((n_events,)))
        energy, mult = o["energy"], o["multiplicity"]
        n_wfs[0] += np.sum(mult)
        summed_wf[0] += np.sum(o["summed"], axis=0)
        for i in range(C):
            li, pi = np.asarray(labels == i).nonzero(), np.asarray(predictions == i).nonzero()
            if len(li[0]) > 0:
                n_wfs[i + 1] += np.sum(mult[li])
                summed_wf[i + 1] += np.sum(o["summed"][li], axis=0)
            if len(pi[0]) > 0:
                n_lab[i] += np.sum(mult[pi])
                summed_lab[i] += np.sum(o["summed"][pi], axis=0)
        raw["metric_accumulate_1d"](res, mult, *results["mult_acc"], [0.5, nm + 0.5], nm)
        raw["confusion_accumulate_1d"](predictions, labels, energy, results["confusion_energy"], [0.0, P["emax"]], ncf)
        raw["confusion_accumulate_1d"](predictions, labels, o["n_SE"], results["confusion_SE"], [-0.5, nse + 0.5], nse + 1)
        for psd in (o["psdl"], o["psdr"]):
            raw["metric_accumulate_2d"](res, np.stack((energy, psd), axis=1), *results["ene_psd_acc"],
                                        [P["emin"], P["emax"]], [P["psd_min"], P["psd_max"]], nb, nb)
        raw["metric_accumulate_2d"](res, o["avg_coo"], *results["pos_acc"], [0.0, float(nx)], [0.0, float(ny)], nx, ny)
        tag = "tab%d_" % b
        out[tag + "coords"], out[tag + "pulses"], out[tag + "labels"] = coords, pulses, labels
        out[tag + "predictions"], out[tag + "exact_energy"] = predictions, exact
        for k in ("energy", "psdl", "psdr", "avg_coo", "multiplicity", "n_SE"):
            out[tag + k] = o[k]
    raw["finalize"](*results["mult_acc"])
    for k, v in results.items():
        if isinstance(v, tuple):
            for i, a in enumerate(v):
                out["tab_%s_%d" % (k, i)] = a
        else:
            out["tab_" + k] = v
    out["tab_summed_waveforms"], out["tab_summed_labelled_waveforms"] = summed_wf, summed_lab
    out["tab_n_wfs"], out["tab_n_labelled_wfs"] = n_wfs, n_lab
    # result keys and shapes after the reference's _init_results for these class names
    names = ["Gamma", "Neutron", "Other"]
    shapes = {"mult_acc": (nm + 2,), "ene_acc": (nb + 2,), "pos_acc": (nx + 2, ny + 2), "ene_psd_acc": (nb + 2, nb + 2),
              "confusion_energy": (ncf + 1, C, C), "confusion_SE": (nse + 2, C, C)}
    for n in names:
        shapes["ene_psd_prec_" + n], shapes["ene_prec_" + n], shapes["mult_prec_" + n] = (nb + 2, nb + 2), (nb + 2,), (nm + 2,)
    out["class_names"] = np.array(names)
    out["result_keys"] = np.array(sorted(shapes))
    out["result_shapes"] = np.array([list(shapes[k]) + [0] * (3 - len(shapes[k])) for k in sorted(shapes)])
    np.savez_compressed(os.path.join(HERE, "evaluator_cases.npz"), **out)
    print("wrote evaluator_cases.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "evaluator_cases.npz"))))


if __name__ == "__main__":
    main()
