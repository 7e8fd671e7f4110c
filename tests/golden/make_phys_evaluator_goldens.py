"""Generates tests/golden/phys_evaluator_cases.npz from the REFERENCE's own arithmetic (the reference tree, this container
only): inputs and the outputs its functions give for them.  No reference text is written anywhere; the npz holds arrays
only.

How the reference is run
  * numba is not installed here, so src/utils/SparseUtils.py cannot be imported.  Its functions are taken from the file's
    syntax tree IN MEMORY, their ``@nb.jit`` decorators dropped, and executed: weighted_average_quantities, find_matches,
    get_bin_index, hist_add_1d, metric_accumulate_1d, metric_accumulate_2d, confusion_accumulate_1d, finalize.
  * numba types ``ene_current`` (``0.0`` unified with ``+= float32``) as float64.  Under this NumPy (2.x) a Python float
    plus a float32 scalar stays float32, so plain Python would accumulate the energy, and with it the coordinate sums, in
    float32.  To record what the reference computes under numba, the two ``ene_current = 0.0`` initialisers of
    weighted_average_quantities are turned into ``float64(0.0)`` in the in-memory tree (nothing else of it is touched):
    float64 + float32 is float64 from then on, ``int32[:] * float64`` is float64, ``float32 /= float64`` is computed in
    float64 and stored as float32 -- all as numba does.  ``hand_event()`` shows it on one event computed by hand.
  * For the same reason the binning helpers get float64 COPIES of float32 values (the same values): numba compares a
    float32 with a float64 edge in float64, this NumPy would compare in float32.
  * PhysEvaluator.add itself is not executed (TensorBoard, plotting); its derived columns (:328-338) are formed with the
    same NumPy expressions and its accumulation calls (:349-397) are repeated here, argument for argument, on the
    reference's helpers.  Where add() passes a three-array result tuple to metric_accumulate_2d (which takes two arrays)
    the first two are passed.  ``list_matches`` is util.py:515's one expression.
  * The spectra are this project's addition: ``hist_add_1d`` over the events of every TRUE class and over the events
    PREDICTED as every class, for the eight entries of ``feature_list``, over AD1Evaluator.default_bins' ranges.

A case is REFUSED (the run fails) when a binned value lies within 1e-4 of an edge it is not exactly on, or when an arrival
at a range's ``high`` is not bit-equal to it.

Run:  python tests/golden/make_phys_evaluator_goldens.py
"""
import ast
import math
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

WANTED = ["weighted_average_quantities", "find_matches", "get_bin_index", "hist_add_1d", "metric_accumulate_1d",
          "metric_accumulate_2d", "confusion_accumulate_1d", "finalize"]
NAMES = ["Gamma", "Neutron", "Other", "Never"]            # no event is labelled or predicted "Never"
# AD1Evaluator.default_bins (E, dt, PE0, PE1, z, PSD, t offset) in feature_list's order, then np.arange(0, 21)'s centres
SPECTRUM_BINS = [(0.0, 12.0, 100), (0.0, 0.6, 100), (-15.0, 15.0, 100), (0.0, 5000.0, 100), (0.0, 5000.0, 100),
                 (-600.0, 600.0, 100), (0.0, 30.0, 100), (-0.5, 20.5, 21)]


def reference_functions():
    tree = ast.parse(open(os.path.join(REF, "src", "utils", "SparseUtils.py")).read())
    keep = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in WANTED:
            node.decorator_list = []
            if node.name == "weighted_average_quantities":
                n_init = 0
                for sub in ast.walk(node):
                    if isinstance(sub, ast.Assign) and getattr(sub.targets[0], "id", None) == "ene_current" and \
                            isinstance(sub.value, ast.Constant) and sub.value.value == 0.0:
                        sub.value = ast.Call(func=ast.Name(id="float64", ctx=ast.Load()), args=[sub.value], keywords=[])
                        n_init += 1
                assert n_init == 2
            keep.append(node)
    assert sorted(n.name for n in keep) == sorted(WANTED)
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = dict(sqrt=math.sqrt, zeros=np.zeros, float64=np.float64)
    exec(compile(mod, "<reference SparseUtils, in memory>", "exec"), ns)
    return ns


def reference_defaults():
    """PSDEvaluator.__init__'s literals, then PhysEvaluator.__init__'s on top."""
    tree = ast.parse(open(os.path.join(REF, "src", "evaluation", "PSDEvaluator.py")).read())
    out = {}
    for cls_name in ("PSDEvaluator", "PhysEvaluator"):
        cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name][0]
        init = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
        for node in ast.walk(init):
            if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Attribute):
                try:
                    v = ast.literal_eval(node.value)
                except ValueError:
                    continue
                if isinstance(v, (int, float)) and not isinstance(v, bool):
                    out[node.targets[0].attr] = float(v)
    return out


def rounded(rows, dtype):
    """The values a tensor of `dtype` holds for `rows`, as float32: what the reference sees after .cpu().numpy()."""
    import torch
    t = torch.from_numpy(np.asarray(rows, np.float32)).to(dict(f32=torch.float32, bf16=torch.bfloat16,
                                                               f16=torch.float16)[dtype])
    return t.float().numpy()


def derived(f):
    """PhysEvaluator.add:328-338."""
    energy = f[:, 0] * 12.
    dt = (f[:, 1] - 0.5) * 30.
    PEL = f[:, 2] * 5000.
    PER = f[:, 3] * 5000.
    z = (f[:, 4] - 0.5) * 1200.
    psd = f[:, 5]
    t0 = f[:, 6] * 30.0
    full = np.stack((energy, psd, dt, PEL, PER, z, t0), axis=0)
    assert full.dtype == np.float32
    return full


def run_events(ns, c, f, E):
    """PhysEvaluator.add:338-346 -> avg_coo [E, 2] float64, feature_list [8, E] (float64 after the stack with mult; the
    first seven rows hold float32 values), mult [E] float64."""
    full = derived(f)
    feature_list = np.zeros((full.shape[0], E), dtype=np.float32)
    avg_coo, feature_list, mult = ns["weighted_average_quantities"](c, full, feature_list, np.zeros((E, 2)),
                                                                    np.zeros((E,)), full.shape[0])
    assert feature_list.dtype == np.float32 and avg_coo.dtype == np.float64
    return avg_coo, feature_list, mult


def hand_event(ns):
    """Two rows whose energies are 3 * 2^24 and 3: in float32 their sum rounds to 50331652, in float64 it is 50331651.
    With x = 1 and 2 the reference's coordinate sum (each row weighed by the RUNNING energy) is
    1 * 50331648 + 2 * 50331651 = 150994950, so x = 150994950 / 50331651 under numba, but
    (50331648 + 2 * 50331652) / 50331652 had the energy been summed in float32."""
    c = np.array([(1, 4, 0), (2, 6, 0)], np.int32)
    f = np.zeros((2, 7), np.float32)
    f[0, 0], f[1, 0] = 4194304.0, 0.25
    f[:, 5] = (0.25, 0.5)                                   # psd: (0.25 * 50331648 + 0.5 * 3) / 50331651 in float32 sums
    avg, feat, mult = run_events(ns, c, f, 1)
    assert float(np.float32(50331648.0) + np.float32(3.0)) == 50331652.0          # what float32 would have given
    assert avg[0, 0] == 150994950.0 / 50331651.0 and avg[0, 0] != (50331648.0 + 2 * 50331652.0) / 50331652.0
    assert avg[0, 1] == (4 * 50331648.0 + 6 * 50331651.0) / 50331651.0
    psd32 = np.float32(np.float32(0.25) * np.float32(50331648.0)) + np.float32(np.float32(0.5) * np.float32(3.0))
    assert feat[1, 0] == np.float32(np.float64(psd32) / 50331651.0)
    assert feat[0, 0] == np.float32(50331651.0) and mult[0] == 2
    return c, f, avg, feat, mult


def make_event(rng, n_rows, e_scale=1.0):
    cells = rng.choice(14 * 11, size=n_rows, replace=False)
    c = np.array([(k // 11, k % 11, 0) for k in cells], np.int32)
    f = np.empty((n_rows, 7), np.float32)
    f[:, 0] = rng.uniform(0.004, 0.08, n_rows) * e_scale
    f[:, 1] = rng.uniform(0.1, 0.9, n_rows)
    f[:, 2:4] = rng.uniform(0.01, 0.9, (n_rows, 2))
    f[:, 4] = rng.uniform(0.05, 0.95, n_rows)
    f[:, 5] = rng.uniform(0.05, 0.5, n_rows)
    f[:, 6] = rng.uniform(0.02, 0.95, n_rows)
    return c, f


def batch_from(events):
    coords = np.concatenate([np.column_stack([c[:, :2], np.full(len(c), e, np.int32)]) for e, (c, _f) in
                             enumerate(events)]).astype(np.int32)
    return coords, np.concatenate([f for _c, f in events]).astype(np.float32)


def edges(lo, hi, nb):
    return np.arange(nb + 1) * ((hi - lo) / nb) + lo


def require_clear(values, lo, hi, nb, what):
    """No value within 1e-4 (absolute; times the bin width where that is above 1) of an edge it is not exactly on.  The
    edges are the reference's own j * width + low, so "on" means bit-equal -- an arrival at `high` included."""
    v = np.asarray(values, np.float64)
    tol = 1e-4 * max(1.0, (hi - lo) / nb)
    d = np.abs(v[:, None] - edges(lo, hi, nb)[None, :]).min(axis=1)
    bad = (d <= tol) & (d > 0)
    if bad.any():
        raise SystemExit("refused: %s has %s within %g of an edge of [%g, %g] / %d" % (what, v[bad], tol, lo, hi, nb))


def is_clear(values, lo, hi, nb):
    v = np.asarray(values, np.float64)
    tol = 1e-4 * max(1.0, (hi - lo) / nb)
    d = np.abs(v[:, None] - edges(lo, hi, nb)[None, :]).min(axis=1)
    return bool(np.all((d > tol) | (d == 0)))


def main():
    ns = reference_functions()
    d = reference_defaults()
    assert d["emax"] == 10.0                                                   # PhysEvaluator's own
    out = {}
    for k in ["n_bins", "n_mult", "emin", "emax", "psd_min", "psd_max", "nx", "ny", "n_confusion", "n_SE_max"]:
        out["default_" + k] = np.float64(d[k])
    out["spectrum_bins"] = np.array(SPECTRUM_BINS, np.float64)
    rng = np.random.default_rng(20241019)

    c, f, avg, feat, mult = hand_event(ns)
    out["hand_coords"], out["hand_feats"], out["hand_avg_coo"], out["hand_features"] = c, f, avg, feat
    out["hand_multiplicity"] = mult

    # ---- per-event outputs: events of 1, 2, 17, 65 rows, total energy 0, negative total, and a last event without rows
    counts = [1, 2, 17, 65, 3, 2]
    for dtype in ("f32", "bf16", "f16"):
        events = [make_event(rng, n) for n in counts]
        events[4][1][:, 0] = (0.05, -0.05, 0.0)                                # sums to exactly 0 in any format
        events[5][1][:, 0] = (0.01, -0.04)                                     # negative total
        c, f = batch_from(events)
        f = rounded(f, dtype)
        E = len(counts) + 1
        avg, feat, mult = run_events(ns, c, f, E)
        assert mult.tolist() == [1, 2, 17, 65, 0, 0, 0] and feat[0, 4] == 0 and feat[0, 5] == 0
        assert np.any(feat[1:, 4] != 0) and np.any(avg[5] != 0) and not avg[6].any() and not feat[:, 6].any()
        tag = "stats_%s_" % dtype
        out[tag + "coords"], out[tag + "feats"] = c, f
        out[tag + "avg_coo"], out[tag + "features"], out[tag + "multiplicity"] = avg, feat, mult

    # ---- tables: two batches, four class names (the last never occurs), twice: the defaults, and emin = 0.5 / n_mult = 6
    C = len(NAMES)
    variants = {"tab": dict(d), "tabk": dict(d, emin=0.5, n_mult=6.0)}

    def bin_ranges(P):
        return dict(e=(P["emin"], P["emax"], int(P["n_bins"])), c=(0.0, P["emax"], int(P["n_confusion"])),
                    p=(P["psd_min"], P["psd_max"], int(P["n_bins"])), x=(0.0, float(P["nx"]), int(P["nx"])),
                    y=(0.0, float(P["ny"]), int(P["ny"])))

    def event_is_clear(avg, feat, mult):
        ok = True
        for P in variants.values():
            r = bin_ranges(P)
            ok = ok and is_clear(feat[0], *r["e"]) and is_clear(feat[0], *r["c"]) and is_clear(feat[1], *r["p"]) \
                and is_clear(avg[:, 0], *r["x"]) and is_clear(avg[:, 1], *r["y"])
        for k, b in enumerate(SPECTRUM_BINS):
            ok = ok and is_clear(mult if k == 7 else feat[k], *b)
        return ok

    def crafted_at_high():
        # one row whose float32 energy is emax = 10 exactly: fl(fl(5 / 6) * 12) == 10
        c = np.array([(3, 4, 0)], np.int32)
        f = np.array([[np.float32(5.0 / 6.0), 0.513, 0.251, 0.257, 0.523, 0.301, 0.413]], np.float32)
        return c, f

    batches = []
    for b, n_events in enumerate((37, 24)):
        plan = [("craft", 1, 1.0)] if b == 0 else [("low", 1, 0.3)]
        plan += [("zero", 2, 1.0), ("neg", 2, 1.0), ("big", 4, 8.0), ("mult", 17, 0.4), ("mult", 65, 0.1), ("mult", 12, 0.5),
                 ("low", 1, 0.2)]
        events = []
        while len(events) < n_events - 1:                                      # the last event has no rows
            # a planned kind stays first in line until an event of it clears every edge
            kind, n_rows, scale = plan[0] if plan else ("rand", int(rng.integers(1, 11)), float(rng.uniform(0.3, 3)))
            if kind == "craft":
                c, f = crafted_at_high()
            else:
                c, f = make_event(rng, n_rows, scale)
                if kind == "zero":
                    f[:, 0] = (0.05, -0.05)
                if kind == "neg":
                    f[:, 0] = (0.01, -0.04)
            avg, feat, mult = run_events(ns, c, f, 1)
            if kind == "craft":
                assert feat[0, 0] == np.float32(10.0) and feat[0, 0] == d["emax"]
            if event_is_clear(avg, feat, mult):
                events.append((c, f))
                if plan:
                    plan.pop(0)
            else:
                assert kind != "craft"
        c, f = batch_from(events)
        labels = rng.integers(0, 3, n_events).astype(np.int64)
        wrong = (labels + rng.integers(1, 3, n_events)) % 3
        predictions = np.where(rng.random(n_events) < 0.7, labels, wrong).astype(np.int64)
        batches.append((c, f, labels, predictions))
        tag = "tab%d_" % b
        out[tag + "coords"], out[tag + "feats"], out[tag + "labels"], out[tag + "predictions"] = c, f, labels, predictions

    for vname, P in variants.items():
        nb, nm, ncf, nx, ny = (int(P[k]) for k in ["n_bins", "n_mult", "n_confusion", "nx", "ny"])
        r = bin_ranges(P)

        def triple(*shape):
            return np.zeros(shape), np.zeros(shape, np.int64), np.zeros(shape)

        results = {"mult_acc": triple(nm + 2), "ene_acc": triple(nb + 2), "pos_acc": triple(nx + 2, ny + 2),
                   "ene_psd_acc": triple(nb + 2, nb + 2), "confusion_energy": np.zeros((ncf + 1, C, C), np.int64),
                   "confusion_SE": np.zeros((int(P["n_SE_max"]) + 2, C, C), np.int64)}
        for n in NAMES:
            results["ene_psd_prec_" + n], results["ene_prec_" + n] = triple(nb + 2, nb + 2), triple(nb + 2)
            results["mult_prec_" + n] = triple(nm + 2)
        spectra = np.zeros((2, C, 8, 102), np.int64)                           # [truth | prediction]; rows padded to 102
        for b, (c, f, labels, predictions) in enumerate(batches):
            E = len(labels)
            avg_coo, fl, mult = run_events(ns, c, f, E)
            assert mult[-1] == 0 and not fl[:, -1].any()
            # the refusal rule, on the whole batch as recorded
            require_clear(fl[0], *r["e"], "energy")
            require_clear(fl[0], *r["c"], "energy (confusion)")
            require_clear(fl[1], *r["p"], "psd")
            require_clear(avg_coo[:, 0], *r["x"], "x")
            require_clear(avg_coo[:, 1], *r["y"], "y")
            feature_list = np.stack((fl[0], fl[1], fl[2], fl[3], fl[4], fl[5], fl[6], mult), axis=0)   # :345, float64
            for k, bins in enumerate(SPECTRUM_BINS):
                require_clear(feature_list[k], *bins, "feature %d" % k)
            if vname == "tab":
                tag = "tab%d_" % b
                out[tag + "avg_coo"], out[tag + "features"], out[tag + "multiplicity"] = avg_coo, fl, mult
            match = ns["find_matches"](predictions, labels, np.zeros((E,)))
            ene64, psd64 = fl[0].astype(np.float64), fl[1].astype(np.float64)  # the same values (see the docstring)
            for i in range(C):
                li = np.asarray(labels == i).nonzero()
                pi = np.asarray(predictions == i).nonzero()
                for k, (lo, hi, nbk) in enumerate(SPECTRUM_BINS):
                    ns["hist_add_1d"](feature_list[k][li], spectra[0, i, k, :nbk + 2], [lo, hi], nbk)
                    ns["hist_add_1d"](feature_list[k][pi], spectra[1, i, k, :nbk + 2], [lo, hi], nbk)
                ns["metric_accumulate_2d"](match[li], np.stack((ene64[li], psd64[li]), axis=1),
                                           *results["ene_psd_prec_" + NAMES[i]][:2], [P["emin"], P["emax"]],
                                           [P["psd_min"], P["psd_max"]], nb, nb)
                ns["metric_accumulate_1d"](match[li], ene64[li], *results["ene_prec_" + NAMES[i]],
                                           [P["emin"], P["emax"]], nb)
                ns["metric_accumulate_1d"](match[li], mult[li], *results["mult_prec_" + NAMES[i]], [0.5, nm + 0.5], nm)
            ns["confusion_accumulate_1d"](predictions, labels, ene64, results["confusion_energy"], [0.0, P["emax"]], ncf)
            ns["metric_accumulate_1d"](match, mult, *results["mult_acc"], [0.5, nm + 0.5], nm)
            ns["metric_accumulate_2d"](match, np.stack((ene64, psd64), axis=1), *results["ene_psd_acc"][:2],
                                       [P["emin"], P["emax"]], [P["psd_min"], P["psd_max"]], nb, nb)
            ns["metric_accumulate_2d"](match, avg_coo, *results["pos_acc"][:2], [0.0, float(nx)], [0.0, float(ny)], nx, ny)
        # PSDEvaluator.finalize
        ns["finalize"](*results["ene_acc"])
        ns["finalize"](*results["mult_acc"])
        for n in NAMES:
            ns["finalize"](*results["ene_prec_" + n])
            ns["finalize"](*results["mult_prec_" + n])
        for k, v in results.items():
            for i, a in enumerate(v if isinstance(v, tuple) else (v,)):
                out["%s_%s_%d" % (vname, k, i)] = a
        out[vname + "_spectra"] = spectra
        out[vname + "_params"] = np.array([P["emin"], P["n_mult"]])
    # what the tables cover
    en = np.concatenate([out["tab0_features"][0], out["tab1_features"][0]])
    mu = np.concatenate([out["tab0_multiplicity"], out["tab1_multiplicity"]])
    assert (en == 10.0).any() and (en > 10.0).any() and ((en > 0) & (en < 0.5)).any() and (mu > 10).any()
    assert (mu == 0).sum() >= 6
    out["class_names"] = np.array(NAMES)
    out["result_keys"] = np.array(sorted(results))
    path = os.path.join(HERE, "phys_evaluator_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote phys_evaluator_cases.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
