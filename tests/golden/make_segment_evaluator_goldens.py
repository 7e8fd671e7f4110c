"""Generates tests/golden/segment_evaluator_cases.npz from the REFERENCE's own row walks (the reference tree, this container
only): inputs and the tables its functions give for them.  No reference text is written anywhere; the npz holds arrays only.

How the reference is run
  * numba is not installed here, so src/utils/SparseUtils.py cannot be imported.  z_deviation, z_deviation_with_E, z_error,
    E_deviation, get_bin_index, increment_metric_mult_SE, is_in_sample and sample_index are taken from the file's syntax
    tree IN MEMORY, their ``@nb.jit`` decorators dropped, and executed unmodified.
  * numba types ``float32 element (op) float literal`` as float64; plain Python on a float32 array would stay in float32.
    The dense maps are therefore handed over as float64 arrays holding the rounded fp32 / bf16 / fp16 VALUES, so the bin
    arithmetic runs in float64 on those values.  The tables the functions add into are the reference's own float32 / int32
    arrays (``_init_results`` / ``register_aggregator`` executed from the syntax tree on a stub object).
  * ZEvaluatorWF.add / EnergyEvaluatorWF.add / EZEvaluatorBase.add themselves are not executed (torch, spconv, plotting
    imports); their calls without a calibration group are repeated here argument for argument.  The energy map of
    z_deviation_with_E is the host-side product the reference forms, ``float32 map * E_scale`` in float32.
  * Constructor defaults are the literal assignments in ``ZEvaluatorBase.__init__`` / ``EnergyEvaluatorBase.__init__`` /
    ``AD1Evaluator.__init__``; seg_status is ``set_SE_segs`` executed on the ``SE_dead_pmts`` literal.

The plane order of the recorded maps is the one EZEvaluatorBase.add reads: plane 0 energy, plane 1 z.

Run:  python tests/golden/make_segment_evaluator_goldens.py
"""
import ast
import os
import sys
from math import floor

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import segment_evaluator_cases as sc  # noqa: E402

WANTED = ["z_deviation", "z_deviation_with_E", "z_error", "E_deviation", "get_bin_index", "increment_metric_mult_SE",
          "is_in_sample", "sample_index"]


def tree_of(*path):
    return ast.parse(open(os.path.join(REF, *path)).read())


def run_nodes(nodes, ns, label):
    mod = ast.Module(body=nodes, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "<reference %s, in memory>" % label, "exec"), ns)
    return ns


def reference_functions():
    keep = []
    for node in tree_of("src", "utils", "SparseUtils.py").body:
        if isinstance(node, ast.FunctionDef) and node.name in WANTED:
            node.decorator_list = []
            keep.append(node)
    assert sorted(n.name for n in keep) == sorted(WANTED)
    return run_nodes(keep, {}, "SparseUtils")


def class_of(tree, name):
    return [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name][0]


def method_of(cls, name):
    return [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name][0]


def literal_attributes(fn):
    """self.<name> = <literal> assignments of a method, first assignment wins."""
    out = {}
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Attribute):
            try:
                out.setdefault(node.targets[0].attr, ast.literal_eval(node.value))
            except ValueError:
                continue
    return out


class Stub:
    pass


def z_reference_setup():
    """(defaults, seg_status, sample_segs, fresh-results factory) of ZEvaluatorBase."""
    cls = class_of(tree_of("src", "evaluation", "ZEvaluator.py"), "ZEvaluatorBase")
    init = method_of(cls, "__init__")
    d = literal_attributes(init)
    dead = None
    for node in ast.walk(init):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "SE_dead_pmts":
            dead = ast.literal_eval(node.value)
    ns = run_nodes([method_of(cls, "set_SE_segs"), method_of(cls, "_init_results")], dict(np=np, floor=floor), "ZEvaluator")
    stub = Stub()
    for k in ("nmult", "nx", "ny", "n_bins", "n_err_bins"):
        setattr(stub, k, d[k])
    stub.seg_status = np.zeros((d["nx"], d["ny"]), dtype=np.float32)
    ns["set_SE_segs"](stub, dead)

    def fresh():
        ns["_init_results"](stub)
        return stub.results, stub.sample_segs
    return d, stub.seg_status, fresh


def energy_reference_setup():
    """(defaults, fresh-results factory) of EnergyEvaluatorBase on StatsAggregator's register_aggregator."""
    cls = class_of(tree_of("src", "evaluation", "EnergyEvaluator.py"), "EnergyEvaluatorBase")
    d = literal_attributes(method_of(cls, "__init__"))
    ad1 = literal_attributes(method_of(class_of(tree_of("src", "evaluation", "AD1Evaluator.py"), "AD1Evaluator"), "__init__"))
    consts = {}
    for node in tree_of("src", "evaluation", "AD1Evaluator.py").body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            try:
                consts[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    d["E_scale"], d["z_scale"] = consts["E_NORMALIZATION_FACTOR"], consts["Z_NORMALIZATION_FACTOR"]
    d["nx"], d["ny"] = ad1["nx"], ad1["ny"]
    agg = class_of(tree_of("src", "utils", "StatsUtils.py"), "StatsAggregator")
    methods = [method_of(agg, n) for n in ("get_metadata", "set_tuple_metadata", "get_tuple_metadata", "set_bin_edges",
                                           "register_duplicates", "register_aggregator")]
    methods.append(method_of(cls, "initialize"))
    from typing import List, Tuple, Union
    ns = run_nodes(methods, dict(np=np, Union=Union, Tuple=Tuple, List=List,
                                 get_bins=lambda lo, hi, n: np.linspace(lo, hi, n + 1)), "StatsAggregator")
    bound = type("Bound", (Stub,), {m.name: ns[m.name] for m in methods})

    def fresh():
        o = bound()
        o.metric_metadata, o.results = {}, {}
        for k in ("E_bounds", "mult_bounds", "n_mult", "n_E", "n_z", "z_bounds", "E_mult_names", "E_z_names",
                  "seg_mult_names", "nx", "ny"):
            setattr(o, k, d[k])
        o.initialize()
        return o.results
    return d, fresh


def rounded(values, dtype):
    import torch
    t = torch.from_numpy(np.asarray(values, np.float64)).to(dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[dtype])
    return t.float().numpy()


def clear_of(v, edges):
    return np.abs(np.asarray(v, np.float64)[..., None] - edges).min(axis=-1) > 1e-4


def build_batch(rng, counts, forced, dtype, zd, ed, crafted):
    """One batch.  counts: rows per event; forced: {event: [cells]} put first in the event; crafted: list of
    (event, k-th row of the event, dict(tz=, pz=, te=)) overriding drawn values with exact dyadic ones.
    Returns coords [N, 3], pred, targ [B, 2, nx, ny] float32 (plane 0 energy, plane 1 z), exact mask [N]."""
    nx, ny = zd["nx"], zd["ny"]
    z_edges = np.arange(zd["n_bins"] + 1) * (zd["z_scale"] / zd["n_bins"]) - zd["z_scale"] / 2.
    err_edges = np.arange(zd["n_err_bins"] + 1) * ((zd["error_high"] - zd["error_low"]) / zd["n_err_bins"]) + zd["error_low"]
    E_edges = np.arange(ed["n_E"] + 1) * ((ed["E_bounds"][1] - ed["E_bounds"][0]) / ed["n_E"]) + ed["E_bounds"][0]
    rows = []
    for e, n in enumerate(counts):
        first = list(forced.get(e, []))[:n]
        rest = [c for c in rng.permutation(nx * ny) if (c // ny, c % ny) not in first][:n - len(first)]
        rows += [(x, y, e) for x, y in first] + [(c // ny, c % ny, e) for c in rest]
    coords = np.array(rows, np.int32).reshape(-1, 3)
    N, B = len(coords), len(counts)
    start = np.concatenate([[0], np.cumsum(counts)])
    fixed = {}
    for e, k, vals in crafted:
        assert k < counts[e]
        fixed[start[e] + k] = vals
    tz, pz, te, pe = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
    for r in range(N):
        f = fixed.get(r, {})
        while True:
            t = f["tz"] if "tz" in f else rng.uniform(0.02, 0.98)
            p = f["pz"] if "pz" in f else t + rng.normal(0, 0.12)
            t, p = rounded([t], dtype)[0], rounded([p], dtype)[0]
            ok_t = "tz" in f or clear_of([(np.float64(t) - 0.5) * zd["z_scale"]], z_edges)[0]
            ok_p = ("tz" in f and "pz" in f) or clear_of([(np.float64(p) - np.float64(t)) * zd["z_scale"]], err_edges)[0]
            if ok_t and ok_p:
                break
            assert not ("tz" in f and "pz" in f)
        tz[r], pz[r] = t, p
        while True:
            t = f["te"] if "te" in f else rng.uniform(0.02, 0.9)
            t = rounded([t], dtype)[0]
            # both products that get binned: float64 t * E_scale (E_deviation) and the float32 one (z_deviation_with_E)
            prods = [np.float64(t) * ed["E_scale"], np.float64(np.float32(t) * np.float32(ed["E_scale"]))]
            if "te" in f or clear_of(prods, E_edges).all():
                break
        te[r] = t
        pe[r] = rounded([np.float64(t) * (1 + rng.normal(0, 0.2))], dtype)[0]
        assert te[r] > 0
    pred, targ = np.zeros((B, 2, nx, ny), np.float32), np.zeros((B, 2, nx, ny), np.float32)
    x, y, e = coords[:, 0], coords[:, 1], coords[:, 2]
    pred[e, 0, x, y], targ[e, 0, x, y], pred[e, 1, x, y], targ[e, 1, x, y] = pe, te, pz, tz
    return coords, pred, targ


def main():
    fn = reference_functions()
    zd, seg, z_fresh = z_reference_setup()
    ed, e_fresh = energy_reference_setup()
    _res, sample_segs = z_fresh()
    out = {"seg_status": seg, "sample_segs": np.asarray(sample_segs)}
    for k in ("nmult", "n_bins", "n_err_bins", "error_low", "error_high", "z_scale", "E_low", "E_high", "true_E_high",
              "E_scale", "nx", "ny"):
        out["z_default_" + k] = np.float64(zd[k])
    for k in ("n_mult", "n_E", "n_z", "E_scale"):
        out["e_default_" + k] = np.float64(ed[k])
    out["e_default_E_bounds"] = np.asarray(ed["E_bounds"], np.float64)
    # result keys, shapes, dtypes of fresh reference objects
    for tag, res in (("z", z_fresh()[0]), ("e", e_fresh())):
        keys = sorted(res)
        first = [res[k][0] if isinstance(res[k], tuple) else res[k] for k in keys]
        out[tag + "_result_keys"] = np.array(keys)
        out[tag + "_result_is_pair"] = np.array([isinstance(res[k], tuple) for k in keys])
        out[tag + "_result_shapes"] = np.array([list(a.shape) + [0] * (3 - a.ndim) for a in first])
        out[tag + "_result_dtypes"] = np.array([str(a.dtype) for a in first])
        for k in keys:
            if isinstance(res[k], tuple):
                assert res[k][0].dtype == np.float32 and res[k][1].dtype == np.int32 and res[k][0].shape == res[k][1].shape

    S = [tuple(int(v) for v in s) for s in sample_segs]
    single = tuple(int(v) for v in np.argwhere(seg == 0.5)[3])
    dead = tuple(int(v) for v in np.argwhere(seg == 1.0)[0])
    dual = [tuple(int(v) for v in c) for c in np.argwhere(seg == 0.0) if tuple(c) not in S][:2]
    assert seg[S[0]] == 0 or seg[S[0]] > 0                                  # whatever they are, they are recorded
    # batch 0: an empty event at id 0 and one in the middle; runs of 1, 2, 6, 7, 10, 11, 12; a last event with rows
    counts0 = [0, 1, 2, 6, 0, 7, 10, 11, 12, 3]
    forced0 = {1: [S[0]], 2: [S[1], S[2]], 3: [S[0], S[1], dead], 5: [S[2], S[0], single], 6: [S[1], dual[0]],
               7: [S[0], S[2], single, dead], 8: [S[1], S[0], S[2], dual[1]], 9: [S[2], dead, single]}
    crafted0 = [(1, 0, dict(tz=0.5, pz=1.0, te=0.75)),                       # on edges: z 0, error +600, energy at E_high
                (2, 0, dict(tz=0.75, pz=0.25)), (2, 1, dict(tz=1.0, pz=0.5)),  # z 300 and zrange / 2; error -600
                (3, 0, dict(tz=0.0, pz=0.5)), (3, 1, dict(tz=0.125, pz=1.0)),  # z = -zrange / 2; error 1050 > error_high
                (5, 0, dict(tz=0.875, pz=0.0)),                               # error -1050 < error_low
                (5, 1, dict(tz=-0.125, pz=0.0)), (6, 0, dict(tz=1.25, pz=1.0)),  # target below 0 and above 1
                (7, 2, dict(tz=0.5, pz=0.0, te=0.75)), (8, 3, dict(tz=1.0, pz=1.5)), (9, 1, dict(tz=0.75, pz=1.25))]
    counts1 = [1, 7, 2, 6, 12, 0, 11, 5]
    forced1 = {0: [S[1]], 1: [S[1], single], 2: [S[0], dead], 3: [S[2], dual[0]], 4: [S[0], S[1], S[2], single],
               6: [S[2], S[1], dead], 7: [S[0], dual[1]]}
    crafted1 = [(0, 0, dict(tz=0.25, pz=0.75)), (1, 0, dict(tz=0.5, pz=0.0, te=0.75)), (4, 0, dict(tz=0.0, pz=-0.5)),
                (6, 1, dict(tz=1.0, pz=0.125)), (7, 0, dict(tz=0.75, pz=-0.125))]
    rng = np.random.default_rng(20240907)
    worst = 0.0
    for dtype in sc.DTYPES:
        zres, _ = z_fresh()
        zres = {k: v for k, v in zres.items()}
        zEres, _ = z_fresh()
        eres = e_fresh()
        host_z = sc.HostZTables(seg, sample_segs=sample_segs)
        host_zE = sc.HostZTables(seg, use_energy=True, sample_segs=sample_segs)
        host_e = sc.HostEnergyTables(seg)
        for b, (counts, forced, crafted) in enumerate(((counts0, forced0, crafted0), (counts1, forced1, crafted1))):
            coords, pred, targ = build_batch(rng, counts, forced, dtype, zd, ed, crafted)
            assert len(coords) <= 300 and np.all(np.diff(coords[:, 2]) >= 0)
            tag = "%s_b%d_" % (dtype, b)
            out[tag + "coords"], out[tag + "pred"], out[tag + "targ"] = coords, pred, targ
            p64, t64 = pred.astype(np.float64), targ.astype(np.float64)
            nx, ny = zd["nx"], zd["ny"]
            # ZEvaluatorWF.add, no calibration group (E only calls set_true_E): z_deviation + z_error on the z plane
            fn["z_deviation"](coords, p64[:, 1], t64[:, 1], zres["seg_mult_mae"][0], zres["seg_mult_mae"][1],
                              zres["z_mult_mae_dual"][0], zres["z_mult_mae_dual"][1], zres["z_mult_mae_single"][0],
                              zres["z_mult_mae_single"][1], seg, nx, ny, zd["nmult"], zd["n_bins"], zd["z_scale"])
            fn["z_error"](coords, p64[:, 1], t64[:, 1], zres["seg_sample_error"], zd["n_err_bins"], zd["error_low"],
                          zd["error_high"], zd["nmult"], sample_segs, zd["z_scale"])
            # use_energy: z_deviation_with_E with E = float32 energy targets * E_scale, E_high = true_E_high
            E = (targ[:, 0] * np.float32(zd["E_scale"])).astype(np.float64)
            fn["z_deviation_with_E"](coords, p64[:, 1], t64[:, 1], zEres["seg_mult_mae"][0], zEres["seg_mult_mae"][1],
                                     zEres["z_mult_mae_dual"][0], zEres["z_mult_mae_dual"][1],
                                     zEres["z_mult_mae_single"][0], zEres["z_mult_mae_single"][1], seg, nx, ny,
                                     zd["nmult"], zd["n_bins"], zd["z_scale"], E, zEres["E_mult_mae_dual"][0],
                                     zEres["E_mult_mae_dual"][1], zEres["E_mult_mae_single"][0],
                                     zEres["E_mult_mae_single"][1], zd["E_low"], zd["true_E_high"])
            fn["z_error"](coords, p64[:, 1], t64[:, 1], zEres["seg_sample_error"], zd["n_err_bins"], zd["error_low"],
                          zd["error_high"], zd["nmult"], sample_segs, zd["z_scale"])
            # EnergyEvaluatorWF.add, no calibration group: E_deviation on the energy plane
            fn["E_deviation"](coords, p64[:, 0], t64[:, 0], eres["seg_mult_Emape"][0], eres["seg_mult_Emape"][1],
                              eres["E_mult_dual"][0], eres["E_mult_dual"][1], eres["E_mult_single"][0],
                              eres["E_mult_single"][1], seg, nx, ny, ed["n_mult"], ed["n_E"], ed["E_bounds"][0],
                              ed["E_bounds"][1], ed["E_scale"])
            host_z.add(coords, pred[:, 1], targ[:, 1], E=targ[:, 0])
            host_zE.add(coords, pred[:, 1], targ[:, 1], E=targ[:, 0])
            host_e.add(coords, pred[:, 0], targ[:, 0])
            acc = "%s_after%d_" % (dtype, b + 1)
            for kind, res, keys in (("z_", zres, sc.Z_PAIRS), ("zE_", zEres, sc.Z_PAIRS), ("e_", eres, sc.E_PAIRS)):
                for k in keys:
                    out[acc + kind + k + "_sum"], out[acc + kind + k + "_n"] = res[k][0].copy(), res[k][1].copy()
            out[acc + "z_seg_sample_error"] = zres["seg_sample_error"].copy()
            out[acc + "zE_seg_sample_error"] = zEres["seg_sample_error"].copy()
            # the condition under which the GPU can be held to these tables: the float64 restatement agrees
            hist = ("seg_sample_error",)
            worst = max(worst, sc.assert_tables_match(host_z.results(), out, acc + "z_", sc.Z_PAIRS + hist, "generator"),
                        sc.assert_tables_match(host_zE.results(), out, acc + "zE_", sc.Z_PAIRS + hist, "generator"),
                        sc.assert_tables_match(host_e.results(), out, acc + "e_", sc.E_PAIRS, "generator"))
        # what the cases reach
        n = out[acc + "z_seg_mult_mae_n"]
        assert n[:, :, zd["nmult"]].sum() > 0 and all(n[:, :, m].sum() > 0 for m in (0, 1, 5))
        ne = out[acc + "e_seg_mult_Emape_n"]
        assert ne[:, :, ed["n_mult"]].sum() > 0 and ne[:, :, 9].sum() > 0 and ne[:, :, 6].sum() > 0
        h = out[acc + "z_seg_sample_error"]
        assert h[:, :, 0].sum() > 0 and h[:, :, -1].sum() > 0 and all((h[s].sum(axis=1) > 0).sum() >= 3 for s in range(3))
        for k in ("z_mult_mae_single", "z_mult_mae_dual"):
            assert out[acc + "z_" + k + "_n"].sum() > 0
        zs = out[acc + "z_z_mult_mae_single_n"] + out[acc + "z_z_mult_mae_dual_n"]
        assert zs[0].sum() > 0 and zs[-1].sum() > 0                          # targets below 0 and from 1
        assert out[acc + "z_E_mult_mae_single_n"].sum() == 0 and out[acc + "zE_E_mult_mae_dual_n"].sum() > 0
        assert (out[acc + "e_E_mult_single_n"] + out[acc + "e_E_mult_dual_n"])[-1].sum() >= 3   # at and above E_high
    path = os.path.join(HERE, "segment_evaluator_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote segment_evaluator_cases.npz: %d arrays, %d bytes; restatement vs reference, worst float error %.3g of scale"
          % (len(out), os.path.getsize(path), worst))


if __name__ == "__main__":
    main()
