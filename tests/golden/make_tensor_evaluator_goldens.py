"""Generates tests/golden/tensor_evaluator_cases.npz from the REFERENCE's own evaluation arithmetic (the reference tree,
this container only): inputs and the tables its functions give for them.  No reference text is written anywhere; the npz
holds arrays only.  The layout of the file is described in tests/tensor_evaluator_cases.py.

How the reference is run (the method of make_pid_evaluator_goldens.py, whose helpers are imported)
  * get_bin_index, metric_accumulate_1d, metric_accumulate_2d, finalize2d (src/utils/SparseUtils.py) and get_bins
    (src/utils/util.py) are taken from the syntax tree IN MEMORY, their ``@nb.jit`` decorators dropped, and executed
    unmodified on float64 arrays that hold the fp32 (or bf16 / f16 rounded) values.
  * The constants of AD1Evaluator.__init__ (normalisation factors, scales, ``phys_names``, ``default_bins``) are read from
    its tree, ``scale_factor`` and ``override_default_bins`` are executed from it.
  * TensorEvaluator.__init__ / _init_results / add, MetricAggregator.add_normalized, MetricPairAggregator.add_normalized
    and StatsAggregator.increment_metric (float32 sums and int32 counts, fed the float32 results) are repeated here call
    for call.
  * A case with ``n_valid`` is the reference run on the valid rows alone.
  * The "pairs" cases drive MetricPairAggregator.add with explicit categories (the dispatch edge of the kernel).

Run:  python tests/golden/make_tensor_evaluator_goldens.py
"""
import ast
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_pid_evaluator_goldens as mpg  # noqa: E402

NX, NY = 14, 11


def reference():
    raw = mpg._functions(mpg._tree("src", "utils", "SparseUtils.py"),
                         ["get_bin_index", "metric_accumulate_1d", "metric_accumulate_2d", "finalize2d"], dict(sqrt=math.sqrt))
    raw.update(mpg._functions(mpg._tree("src", "utils", "util.py"), ["get_bins"], dict(np=np)))
    ad1 = mpg._tree("src", "evaluation", "AD1Evaluator.py")
    consts = {}
    for node in ad1.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            try:
                consts[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    init = mpg._method(ad1, "AD1Evaluator", "__init__")
    methods = {}
    for name in ("scale_factor", "override_default_bins"):
        fn = mpg._method(ad1, "AD1Evaluator", name)
        for a in fn.args.args:
            a.annotation = None                               # ``Dict`` is not imported here
        mod = ast.Module(body=[fn], type_ignores=[])
        ast.fix_missing_locations(mod)
        exec(compile(mod, "<reference, in memory>", "exec"), methods)

    def make(e_scale=None):
        me = types.SimpleNamespace(E_scale=consts["E_NORMALIZATION_FACTOR"], z_scale=consts["Z_NORMALIZATION_FACTOR"],
                                   E_adjust=1.0)
        if e_scale:                                           # AD1Evaluator.__init__:40-44
            me.E_adjust = me.E_scale / e_scale
            me.E_scale = e_scale
        for node in init.body:                                # the plain ``self.<attr> = <expr>`` lines, in order
            if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Attribute) and \
                    node.targets[0].attr in ("dt_scale", "toffset_scale", "PE_scale", "dp_scale", "E_index", "dt_index",
                                             "PE0_index", "PE1_index", "z_index", "PSD_index", "toffset_index", "dp_index",
                                             "phys_names", "phys_units", "default_bins"):
                setattr(me, node.targets[0].attr, mpg._eval(node.value, self=me, **consts))
        me.scale_factor = lambda index: methods["scale_factor"](me, index)
        me.override_default_bins = lambda ov: methods["override_default_bins"](me, ov)
        return me
    return raw, make


class RefRealPairs(mpg.RefPairs):
    def store(self, out, name):
        """Packed, to keep the archive's per-array overhead down: <name>_one = rows (mean, n, dev) over the 1-D cells of
        all metrics in order, <name>_two = rows (sum, n) over the cells of all pairs in the order 0_1, 0_2, .., 1_2, ..
        (float64 holds every count exactly)."""
        for i in range(len(self.nbins)):
            self.raw["finalize2d"](self.val[i], self.num[i], self.M2[i])      # MetricAggregator.finalize
        flat = lambda tabs: np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in tabs]) if tabs else np.zeros(0)
        out[name + "_one"] = np.stack([flat(self.val), flat(self.num), flat(self.M2)])
        keys = list(self.val2)
        out[name + "_two"] = np.stack([flat([self.val2[k] for k in keys]), flat([self.num2[k] for k in keys])])


def init_results(me, raw, target_has_phys, target_index, metric_name, bin_overrides):
    """TensorEvaluator.__init__ / _init_results: the metrics as (name, low, high, n_bins, norm_factor, scale_factor)."""
    if bin_overrides is not None:
        me.override_default_bins(bin_overrides)
    if target_index is not None and metric_name is None:
        metric_name = "mean absolute error"
    metrics = []
    i = 0
    if target_has_phys:
        if target_index is None:
            raise RuntimeError("target is tensor of phys quantities, must pass the target index to the evaluator")
        for name in me.phys_names:
            metrics.append((name, *me.default_bins[i], me.scale_factor(i), me.scale_factor(target_index)))
            i += 1
    else:
        if target_index is not None:
            name, bins, scale_factor = me.phys_names[target_index], me.default_bins[target_index], me.scale_factor(target_index)
        else:
            name = "unknown" if metric_name is None else metric_name
            bins, scale_factor = [0., 1., 40], 1.
        metrics.append((name, *bins, None, scale_factor))
    return metrics, metric_name


def main():
    import tensor_evaluator_cases as tc
    raw, make = reference()
    rng = np.random.default_rng(20241018)
    out, names = {}, []
    SMALL = {0: [0.0, 12.0, 7], 1: [-15.0, 15.0, 5], 2: [0.0, 5000.0, 6], 3: [0.0, 5000.0, 9], 4: [-600.0, 600.0, 12],
             5: [0.0, 0.6, 8], 6: [0.0, 30.0, 10], 7: [0.0, 1176.0, 11]}

    def setup(has_phys, target_index, metric_name, overrides):
        me = make()
        metrics, metric_name = init_results(me, raw, has_phys, target_index, metric_name, overrides)
        nbins = [int(m[3]) for m in metrics]
        edges = [mpg.edges_of(raw, m[1], m[2], m[3]) for m in metrics]
        ranges = [mpg.normalized(lo, hi, m[4]) for (lo, hi), m in zip(edges, metrics)]
        return metrics, metric_name, nbins, ranges

    def tensor_case(name, batches, has_phys=True, target_index=7, metric_name="mean absolute error", overrides=SMALL,
                    dtype="f32", n_classes=1):
        metrics, metric_name, nbins, ranges = setup(has_phys, target_index, metric_name, overrides)
        pairs = RefRealPairs(raw, nbins, n_classes)
        host = tc.HostTensorTables(nbins, ranges, [m[0] for m in metrics], metric_name, n_classes)
        det = (np.zeros((NX, NY, 2), np.float32), np.zeros((NX, NY, 2), np.int32))       # register_aggregator
        for b, bt in enumerate(batches):
            nv = len(bt["results"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            c, target, results = bt["c"][:nv], bt["target"][:nv], bt["results"][:nv]
            assert results.dtype == np.float32
            # TensorEvaluator.add, call for call
            if target.ndim >= 2:
                target = target.transpose(1, 0)
            c_is_det = len(c.shape) == 1
            r64, t64 = results.astype(np.float64), target.astype(np.float64)
            if has_phys:
                pairs.add(r64, t64, 0, ranges)                                          # metric_pairs.add_normalized
            else:
                raw["metric_accumulate_1d"](r64, t64, pairs.val[-1][0], pairs.num[-1][0], pairs.M2[-1][0],
                                            list(ranges[-1]), nbins[-1])                # metrics[-1].add_normalized
            for i in range(NX):
                for j in range(NY):
                    for k in range(2):
                        if c_is_det:
                            inds = c == 2 * (14 * j + i) + k
                        else:
                            inds = np.where((c == (i, j, k)).all(axis=1))
                        sel = results[inds]                                             # increment_metric, dim 3
                        det[1][i, j, k] += sel.shape[0]
                        det[0][i, j, k] += np.sum(sel)
            for k, v in bt.items():
                out["%s_b%d_%s" % (name, b, k)] = v
            host.add(bt["c"], bt["target"], bt["results"], int(bt["n_valid"]))
        ov = overrides or {}
        out[name + "_strs"] = np.array(["tensor", dtype, metric_name or ""])
        out[name + "_meta"] = np.array([len(batches), n_classes, int(has_phys), -1 if target_index is None else target_index],
                                       np.int64)
        out[name + "_ov"] = np.array([[k] + list(ov[k]) for k in sorted(ov)], np.float64).reshape(len(ov), 4)
        out[name + "_metric_names"] = np.array([m[0] for m in metrics])
        out[name + "_metric_table"] = np.array([[m[1], m[2], m[3], r[0], r[1], m[5]] for m, r in zip(metrics, ranges)],
                                               np.float64)
        pairs.store(out, name)
        out[name + "_det"] = np.stack([det[0].astype(np.float64), det[1].astype(np.float64)])
        tc.compare(tc.expected(out, name), name, host.results(), [m[0] for m in metrics], host.det_name)   # the restatement agrees
        names.append(name)

    def pairs_case(name, nb, ranges, C, batches):
        pairs = RefRealPairs(raw, nb, C)
        host = tc.HostRealPairTables(nb, ranges, C)
        for b, bt in enumerate(batches):
            nv = len(bt["results"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            par, res, cat = bt["params"][:, :nv].astype(np.float64), bt["results"][:nv].astype(np.float64), bt["category"][:nv]
            for i in range(C):
                inds = np.asarray(cat == i).nonzero()[0]
                pairs.add(res[inds], par[:, inds], i, ranges)
            for k, v in bt.items():
                out["%s_b%d_%s" % (name, b, k)] = v
            host.add(bt["params"][:, :nv], bt["results"][:nv], bt["category"][:nv])
        out[name + "_strs"] = np.array(["pairs", "f32", ""])
        out[name + "_meta"] = np.array([len(batches), C, 0, -1], np.int64)
        out[name + "_metric_names"] = np.array(["m%d" % i for i in range(len(nb))])
        out[name + "_metric_table"] = np.array([[r[0], r[1], n, r[0], r[1], 1.0] for r, n in zip(ranges, nb)], np.float64)
        pairs.store(out, name)
        tc.compare(tc.expected(out, name), name, host.results(["m%d" % i for i in range(len(nb))]), ["m%d" % i for i in range(len(nb))])
        names.append(name)

    def phys(n, dtype="f32"):
        return mpg.rounded(rng.random((n, 8)) * 1.2 - 0.1, dtype)

    def losses(n):
        return (rng.random(n) * 0.3).astype(np.float32)

    def dets(n, dtype=np.int32):
        return rng.integers(0, 308, n).astype(dtype)

    def xyz(n, dtype=np.int32):
        return np.column_stack([rng.integers(0, NX, n), rng.integers(0, NY, n), rng.integers(0, 2, n)]).astype(dtype)

    def batch(c, target, results, n_valid=-1):
        return dict(c=c, target=target, results=np.asarray(results, np.float32), n_valid=np.int64(n_valid))

    # (a) the forms of c
    tensor_case("det_i32", [batch(dets(48), phys(48), losses(48))])
    tensor_case("det_i64", [batch(dets(48, np.int64), phys(48), losses(48))])
    tensor_case("xyz_i32", [batch(xyz(48), phys(48), losses(48))])
    tensor_case("xyz_i64", [batch(xyz(48, np.int64), phys(48), losses(48))])
    tensor_case("one_row", [batch(dets(1), phys(1), losses(1))])
    c = dets(40)
    c[:8] = [308, 309, 615, 616, -1, -2, 100000, 2 ** 31 - 1]                # beyond the last PMT, negative, large
    tensor_case("outside_grid_det", [batch(c, phys(40), losses(40))])
    c = xyz(40, np.int64)
    c[:8] = [[14, 0, 0], [0, 11, 0], [0, 0, 2], [-1, 3, 1], [3, -1, 1], [3, 3, -1], [2 ** 40, 1, 1], [13, 10, 1]]
    tensor_case("outside_grid_xyz", [batch(c, phys(40), losses(40))])
    tensor_case("one_pmt", [batch(np.full(64, 2 * (14 * 6 + 9) + 1, np.int32), phys(64), losses(64))])
    # (b) the target's dtypes, two adds each
    for dt in ("f32", "bf16", "f16"):
        tensor_case("two_adds_" + dt, [batch(dets(40), phys(40, dt), losses(40)), batch(xyz(24), phys(24, dt), losses(24))],
                    dtype=dt)
    # (c) a single target
    tensor_case("single_float", [batch(dets(48), (rng.random(48) * 1.2 - 0.1).astype(np.float32), losses(48))],
                has_phys=False, target_index=None, metric_name="mean squared error", overrides=None)
    tensor_case("single_float_f16", [batch(dets(48), mpg.rounded(rng.random(48) * 1.2 - 0.1, "f16"), losses(48))],
                has_phys=False, target_index=None, metric_name=None, overrides=None, dtype="f16")
    tensor_case("single_index", [batch(xyz(48), (rng.random(48) * 1.2 - 0.1).astype(np.float32), losses(48))],
                has_phys=False, target_index=4, metric_name=None, overrides=None)
    tensor_case("class_i64", [batch(dets(48), rng.integers(0, 2, 48).astype(np.int64), losses(48) * 5)],
                has_phys=False, target_index=None, metric_name="Accuracy", overrides=None, dtype="i64")
    # (d) bin edges of the eight default ranges: 100 bins in fp32 (the one case of the default size), the small bins in
    # the 16-bit types
    for dt, ov in (("f32", None), ("bf16", SMALL), ("f16", SMALL)):
        _m, _n, nbins, ranges = setup(True, 7, "mean absolute error", ov)
        probes = []
        for i, (r, n) in enumerate(zip(ranges, nbins)):
            fall = mpg.find_fall_through(raw, r[0], r[1], n)
            print("%s range %d [%r, %r] / %d: fall-through value %s" % (
                dt, i, r[0], r[1], n, "none exists among the fp32 values searched" if fall is None else repr(fall)))
            probes.append(mpg.rounded(mpg.edge_values(r[0], r[1], n, fall), dt))
        N = max(len(p) for p in probes)
        t = np.stack([np.resize(p, N) for p in probes], axis=1)
        t = np.concatenate([t, np.stack([rng.permutation(col) for col in t.T], axis=1)])     # edges against edges
        assert len(t) <= 64
        tensor_case("edges_" + dt, [batch(dets(len(t)), t.astype(np.float32), losses(len(t)))], overrides=ov, dtype=dt)
    # (e) n_valid inside the batch, garbage behind it
    c, t, r = xyz(32), phys(32), losses(32)
    c[20:], t[20:], r[20:] = [-7, 99, 5], np.nan, np.nan
    r[25] = np.inf
    tensor_case("padded", [batch(c, t, r, 20)])
    # (f) result values that stress the arithmetic
    tensor_case("res_zero", [batch(dets(40), phys(40), np.zeros(40))])
    tensor_case("res_constant", [batch(dets(40), phys(40), np.full(40, 0.375))])
    tensor_case("res_near_constant", [batch(dets(64), phys(64), 1000.0 + np.arange(64) * 1e-4)])
    low = (2.0 ** -10 + np.arange(20) * 2.0 ** -33 + rng.integers(0, 2, 20) * 2.0 ** -34).astype(np.float32)
    assert (np.rint(low.astype(np.float64) * 2.0 ** 32) != low.astype(np.float64) * 2.0 ** 32).any()
    tensor_case("res_low_bits", [batch(dets(40), phys(40), np.r_[low, losses(20) + 0.5])])
    tensor_case("res_negative", [batch(dets(40), phys(40), (rng.random(40) - 0.5) * 60000.0)])
    t = np.repeat(np.array([0.01, 0.11, 0.21, 0.31, 0.41], np.float32), [1, 2, 3, 4, 5])    # finalize2d's n > 2
    tensor_case("res_n123", [batch(dets(len(t)), t, losses(len(t)))], has_phys=False, target_index=None,
                metric_name="mean squared error", overrides=None)
    # (g) the kernel keeps the 1-D cells in an LDS image of at most 1024 cells and goes to global atomics above it:
    # 2 metrics of 506 + 2 bins are 1024 cells with 2 classes and 1536 with 3; the third class stays empty, so the
    # tables of the first two are the same on both sides
    M = 64
    dpar = np.stack([np.r_[mpg.edge_values(0.0, 1.0, 506, None), rng.random(M).astype(np.float32)][:M],
                     (rng.random(M) * 1.2 - 0.1).astype(np.float32)])
    dbatch = dict(params=dpar, results=(rng.random(M) * 4 - 1).astype(np.float32),
                  category=rng.integers(-1, 2, M).astype(np.int32), n_valid=np.int64(-1))
    for C in (2, 3):
        pairs_case("dispatch_C%d" % C, [506, 2], [(0.0, 1.0), (0.0, 1.0)], C, [dbatch])

    out["case_names"] = np.array(names)
    path = os.path.join(HERE, "tensor_evaluator_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote tensor_evaluator_cases.npz: %d arrays, %d cases, %d bytes" % (len(out), len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
