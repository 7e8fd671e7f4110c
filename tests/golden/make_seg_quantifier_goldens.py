"""Generates tests/golden/seg_quantifier_cases.npz from the REFERENCE's own evaluation arithmetic (the reference tree, this
container only): inputs and the tables its functions give for them.  No reference text is written anywhere; the npz holds
arrays only.  The layout of the file is described in tests/seg_quantifier_cases.py.

How the reference is run (the method of make_pid_evaluator_goldens.py, whose helpers are used)
  * numba is not installed here, so the functions are taken from src/utils/SparseUtils.py's syntax tree IN MEMORY, their
    ``@nb.jit`` decorators dropped, and executed unmodified: get_bin_index, hist_add_1d, hist_add_2d,
    metric_accumulate_1d, metric_accumulate_2d, finalize2d, gen_multiplicity_list, gen_SE_mask; get_bins from
    src/utils/util.py and retrieve_class_names_PIDS (with PID_MAP / PID_MAPPED_NAMES) from src/evaluation/PIDEvaluator.py
    the same way.  Constructor constants come from the classes' trees as in make_pid_evaluator_goldens.reference().
  * The bodies of SegEvaluator.add, MetricPairAggregator.add_normalized and ErrorAggregator.add_norm are repeated here
    call for call.
  * Float widths: the functions get float64 arrays holding the fp32 (or bf16 / f16 rounded) values, so ``pred - actual``
    is the fp64 difference of the stored values.  The reference subtracts in float32; every recorded error is asserted to
    lie further than 1e-6 of the class's range from every interior error-bin edge (or exactly on one), so both
    differences fall into the same bin.
  * gen_multiplicity_list looks ahead past the end of the batch: it runs on the case with ONE sentinel event index (-1)
    appended, through a view that reports the case's own row count.
  * ``error_edges`` fixed in advance has no counterpart in the reference's constructor: the case presets the class's
    ``error_edges`` entry, which ``add_norm`` then leaves alone.

Run:  python tests/golden/make_seg_quantifier_goldens.py
"""
import ast
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_pid_evaluator_goldens as mp  # noqa: E402

WANTED = ["get_bin_index", "hist_add_1d", "hist_add_2d", "metric_accumulate_1d", "metric_accumulate_2d", "finalize2d",
          "gen_multiplicity_list", "gen_SE_mask"]


def reference():
    _raw, me, seg = mp.reference()
    raw = mp._functions(mp._tree("src", "utils", "SparseUtils.py"), WANTED, dict(sqrt=math.sqrt))
    raw.update(mp._functions(mp._tree("src", "utils", "util.py"), ["get_bins"], dict(np=np)))
    pid = mp._tree("src", "evaluation", "PIDEvaluator.py")
    ns = {}
    for node in pid.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and \
                node.targets[0].id in ("PID_MAP", "PID_MAPPED_NAMES"):
            ns[node.targets[0].id] = ast.literal_eval(node.value)
    mp._functions(pid, ["retrieve_class_names_PIDS"], ns)
    me.class_names, me.class_PIDs = ns["retrieve_class_names_PIDS"]()
    return raw, me, seg


class RefError:
    """ErrorAggregator's arrays, on the reference's functions."""

    def __init__(self, raw, nb, C):
        self.raw, self.n_bins = raw, nb
        self.error_edges = [None] * C
        self.error_hist = np.zeros((C, nb + 2), dtype=np.double)
        self.error_2d = np.zeros((C, nb + 2, nb + 2), dtype=np.double)
        self.errors = [[] for _ in range(C)]

    def add_norm(self, pred, actual, class_ind):                 # ErrorAggregator.add_norm, call for call
        error = pred - actual
        if self.error_edges[class_ind] is None:
            max_error = np.max(np.abs(error))
            error_low = -1.1 * max_error
            error_high = 1.1 * max_error
            self.error_edges[class_ind] = self.raw["get_bins"](error_low, error_high, self.n_bins)
        e = self.error_edges[class_ind]
        self.raw["hist_add_1d"](error, self.error_hist[class_ind], [e[0], e[-1]], self.n_bins)
        self.raw["hist_add_2d"](actual, pred, self.error_2d[class_ind], [0., 1.], [0., 1.], self.n_bins, self.n_bins)
        self.errors[class_ind].append(error)

    def clearance(self):
        """Smallest distance of a recorded error from an interior edge of its class, relative to the range; errors
        exactly on an edge are left out."""
        worst = np.inf
        for c, e in enumerate(self.error_edges):
            if e is None or not self.errors[c]:
                continue
            lo, hi = float(e[0]), float(e[-1])
            w = (hi - lo) / self.n_bins
            edges = np.arange(1, self.n_bins + 1) * w + lo
            v = np.concatenate(self.errors[c])
            v = v[np.isfinite(v)]
            d = np.abs(v[:, None] - edges[None, :])
            d = d[~np.isin(v, edges)]
            if d.size:
                worst = min(worst, float(d.min() / (hi - lo)))
        return worst


def main():
    import seg_quantifier_cases as sc
    raw, me, seg = reference()
    assert [list(p) for p in me.class_PIDs] == sc.CLASS_PIDS
    rng = np.random.default_rng(20241018)
    out = {"seg_status": seg, "class_names": np.array(me.class_names)}
    se_cells, de_cells = np.argwhere(seg == 0.5), np.argwhere(seg == 0.0)
    names, clear_all = [], []
    SMALL = {0: [0.0, 12.0, 8], 4: [-600.0, 600.0, 9], 5: [0.0, 0.6, 6]}   # 9: an error of exactly 0 (16-bit rows) is mid-bin

    def cells(n, n_se):
        pick = np.concatenate([se_cells[rng.choice(len(se_cells), n_se, replace=n_se > len(se_cells))],
                               de_cells[rng.choice(len(de_cells), n - n_se, replace=n - n_se > len(de_cells))]])
        return pick[rng.permutation(n)]

    def make_batch(counts, n_se, dtype="f32", pids=(1, 4, 6, 258, 256, 512), ti=4, err=0.2):
        co = np.concatenate([np.column_stack([cells(n, k), np.full(n, e)]) for e, (n, k) in enumerate(zip(counts, n_se))])
        N = len(co)
        tg = rng.random((N, 8)).astype(np.float32)
        tg[:, 0] = rng.random(N) * 1.1 - 0.02
        tg[:, 5] = rng.random(N) * 0.7 - 0.03
        tg[:, 4] = rng.random(N) * 1.1 - 0.05
        tg = mp.rounded(tg, dtype)
        res = mp.rounded(tg[:, ti] + (rng.random(N) * 2 - 1) * err, dtype)
        return dict(coords=co.astype(np.int32), results=res.astype(np.float32), target=tg.astype(np.float32),
                    pid=np.asarray(pids)[rng.integers(0, len(pids), N)].astype(np.int64), n_valid=np.int64(-1))

    def spread(n, biggest=9):
        """Event sizes summing to n: a 1-row event, one of 7+ rows, the rest random; (sizes, single-ended rows of each)."""
        sizes = [1, min(biggest, max(1, n - 1))] if n > 1 else [1]
        while sum(sizes) < n:
            sizes.append(int(min(rng.integers(1, 7), n - sum(sizes))))
        sizes = [s for s in sizes if s > 0]
        if sum(sizes) > n:
            sizes = [n]
        return sizes, [int(rng.integers((s + 1) // 2, s + 1)) for s in sizes]

    def case(name, batches, ti=4, ov=SMALL, has_pid=True, dtype="f32", fixed=None, raises=False, nan_rows=False):
        nbins, ranges, bins = sc.metric_setup(ov)
        params = [bins[0], bins[5], [0.5, 6.5, 6], bins[4]]
        ref_ranges = [mp.normalized(*mp.edges_of(raw, *p), s) for p, s in zip(params, me.scales)]
        assert np.array_equal(np.array(ref_ranges), np.array(ranges))
        C = 5 if has_pid else 1
        nb = int(bins[ti][2])
        pairs, agg = mp.RefPairs(raw, nbins, C), RefError(raw, nb, C)
        if fixed is not None:
            agg.error_edges = [np.array(fixed, np.float64) for _ in range(C)]
        host = sc.HostSegTables(seg, ti, ov, has_pid, fixed)
        failed = False
        for b, bt in enumerate(batches):
            nv = len(bt["coords"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            coo, PID = bt["coords"][:nv], bt["pid"][:nv]
            results, target = bt["results"][:nv].astype(np.float64), bt["target"][:nv].astype(np.float64)
            # SegEvaluator.add, call for call
            mae = np.absolute(results - target[:, ti])
            mult = np.zeros((target.shape[0],))
            raw["gen_multiplicity_list"](mp.Lookahead(coo[:, 2], np.array(-1, coo.dtype)), mult)
            parameters = np.stack((target[:, me.E_index], target[:, me.PSD_index], mult, target[:, me.z_index]), axis=1)
            parameters = np.swapaxes(parameters, 0, 1)
            se_mask = np.zeros((coo.shape[0],), dtype=bool)
            raw["gen_SE_mask"](coo, seg, se_mask)
            cat, slot, at = np.full(nv, -1, np.int32), np.full(nv, -1, np.int32), 0
            try:
                if has_pid:
                    for i in range(len(me.class_names)):
                        for pid in me.class_PIDs[i]:
                            ind_match = PID == pid
                            ind_match = ind_match * se_mask
                            if results[ind_match].shape[0] > 0:
                                pairs.add(mae[ind_match], parameters[:, ind_match], i, ref_ranges)
                                agg.add_norm(results[ind_match], target[ind_match, ti], i)
                            cat[ind_match], slot[ind_match] = i, at
                            at += 1
                else:
                    pairs.add(mae, parameters, 0, ref_ranges)
                    agg.add_norm(results, target[:, ti], 0)
                    cat[:], slot[:] = 0, 0
            except (ZeroDivisionError, ValueError) as e:          # np.arange over a range of width 0
                assert raises, (name, e)
                failed = True
            for k, v in bt.items():
                out["%s_b%d_%s" % (name, b, k)] = v
            out["%s_b%d_rows" % (name, b)] = np.stack([mult.astype(np.int32), se_mask.astype(np.int32), cat, slot])
            if failed:
                break
            host.add(bt["results"], bt["target"], bt["coords"], bt["pid"], int(bt["n_valid"]))
            r = sc.seg_rows(bt["coords"], bt["pid"], seg, int(bt["n_valid"]), has_pid)
            assert np.array_equal(r["mult"], mult) and np.array_equal(r["se"], se_mask) and \
                np.array_equal(r["category"], cat) and np.array_equal(r["slot"], slot), name
        assert failed == raises, name
        out[name + "_meta"] = np.array([len(batches), has_pid, ti, raises, fixed is not None, nan_rows], np.int64)
        out[name + "_dtype"] = np.array(dtype)
        out[name + "_ov"] = np.array([[k, *v] for k, v in (ov or {}).items()], np.float64).reshape(-1, 4)
        if fixed is not None:
            out[name + "_fixed"] = np.array(fixed, np.float64)
        names.append(name)
        if raises:
            return
        clear = agg.clearance()
        assert clear > 1e-6, (name, clear)
        clear_all.append(clear)
        for i in range(4):
            raw["finalize2d"](pairs.val[i], pairs.num[i], pairs.M2[i])
        out[name + "_one"] = np.stack([np.concatenate([t[i].reshape(-1).astype(np.float64) for i in range(4)])
                                       for t in (pairs.val, pairs.num, pairs.M2)])
        keys = sorted(pairs.val2)
        out[name + "_two"] = np.stack([np.concatenate([pairs.val2[k].reshape(-1) for k in keys]),
                                       np.concatenate([pairs.num2[k].reshape(-1).astype(np.float64) for k in keys])])
        assert np.array_equal(agg.error_hist, np.round(agg.error_hist)) and np.array_equal(agg.error_2d, np.round(agg.error_2d))
        out[name + "_error_hist"], out[name + "_error_2d"] = agg.error_hist.astype(np.int64), agg.error_2d.astype(np.int64)
        out[name + "_error_edges"] = np.array([[e[0], e[-1]] if e is not None else [0.0, 0.0] for e in agg.error_edges])
        out[name + "_error_edges_set"] = np.array([e is not None for e in agg.error_edges], np.int32)
        # the restatement agrees with the reference (a NaN error makes the metric tables NaN on both sides: error tables only)
        sc.compare(sc.expected(out, name), name, host.results(), errors_only=nan_rows)

    # ---- event structure and row counts
    case("one_row", [make_batch([1], [1], pids=(1,))])
    for n in (63, 64, 65, 255, 256, 257):
        sizes, n_se = spread(n)
        case("rows_%d" % n, [make_batch(sizes, n_se)])
    b = make_batch([4, 9, 3, 5], [3, 6, 2, 4])
    b["n_valid"] = np.int64(14)                                          # ends inside event 2
    b["coords"][14:] = [[-5, 40, 999]] * (len(b["coords"]) - 14)
    b["results"][14:], b["target"][14:], b["pid"][14:] = np.nan, np.nan, -7
    case("padded", [b])
    case("no_se", [make_batch([3, 8, 2], [0, 0, 0])])
    case("pid_outside", [make_batch([5, 8, 4], [4, 6, 3], pids=(1, 4, 2, 1000, -1, 6, 512, 0))])
    # ---- class 2's edges
    first = make_batch([6, 8, 5], [5, 7, 4], pids=(1, 258, 256), err=0.3)
    second = make_batch([7, 7, 6], [6, 6, 5], pids=(1, 6, 258, 4), err=0.5)     # wider: the edges of batch one hold
    case("c2_258_first", [first, second])
    b = make_batch([9, 9, 8, 8], [8, 8, 7, 7], pids=(6, 258, 1))
    is6 = b["pid"] == 6
    b["results"] = np.where(is6, b["target"][:, 4] + (b["results"] - b["target"][:, 4]) * np.float32(0.25),
                            b["results"]).astype(np.float32)             # pid 6's errors are the smaller ones
    case("c2_both", [b])
    case("class_second_add", [make_batch([6, 7], [5, 6], pids=(1, 4, 6)), make_batch([8, 5], [7, 4], pids=(1, 512, 256, 6))])
    # ---- two adds against one add of the concatenation, where no class's first subset changes: the second batch's
    # errors are smaller, and every slot of the second batch is in the first
    a, b2 = make_batch([7, 9, 6, 8], [6, 8, 5, 7], err=0.3), make_batch([5, 8, 7], [4, 7, 6], err=0.1)
    for dt in ("f32", "bf16", "f16"):
        ad, bd = ({k: (mp.rounded(v, dt).astype(np.float32) if k in ("results", "target") else v) for k, v in x.items()}
                  for x in (a, b2))
        case("two_adds_" + dt, [ad, bd], dtype=dt)
        if dt == "f32":
            cc = {k: np.concatenate([ad[k], bd[k]]) for k in ("results", "target", "pid")}
            cc["coords"] = np.concatenate([ad["coords"], bd["coords"] + np.array([0, 0, 4], np.int32)])
            cc["n_valid"] = np.int64(-1)
            case("concat_f32", [cc])
    # ---- values at the ends of the ranges: the parameters (E and z normalised to [0, 1], PSD over [0, 0.6]) and the
    # error_2d axes exactly at 0, at high, below low; a NaN PSD
    b = make_batch([6, 7, 8], [6, 7, 8], pids=(1, 4))
    probe = np.array([0.0, 1.0, -0.01, 1.25, 0.5], np.float32)
    b["target"][:5, 0], b["target"][5:10, 4] = probe, probe
    b["target"][:4, 5] = [0.0, 0.6, -0.01, np.nan]
    b["results"][10:15] = probe
    case("range_ends", [b])
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    b["results"] = (b["target"][:, 0] + (rng.random(len(b["results"])).astype(np.float32) * 2 - 1) * 0.2).astype(np.float32)
    b["results"][10:15] = probe
    case("range_ends_ti0", [b], ti=0)
    # ---- target_index 0 with its default 100 bins, and the default bins of z
    sizes, n_se = spread(40)
    case("ti0_default_bins", [make_batch(sizes, n_se, ti=0)], ti=0, ov=None)
    case("ti4_default_bins", [make_batch(sizes, n_se)], ov=None)
    # ---- the single class without PID (no single-ended mask), edges fixed in advance, a largest error of 0
    case("no_pid", [make_batch([5, 9, 4], [2, 5, 1]), make_batch([3, 8], [1, 4])], has_pid=False)
    case("fixed_edges", [make_batch([6, 8, 5], [5, 7, 4]), make_batch([4, 9], [3, 8])], fixed=(-0.15, 0.15))
    b = make_batch([5, 6], [5, 6], pids=(1,))
    b["results"] = b["target"][:, 4].copy()
    case("max_zero", [b], raises=True)
    # ---- a NaN error (a NaN in target[:, ti], and one in results) in a class whose edges are already set -- by an earlier
    # add, or in advance: bin 0 of error_hist, bin 0 of the NaN axis of error_2d, recorded from hist_add_1d / hist_add_2d
    def with_nans(b):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        b["pid"][:4] = [1, 1, 4, 4]
        b["target"][0, 4], b["results"][1] = np.nan, np.nan
        b["target"][2, 4], b["results"][3] = np.nan, np.nan
        b["results"][2], b["target"][3, 4] = 1.5, -0.25             # the other axis of error_2d: overflow, underflow
        return b
    case("nan_second_add", [make_batch([6, 7], [6, 7], pids=(1, 4, 6)), with_nans(make_batch([5, 8], [5, 8], pids=(1, 4, 6)))],
         nan_rows=True)
    case("nan_fixed_edges", [with_nans(make_batch([7, 6], [7, 6], pids=(1, 4, 512)))], fixed=(-0.15, 0.15), nan_rows=True)
    # ---- the NaN in a class's FIRST subset: np.max gives NaN, np.arange fails, the edges stay unset
    b = make_batch([6, 5], [6, 5], pids=(1, 4))
    b["pid"][0], b["target"][0, 4] = 1, np.nan
    case("nan_first_target", [b], raises=True, nan_rows=True)
    b = make_batch([6, 5], [6, 5], pids=(1, 4))
    b["pid"][2], b["results"][2] = 4, np.nan
    case("nan_first_results", [b], raises=True, nan_rows=True)

    out["case_names"] = np.array(names)
    out["clearance"] = np.array(min(clear_all))
    print("smallest distance of a recorded error from an interior error-bin edge, relative to its range: %.3g" % min(clear_all))
    path = os.path.join(HERE, "seg_quantifier_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote seg_quantifier_cases.npz: %d arrays, %d cases, %d bytes" % (len(out), len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
