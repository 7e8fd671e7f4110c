"""Shared by tests/test_z_real_evaluator_host.py and tests/test_gpu_z_real_evaluator.py: the layout of
tests/golden/z_real_evaluator_cases.npz (written by tests/golden/make_z_real_evaluator_goldens.py from the reference's own
functions) and the comparison of an evaluator's ``results()`` with it.

Constants: ``seg_status``, ``blind_detl``, ``E_scale``, ``z_scale``, ``phys_indices`` (E, PSD, z), ``n_mult``, ``n_z``,
``n_E``, ``E_bounds``, ``mult_bounds``, ``z_bounds``, ``default_bins``, ``n_samples``, ``n_zbins``, ``pid_map``,
``class_nbins`` / ``class_ranges``, ``sample_params`` / ``sample_nbins`` / ``sample_ranges``, ``E_range``,
``table_names`` with ``shape_<table>``.

Alignment cases ``align_names``: ``<n>_rows`` float64 [N, 2 L] holding the dtype's values, ``<n>_samples`` [N, 2, 5],
``<n>_start`` int32 [N, 2], ``<n>_L``, ``<n>_dtype``; ``al_patterns_L<L>`` names the first rows' left-side patterns.

Evaluator cases ``case_names``: ``<n>_nb`` batches ``<n>_b<k>_{coords, pred, targ, feats, pid, n_valid}`` (dense maps
[B, 1 | 7, 14, 11], float64 arrays holding the dtype's values), per batch the recorded ``samples``, ``start`` and the
float32 ``baseline`` of the valid rows; ``<n>_has_pid``, ``<n>_wf``, ``<n>_dtype``; the fourteen tables
``<n>_<table>_{sum, n}``; the class tables ``<n>_class_*``, the twelve sliced sample aggregators ``<n>_smp_*`` with the
category ``slice * C + class`` as leading axis, and the all-z one ``<n>_allz_*``: per metric ``_m<i>_{mean, n, dev}``
(after finalize2d), per pair ``_p<i>_<j>_{idx, n, val}`` sparse over the flattened [C, nb_i + 2, nb_j + 2] table.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "z_real_evaluator_cases.npz")
TOL = 1e-5                       # the project's bar: of each output's largest magnitude
TORCH_DTYPES = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}
BATCH_KEYS = ("coords", "pred", "targ", "feats", "pid", "n_valid")


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def case_names(gold):
    return [str(n) for n in gold["case_names"]]


def meta_of(gold, name):
    return dict(has_pid=bool(gold[name + "_has_pid"]), wf=bool(gold[name + "_wf"]), dtype=str(gold[name + "_dtype"]),
                nb=int(gold[name + "_nb"]))


def batches_of(gold, name):
    out = []
    for b in range(int(gold[name + "_nb"])):
        bt = {k: gold["%s_b%d_%s" % (name, b, k)] for k in BATCH_KEYS}
        for k in ("samples", "start", "baseline"):
            key = "%s_b%d_%s" % (name, b, k)
            if key in gold:
                bt[k] = gold[key]
        out.append(bt)
    return out


def table_names(gold):
    return [str(n) + cal for cal in ("", "_cal") for n in gold["table_names"]]


def _close(what, got, want, worst):
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    if worst is not None and scale > 0:
        worst[what] = max(worst.get(what, 0.0), err / scale)
    assert err <= TOL * scale, "%s: error %g against a largest magnitude of %g" % (what, err, scale)


def _dense(gold, key, shape):
    n, v = np.zeros(int(np.prod(shape)), np.int64), np.zeros(int(np.prod(shape)))
    n[gold[key + "_idx"]], v[gold[key + "_idx"]] = gold[key + "_n"], gold[key + "_val"]
    return v.reshape(shape), n.reshape(shape)


def compare_pairs(gold, prefix, got, names, what, worst=None):
    """``got`` = {"metrics": {name: (mean, n, dev)}, "pairs": {"i_j": (sum, n)}} against the recorded group ``prefix``."""
    for i, nm in enumerate(names):
        mean, n, dev = got["metrics"][nm]
        assert np.array_equal(n, gold["%s_m%d_n" % (prefix, i)]), "%s %s: counts of metric %d" % (what, prefix, i)
        _close("%s mean" % what, mean, gold["%s_m%d_mean" % (prefix, i)], worst)
        _close("%s dev" % what, dev, gold["%s_m%d_dev" % (prefix, i)], worst)
    for key, (s, n) in got["pairs"].items():
        ws, wn = _dense(gold, "%s_p%s" % (prefix, key), n.shape)
        assert np.array_equal(n, wn), "%s %s: counts of pair %s" % (what, prefix, key)
        _close("%s pair sums" % what, s, ws, worst)


def stack_slices(per_slice):
    """The twelve per-slice results as one result whose leading axis is ``slice * C + class``."""
    first = per_slice[0]
    return {"metrics": {k: tuple(np.concatenate([r["metrics"][k][t] for r in per_slice]) for t in range(3))
                        for k in first["metrics"]},
            "pairs": {k: tuple(np.concatenate([r["pairs"][k][t] for r in per_slice]) for t in range(2))
                      for k in first["pairs"]}}


def compare(gold, name, res, ev, worst=None):
    """Counts exactly, real-valued tables within TOL of each output's largest magnitude."""
    m = meta_of(gold, name)
    for t in table_names(gold):
        s, n = res[t]
        assert s.dtype == np.float64 and n.dtype == np.int64 and s.shape == tuple(gold["shape_" + t.replace("_cal", "")])
        assert np.array_equal(n, gold["%s_%s_n" % (name, t)]), "%s: counts of %s" % (name, t)
        _close("fourteen tables", s, gold["%s_%s_sum" % (name, t)], worst)
    assert ("metric_pairs" in res) == m["has_pid"] and ("z_binned_metric_pairs" in res) == m["wf"]
    if m["has_pid"]:
        compare_pairs(gold, name + "_class", res["metric_pairs"], ev.metric_names, "class tables", worst)
    if m["wf"]:
        zb = res["z_binned_metric_pairs"]
        assert len(zb) == 13
        compare_pairs(gold, name + "_smp", stack_slices(zb[:-1]), ev.sample_names, "sample tables", worst)
        compare_pairs(gold, name + "_allz", zb[-1], ev.sample_names, "all-z sample tables", worst)
