"""CPU checks of the TensorEvaluator's host side: the NumPy restatement of tests/tensor_evaluator_cases.py against the
values RECORDED from the reference (tests/golden/tensor_evaluator_cases.npz: counts exactly, float tables within 1e-5 of
each output's largest magnitude), the integer -> (mean, dev) arithmetic of psd/metric_pairs.real_triple_1d on hand-made
n / S / Q, the metric construction of the three constructor modes against the recorded names, ranges and bins, and
LitWaveform.evaluator refusing a CPU device.  No kernel is launched here."""
import copy
import json
import os

import numpy as np
import pytest

import tensor_evaluator_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return tc.load_golden()


def test_fixture_is_small_and_holds_arrays_only(gold):
    assert os.path.getsize(tc.GOLDEN) < 355399                     # the largest fixture before it
    assert len(tc.case_names(gold, "tensor")) >= 20 and tc.case_names(gold, "pairs") == ["dispatch_C2", "dispatch_C3"]
    for n in tc.case_names(gold):
        for b in tc.batches_of(gold, n):
            assert len(b["results"]) <= 64


def test_numpy_restatement_equals_the_recorded_reference(gold):
    worst = {}
    for name in tc.case_names(gold, "tensor"):
        names, nbins, ranges, C = tc.metrics_of(gold, name)
        host = tc.HostTensorTables(nbins, ranges, names, str(gold[name + "_strs"][2]), C)
        for b in tc.batches_of(gold, name):
            host.add(b["c"], b["target"], b["results"], int(b["n_valid"]))
        tc.compare(tc.expected(gold, name), name, host.results(), names, host.det_name, worst=worst)
    for name in tc.case_names(gold, "pairs"):
        names, nbins, ranges, C = tc.metrics_of(gold, name)
        host = tc.HostRealPairTables(nbins, ranges, C)
        for b in tc.batches_of(gold, name):
            nv = len(b["results"]) if int(b["n_valid"]) < 0 else int(b["n_valid"])
            host.add(b["params"][:, :nv], b["results"][:nv], b["category"][:nv])
        tc.compare(tc.expected(gold, name), name, host.results(names), names, worst=worst)
    print("host restatement, largest error / scale:", worst)


def test_cases_cover_what_they_are_named_for(gold):
    e = tc.expected(gold, "res_n123")
    assert sorted(set(e["m0_n"].reshape(-1))) == [0, 1, 2, 3, 4, 5]
    assert (e["m0_dev"][e["m0_n"] <= 2] == 0).all() and (e["m0_dev"][e["m0_n"] > 2] > 0).all()
    e = tc.expected(gold, "res_constant")
    assert all(np.abs(e["m%d_dev" % i]).max() == 0 for i in range(8)) and e["m0_mean"].max() == 0.375
    e = tc.expected(gold, "res_zero")
    assert np.abs(e["m0_mean"]).max() == 0 and e["det_sum"].max() == 0 and e["det_n"].sum() == 40
    assert tc.expected(gold, "outside_grid_det")["det_n"].sum() == 32 and tc.expected(gold, "outside_grid_det")["m0_n"].sum() == 40
    assert tc.expected(gold, "outside_grid_xyz")["det_n"].sum() == 33
    assert tc.expected(gold, "one_pmt")["det_n"][9, 6, 1] == 64
    assert tc.expected(gold, "padded")["m0_n"].sum() == 20
    assert np.isnan(tc.batches_of(gold, "edges_f32")[0]["target"]).any()
    assert [int(v) for v in gold["edges_f32_metric_table"][:, 2]] == [100] * 8
    e2, e3 = tc.expected(gold, "dispatch_C2"), tc.expected(gold, "dispatch_C3")
    assert e2["m0_n"].size + e2["m1_n"].size == 1024 and e3["m0_n"].size + e3["m1_n"].size == 1536
    assert np.array_equal(e2["m0_n"], e3["m0_n"][:2]) and np.array_equal(e2["p0_1_val"], e3["p0_1_val"][:2])


def test_integers_to_mean_and_dev():
    from waveformml_amd.psd.metric_pairs import real_triple_1d
    one = 1 << 32

    def tables(values):
        v = [int(np.rint(np.float64(np.float32(x)) * one)) for x in values]
        q = sum(x * x for x in v)
        return len(v), sum(v), q & 0xffffffff, (q >> 32) & 0xffffffff, q >> 64

    # limb SUMS are not normalised: carry the pieces as the kernel does, one element at a time
    def limb_tables(values):
        v = [int(np.rint(np.float64(np.float32(x)) * one)) for x in values]
        return len(v), sum(v), sum((x * x) & 0xffffffff for x in v), sum(((x * x) >> 32) & 0xffffffff for x in v), \
            sum((x * x) >> 64 for x in v)

    cells = [[], [0.25], [0.25, 0.75], [0.25, 0.75, 0.5], [0.375] * 7, [1000.0 + k * 1e-4 for k in range(64)],
             [-3.5, 2.0, 32767.0, -32767.0], [0.0] * 5]
    for make in (tables, limb_tables):
        cols = list(zip(*[make(c) for c in cells]))
        n = np.array(cols[0], np.int64)
        S, Q0, Q1, Q2 = (np.array(c, np.int64) for c in cols[1:])
        mean, n_out, dev = real_triple_1d(n, S, Q0, Q1, Q2)
        assert np.array_equal(n_out, n) and n_out is not n
        assert mean[0] == 0 and dev[0] == 0 and mean[1] == 0.25 and dev[1] == 0
        assert mean[2] == 0.5 and dev[2] == 0                         # n = 2: finalize2d keeps 0
        assert mean[3] == 0.5 and dev[3] == 0.25                      # n = 3: sqrt(0.125 / 2)
        assert mean[4] == 0.375 and dev[4] == 0                       # a constant: exactly 0
        x = np.array([np.float32(v) for v in cells[5]], np.float64)   # the cancellation case
        assert abs(mean[5] - x.mean()) < 1e-12 and abs(dev[5] - x.std(ddof=1)) <= 1e-12 * x.std(ddof=1) + 2.0 ** -33
        y = np.array(cells[6])
        assert abs(mean[6] - y.mean()) < 1e-12 and abs(dev[6] - y.std(ddof=1)) < 1e-9
        assert mean[7] == 0 and dev[7] == 0
    # 2^31 elements of the largest image: every limb sum still fits an int64
    v = (1 << 47) - 1
    assert max(((v * v) >> s) & 0xffffffff for s in (0, 32, 64)) * (1 << 31) < (1 << 63)


MODES = {"two_adds_f32": "phys", "edges_f32": "phys", "single_float": "single", "single_float_f16": "single",
         "single_index": "index", "class_i64": "single"}


@pytest.mark.parametrize("name", sorted(MODES))
def test_metric_construction_equals_the_recorded_reference(gold, name):
    from waveformml_amd.psd.metric_pairs import bin_edge_range, normalized_range
    from waveformml_amd.psd.tensor_evaluator import metric_setup
    kw = tc.constructor_kwargs(gold, name)
    s = metric_setup(**kw)
    names, nbins, ranges, _C = tc.metrics_of(gold, name)
    table = gold[name + "_metric_table"]
    assert [m[0] for m in s["metrics"]] == names and len(names) == (8 if MODES[name] == "phys" else 1)
    assert [int(m[3]) for m in s["metrics"]] == nbins
    assert np.array_equal(np.array([[m[1], m[2]] for m in s["metrics"]], np.float64), table[:, :2])
    got = [normalized_range(*bin_edge_range(float(m[1]), float(m[2]), int(m[3])), nf)
           for m, nf in zip(s["metrics"], s["norm_factors"])]
    assert np.array_equal(np.array(got), np.array(ranges))
    assert s["scale_factor"] == float(table[0, 5])
    if MODES[name] != "phys":
        assert s["norm_factors"] == [None] and got == [(0.0, 1.0)]
    assert s["metric_name"] == (str(gold[name + "_strs"][2]) or None)


def test_metric_setup_details():
    from waveformml_amd.psd.tensor_evaluator import metric_setup
    with pytest.raises(RuntimeError, match="must pass the target index"):
        metric_setup(target_has_phys=True)
    s = metric_setup(target_index=4, metric_name="mean squared error")
    assert s["metric_unit"] == "mm^2" and s["metrics"] == [("z", -600.0, 600.0, 100)] and s["scale_factor"] == 1200.0
    assert metric_setup()["metrics"] == [("unknown", 0.0, 1.0, 40)]
    s = metric_setup(e_scale=6.0, target_has_phys=True, target_index=0, bin_overrides={"5": [0.0, 0.5, 10]})
    assert s["metrics"][0][1:] == (0.0, 6.0, 100) and s["metrics"][2][1:] == (0.0, 2500.0, 100)
    assert s["metrics"][5][1:] == (0.0, 0.5, 10) and s["norm_factors"][:3] == [6.0, 30.0, 2500.0]
    with pytest.raises(IOError):
        metric_setup(bin_overrides={"x": [0, 1, 2]})


def _config(phys):
    with open(os.path.join(ROOT, "config", "waveform_tcn_z.json")) as f:
        cfg = json.load(f)
    cfg["optimize_config"].pop("scheduler_class", None)
    if phys:
        cfg["dataset_config"]["test_dataset_params"] = {"label_name": "phys"}
    return cfg


def test_lit_waveform_names_an_evaluator_and_refuses_the_cpu():
    import torch
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.litwaveform import LitWaveform
    torch.manual_seed(1)
    m = LitWaveform(DictionaryUtility.to_object(copy.deepcopy(_config(True)))).eval()
    assert m.test_has_phys and m.target_index == 7 and m.last_test_outputs is None
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        m.evaluator
    cfg = _config(False)
    cfg["dataset_config"]["calgroup"] = "x"
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        LitWaveform(DictionaryUtility.to_object(cfg)).evaluator
    from waveformml_amd.psd.tensor_evaluator import TensorEvaluator
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        TensorEvaluator("cpu")
    import inspect
    assert list(inspect.signature(TensorEvaluator.__init__).parameters)[1:] == [
        "device", "calgroup", "e_scale", "target_has_phys", "target_index", "metric_name", "metric_unit", "class_names",
        "bin_overrides"]


def test_entry_points_validate_on_the_host():
    """WFS_REQUIRE front doors of the new entry points: every call here returns before anything is launched."""
    import ctypes
    from waveformml_amd import _lib
    from waveformml_amd.psd.metric_pairs import real_table_layout
    lib = _lib.load()
    nb = _lib.i32_array([5, 7, 3])
    n = lib.wfs_metric_pairs_real_table_ints(3, nb, 2)
    assert n == sum(t * int(np.prod(s)) for _k, s, t in real_table_layout([5, 7, 3], 2)) == 2 * (5 * (7 + 9 + 5) + 2 * (63 + 35 + 45))
    assert lib.wfs_metric_pairs_real_table_ints(0, nb, 2) == 0 and lib.wfs_metric_pairs_real_table_ints(17, nb, 2) == 0
    lo, hi = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
    bad_hi = (ctypes.c_double * 3)(1, 0, 1)
    fake = ctypes.c_void_p(4096)                                     # never dereferenced: every call fails validation
    acc = lib.wfs_metric_pairs_accumulate_real
    assert acc(fake, fake, fake, 8, None, 3, lo, bad_hi, nb, 2, fake, fake, None) == _lib.WFS_EINVAL
    assert "high > low" in _lib.last_error()
    assert acc(fake, fake, fake, 8, None, 17, lo, hi, nb, 2, fake, fake, None) == _lib.WFS_EINVAL
    assert acc(fake, fake, fake, 1 << 31, None, 3, lo, hi, nb, 2, fake, fake, None) == _lib.WFS_EINVAL
    assert acc(fake, None, fake, 8, None, 3, lo, hi, nb, 2, fake, fake, None) == _lib.WFS_EINVAL
    assert acc(fake, fake, fake, 8, None, 3, lo, hi, nb, 2, None, fake, None) == _lib.WFS_EINVAL
    assert "NULL" in _lib.last_error()
    assert acc(None, None, None, 0, None, 3, lo, hi, nb, 2, fake, fake, None) == _lib.WFS_OK      # nothing to do
    rows = lib.wfs_tensor_rows
    ok = dict(c=fake, c64=0, cols=1, target=fake, dt=_lib.WFS_F32, P=8, res=fake, N=4, nx=14, ny=11)

    def call(**kw):
        a = dict(ok, **kw)
        return rows(a["c"], a["c64"], a["cols"], a["target"], a["dt"], a["P"], a["res"], a["N"], None, a["nx"], a["ny"],
                    fake, fake, fake, fake, None)
    for kw in (dict(dt=7), dict(cols=2), dict(c64=2), dict(P=0), dict(P=17), dict(N=1 << 31), dict(nx=15), dict(c=None),
               dict(res=None)):
        assert call(**kw) == _lib.WFS_EINVAL, kw
    assert call(N=0) == _lib.WFS_OK
