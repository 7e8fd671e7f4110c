"""GPU PIDEvaluator / MetricPairTables / PSDEvaluator(metric_pairs=True) (csrc/metricpairs.hip, psd/pid_evaluator.py,
psd/metric_pairs.py) against values RECORDED from the reference's own functions (tests/golden/pid_evaluator_cases.npz, made
by tests/golden/make_pid_evaluator_goldens.py).  Nothing here reads the reference tree.

Bounds: every integer table exactly; the (mean, dev) of the 1-D triples to 1e-12 (they are derived from exact integers).
The LitSegClassifier loop is held against the NumPy restatement of tests/pid_evaluator_cases.py (exactly, integers)."""
import copy
import os

import numpy as np
import pytest
import torch

import evaluator_cases as ec
import pid_evaluator_cases as pc
from test_segment_callers import IONI

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)


@pytest.fixture(scope="module")
def gold():
    return pc.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n_valid_of(b):
    return None if int(b["n_valid"]) < 0 else torch.tensor(int(b["n_valid"]), dtype=torch.int64, device=DEV)


def make_pid(gold, **kw):
    from waveformml_amd.psd.pid_evaluator import PIDEvaluator
    return PIDEvaluator(DEV, seg_status=gold["seg_status"], **kw)


def add_pid(ev, b, dtype, **kw):
    ev.add(dev(b["pred"]), dev(b["targ"]), dev(b["coords"]), [dev(b["phys"]).to(TORCH_DTYPE[dtype])],
           n_valid=n_valid_of(b), **kw)


def check_pairs(gold, name, res, names, scale=1):
    for i, mname in enumerate(names):
        mean, n, devi = res["metrics"][mname]
        assert n.dtype == np.int64 and np.array_equal(n, scale * gold["%s_m%d_n" % (name, i)]), (name, mname)
        assert np.abs(mean - gold["%s_m%d_mean" % (name, i)]).max() <= 1e-12, (name, mname)
        if scale == 1:
            assert np.abs(devi - gold["%s_m%d_dev" % (name, i)]).max() <= 1e-12, (name, mname)
    P = len(names)
    assert sorted(res["pairs"]) == sorted("%d_%d" % (i, j) for i in range(P - 1) for j in range(i + 1, P))
    for key, (val, n) in res["pairs"].items():
        assert val.dtype == np.float64 and n.dtype == np.int64
        assert np.array_equal(n, scale * gold["%s_p%s_n" % (name, key)]), (name, key)
        assert np.array_equal(val, (scale * gold["%s_p%s_val" % (name, key)]).astype(np.float64)), (name, key)


def check_pid(gold, name, res, scale=1):
    for k in ("SE_confusion", "confusion_SE", "confusion_energy"):
        assert res[k].dtype == np.int64 and np.array_equal(res[k], scale * gold["%s_%s" % (name, k)]), (name, k)
    check_pairs(gold, name, res["metric_pairs"], [str(n) for n in gold["metric_names"]], scale)


PID_CASES = ["one_row", "last_event_se", "seven_se", "padded", "empty_class", "one_class", "all_wrong", "two_adds_f32",
             "two_adds_bf16", "two_adds_f16", "edges_f32", "edges_bf16", "edges_f16"]


@pytest.mark.parametrize("name", PID_CASES)
def test_pid_tables_equal_the_recorded_reference(gold, name):
    assert sorted(PID_CASES) == sorted(pc.case_names(gold, "pid"))
    ev = make_pid(gold)
    dtype = str(gold[name + "_dtype"])
    for k, b in enumerate(pc.batches_of(gold, name)):
        add_pid(ev, b, dtype)
        nv = len(b["coords"]) if int(b["n_valid"]) < 0 else int(b["n_valid"])
        rec = gold["%s_b%d_rows" % (name, k)]
        for j, t in enumerate((ev.accuracy, ev.multiplicity, ev.se_mask, ev.n_SE)):
            assert np.array_equal(t.cpu().numpy()[:nv], rec[j]), (name, j)
        assert (ev.category.cpu().numpy()[nv:] == -1).all()
    check_pid(gold, name, ev.results())


def test_pid_n_events_given_and_reset(gold):
    ev = make_pid(gold)
    for b in pc.batches_of(gold, "two_adds_f32"):
        add_pid(ev, b, "f32", n_events=int(b["coords"][:, 2].max()) + 1)
    check_pid(gold, "two_adds_f32", ev.results())
    ev.reset()
    assert all(int(t.abs().sum()) == 0 for t in ev.state_tensors())
    add_pid(ev, pc.batches_of(gold, "seven_se")[0], "f32")
    check_pid(gold, "seven_se", ev.results())
    ev.add(None, None, None, None)                                      # the reference returns at once
    check_pid(gold, "seven_se", ev.results())


def test_pid_batch_of_many_blocks_is_the_small_batch_many_times(gold):
    """110 copies of the 14-row case as one batch of 1540 rows: more than one workgroup of the row kernel (256 rows) and
    more than one slice of the pair kernel (1024 elements); every count is 110 times the recorded one."""
    b = pc.batches_of(gold, "seven_se")[0]
    K, E = 110, int(b["coords"][:, 2].max()) + 1
    big = {k: np.concatenate([b[k]] * K) for k in ("pred", "targ", "phys")}
    big["coords"] = np.concatenate([b["coords"] + np.array([0, 0, k * E], np.int32) for k in range(K)])
    big["n_valid"] = b["n_valid"]
    ev = make_pid(gold)
    add_pid(ev, big, "f32")
    check_pid(gold, "seven_se", ev.results(), scale=K)


PAIR_CASES = ["psd_edges", "psd_skipped", "psd_empty_class", "dispatch_C2", "dispatch_C3"]


@pytest.mark.parametrize("name", PAIR_CASES)
def test_metric_pair_tables_equal_the_recorded_reference(gold, name):
    from waveformml_amd.psd.metric_pairs import MetricPairTables
    assert sorted(PAIR_CASES) == sorted(pc.case_names(gold, "pairs"))
    nb, rg, C = gold[name + "_nbins"], gold[name + "_ranges"], int(gold[name + "_C"])
    names = ["m%d" % i for i in range(len(nb))]
    mp = MetricPairTables(DEV, [(n, float(r[0]), float(r[1]), int(k)) for n, r, k in zip(names, rg, nb)],
                          ["c%d" % i for i in range(C)])
    assert np.array_equal(np.array(mp.ranges), rg)
    for b in pc.batches_of(gold, name):
        mp.add(dev(b["params"]), dev(b["result"]), dev(b["category"]), n_valid=n_valid_of(b))
    check_pairs(gold, name, mp.results(), names)
    if name == "dispatch_C3":                                           # both sides of the LDS / direct edge agree
        assert np.array_equal(gold["dispatch_C2_p0_1_n"], mp.results()["pairs"]["0_1"][1][:2])
        assert np.array_equal(gold["dispatch_C2_m0_n"], mp.results()["metrics"]["m0"][1][:2])


def test_metric_pair_tables_flags_and_explicit_ranges(gold):
    from waveformml_amd.psd.metric_pairs import MetricPairTables
    mp = MetricPairTables(DEV, [("a", 0.0, 1.0, 4), ("b", -1.0, 1.0, 2)], ["x", "y"])
    par = dev(np.array([[0.1, 0.6, 0.9], [0.0, 0.5, 2.0]], np.float32))
    mp.add(par, dev(np.array([1, 0, 1], np.int32)), dev(np.array([0, 1, -1], np.int32)), ranges=[(0.0, 2.0), (0.0, 1.0)])
    r = mp.results()
    assert r["metrics"]["a"][1].tolist() == [[0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]]
    assert r["pairs"]["0_1"][1][1, 2, 2] == 1 and r["pairs"]["0_1"][0].sum() == 1.0
    with pytest.raises(RuntimeError, match="int32"):
        mp.add(par, dev(np.array([1., 0., 1.], np.float32)), dev(np.array([0, 1, -1], np.int32)))
    mp.add(par, dev(np.array([1, 0, 1], np.int32)), dev(np.array([0, 2, -1], np.int32)))
    with pytest.raises(RuntimeError, match="category"):
        mp.results()
    mp.reset()
    mp.add(par, dev(np.array([1, 2, 1], np.int32)), dev(np.array([0, 1, -1], np.int32)))
    with pytest.raises(RuntimeError, match="neither 0 nor 1"):
        mp.results()


def _psd_batches(eg):
    def batch_of(b):
        return ([dev(eg["tab%d_coords" % b]), dev(eg["tab%d_pulses" % b])], dev(eg["tab%d_labels" % b]))
    return [(batch_of(b), dev(eg["tab%d_predictions" % b])) for b in range(2)]


def test_psd_evaluator_metric_pairs_on_the_existing_table_batches(gold):
    from waveformml_amd.psd.evaluator import PSDEvaluator
    eg = ec.load_golden()
    names = ["Gamma", "Neutron", "Other"]
    ev = PSDEvaluator(names, DEV, gains=eg["gains"], seg_status=eg["seg_status"], n_samples=20, metric_pairs=True)
    plain = PSDEvaluator(names, DEV, gains=eg["gains"], seg_status=eg["seg_status"], n_samples=20)
    assert [str(n) for n in gold["psd_metric_names"]] == ev.metric_pairs.names
    assert np.array_equal(np.array(ev.metric_pairs.ranges), gold["psd_ranges"]) and ev.metric_pairs.n_bins == list(gold["psd_nbins"])
    for batch, pred in _psd_batches(eg):
        ev.add(batch, None, pred)
        plain.add(batch, None, pred)
    res, base = ev.results(), plain.results()
    assert len(res["metric_pairs"]["metrics"]) == 9 and len(res["metric_pairs"]["pairs"]) == 36
    check_pairs(gold, "psd_tab", res["metric_pairs"], ev.metric_pairs.names)
    # without the flag: the keys of before, the same numbers, nothing new allocated or launched
    assert sorted(res) == sorted(list(base) + ["metric_pairs"]) and "metric_pairs" not in base
    for k in base:
        for x, y in zip(base[k] if isinstance(base[k], tuple) else (base[k],), res[k] if isinstance(res[k], tuple) else (res[k],)):
            assert np.array_equal(x, y), k
    assert plain.metric_pairs is None and len(plain.state_tensors()) == 3 and len(ev.state_tensors()) == 4
    assert not hasattr(plain, "_match")
    ev.reset()
    assert int(ev.metric_pairs.tables.abs().sum()) == 0


def test_psd_evaluator_without_the_flag_returns_todays_keys():
    from waveformml_amd.psd.evaluator import PSDEvaluator, result_shapes
    eg = ec.load_golden()
    names = ["Gamma", "Neutron", "Other"]
    ev = PSDEvaluator(names, DEV, gains=eg["gains"], seg_status=eg["seg_status"], n_samples=20)
    for batch, pred in _psd_batches(eg):
        ev.add(batch, None, pred)
    want = sorted(list(result_shapes(names)) + ["summed_waveforms", "n_wfs", "summed_labelled_waveforms", "n_labelled_wfs"])
    assert sorted(ev.results()) == want


@pytest.mark.parametrize("what", ["unsorted", "outside_grid", "label_5", "event_outside"])
def test_each_flag_bit_raises(gold, what):
    b = {k: v.copy() for k, v in pc.batches_of(gold, "two_adds_f32")[0].items()}
    kw = {}
    if what == "unsorted":
        b["coords"][[0, -1], 2] = b["coords"][[-1, 0], 2]
        match = "not sorted"
    elif what == "outside_grid":
        b["coords"][3, 0] = 14
        match = "outside the detector grid"
    elif what == "label_5":
        b["targ"][2] = 5
        match = "outside the five PID classes"
    else:
        kw["n_events"] = int(b["coords"][:, 2].max())
        match = "outside the batch"
    ev = make_pid(gold)
    add_pid(ev, b, "f32", **kw)
    with pytest.raises(RuntimeError, match=match):
        ev.results()


def _ioni_module_and_loader():
    from torch.utils.data import DataLoader
    from waveformml_amd.psd import data as psd_data, h5data
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litseg import LitSegClassifier
    root = os.path.join(HERE, "golden", "h5", "r3", "ioni")
    label_map = {"1": 0, "4": 1, "6": 2, "256": 3, "258": 2, "512": 4}
    ds = h5data.HDF5Dataset([root], "*WaveformPairSim.h5", "WaveformPairs", "coord", "waveform", 12, label_name="PID",
                            label_map=label_map, normalize=True, additional_fields=["phys"])
    (c0, f0), _y0 = ds[0]
    assert isinstance(f0, list) and f0[1].shape[1] == 8                   # the fixture's table carries phys
    cfg = copy.deepcopy(IONI)
    cfg["net_config"]["imports"] = ["waveformml_amd.spconv" if m == "oracle.spconv" else m for m in cfg["net_config"]["imports"]]
    cfg["system_config"]["n_samples"] = int(f0[0].shape[1]) // 2
    cfg["dataset_config"]["test_dataset_params"] = {"additional_fields": ["phys"]}
    torch.manual_seed(3)
    mod = LitSegClassifier(load_config(cfg)).to(DEV)
    loader = list(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=psd_data.collate_fn))
    return mod, loader


def test_lit_seg_classifier_test_loop_fills_the_pid_tables(gold):
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.pid_evaluator import PIDEvaluator
    mod, loader = _ioni_module_and_loader()
    assert isinstance(mod.evaluator, PIDEvaluator) and mod.evaluator is mod.evaluator
    assert mod.evaluator.additional_field_names == ["phys"]
    plain = segment_test_loop(mod, copy.deepcopy(loader), DEV)
    out = segment_test_loop(mod, copy.deepcopy(loader), DEV, evaluator=mod.evaluator)
    assert sorted(plain) == ["rows", "test_acc", "test_loss"] and sorted(out) == sorted(list(plain) + ["evaluation"])
    assert abs(out["test_loss"] - plain["test_loss"]) <= 1e-6 * abs(plain["test_loss"]) and out["test_acc"] == plain["test_acc"]
    # the same tables on the host, from the predictions the module makes
    host = pc.HostPIDTables(mod.evaluator.seg_status.cpu().numpy(), mod.evaluator.metric_pairs.n_bins,
                            mod.evaluator.normalized_ranges, mod.evaluator.E_scale)
    hits = rows = 0
    for i, ((c, f), y) in enumerate(copy.deepcopy(loader)):
        mod.test_step(([c.to(DEV), [t.to(DEV) for t in f]], y.to(DEV)), i)
        pred, target, cc, fields = mod.last_test_outputs
        assert len(fields) == 1 and fields[0].shape == (len(c), 8)
        host.add(cc.cpu().numpy(), pred.cpu().numpy(), target.cpu().numpy(), fields[0].cpu().numpy())
        hits += int((pred == target).sum())
        rows += len(c)
    res = out["evaluation"]
    assert rows == out["rows"] and abs(hits / rows - out["test_acc"]) < 1e-6
    assert res["confusion_SE"].sum() > 0 and res["confusion_energy"].sum() > 0
    for k in ("SE_confusion", "confusion_SE", "confusion_energy"):
        assert np.array_equal(res[k], getattr(host, k)), k
    names = mod.evaluator.metric_names
    for i, n in enumerate(names):
        assert np.array_equal(res["metric_pairs"]["metrics"][n][1], host.pairs.n1[i]), n
        m = host.pairs.m1[i]
        assert np.abs(res["metric_pairs"]["metrics"][n][0] * host.pairs.n1[i] - m).max() < 1e-9, n
    for (i, j), n in host.pairs.n2.items():
        val, num = res["metric_pairs"]["pairs"]["%d_%d" % (i, j)]
        assert np.array_equal(num, n) and np.array_equal(val, host.pairs.m2[(i, j)].astype(np.float64)), (i, j)


def test_two_runs_give_bit_identical_state(gold):
    states = []
    for _ in range(2):
        ev = make_pid(gold)
        for name in ("two_adds_f32", "edges_f32", "padded"):
            for b in pc.batches_of(gold, name):
                add_pid(ev, b, "f32")
        states.append([t.cpu() for t in ev.state_tensors()])
    assert len(states[0]) == 2
    for a, b in zip(*states):
        assert a.dtype == torch.int64 and torch.equal(a, b)
