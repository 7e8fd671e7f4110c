"""GPU TensorEvaluator / RealMetricPairTables (csrc/metricpairs.hip, psd/tensor_evaluator.py, psd/metric_pairs.py) against
values RECORDED from the reference's own functions (tests/golden/tensor_evaluator_cases.npz, made by
tests/golden/make_tensor_evaluator_goldens.py).  Nothing here reads the reference tree.

Bounds: every count exactly; mean, dev, pair sums and per-PMT sums within 1e-5 of the recorded output's largest magnitude
(tests/tensor_evaluator_cases.compare).  The integer state is compared exactly where it must scale or repeat.  The
LitWaveform loop is held against the NumPy restatement of tests/tensor_evaluator_cases.py fed the module's own
``last_test_outputs``, at the same bounds."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import tensor_evaluator_cases as tc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16, i64=torch.int64)
WORST = {}


@pytest.fixture(scope="module")
def gold():
    return tc.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n_valid_of(b):
    return None if int(b["n_valid"]) < 0 else torch.tensor(int(b["n_valid"]), dtype=torch.int64, device=DEV)


def make(gold, name, **kw):
    from waveformml_amd.psd.tensor_evaluator import TensorEvaluator
    return TensorEvaluator(DEV, **dict(tc.constructor_kwargs(gold, name), **kw))


def add(ev, b, dtype):
    ev.add(dev(b["c"]), None, dev(b["target"]).to(TORCH_DTYPE[dtype]), dev(b["results"]), n_valid=n_valid_of(b))


def run_case(gold, name, ev=None):
    ev = make(gold, name) if ev is None else ev
    for b in tc.batches_of(gold, name):
        add(ev, b, tc.dtype_of(gold, name))
    return ev


TENSOR_CASES = ["det_i32", "det_i64", "xyz_i32", "xyz_i64", "one_row", "outside_grid_det", "outside_grid_xyz", "one_pmt",
                "two_adds_f32", "two_adds_bf16", "two_adds_f16", "single_float", "single_float_f16", "single_index",
                "class_i64", "edges_f32", "edges_bf16", "edges_f16", "padded", "res_zero", "res_constant",
                "res_near_constant", "res_low_bits", "res_negative", "res_n123"]


@pytest.mark.parametrize("name", TENSOR_CASES)
def test_tables_equal_the_recorded_reference(gold, name):
    assert sorted(TENSOR_CASES) == sorted(tc.case_names(gold, "tensor"))
    ev = run_case(gold, name)
    names, nbins, ranges, _C = tc.metrics_of(gold, name)
    assert ev.metric_names == names and ev.metric_pairs.n_bins == nbins
    assert np.array_equal(np.array(ev.normalized_ranges), np.array(ranges))
    res = ev.results()
    assert sorted(res) == sorted(["metrics", "pairs", ev.det_name, "scale_factor"])
    assert res["scale_factor"] == float(gold[name + "_metric_table"][0, 5])
    tc.compare(tc.expected(gold, name), name, res, names, ev.det_name, worst=WORST)
    print("largest error / scale so far:", WORST)
    b = tc.batches_of(gold, name)[-1]
    if int(b["n_valid"]) >= 0:                                        # the rows behind n_valid: category -1, zeros
        nv = int(b["n_valid"])
        assert (ev.category.cpu().numpy()[nv:] == -1).all() and (ev.category.cpu().numpy()[:nv] == 0).all()
        assert (ev.parameters.cpu().numpy()[:, nv:] == 0).all()
    if name == "res_constant":
        assert all(np.abs(res["metrics"][n][2]).max() == 0 for n in names)         # dev exactly 0


PAIR_CASES = ["dispatch_C2", "dispatch_C3"]


@pytest.mark.parametrize("name", PAIR_CASES)
def test_real_metric_pair_tables_on_both_sides_of_the_lds_edge(gold, name):
    from waveformml_amd.psd.metric_pairs import RealMetricPairTables
    assert PAIR_CASES == tc.case_names(gold, "pairs")
    names, nbins, ranges, C = tc.metrics_of(gold, name)
    mp = RealMetricPairTables(DEV, [(n, r[0], r[1], k) for n, r, k in zip(names, ranges, nbins)], ["c%d" % i for i in range(C)])
    assert sum(C * (k + 2) for k in nbins) == (1024 if C == 2 else 1536)             # MPR_LDS_CELLS = 1024
    for b in tc.batches_of(gold, name):
        mp.add(dev(b["params"]), dev(b["results"]), dev(b["category"]), n_valid=n_valid_of(b))
    res = mp.results()
    tc.compare(tc.expected(gold, name), name, res, names, worst=WORST)
    if C == 3:                                                        # both sides of the edge keep the same integers
        two = RealMetricPairTables(DEV, [(n, r[0], r[1], k) for n, r, k in zip(names, ranges, nbins)], ["c0", "c1"])
        for b in tc.batches_of(gold, name):
            two.add(dev(b["params"]), dev(b["results"]), dev(b["category"]))
        a, at2, at3 = two.tables.cpu().numpy(), 0, 0
        t3 = mp.tables.cpu().numpy()
        for key, shape, tabs in mp._layout:
            size3 = int(np.prod(shape))
            size2 = size3 // 3 * 2
            for k in range(tabs):
                assert np.array_equal(t3[at3:at3 + size3].reshape(shape)[:2].reshape(-1), a[at2:at2 + size2]), (key, k)
                at2, at3 = at2 + size2, at3 + size3
        assert at2 == len(a) and at3 == len(t3)


def test_reset_between_runs_and_two_runs_bit_identical(gold):
    ev = run_case(gold, "two_adds_f32")
    first = [t.clone() for t in ev.state_tensors()]
    assert len(first) == 2 and all(t.dtype == torch.int64 for t in first)
    ev.reset()
    assert all(int(t.abs().sum()) == 0 for t in ev.state_tensors())
    run_case(gold, "two_adds_f32", ev)
    assert all(torch.equal(a, b) for a, b in zip(first, ev.state_tensors()))
    ev.reset()
    run_case(gold, "det_i32", ev)                                     # the same constructor arguments
    tc.compare(tc.expected(gold, "det_i32"), "det_i32", ev.results(), ev.metric_names, ev.det_name)


def test_row_order_does_not_change_the_state(gold):
    b = tc.batches_of(gold, "res_negative")[0]
    perm = np.random.default_rng(3).permutation(len(b["results"]))
    a, p = make(gold, "res_negative"), make(gold, "res_negative")
    add(a, b, "f32")
    add(p, {k: (v[perm] if k != "n_valid" else v) for k, v in b.items()}, "f32")
    for x, y in zip(a.state_tensors(), p.state_tensors()):
        assert torch.equal(x, y)


def test_tiled_batch_scales_every_integer_exactly(gold):
    """26240 copies of a 40-row case as one batch of 1 049 600 rows: the accumulate's 1024 workgroups take 256 elements
    per pass and four grid-stride passes and a bit, the row kernel runs 4100 workgroups; n, S and the limbs of Q are K
    times the small batch's, exactly."""
    b = tc.batches_of(gold, "res_low_bits")[0]
    K = 26240
    small = make(gold, "res_low_bits")
    add(small, b, "f32")
    big = make(gold, "res_low_bits")
    add(big, {k: (np.concatenate([v] * K) if k != "n_valid" else v) for k, v in b.items()}, "f32")
    assert len(b["results"]) * K > 1024 * 1024
    for s, t in zip(small.state_tensors(), big.state_tensors()):
        assert torch.equal(s * K, t)
    tc.compare(tc.expected(gold, "res_low_bits"), "res_low_bits", big.results(), big.metric_names, big.det_name, scale=K)


@pytest.mark.parametrize("bad,match", [(float("nan"), "no fixed-point image"), (32768.0, "no fixed-point image"),
                                       (float("-inf"), "no fixed-point image")])
def test_a_result_without_an_image_raises(gold, bad, match):
    b = {k: v.copy() for k, v in tc.batches_of(gold, "det_i32")[0].items()}
    b["results"][5] = bad
    ev = make(gold, "det_i32")
    add(ev, b, "f32")
    with pytest.raises(RuntimeError, match=match):
        ev.results()
    ev.reset()
    b["results"][5] = np.float32(32767.998)                           # the largest fp32 below 2^15 has an image
    add(ev, b, "f32")
    assert ev.results()[ev.det_name][1].sum() == 48


def test_constructor_and_add_refuse_what_they_do_not_support(gold):
    from waveformml_amd.psd.tensor_evaluator import TensorEvaluator
    with pytest.raises(RuntimeError, match="calgroup"):
        TensorEvaluator(DEV, calgroup="x")
    with pytest.raises(RuntimeError, match="must pass the target index"):
        TensorEvaluator(DEV, target_has_phys=True)
    ev = make(gold, "det_i32")
    b = tc.batches_of(gold, "det_i32")[0]
    with pytest.raises(RuntimeError, match="target must be"):
        ev.add(dev(b["c"]), None, dev(b["target"][:, 0]), dev(b["results"]))
    with pytest.raises(RuntimeError, match="detector numbers"):
        ev.add(dev(b["c"]).float(), None, dev(b["target"]), dev(b["results"]))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ev.add(torch.from_numpy(b["c"]), None, dev(b["target"]), dev(b["results"]))
    assert all(int(t.abs().sum()) == 0 for t in ev.state_tensors())
    ev.add(dev(b["c"]).reshape(-1, 1), None, dev(b["target"]), dev(b["results"]))   # a column of detector numbers
    tc.compare(tc.expected(gold, "det_i32"), "det_i32", ev.results(), ev.metric_names, ev.det_name)


def _module(phys):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.litwaveform import LitWaveform
    with open(os.path.join(ROOT, "config", "waveform_tcn_z.json")) as f:
        cfg = json.load(f)
    cfg["optimize_config"].pop("scheduler_class", None)
    cfg["evaluation_config"] = {"bin_overrides": {"0": [0.0, 12.0, 6], "7": [0.0, 1176.0, 9]}}
    if phys:
        cfg["dataset_config"]["test_dataset_params"] = {"label_name": "phys"}
    torch.manual_seed(11)
    return LitWaveform(DictionaryUtility.to_object(cfg)).to(DEV)


@pytest.mark.parametrize("phys", [False, True], ids=["label_index", "phys"])
def test_lit_waveform_test_loop_fills_the_tables(phys):
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.tensor_evaluator import TensorEvaluator
    mod = _module(phys)
    ev = mod.evaluator
    assert isinstance(ev, TensorEvaluator) and ev is mod.evaluator and ev.target_has_phys == phys
    assert ev.target_index == 7 and ev.metric_name == "mean absolute error" and ev.P == (8 if phys else 1)
    assert ev.metric_pairs.n_bins == ([6, 100, 100, 100, 100, 100, 100, 9] if phys else [9])
    g = torch.Generator().manual_seed(5)
    loader = []
    for n in (300, 257, 1):
        c = torch.randint(0, 330, (n,), generator=g, dtype=torch.int32)
        y = torch.rand((n, 8) if phys else (n,), generator=g) * 1.2 - 0.1
        loader.append(([c, torch.rand(n, 59, generator=g)], y))
    plain = segment_test_loop(mod, copy.deepcopy(loader), DEV)
    out = segment_test_loop(mod, copy.deepcopy(loader), DEV, evaluator=ev)
    assert sorted(plain) == ["rows", "test_loss"] and sorted(out) == ["evaluation", "rows", "test_loss"]
    assert out["test_loss"] == plain["test_loss"] and out["rows"] == 558
    host = tc.HostTensorTables(ev.metric_pairs.n_bins, ev.normalized_ranges, ev.metric_names, ev.metric_name)
    total = 0.0
    for i, ((c, f), y) in enumerate(copy.deepcopy(loader)):
        res = mod.test_step(([c.to(DEV), f.to(DEV)], y.to(DEV)), i)
        cc, ff, target, results = mod.last_test_outputs
        assert results.shape == (len(c),) and results.dtype == torch.float32 and target.shape == y.shape
        assert abs(float(results.mean()) - float(res["test_loss"])) <= 1e-6 * float(res["test_loss"])
        host.add(cc.cpu().numpy(), target.cpu().numpy(), results.cpu().numpy())
        total += float(results.double().sum())
    assert abs(total / 558 - out["test_loss"]) <= 1e-6 * out["test_loss"]
    res = out["evaluation"]
    want = host.results()
    assert res[ev.det_name][1].sum() == want[ev.det_name][1].sum() < 558          # some detector numbers beyond 307
    assert res["metrics"][ev.metric_names[0]][1].sum() == 558
    tc.compare(tc.as_expected(want, ev.metric_names, ev.det_name), "loop", res, ev.metric_names, ev.det_name, worst=WORST)
    print("largest error / scale so far:", WORST)
