"""GPU PSDEvaluator (csrc/evalstats.hip, psd/evaluator.py) against values RECORDED from the reference's own functions
(tests/golden/evaluator_cases.npz, made by tests/golden/make_evaluator_goldens.py).  Nothing here reads the reference tree.

Bounds: every per-event output within 1e-5 of that output's own scale (its largest recorded magnitude over the case);
integer tables exactly; accuracy means and M2 to 1e-12; summed waveforms to 1e-5 of their maximum."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import evaluator_cases as ec

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)


@pytest.fixture(scope="module")
def gold():
    return ec.load_golden()


def make(gold, T, names=("Gamma", "Neutron", "Other"), **kw):
    from waveformml_amd.psd.evaluator import PSDEvaluator
    return PSDEvaluator(list(names), DEV, gains=gold["gains"], seg_status=gold["seg_status"], n_samples=T, **kw)


def batch_of(coords, pulses, labels, dtype=torch.float32):
    return ([torch.from_numpy(np.ascontiguousarray(coords)).to(DEV),
             torch.from_numpy(np.ascontiguousarray(pulses)).to(DEV).to(dtype)], torch.from_numpy(labels).to(DEV))


def table_batches(gold):
    return [(batch_of(gold["tab%d_coords" % b], gold["tab%d_pulses" % b], gold["tab%d_labels" % b]),
             torch.from_numpy(gold["tab%d_predictions" % b]).to(DEV)) for b in range(2)]


def same_results(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        for x, y in zip(a[k] if isinstance(a[k], tuple) else (a[k],), b[k] if isinstance(b[k], tuple) else (b[k],)):
            assert x.dtype == y.dtype and np.array_equal(x, y), k


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("T", [20, 150])
def test_event_statistics_match_the_recorded_reference(gold, T, dtype):
    tag = "stats_T%d_%s_" % (T, dtype)
    ev = make(gold, T)
    zeros = torch.zeros(7, dtype=torch.int64, device=DEV)
    batch = batch_of(gold[tag + "coords"], gold[tag + "pulses"], np.zeros(7, np.int64), TORCH_DTYPE[dtype])
    assert np.array_equal(batch[0][1].float().cpu().numpy(), gold[tag + "pulses"])     # the reference saw these very values
    before = batch[0][1].clone()
    ev.add(batch, None, zeros)
    assert torch.equal(batch[0][1], before)                                             # rows are only read
    got = dict(avg_coo=ev.avg_coo, summed=ev.summed_pulses, psdl=ev.psdl, psdr=ev.psdr, energy=ev.energy)
    worst = {}
    for k, v in got.items():
        ref = gold[tag + k].astype(np.float64)
        worst[k] = np.abs(v.cpu().numpy().astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30)
    stats = ev.output_stats.cpu().numpy().astype(np.float64)
    for k, name in enumerate(ec.METRIC_NAMES[3:]):
        ref = gold[tag + "stats"][k].astype(np.float64)
        worst[name] = np.abs(stats[k] - ref).max() / max(np.abs(ref).max(), 1e-30)
    print(tag, {k: float("%.3g" % v) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-5, (k, v)
    assert ev.multiplicity.cpu().tolist() == gold[tag + "multiplicity"].tolist()
    assert ev.n_SE.cpu().tolist() == gold[tag + "n_SE"].tolist() and gold[tag + "n_SE"][-1] == 0
    # the special rows of the case: an event without charge, and an all-zero row, leave exact zeros where the reference does
    assert float(ev.energy[1]) == 0 and float(ev.psdl[1]) == 0 and ev.avg_coo[1].cpu().tolist() == [0.0, 0.0]
    feat = ev.features.cpu().numpy()
    assert np.array_equal(feat[0], ev.energy.cpu().numpy()) and np.array_equal(feat[1], ev.psdl.cpu().numpy())
    assert feat[2].tolist() == [1, 2, 3, 5, 1, 17, 64] and np.array_equal(feat[3:], ev.output_stats.cpu().numpy())
    ev.results()                                                                        # no error flag was raised


def test_fix_last_event_n_se(gold):
    tag = "stats_T20_f32_"
    c = gold[tag + "coords"]
    true_last = int((gold["seg_status"][c[c[:, 2] == 6, 0], c[c[:, 2] == 6, 1]] == 0.5).sum())
    assert true_last > 0
    zeros = torch.zeros(7, dtype=torch.int64, device=DEV)
    batch = batch_of(c, gold[tag + "pulses"], np.zeros(7, np.int64))
    for fix, last in ((False, 0), (True, true_last)):
        ev = make(gold, 20, fix_last_event_n_SE=fix)
        ev.add(batch, None, zeros)
        assert ev.n_SE.cpu().tolist() == gold[tag + "n_SE"].tolist()[:-1] + [last]


def check_no_value_near_an_edge(gold):
    """The condition under which integer tables can be compared exactly, checked on the REFERENCE's values: no binned
    float lies within 1e-4 of a bin edge -- except the events built to sit exactly on `high`, whose recorded energy must
    then equal it bit for bit."""
    edges = dict(e=ec.bin_edges(0.0, 5.0, 100), c=ec.bin_edges(0.0, 5.0, 10), p=ec.bin_edges(0.0, 0.6, 100),
                 x=ec.bin_edges(0.0, 14.0, 14), y=ec.bin_edges(0.0, 11.0, 11))

    def dist(v, e):
        return np.abs(np.asarray(v, np.float64)[:, None] - e[None, :]).min(axis=1)
    for b in range(2):
        tag = "tab%d_" % b
        exact = gold[tag + "exact_energy"]
        en = gold[tag + "energy"]
        assert np.all(en[exact] == np.float32(5.0))
        assert np.all(dist(en[~exact], edges["e"]) > 1e-4) and np.all(dist(en[~exact], edges["c"]) > 1e-4)
        assert np.all(dist(gold[tag + "psdl"], edges["p"]) > 1e-4) and np.all(dist(gold[tag + "psdr"], edges["p"]) > 1e-4)
        assert np.all(dist(gold[tag + "avg_coo"][:, 0], edges["x"]) > 1e-4)
        assert np.all(dist(gold[tag + "avg_coo"][:, 1], edges["y"]) > 1e-4)
    en = np.concatenate([gold["tab0_energy"], gold["tab1_energy"]])
    assert (en < 0).any() and (en > 5).any() and (en == 5).any()                        # below low, above high, at high
    assert max(gold["tab0_multiplicity"].max(), gold["tab1_multiplicity"].max()) > 10


def test_tables_after_two_batches(gold):
    from waveformml_amd.psd.evaluator import result_shapes
    check_no_value_near_an_edge(gold)
    ev = make(gold, 20)
    for batch, pred in table_batches(gold):
        ev.add(batch, None, pred)
    res = ev.results()
    shapes = result_shapes(ev.class_names)
    assert sorted(k for k in res if k not in ("summed_waveforms", "n_wfs", "summed_labelled_waveforms",
                                              "n_labelled_wfs")) == sorted(shapes) == [str(k) for k in gold["result_keys"]]
    for k, shape in shapes.items():
        for a in (res[k] if isinstance(res[k], tuple) else (res[k],)):
            assert a.shape == shape, k
    for k in ("confusion_energy", "confusion_SE", "n_wfs", "n_labelled_wfs"):
        assert res[k].dtype == np.int64 and np.array_equal(res[k], gold["tab_" + k]), k
    assert res["confusion_energy"][:, 2].sum() == 0 and res["n_wfs"][3] == 0            # the class no event has
    assert np.array_equal(res["mult_acc"][1], gold["tab_mult_acc_1"])
    assert np.array_equal(res["ene_psd_acc"][1], gold["tab_ene_psd_acc_1"])
    assert np.array_equal(res["ene_psd_acc"][0], gold["tab_ene_psd_acc_0"])             # sums of 0/1: exact in fp64
    assert np.array_equal(res["pos_acc"][1], gold["tab_pos_acc_1"])
    assert np.array_equal(res["pos_acc"][0], gold["tab_pos_acc_0"])
    assert res["ene_psd_acc"][1].sum() == 2 * 61 and res["ene_psd_acc"][1][101].sum() > 0 and res["ene_psd_acc"][1][0].sum() > 0
    for i in (0, 2):                                                                    # mean and finalized M2
        ref = gold["tab_mult_acc_%d" % i]
        assert np.all(np.abs(res["mult_acc"][i] - ref) <= 1e-12 * np.maximum(np.abs(ref), 1.0)), i
    for k in ("summed_waveforms", "summed_labelled_waveforms"):
        ref = gold["tab_" + k].astype(np.float64)
        assert res[k].dtype == np.float32 and np.abs(res[k] - ref).max() <= 1e-5 * np.abs(ref).max(), k


def test_padding_determinism_reset(gold):
    batches = table_batches(gold)
    ev = make(gold, 20)
    for batch, pred in batches:
        ev.add(batch, None, pred)
    first = ev.results()
    # the same batches inside capacity-padded buffers, garbage beyond n_valid
    pad = make(gold, 20)
    g = torch.Generator(device="cpu").manual_seed(3)
    for ((coords, feats), labels), pred in batches:
        n, cap = coords.shape[0], coords.shape[0] + 77
        pc = torch.randint(-5, 100, (cap, 3), generator=g, dtype=torch.int32).to(DEV)
        pf = (torch.rand((cap, 40), generator=g) * 1e6).to(DEV)
        pc[:n], pf[:n] = coords, feats
        pad.add(([pc, pf, torch.tensor([n], dtype=torch.int64, device=DEV)], labels), None, pred)
    same_results(first, pad.results())
    # a second run, and a run after reset(), give the same bits
    again = make(gold, 20)
    for batch, pred in batches:
        again.add(batch, None, pred)
    same_results(first, again.results())
    ev.reset()
    empty = ev.results()
    assert all(np.count_nonzero(a) == 0 for v in empty.values() for a in (v if isinstance(v, tuple) else (v,)))
    for batch, pred in batches:
        ev.add(batch, None, pred)
    same_results(first, ev.results())


def test_one_event_batch_and_cpu_tensors(gold):
    tag = "stats_T20_f32_"
    rows = gold[tag + "coords"][:, 2] == 5
    c = gold[tag + "coords"][rows].copy()
    c[:, 2] = 0
    ev = make(gold, 20, fix_last_event_n_SE=True)
    one = np.ones(1, np.int64)
    ev.add(batch_of(c, gold[tag + "pulses"][rows], one), None, torch.from_numpy(one).to(DEV))
    assert ev.multiplicity.cpu().tolist() == [17]
    for k, v in dict(psdl=ev.psdl, energy=ev.energy).items():
        assert abs(float(v[0]) - float(gold[tag + k][5])) <= 1e-5 * abs(float(gold[tag + k][5])), k
    ref = gold[tag + "stats"][:, 5].astype(np.float64)
    assert np.all(np.abs(ev.output_stats[:, 0].cpu().numpy() - ref) <= 1e-5 * np.abs(gold[tag + "stats"]).max(axis=1))
    res = ev.results()
    counted = int(0.0 <= float(gold[tag + "energy"][5]) <= 5.0)                        # above `high` is not counted
    assert res["n_wfs"].tolist() == [17, 0, 17, 0] and res["confusion_energy"].sum() == counted
    assert res["mult_acc"][1].sum() == 1 and res["mult_acc"][1][11] == 1 and res["confusion_SE"].sum() <= 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.add(([torch.from_numpy(c), torch.from_numpy(gold[tag + "pulses"][rows])], torch.from_numpy(one)), None,
               torch.from_numpy(one))


@pytest.mark.parametrize("capture", [False, True])
def test_test_loop_with_an_evaluator(capture):
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import test_loop
    from waveformml_amd.psd.evaluator import PSDEvaluator
    from waveformml_amd.psd.lit import LitPSD
    with open(os.path.join(HERE, "golden", "gep_config.json")) as fh:
        cfg = json.load(fh)
    torch.manual_seed(0)
    mod = LitPSD(load_config(copy.deepcopy(cfg))).to(DEV)
    mod.eval()
    batches = []
    for s in range(3):
        c, f, y = synthetic.generate(8, 150, len(cfg["system_config"]["type_names"]), seed=70 + s, layout="2d")
        batches.append(([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV)], torch.from_numpy(y).to(DEV)))
    plain = test_loop(mod, batches, DEV, capture=capture)
    assert "evaluation" not in plain
    ev = mod.evaluator
    assert isinstance(ev, PSDEvaluator) and ev.class_names == list(cfg["system_config"]["type_names"])
    with_ev = test_loop(mod, batches, DEV, capture=capture, evaluator=ev)
    assert with_ev["test_loss"] == plain["test_loss"] and with_ev["test_acc"] == plain["test_acc"]
    direct = PSDEvaluator(ev.class_names, DEV, n_samples=150)
    with torch.no_grad():
        for (c, f), y in batches:
            logits = mod.model([c, f]).float()
            direct.add(([c, f], y), logits, torch.argmax(logits, dim=1))
    same_results(with_ev["evaluation"], direct.results())
    assert with_ev["evaluation"]["n_wfs"][0] == sum(int(b[0][0].shape[0]) for b in batches)
