"""GPU PhysEvaluator (csrc/physstats.hip, psd/phys_evaluator.py) against values RECORDED from the reference's own functions
(tests/golden/phys_evaluator_cases.npz, made by tests/golden/make_phys_evaluator_goldens.py).  Nothing here reads the
reference tree.

Bounds: every per-event output within 1e-5 of that output's own scale (its largest recorded magnitude over the case), the
multiplicity exactly; integer tables and spectra exactly; derived means and deviations to 1e-12.  The block-boundary batches
have no recording and are held against the NumPy restatement in tests/phys_evaluator_cases.py, which
tests/test_phys_evaluator_host.py holds against the recording bit for bit."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import phys_evaluator_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)


@pytest.fixture(scope="module")
def gold():
    return pc.load_golden()


def names_of(gold):
    return [str(n) for n in gold["class_names"]]


def make(gold, **kw):
    from waveformml_amd.psd.phys_evaluator import PhysEvaluator
    return PhysEvaluator(names_of(gold), DEV, **kw)


def batch_of(coords, feats, labels, dtype=torch.float32):
    return ([torch.from_numpy(np.ascontiguousarray(coords)).to(DEV),
             torch.from_numpy(np.ascontiguousarray(feats)).to(DEV).to(dtype)], torch.from_numpy(labels).to(DEV))


def table_batches(gold):
    return [(batch_of(gold["tab%d_coords" % b], gold["tab%d_feats" % b], gold["tab%d_labels" % b]),
             torch.from_numpy(gold["tab%d_predictions" % b]).to(DEV)) for b in range(2)]


def flat(res):
    """Every array of a results() dict under a path name."""
    out = {}

    def walk(prefix, v):
        if isinstance(v, dict):
            for k in v:
                walk(prefix + "/" + str(k), v[k])
        elif isinstance(v, tuple):
            for i, a in enumerate(v):
                out["%s/%d" % (prefix, i)] = a
        elif isinstance(v, np.ndarray):
            out[prefix] = v
    walk("", res)
    return out


def same_results(a, b):
    fa, fb = flat(a), flat(b)
    assert sorted(fa) == sorted(fb)
    for k in fa:
        assert fa[k].dtype == fb[k].dtype and np.array_equal(fa[k], fb[k]), k


def check_events(ev, avg_coo, features, multiplicity, tag):
    """The bar of the per-event outputs: 1e-5 of each output's largest recorded magnitude; multiplicity exact."""
    got_feat = ev.features.cpu().numpy().astype(np.float64)
    worst = {"avg_coo": np.abs(ev.avg_coo.cpu().numpy() - avg_coo).max() / max(np.abs(avg_coo).max(), 1e-30)}
    for k, name in enumerate(pc.FEATURES[:7]):
        ref = np.asarray(features[k], np.float64)
        worst[name] = np.abs(got_feat[k] - ref).max() / max(np.abs(ref).max(), 1e-30)
    print(tag, {k: float("%.3g" % v) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-5, (k, v)
    assert ev.multiplicity.cpu().tolist() == [int(m) for m in multiplicity]
    assert got_feat[7].tolist() == [float(m) for m in multiplicity]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_event_outputs_match_the_recorded_reference(gold, dtype):
    tag = "stats_%s_" % dtype
    E = len(gold[tag + "multiplicity"])
    ev = make(gold)
    zeros = torch.zeros(E, dtype=torch.int64, device=DEV)
    batch = batch_of(gold[tag + "coords"], gold[tag + "feats"], np.zeros(E, np.int64), TORCH_DTYPE[dtype])
    assert np.array_equal(batch[0][1].float().cpu().numpy(), gold[tag + "feats"])       # the reference saw these very values
    before = [batch[0][0].clone(), batch[0][1].clone(), batch[1].clone(), zeros.clone()]
    ev.add(batch, None, zeros)
    for t, b in zip([batch[0][0], batch[0][1], batch[1], zeros], before):
        assert torch.equal(t, b)                                                        # the caller's tensors are only read
    check_events(ev, gold[tag + "avg_coo"], gold[tag + "features"], gold[tag + "multiplicity"], tag)
    assert gold[tag + "multiplicity"].tolist() == [1, 2, 17, 65, 0, 0, 0]
    feat, coo = ev.features.cpu().numpy(), ev.avg_coo.cpu().numpy()
    # beyond the bar: the sums are IEEE operations in a fixed order, so every bit is the reference's -- a product contracted
    # into the sum that takes it (an fma) shows here as a last-place difference and nowhere else
    assert np.array_equal(feat[:7], gold[tag + "features"]) and np.array_equal(coo, gold[tag + "avg_coo"])
    # energy 0 and negative: the un-normalised sums stay, energy and multiplicity 0; no rows: zeros
    assert feat[0, 4] == 0 and feat[0, 5] == 0 and np.any(feat[1:7, 4] != 0) and np.any(coo[5] != 0)
    assert not feat[:, 6].any() and not coo[6].any()
    ev.results()                                                                        # no error flag was raised


def test_hand_computed_event_keeps_the_float64_energy(gold):
    ev = make(gold)
    one = torch.zeros(1, dtype=torch.int64, device=DEV)
    ev.add(batch_of(gold["hand_coords"], gold["hand_feats"], np.zeros(1, np.int64)), None, one)
    coo = ev.avg_coo.cpu().numpy()
    assert coo[0, 0] == 150994950.0 / 50331651.0 and coo[0, 1] == (4 * 50331648.0 + 6 * 50331651.0) / 50331651.0
    assert np.array_equal(coo, gold["hand_avg_coo"])
    assert np.array_equal(ev.features.cpu().numpy()[:7], gold["hand_features"]) and ev.multiplicity.cpu().tolist() == [2]


def expect_tables(res, gold, vname):
    names = names_of(gold)
    exact = ["confusion_energy", "confusion_SE"]
    pairs = ["pos_acc", "ene_psd_acc"] + ["ene_psd_prec_" + n for n in names]
    triples = ["mult_acc", "ene_acc"] + [p + n for n in names for p in ("ene_prec_", "mult_prec_")]
    assert sorted(exact + pairs + triples) == sorted(str(k) for k in gold["result_keys"])
    for k in exact:
        assert res[k].dtype == np.int64 and np.array_equal(res[k], gold["%s_%s_0" % (vname, k)]), k
    for k in pairs:                                                                     # sums of 0/1: exact in fp64
        for i in (0, 1):
            assert np.array_equal(res[k][i], gold["%s_%s_%d" % (vname, k, i)]), (k, i)
        assert not res[k][2].any()
    for k in triples:
        assert res[k][1].dtype == np.int64 and np.array_equal(res[k][1], gold["%s_%s_1" % (vname, k)]), k
        for i in (0, 2):                                                                # mean and finalized deviation
            ref = gold["%s_%s_%d" % (vname, k, i)]
            assert np.all(np.abs(res[k][i] - ref) <= 1e-12 * np.maximum(np.abs(ref), 1.0)), (k, i)


def expect_spectra(res, gold, vname):
    rec = gold[vname + "_spectra"]
    for s, side in enumerate(("by_truth", "by_prediction")):
        for c, name in enumerate(names_of(gold)):
            for f, fname in enumerate(pc.FEATURES):
                got = res["spectra"][side][name][fname]
                nb = pc.SPECTRUM_BINS[f][2]
                assert got.dtype == np.int64 and got.shape == (nb + 2,)
                assert np.array_equal(got, rec[s, c, f, :nb + 2]), (side, name, fname)


@pytest.mark.parametrize("vname", ["tab", "tabk"])
def test_tables_and_spectra_after_two_batches(gold, vname):
    from waveformml_amd.psd.evaluator import result_shapes
    emin, n_mult = gold[vname + "_params"]
    ev = make(gold, spectra=True, emin=float(emin), n_mult=int(n_mult))
    for batch, pred in table_batches(gold):
        ev.add(batch, None, pred)
    if vname == "tab":
        check_events(ev, gold["tab1_avg_coo"], gold["tab1_features"], gold["tab1_multiplicity"], "tab1")
    res = ev.results()
    shapes = result_shapes(ev.class_names, n_mult=int(n_mult))
    assert sorted(k for k in res if k not in ("features", "feature_names", "spectra")) == sorted(shapes)
    for k, shape in shapes.items():
        for a in (res[k] if isinstance(res[k], tuple) else (res[k],)):
            assert a.shape == shape, k
    assert res["feature_names"] == pc.FEATURES                                          # and the last batch's matrix
    assert res["features"].dtype == np.float32 and np.array_equal(res["features"], ev.features.cpu().numpy())
    assert np.array_equal(res["features"][:7], gold["tab1_features"])
    expect_tables(res, gold, vname)
    expect_spectra(res, gold, vname)
    assert not res["confusion_SE"].any() and not res["ene_acc"][1].any()              # never filled by PhysEvaluator.add
    assert res["mult_acc"][1].sum() == 61 and res["ene_psd_acc"][1].sum() == 61
    assert not res["mult_prec_Never"][1].any() and res["confusion_energy"][:, 3].sum() == 0
    total = sum(res["mult_prec_" + n][1] for n in ev.class_names)
    assert np.array_equal(total, res["mult_acc"][1])                                    # the classes partition the events
    # without spectra the tables are the same and the key is absent
    plain = make(gold, emin=float(emin), n_mult=int(n_mult))
    for batch, pred in table_batches(gold):
        plain.add(batch, None, pred)
    pres = plain.results()
    assert "spectra" not in pres
    same_results({k: v for k, v in res.items() if k != "spectra"}, pres)


@pytest.mark.parametrize("E", [7, 257])
def test_block_boundary_one_row_events(E):
    """E = 257: one event past a 256-thread accumulate block and past 64 four-event statistics blocks."""
    from waveformml_amd.psd.phys_evaluator import PhysEvaluator
    rng = np.random.default_rng(1000 + E)
    cells = rng.integers(0, 14 * 11, E)
    coords = np.column_stack([cells // 11, cells % 11, np.arange(E)]).astype(np.int32)
    # values on a coarse dyadic grid, away from every edge: k / 1024 + 1 / 4096
    feats = (rng.integers(40, 700, (E, 7)) / 1024.0 + 1.0 / 4096.0).astype(np.float32)
    labels = rng.integers(0, 3, E).astype(np.int64)
    pred = rng.integers(0, 3, E).astype(np.int64)
    ev = PhysEvaluator(["a", "b", "c"], DEV, spectra=True)
    ev.add(batch_of(coords, feats, labels), None, torch.from_numpy(pred).to(DEV))
    avg, feat, mult = pc.event_averages(coords, feats, E)
    check_events(ev, avg, feat, mult, "E%d" % E)
    assert mult.tolist() == [1] * E
    host = pc.HostTables(3, spectra=True)
    host.add(avg, feat, mult, pred, labels)
    res = ev.results()
    cur = ev.tables.cpu().numpy()
    at = 0
    for name, shape in ev._layout:
        n = int(np.prod(shape))
        assert np.array_equal(cur[at:at + n].reshape(shape), host.t[name]), name
        at += n
    assert res["mult_acc"][1][1] == E
    for s, side in enumerate(("by_truth", "by_prediction")):
        for c, name in enumerate(ev.class_names):
            for f, fname in enumerate(pc.FEATURES):
                assert np.array_equal(res["spectra"][side][name][fname], host.spectra[s][c][f]), (side, name, fname)


def test_padding_determinism_reset(gold):
    batches = table_batches(gold)
    ev = make(gold, spectra=True)
    for batch, pred in batches:
        ev.add(batch, None, pred)
    first = ev.results()
    # the same batches inside capacity-padded buffers, garbage beyond n_valid
    pad = make(gold, spectra=True)
    g = torch.Generator(device="cpu").manual_seed(3)
    for ((coords, feats), labels), pred in batches:
        n, cap = coords.shape[0], coords.shape[0] + 77
        pc_ = torch.randint(-5, 100, (cap, 3), generator=g, dtype=torch.int32).to(DEV)
        pf = (torch.rand((cap, 7), generator=g) * 1e6).to(DEV)
        pc_[:n], pf[:n] = coords, feats
        pad.add(([pc_, pf, torch.tensor([n], dtype=torch.int64, device=DEV)], labels), None, pred)
    same_results(first, pad.results())
    # a second run, and a run after reset(), give the same bits
    again = make(gold, spectra=True)
    for batch, pred in batches:
        again.add(batch, None, pred)
    same_results(first, again.results())
    assert all(torch.equal(a, b) for a, b in zip(ev.state_tensors(), again.state_tensors()))
    ev.reset()
    assert all(not t.any() for t in ev.state_tensors())
    cleared = ev.results()
    assert all(np.count_nonzero(a) == 0 for a in flat(cleared).values()) and cleared["features"].shape == (8, 0)
    for batch, pred in batches:
        ev.add(batch, None, pred)
    same_results(first, ev.results())


def test_flags_and_argument_checks(gold):
    (batch, pred) = table_batches(gold)[0]
    (coords, feats), labels = batch
    ev = make(gold)
    shuffled = coords.clone()
    shuffled[:, 2] = torch.flip(coords[:, 2], dims=[0])
    ev.add(([shuffled, feats], labels), None, pred)
    with pytest.raises(RuntimeError, match="not sorted"):
        ev.results()
    ev = make(gold)
    bad = pred.clone()
    bad[3] = len(ev.class_names)
    ev.add(batch, None, bad)
    with pytest.raises(RuntimeError, match="outside class_names"):
        ev.results()
    ev = make(gold)
    with pytest.raises(RuntimeError, match=r"\[N, 7\]"):
        ev.add(([coords, torch.zeros((coords.shape[0], 300), device=DEV)], labels), None, pred)
    with pytest.raises(RuntimeError, match="int64"):
        ev.add(batch, None, pred.int())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.add(([coords.cpu(), feats.cpu()], labels.cpu()), None, pred.cpu())
    assert not ev.tables.any()


def det_setup():
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    with open(os.path.join(ROOT, "config", "psd_features_det.json")) as fh:
        cfg = json.load(fh)
    cfg["dataset_config"]["base_path"] = os.path.join(HERE, "golden", "h5", "det")
    torch.manual_seed(0)
    config = load_config(copy.deepcopy(cfg))
    mod = LitPSD(config).to(DEV)
    mod.eval()
    dm = PSDDataModule(config, DEV)
    dm.setup("test")
    return mod, [b for b in dm.test_dataloader()]


def test_captured_test_loop_equals_the_eager_loop_on_the_det_fixture():
    from waveformml_amd.psd.evaluate import test_loop
    from waveformml_amd.psd.phys_evaluator import PhysEvaluator
    mod, batches = det_setup()
    assert len(batches) >= 2
    ev = mod.evaluator
    assert isinstance(ev, PhysEvaluator) and ev.spectra is not None           # evaluation_config asks for the spectra
    eager = test_loop(mod, batches, DEV, capture=False, evaluator=ev)
    ev.reset()
    captured = test_loop(mod, batches, DEV, capture=True, evaluator=ev)
    assert eager["events"] == captured["events"] == sum(int(b[1].shape[0]) for b in batches)
    assert eager["test_loss"] == captured["test_loss"] and eager["test_acc"] == captured["test_acc"]
    same_results(eager["evaluation"], captured["evaluation"])
    assert eager["evaluation"]["mult_acc"][1].sum() == eager["events"]
