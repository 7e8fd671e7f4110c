"""The recording behind the GPU PhysEvaluator tests (tests/golden/phys_evaluator_cases.npz, made from the reference's own
functions by tests/golden/make_phys_evaluator_goldens.py) and the NumPy restatement in tests/phys_evaluator_cases.py,
without a GPU: the recording's own edge conditions and coverage, the restatement against it bit for bit, the closed-form
(mean, n, deviation) triples, result keys and shapes, and the argument checks that need no device."""
import numpy as np
import pytest
import torch

import phys_evaluator_cases as pc
from evaluator_cases import bin_edges


@pytest.fixture(scope="module")
def gold():
    return pc.load_golden()


def names_of(gold):
    return [str(n) for n in gold["class_names"]]


def test_defaults_are_psd_evaluators_with_emax_10(gold):
    import inspect
    from waveformml_amd.psd.phys_evaluator import PhysEvaluator
    sig = inspect.signature(PhysEvaluator.__init__).parameters
    for k, v in pc.DEFAULTS.items():
        assert float(gold["default_" + k]) == float(v) == float(sig[k].default), k
    assert sig["emax"].default == 10.0 and sig["spectra"].default is False
    assert np.array_equal(gold["spectrum_bins"], np.array(pc.SPECTRUM_BINS, np.float64))


def test_no_recorded_value_is_near_an_edge_it_is_not_on(gold):
    """The condition under which integer tables can be compared exactly, checked on the REFERENCE's values."""
    def clear(v, lo, hi, nb):
        d = np.abs(np.asarray(v, np.float64)[:, None] - bin_edges(lo, hi, nb)[None, :]).min(axis=1)
        return bool(np.all((d > 1e-4) | (d == 0)))
    for emin in (0.0, 0.5):
        for b in range(2):
            tag = "tab%d_" % b
            feat, coo = gold[tag + "features"], gold[tag + "avg_coo"]
            assert clear(feat[0], emin, 10.0, 100) and clear(feat[0], 0.0, 10.0, 10) and clear(feat[1], 0.0, 0.6, 100)
            assert clear(coo[:, 0], 0.0, 14.0, 14) and clear(coo[:, 1], 0.0, 11.0, 11)
            for k, (lo, hi, nb) in enumerate(pc.SPECTRUM_BINS[:7]):
                assert clear(feat[k], lo, hi, nb), k


def test_recording_covers_the_cases(gold):
    en = np.concatenate([gold["tab0_features"][0], gold["tab1_features"][0]])
    mu = np.concatenate([gold["tab0_multiplicity"], gold["tab1_multiplicity"]])
    assert en.dtype == np.float32 and (en == np.float32(10.0)).any() and (en > 10).any()      # at emax exactly, above it
    assert ((en > 0) & (en < 0.5)).any()                                                       # below emin = 0.5 (tabk)
    assert (mu > 10).any() and (mu == 0).sum() >= 6 and mu[len(gold["tab0_multiplicity"]) - 1] == 0
    assert gold["tabk_params"].tolist() == [0.5, 6.0] and gold["tab_params"].tolist() == [0.0, 10.0]
    labels = np.concatenate([gold["tab0_labels"], gold["tab1_labels"]])
    preds = np.concatenate([gold["tab0_predictions"], gold["tab1_predictions"]])
    assert set(labels.tolist()) == {0, 1, 2} == set(preds.tolist()) and len(names_of(gold)) == 4
    assert 0 < (labels == preds).sum() < len(labels)
    for dtype in ("f32", "bf16", "f16"):
        tag = "stats_%s_" % dtype
        assert gold[tag + "multiplicity"].tolist() == [1, 2, 17, 65, 0, 0, 0]
        counts = np.bincount(gold[tag + "coords"][:, 2], minlength=7)
        assert counts.tolist() == [1, 2, 17, 65, 3, 2, 0]
        f = torch.from_numpy(gold[tag + "feats"])
        td = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[dtype]
        assert torch.equal(f.to(td).float(), f)                                                # values of that format
    assert not np.array_equal(gold["stats_bf16_feats"], gold["stats_f32_feats"])


def test_hand_computed_event(gold):
    """numba's float64 energy sum, shown on two rows of energies 3 * 2^24 and 3 (the generator's docstring)."""
    assert float(np.float32(50331648.0) + np.float32(3.0)) == 50331652.0
    assert gold["hand_avg_coo"][0, 0] == 150994950.0 / 50331651.0
    assert gold["hand_avg_coo"][0, 0] != (50331648.0 + 2 * 50331652.0) / 50331652.0
    avg, feat, mult = pc.event_averages(gold["hand_coords"], gold["hand_feats"], 1)
    assert np.array_equal(avg, gold["hand_avg_coo"]) and np.array_equal(feat[:7], gold["hand_features"])
    assert mult.tolist() == [2]


@pytest.mark.parametrize("tag", ["stats_f32_", "stats_bf16_", "stats_f16_", "tab0_", "tab1_"])
def test_restatement_equals_the_recording_bit_for_bit(gold, tag):
    E = len(gold[tag + "multiplicity"])
    avg, feat, mult = pc.event_averages(gold[tag + "coords"], gold[tag + "feats"], E)
    assert np.array_equal(avg, gold[tag + "avg_coo"])
    assert feat.dtype == np.float32 and np.array_equal(feat[:7], gold[tag + "features"])
    assert np.array_equal(mult, gold[tag + "multiplicity"].astype(np.int32))
    assert np.array_equal(feat[7], gold[tag + "multiplicity"].astype(np.float32))


@pytest.mark.parametrize("vname", ["tab", "tabk"])
def test_host_tables_equal_the_recording(gold, vname):
    from waveformml_amd.psd.metric_pairs import triple_1d
    emin, n_mult = gold[vname + "_params"]
    names = names_of(gold)
    host = pc.HostTables(len(names), spectra=True, emin=float(emin), n_mult=int(n_mult))
    for b in range(2):
        tag = "tab%d_" % b
        avg, feat, mult = pc.event_averages(gold[tag + "coords"], gold[tag + "feats"], len(gold[tag + "labels"]))
        host.add(avg, feat, mult, gold[tag + "predictions"], gold[tag + "labels"])
    t = host.t
    rec = lambda k, i: gold["%s_%s_%d" % (vname, k, i)]                                        # noqa: E731
    assert np.array_equal(t["confusion_energy"], rec("confusion_energy", 0))
    assert not rec("confusion_SE", 0).any() and not rec("ene_acc", 1).any()                    # never filled
    for k in ("pos", "ene_psd"):
        assert np.array_equal(t[k + "_n"], rec(k + "_acc", 1)) and np.array_equal(t[k + "_m"], rec(k + "_acc", 0))
    triples = [("mult_acc", t["mult_m"], t["mult_n"])]
    for c, name in enumerate(names):
        assert np.array_equal(t["ene_psd_prec"][c, 0], rec("ene_psd_prec_" + name, 1))
        assert np.array_equal(t["ene_psd_prec"][c, 1], rec("ene_psd_prec_" + name, 0))
        triples.append(("ene_prec_" + name, t["ene_prec"][c, 1], t["ene_prec"][c, 0]))
        triples.append(("mult_prec_" + name, t["mult_prec"][c, 1], t["mult_prec"][c, 0]))
    for key, m, n in triples:
        mean, cnt, dev = triple_1d(m, n)
        assert np.array_equal(cnt, rec(key, 1)), key
        for got, i in ((mean, 0), (dev, 2)):                                   # Welford in sequence vs the closed form
            assert np.all(np.abs(got - rec(key, i)) <= 1e-12 * np.maximum(np.abs(rec(key, i)), 1.0)), (key, i)
    assert (rec("mult_acc", 2) > 0).any()
    spectra = gold[vname + "_spectra"]
    for s in range(2):
        for c in range(len(names)):
            for f, (_lo, _hi, nb) in enumerate(pc.SPECTRUM_BINS):
                assert np.array_equal(host.spectra[s][c][f], spectra[s, c, f, :nb + 2]), (s, c, f)
                assert not spectra[s, c, f, nb + 2:].any()
    assert spectra[0].sum() == spectra[1].sum() == 8 * 61 and not spectra[:, 3].any()


def test_result_keys_and_shapes(gold):
    from waveformml_amd.psd.evaluator import result_shapes
    shapes = result_shapes(names_of(gold))
    assert sorted(shapes) == [str(k) for k in gold["result_keys"]]
    for k, shape in shapes.items():
        assert gold["tab_%s_0" % k].shape == shape, k
    assert result_shapes(names_of(gold), n_mult=6)["mult_prec_Gamma"] == gold["tabk_mult_prec_Gamma_0"].shape == (8,)


def test_spectrum_bins_and_argument_checks():
    from waveformml_amd.psd import phys_evaluator as pe
    assert pe.spectrum_bins() == pc.SPECTRUM_BINS and pe.FEATURE_NAMES == pc.FEATURES
    over = pe.spectrum_bins({"0": [0.0, 10.0, 50], 2: [0.0, 4000.0, 80]})
    assert over[0] == (0.0, 10.0, 50) and over[3] == over[4] == (0.0, 4000.0, 80) and over[1] == pc.SPECTRUM_BINS[1]
    assert over[7] == (-0.5, 20.5, 21)
    with pytest.raises(IOError, match="must be integers"):
        pe.spectrum_bins({"energy": [0, 1, 2]})
    with pytest.raises(RuntimeError, match="no CPU path"):
        pe.PhysEvaluator(["a", "b"], "cpu")
