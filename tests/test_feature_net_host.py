"""``ExtractedFeatureConv`` / ``ExtractedFeatureConvNet`` (psd/blocks.py, psd/featurenet.py) without a GPU: the builder
against the layer lists the REFERENCE's own constructor produced for the same arguments
(tests/golden/feature_net_schedules.json, made by tests/golden/make_feature_net_goldens.py with a recording stand-in for
spconv), the net on the CPU oracle operators, and ``LitPSD.evaluator``'s choice by dataset class."""
import copy
import json
import os

import pytest
import torch

from test_block_schedules import _build, _layers_of, _recording_spconv

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "feature_net_schedules.json")) as _f:
    GOLD = json.load(_f)


def config_dict(cpu=True):
    with open(os.path.join(ROOT, "config", "psd_features_det.json")) as fh:
        cfg = json.load(fh)
    if cpu:
        cfg["net_config"]["imports"] = ["oracle.spconv" if m == "waveformml_amd.spconv" else m
                                        for m in cfg["net_config"]["imports"]]
    cfg["dataset_config"]["base_path"] = os.path.join(HERE, "golden", "h5", "det")
    return cfg


def test_golden_covers_what_it_should():
    ok = [c for c in GOLD if c["error"] is None]
    assert {c["args"]["n"] for c in ok} == {2, 3, 5}
    assert all(c["error"] == "AssertionError" for c in GOLD if c["args"]["n"] == 1) and len(ok) == len(GOLD) - 24
    assert any(c["args"].get("dropout") for c in ok) and any(c["args"].get("stride_factor") == 2 for c in ok)
    assert any(c["args"].get("pad_factor") == 1.0 for c in ok) and any(not c["args"].get("pad_factor") for c in ok)
    convs = [l for c in ok for l in c["layers"] if l["cls"] == "SparseConv2d"]
    assert any(l["args"][7] is True for l in convs) and all(l["args"][2] >= 2 for l in convs)      # bias slot; fs >= 2
    assert any(l["args"][3] == 2 for l in convs) and any(l["args"][4] > 0 for l in convs)
    for c in ok:                                                               # the repeated second channel count
        cs = [l for l in c["layers"] if l["cls"] == "SparseConv2d"]
        assert cs[1]["args"][0] == cs[1]["args"][1] == cs[0]["args"][1]


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_builder_matches_the_recorded_reference(n):
    from waveformml_amd.psd.blocks import ExtractedFeatureConv
    cases = [c for c in GOLD if c["args"]["n"] == n]
    assert len(cases) == 24
    for case in cases:
        a = dict(case["args"])
        a["size"] = list(a["size"])
        blk, err = _build(lambda: ExtractedFeatureConv(_recording_spconv(), **a))
        assert err == case["error"], a
        if err is None:
            assert _layers_of(blk.alg) == case["layers"], a
            assert [int(v) for v in blk.out_size] == case["out_size"], a
            assert blk.schedule[-1]["out_size"] == case["out_size"] and len(blk.schedule) == n


def test_net_builds_from_the_config_and_runs_on_the_cpu_oracle():
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.featurenet import ExtractedFeatureConvNet
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(0)
    mod = LitPSD(load_config(config_dict()))
    net = mod.model
    assert isinstance(net, ExtractedFeatureConvNet) and net.nfeatures == 7
    assert [(s["nin"], s["nout"], s["kernel"], s["padding"]) for s in net.schedule] == [(7, 42, 3, 2), (42, 42, 2, 0),
                                                                                         (42, 29, 2, 0)]
    assert net.n_linear == 14 * 11 * 29 and net.linear[-1].out_features == 2
    keys = list(net.state_dict())
    assert "model.network.0.weight" in keys and "linear.0.weight" in keys and not any("sparseModel" in k for k in keys)
    assert net.model.network[0].bias is None                                   # trainable_weights=False in the bias slot
    c = torch.tensor([[1, 2, 0], [3, 4, 0], [13, 10, 1], [0, 0, 2]], dtype=torch.int32)
    f = torch.rand(4, 7)
    net.eval()
    out = net([c, f])
    assert out.shape == (3, 2) and torch.equal(out, net([c, f, None]))
    loss = mod.training_step(([c, f], torch.tensor([0, 1, 1])), 0)
    loss.backward()
    assert all(p.grad is not None for p in net.parameters())


def test_net_type_is_checked():
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.featurenet import ExtractedFeatureConvNet
    cfg = config_dict()
    cfg["net_config"]["net_type"] = "3DConvolution"
    with pytest.raises(IOError, match="must be 2DConvolution"):
        ExtractedFeatureConvNet(load_config(cfg))
    import waveformml_amd.psd.ExtractedFeatureConvNet as alias
    assert alias.ExtractedFeatureConvNet is ExtractedFeatureConvNet


class _Stub:
    def __init__(self, names, device, **kw):
        self.names, self.device, self.kw = names, device, kw


def test_lit_psd_picks_the_evaluator_by_dataset_class(monkeypatch):
    import waveformml_amd.psd.evaluator as ev_mod
    import waveformml_amd.psd.phys_evaluator as phys_mod
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.lit import LitPSD
    phys, psd = type("Phys", (_Stub,), {}), type("Psd", (_Stub,), {})
    monkeypatch.setattr(phys_mod, "PhysEvaluator", phys)
    monkeypatch.setattr(ev_mod, "PSDEvaluator", psd)
    ev = LitPSD(load_config(config_dict())).evaluator
    assert type(ev) is phys and ev.names == ["Gamma", "Neutron"] and ev.device == torch.device("cpu")
    assert ev.kw == {"spectra": True, "bin_overrides": {"0": [0.0, 10.0, 100]}}                # evaluation_config
    cfg = config_dict()
    del cfg["evaluation_config"]
    cfg["dataset_config"]["dataset_class"] = "src.datasets.PulseDataset.PulseDatasetDet"       # the last component counts
    cfg["dataset_config"]["imports"] = []
    assert LitPSD(load_config(cfg)).evaluator.kw == {}
    for other in ("PulseDataset.PulseDataset2D", "PulseDataset.PulseDatasetWaveformNorm", "SyntheticPulseDataset",
                  "PulseDataset.PulseDatasetDetX"):
        cfg = config_dict()
        cfg["dataset_config"]["dataset_class"] = other
        ev = LitPSD(load_config(copy.deepcopy(cfg))).evaluator
        assert type(ev) is psd and ev.kw == {"n_samples": 150}, other
    cfg = config_dict()
    del cfg["system_config"]["type_names"]
    assert LitPSD(load_config(cfg)).evaluator is None
