"""Host-side checks of the dense conv front end (psd/convnet.py, psd/waveform.py ConvWaveformNet / LinearWaveformNet):
the plans, module trees and state_dict layouts against tests/golden/conv1d_plans.json (recorded from the reference's own
classes by tests/golden/make_conv1d_goldens.py), the reference's error cases, the CPU path of Conv1DNet(fused=True), a
CPU training step of LitWaveform on config/waveform_cnn_z.json, and the C ABI's new entries."""
import copy
import json
import os

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "conv1d_plans.json")) as _f:
    GOLD = json.load(_f)

_ERRORS = {"OSError": IOError, "AttributeError": AttributeError}


def _state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _linears(seq):
    return [[m.in_features, m.out_features] for m in seq if isinstance(m, nn.Linear)]


def _config(n_samples, net_config, hparams):
    from waveformml_amd.psd.config import DictionaryUtility
    return DictionaryUtility.to_object({"system_config": {"n_samples": n_samples},
                                        "net_config": dict(copy.deepcopy(net_config), hparams=copy.deepcopy(hparams))})


def _check_conv(net, rec):
    convs = [m for m in net.network if isinstance(m, nn.Conv1d)]
    assert [convs[0].in_channels] + [c.out_channels for c in convs] == rec["planes"] == net.planes
    assert [[c.kernel_size[0], c.stride[0], c.padding[0]] for c in convs] == rec["layers"]
    assert [c.bias is not None for c in convs] == rec["bias"]
    assert list(net.out_size) == rec["out_size"]
    assert [type(m).__name__ for m in net.network] == rec["modules"]
    assert _state(net) == rec["state"]


@pytest.mark.parametrize("rec", GOLD["conv1d"], ids=[str(i) for i in range(len(GOLD["conv1d"]))])
def test_conv1d_plan_and_module_tree_match_the_reference(rec):
    from waveformml_amd.psd.convnet import Conv1DNet, conv1d_plan
    planes, layers, out_size = conv1d_plan(**rec["args"])
    assert planes == rec["planes"] and out_size == rec["out_size"]
    assert [list(l[:3]) for l in layers] == rec["layers"] and layers[-1][3] == rec["out_size"][0]
    net = Conv1DNet(**rec["args"])
    assert not net.fused
    _check_conv(net, rec)
    # the recorded lengths are what the convolutions produce
    net.eval()
    with torch.no_grad():
        y = net(torch.zeros(2, rec["args"]["num_channels"], rec["args"]["length"]))
    assert list(y.shape) == [2, rec["out_size"][1], rec["out_size"][0]]


def test_the_goldens_cover_the_quirks():
    args = [r["args"] for r in GOLD["conv1d"]]
    assert any(a["num_expand"] + a["num_contract"] == 1 for a in args)                       # n == 1
    assert {0, 3} <= {a.get("stride_factor", 0) for a in args}
    assert any(l[0] == r["args"].get("min_kernel", 2) and r["args"].get("size_factor", 3) < l[0]
               for r in GOLD["conv1d"] for l in r["layers"])                                # a clamped kernel
    assert any(r["planes"] == [2, 8, 6, 5] for r in GOLD["conv1d"])                          # 6.5 rounds to even
    dets = [r["net_config"].get("use_detector_number") for r in GOLD["conv_nets"] if r["raises"] is None]
    assert True in dets and None in dets


@pytest.mark.parametrize("rec", GOLD["conv_nets"], ids=[str(i) for i in range(len(GOLD["conv_nets"]))])
def test_conv_waveform_net_matches_the_reference(rec):
    from waveformml_amd.psd.WaveformModels import ConvWaveformNet
    cfg = _config(rec["n_samples"], rec["net_config"], rec["hparams"])
    if rec["raises"]:
        with pytest.raises(_ERRORS[rec["raises"]]):
            ConvWaveformNet(cfg)
        return
    net = ConvWaveformNet(cfg)
    assert net.model.fused and net.takes_n_valid and net.n_valid is None
    assert net.num_inputs == rec["num_inputs"]
    _check_conv(net.model, rec["conv"])
    if rec["linears"] is None:
        assert not hasattr(net, "linear")
    else:
        assert _linears(net.linear.net) == rec["linears"]
        assert [type(m).__name__ for m in net.linear.net] == rec["linear_modules"]
    assert _state(net) == rec["state"]


@pytest.mark.parametrize("rec", GOLD["linear_nets"], ids=[str(i) for i in range(len(GOLD["linear_nets"]))])
def test_linear_waveform_net_matches_the_reference(rec):
    from waveformml_amd.psd.WaveformModels import LinearWaveformNet
    cfg = _config(rec["n_samples"], {"net_type": "Linear"}, rec["hparams"])
    if rec["raises"]:
        with pytest.raises(_ERRORS[rec["raises"]]):
            LinearWaveformNet(cfg)
        return
    net = LinearWaveformNet(cfg)
    if rec["kind"] == "LinearPlanes":
        assert _linears(net.linear.net) == rec["linears"]
        assert [type(m).__name__ for m in net.linear.net] == rec["linear_modules"]
        assert _state(net) == rec["state"]
    else:
        # the reference keeps a LinearBlock OBJECT there (no registered parameter: its recorded state_dict is empty,
        # and the object cannot be called); here its Sequential is the module, same widths
        assert rec["state"] == [] and _linears(net.linear) == rec["linears"]
        assert [k for k, _s in _state(net)] == ["linear.%d.%s" % (i, p) for i in range(len(rec["linears"]))
                                                 for p in ("weight", "bias")]
    y = net(torch.zeros(3, 1, rec["n_samples"]))
    assert list(y.shape) == [3, 1, rec["linears"][-1][1]]


def test_fused_flag_on_cpu_tensors_is_the_torch_composition_bit_for_bit():
    from waveformml_amd.psd import convnet
    kw = GOLD["conv1d"][0]["args"]
    a = convnet.Conv1DNet(fused=True, **kw)
    b = convnet.Conv1DNet(**kw)
    b.load_state_dict(a.state_dict())
    x = torch.randn(5, 1, kw["length"])
    before = convnet.CONV1D_CALLS[0]
    for mode in (True, False):
        a.train(mode), b.train(mode)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = a(xa), b.network(xb)
        ya.sum().backward(), yb.sum().backward()
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), k
    assert convnet.CONV1D_CALLS[0] == before
    with pytest.raises(RuntimeError):          # a valid-row count cannot be honoured by the torch composition
        a(x, n_valid=torch.tensor([3]))


def test_lit_waveform_takes_a_cpu_training_step_on_the_cnn_config():
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.litwaveform import LitWaveform
    from waveformml_amd.psd.waveform import ConvWaveformNet
    with open(os.path.join(ROOT, "config", "waveform_cnn_z.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(ROOT, "config", "waveform_tcn_z.json")) as f:
        tcn = json.load(f)
    for key in ("optimize_config", "dataset_config"):
        assert cfg[key] == tcn[key]
    torch.manual_seed(0)
    m = LitWaveform(DictionaryUtility.to_object(cfg)).train()
    assert isinstance(m.model, ConvWaveformNet) and m.squeeze_index == 1
    assert m.model.model.planes == [1, 8, 16, 12, 8]
    assert m.model.model.layers == [(5, 1, 2, 59), (4, 1, 1, 58), (2, 1, 0, 57), (2, 2, 0, 28)]
    assert _linears(m.model.linear.net) == [[224, 112], [112, 1]]
    g = torch.Generator().manual_seed(1)
    batch = ([torch.zeros(16, 1, dtype=torch.int32), torch.rand(16, 59, generator=g)], torch.rand(16, generator=g))
    loss = m.training_step(batch, 0)
    loss.backward()
    assert torch.isfinite(loss) and m.model.n_valid is None
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.model.parameters())
    assert int(m.model.model.network[1].num_batches_tracked) == 1
    assert float(m.model.model.network[1].running_mean.abs().max()) > 0


def test_the_conv1d_entries_are_in_the_binding():
    from waveformml_amd import _lib
    for name in ("wfs_conv1d_ok", "wfs_conv1d_saved_floats", "wfs_conv1d_bwd_workspace_floats", "wfs_conv1d_fwd",
                 "wfs_conv1d_bwd"):
        assert name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "wfsparse.h")) as f:
        header = f.read()
    for name, (_res, args) in _lib.SIGNATURES.items():
        if name.startswith("wfs_conv1d_"):
            decl = header[header.index(name + "("):]
            assert decl[: decl.index(")")].count(",") + 1 == len(args), name
    assert _lib.WFS_ABI_VERSION == 6
