"""Host side of the recurrent pulse net (psd/recurrent.py, RecurrentWaveformNet, config/waveform_rnn_z.json): class
resolution, the reference's state_dict and initialisation, the CPU twin (nn.RNN itself), the n_lin == 0 quirks, one CPU
training step from the pulse fixture, wfs_rnn_ok's bounds, and the live-parameter recipe of the GPU tests."""
import copy
import json
import os

import pytest
import torch

from recurrent_cases import CASES, assert_live, case_id, make_inputs, make_rnn, run_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    with open(os.path.join(ROOT, "config", "waveform_rnn_z.json")) as f:
        return json.load(f)


def _lit(cfg, seed=7):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.litwaveform import LitWaveform
    torch.manual_seed(seed)
    return LitWaveform(DictionaryUtility.to_object(copy.deepcopy(cfg)))


def _composition(seed=7):
    from waveformml_amd.psd.blocks import LinearBlock
    torch.manual_seed(seed)
    rnn = torch.nn.RNN(1, 4, 4, nonlinearity="relu", bias=False, batch_first=True)
    lin = LinearBlock(4 * 59, 1, 4).func
    return rnn, lin


def test_config_resolves_and_builds_the_reference_state_dict():
    from waveformml_amd.psd.config import ModuleUtility
    from waveformml_amd.psd import recurrent, waveform
    cfg = _cfg()
    util = ModuleUtility(cfg["net_config"]["imports"])
    assert util.retrieve_class("WaveformModels.RecurrentWaveformNet") is waveform.RecurrentWaveformNet
    from waveformml_amd.psd import RecurrentBlocks
    assert RecurrentBlocks.RecurrentNet is recurrent.RecurrentNet and RecurrentBlocks.RecurrentBlock is recurrent.RecurrentBlock
    lit = _lit(cfg)
    assert lit.squeeze_index == 2
    net = lit.model.model
    assert isinstance(net, recurrent.RecurrentNet) and net.rnn_block.fused and isinstance(net.rnn_block.rnn, torch.nn.RNN)
    rnn, lin = _composition()
    want = [("rnn_block.rnn." + k, v) for k, v in rnn.state_dict().items()] + [("linear." + k, v) for k, v in lin.state_dict().items()]
    got = list(net.state_dict().items())
    assert [k for k, _ in got] == [k for k, _ in want]
    assert [k for k, _ in got][:2] == ["rnn_block.rnn.weight_ih_l0", "rnn_block.rnn.weight_hh_l0"]
    for (k, a), (_k, b) in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b), k          # same seed: bit-equal initial parameters


def test_cpu_forward_is_the_torch_composition_and_never_touches_the_library():
    from waveformml_amd.psd import recurrent
    torch.manual_seed(3)
    net = recurrent.RecurrentNet(59, 1, 4, 4, 4, 1, bias=False, fused=True)
    rnn, lin = _composition(3)
    x = torch.rand(9, 59, 1)
    before = recurrent.RNN_CALLS[0]
    y = net(x)
    assert recurrent.RNN_CALLS[0] == before
    want = lin(torch.flatten(rnn(x)[0], 1))
    assert y.shape == (9, 1) and torch.equal(y, want)
    out, hidden = net.rnn_block(x)
    ro, rh = rnn(x)
    assert torch.equal(out, ro) and torch.equal(hidden, rh)
    assert net.rnn_block.init_hidden(5).shape == (4, 5, 4)


def test_n_lin_zero_branches_and_wrong_net_type():
    from waveformml_amd.psd import recurrent
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.waveform import RecurrentWaveformNet
    torch.manual_seed(1)
    x = torch.rand(5, 7, 1)
    net = recurrent.RecurrentNet(7, 1, 3, 2, 0, 1)
    assert net.linear is None
    flat = torch.flatten(net.rnn_block.rnn(x)[0], 1)
    y = net(x)
    assert y.shape == (5,) and torch.equal(y, flat[:, -1])           # the last element of the FLATTENED output
    with pytest.raises(IOError, match="must have n_lin > 0 if out_size is > 1"):
        recurrent.RecurrentNet(7, 1, 3, 2, 0, 2)(x)
    cfg = _cfg()
    cfg["net_config"]["net_type"] = "LSTM"
    with pytest.raises(IOError, match="LSTM not supported net type"):
        RecurrentWaveformNet(DictionaryUtility.to_object(cfg))


def test_one_cpu_training_step_on_the_pulse_fixture():
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    cfg = _cfg()
    cfg["system_config"]["n_samples"] = 12                  # the fixture's pulses are 12 samples long
    dc = cfg["dataset_config"]
    dc["base_path"] = os.path.join(ROOT, "tests", "golden", "h5", "r3")
    dc["paths"] = ["pulses"]
    dc["dataset_params"]["label_index"] = 1
    dc["n_train"] = 23
    lit = _lit(cfg).train()
    with torch.no_grad():                                   # (the default init of a 4-unit bias-free ReLU net can be dead)
        for n, p in lit.model.named_parameters():
            if "rnn" in n:
                p.abs_().add_(0.05)
    loader = PSDDataModule(DictionaryUtility.to_object(copy.deepcopy(cfg)), "cpu").train_dataloader()
    batch = next(iter(loader))
    loss = lit.training_step(batch, 0)
    assert torch.isfinite(loss)
    loss.backward()
    for n, p in lit.model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n


def test_rnn_ok_bounds():
    from waveformml_amd import _lib
    lib = _lib.load()
    R, TH, F32 = _lib.WFS_RNN_RELU, _lib.WFS_RNN_TANH, _lib.WFS_F32
    ok = lambda *a: lib.wfs_rnn_ok(*a)  # noqa: E731  (I, H, layers, dirs, nonlinearity, T, dtype)
    assert ok(1, 4, 4, 1, R, 59, F32) == _lib.WFS_OK
    assert ok(33, 4, 4, 1, R, 59, F32) == _lib.WFS_EINVAL
    assert ok(1, 33, 4, 1, R, 59, F32) == _lib.WFS_EINVAL
    assert ok(1, 4, 9, 1, R, 59, F32) == _lib.WFS_EINVAL
    assert ok(1, 4, 4, 1, R, 4097, F32) == _lib.WFS_EINVAL
    assert ok(1, 4, 4, 1, R, 0, F32) == _lib.WFS_EINVAL
    assert ok(1, 4, 4, 1, 2, 59, F32) == _lib.WFS_EINVAL           # an unknown nonlinearity code
    assert ok(1, 4, 4, 3, R, 59, F32) == _lib.WFS_EINVAL
    assert ok(1, 4, 4, 1, R, 59, 7) == _lib.WFS_EINVAL
    assert ok(0, 4, 4, 1, R, 59, F32) == _lib.WFS_EINVAL and ok(1, 0, 4, 1, R, 59, F32) == _lib.WFS_EINVAL
    for dt in (_lib.WFS_F32, _lib.WFS_BF16, _lib.WFS_F16):
        assert ok(32, 32, 8, 2, TH, 4096, dt) == _lib.WFS_OK       # the corner
    assert lib.wfs_rnn_n_params(4, 2) == 8 and lib.wfs_rnn_n_params(9, 1) == 0
    # saved: X and every layer's outputs at N rounded up to 64; nothing for a refused shape
    assert lib.wfs_rnn_saved_floats(100, 59, 1, 4, 4, 1) == 128 * 59 * (1 + 4 * 4)
    assert lib.wfs_rnn_saved_floats(100, 59, 1, 33, 4, 1) == 0
    assert lib.wfs_rnn_bwd_workspace_floats(100, 59, 1, 4, 4, 2) > 2 * 8 * 59 * 128
    # entry points refuse what the predicate refuses, before they touch a pointer
    assert lib.wfs_rnn_fwd(None, 4, 59, 1, 33, 4, 1, R, None, None, None, None, F32, 0.0, None, None) == _lib.WFS_EINVAL
    assert lib.wfs_rnn_bwd(None, 4, 4097, 1, 4, 4, 1, R, None, None, None, None, F32, 0.0, None, None) == _lib.WFS_EINVAL
    assert lib.wfs_rnn_fwd(None, 4, 59, 1, 4, 4, 1, R, None, None, None, None, F32, 0.5, None, None) == _lib.WFS_EINVAL


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_the_gpu_cases_are_live_in_float64(case, dtype):
    """The GPU tests' parameter recipe on this machine's CPU, every case and row dtype: every compared tensor non-zero,
    at most half of Y exactly zero, max|Y| in [1e-2, 1e3]."""
    i = CASES.index(case)
    x, dy = make_inputs(case, 6, dtype, seed=i)
    assert_live(run_torch(make_rnn(case, seed=i), x, dy, torch.float64))
