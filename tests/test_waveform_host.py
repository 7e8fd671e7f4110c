"""CPU checks of the per-pulse path: TemporalWaveformNet's channel plan and head sizes against the reference formulas
(src/models/WaveformModels.py:8-45, ConvBlocks.py LinearBlock) worked by hand, the example config as shipped,
LitWaveform's detector-number handling, PulseDatasetWaveformNorm on the r3 pulse fixture, and the wfs_tcnc_* exports."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = os.path.join(ROOT, "tests", "golden", "h5")
EXP3 = np.load(os.path.join(ROOT, "tests", "golden", "expected_r3.npz"))


def _cfg(**hparams):
    with open(os.path.join(ROOT, "config", "waveform_tcn_z.json")) as f:
        cfg = json.load(f)
    cfg["net_config"]["hparams"].update(hparams)
    return cfg


def _obj(cfg):
    from waveformml_amd.psd.config import DictionaryUtility
    return DictionaryUtility.to_object(copy.deepcopy(cfg))


# (hparams, planes, LinearBlock widths at n_samples = 59), worked by hand from the reference's formulas:
#   expand = ef / ne; planes = round(expand (i + 1)), i < ne; contract = (ef - op) / nc;
#   planes += round(contract (nc - i - 1)), i < nc; planes[-1] = op;   widths = round(nin f^i), f = (out / nin)^(1 / n)
PLANS = [
    # 16/2 = 8 -> 8, 16; (16 - 8)/1 = 8 -> round(0) = 0, replaced by 8.  nin = 472: f = 472^-1/4 = 0.21486
    (dict(expansion_factor=16, n_expand=2, n_contract=1, out_planes=8, n_lin=4),
     [8, 16, 8], [472, 101, 22, 5, 1]),
    # 10/3 = 3.33 -> 3, 7, 10; (10 - 1)/3 = 3 -> 6, 3, 0 -> last = 1.  nin = 59: f = 59^-1/2 = 0.13019
    (dict(expansion_factor=10, n_expand=3, n_contract=3, out_planes=1, n_lin=2),
     [3, 7, 10, 6, 3, 1], [59, 8, 1]),
    # 5/2 = 2.5 -> round half to even: 2, then 5; (5 - 2)/2 = 1.5 -> round(1.5) = 2, 0 -> last = 2.  nin = 118, out 2
    (dict(expansion_factor=5, n_expand=2, n_contract=2, out_planes=2, n_lin=1, out_size=2),
     [2, 5, 2, 2], [118, 2]),
    # 32/4 = 8 -> 8, 16, 24, 32; (32 - 4)/2 = 14 -> 14, 0 -> last = 4.  nin = 236: f = 236^-1/3 = 0.16181
    (dict(expansion_factor=32, n_expand=4, n_contract=2, out_planes=4, n_lin=3),
     [8, 16, 24, 32, 14, 4], [236, 38, 6, 1]),
]


@pytest.mark.parametrize("hp,planes,widths", PLANS)
def test_planes_and_linear_block_sizes(hp, planes, widths):
    from waveformml_amd.psd.WaveformModels import TemporalWaveformNet
    net = TemporalWaveformNet(_obj(_cfg(**hp)))
    assert net.planes == planes
    assert [blk.convs[0].weight_v.shape[0] for blk in net.model.network] == planes
    assert net.model.fused and net.output_size == hp.get("out_size", 1)
    lin = list(net.linear)
    assert [lin[0].in_features] + [layer.out_features for layer in lin] == widths
    y = net(torch.randn(3, 1, 59))                          # CPU: the torch composition
    assert y.shape == (3, hp.get("out_size", 1))


def test_shipped_example_config_raises_attribute_error():
    """config/examples/SingleWaveformTCN.json has no expansion_factor / n_expand / n_contract / out_planes: the
    reference's net raises AttributeError, and so does the mirror."""
    from waveformml_amd.psd.LitWaveform import LitWaveform
    cfg = _cfg()
    for k in ("expansion_factor", "n_expand", "n_contract", "out_planes"):
        cfg["net_config"]["hparams"].pop(k)
    with pytest.raises(AttributeError):
        LitWaveform(_obj(cfg))


def test_detector_numbers():
    from waveformml_amd.psd.LitWaveform import LitWaveform
    cfg = _cfg()
    cfg["net_config"]["use_detector_number"] = True
    cfg["net_config"]["num_detectors"] = 154
    with pytest.raises(IOError):
        LitWaveform(_obj(cfg))
    del cfg["net_config"]["num_detectors"]
    with pytest.raises(IOError):
        LitWaveform(_obj(cfg))
    cfg["net_config"]["num_detectors"] = 308
    conf = _obj(cfg)
    m = LitWaveform(conf)
    assert conf.system_config.n_samples == 62 and m.model.nsamples == 62 and m.model.linear[0].in_features == 62 * 8
    det = torch.tensor([0, 1, 27, 28, 615])
    coords = torch.zeros((5, 3))
    m.fill_coords(coords, det)
    # segment det // 2 = 0, 0, 13, 14, 307: x = (seg % 14) / 13, y = (seg // 14) / 10, end = det % 2
    want = torch.tensor([[0., 0., 0.], [0., 0., 1.], [1., 0., 1.], [0., 0.1, 0.], [1., 2.1, 1.]])
    assert torch.allclose(coords, want, atol=1e-7)
    f = torch.rand(5, 59)
    loss = m.training_step(([det.reshape(5, 1).int(), f], torch.rand(5)), 0)
    assert torch.isfinite(loss)


def test_no_detector_number_and_squeeze_index():
    from waveformml_amd.psd.LitWaveform import LitWaveform
    m = LitWaveform(_obj(_cfg()))
    assert not m.use_detector_number and m.squeeze_index == 1 and m.target_index == 7 and not m.use_accuracy
    assert m.per_row_targets and m.loss_no_reduce.reduction == "none" and m.criterion.reduction == "mean"


def test_masked_loss_of_a_padded_batch_ignores_the_padding():
    """The captured step's loss: the mean over the first n_valid rows, whatever the padding rows hold."""
    from waveformml_amd.psd.LitWaveform import LitWaveform
    m = LitWaveform(_obj(_cfg()))
    p, t = torch.randn(10, requires_grad=True), torch.randn(10)
    loss = m._loss(p, t, torch.tensor([6]))
    assert torch.allclose(loss, (p[:6] - t[:6]).abs().mean())
    loss.backward()
    assert torch.all(p.grad[6:] == 0)


def test_pulse_dataset_waveform_norm_from_config():
    from waveformml_amd.psd.PulseDataset import PulseDatasetWaveformNorm
    cfg = _cfg()
    cfg["dataset_config"]["base_path"] = os.path.join(H5, "r3")
    cfg["dataset_config"]["paths"] = ["pulses"]
    for idx in (0, 1, 2):
        ds = PulseDatasetWaveformNorm(_obj(cfg), "train", 23, "cpu", label_name="phys", label_index=idx)
        assert len(ds) == 1 and ds.info["data_info"][0]["event_range"] == [0, 22]
        (c, f), y = ds[0]
        assert np.array_equal(c.numpy()[:, 0], EXP3["pulses/p_1/det"])
        assert np.array_equal(f.numpy(), EXP3["pulses/p_1/pulse"])
        assert y.dtype == torch.float32 and np.array_equal(y.numpy(), EXP3["pulses/p_1/phys"][:, idx])
    ds = PulseDatasetWaveformNorm(_obj(cfg), "train", 23, "cpu", label_name="phys")
    assert np.array_equal(ds[0][1].numpy(), EXP3["pulses/p_1/phys"])


def test_data_module_builds_the_pulse_dataset():
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    cfg = _cfg()
    cfg["dataset_config"]["base_path"] = os.path.join(H5, "r3")
    cfg["dataset_config"]["paths"] = ["pulses"]
    cfg["dataset_config"]["dataset_params"]["label_index"] = 2
    cfg["dataset_config"]["n_train"] = 23
    (c, f), y = next(iter(PSDDataModule(_obj(cfg), "cpu").train_dataloader()))
    assert c.shape == (23, 1) and f.shape == (23, 12)
    assert np.array_equal(y.numpy(), EXP3["pulses/p_1/phys"][:, 2])


def test_tcnc_symbols_are_exported():
    from waveformml_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = ["wfs_tcnc_ok", "wfs_tcnc_n_conv", "wfs_tcnc_weights_floats", "wfs_tcnc_saved_floats",
             "wfs_tcnc_bwd_workspace_floats", "wfs_tcnc_taps_fwd", "wfs_tcnc_fwd", "wfs_tcnc_bwd"]
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    L = _lib.load()
    ch = _lib.i32_array([8, 16, 8])
    assert L.wfs_tcnc_ok(1, ch, 3, 3, 59, _lib.WFS_F32) == _lib.WFS_OK
    assert L.wfs_tcnc_n_conv(1, ch, 3, 3) == 9                 # every level changes its channel count: 3 convs each
    # conv1 / conv2 / downsample taps + biases: (24+8 + 192+8 + 8+8) + (384+16 + 768+16 + 128+16) + (384+8 + 192+8 + 128+8)
    assert L.wfs_tcnc_weights_floats(1, ch, 3, 3) == 2304
    assert L.wfs_tcnc_saved_floats(10, 59, 1, ch, 3) == 3 * 10 * 59 * 32
    assert L.wfs_tcnc_ok(1, _lib.i32_array([8, 0]), 2, 3, 59, _lib.WFS_F32) == _lib.WFS_EINVAL


def test_fused_flag_keeps_the_state_dict():
    from waveformml_amd.psd.tcn import TemporalConvNet
    a = TemporalConvNet(1, [8, 16, 8], 3, 0.0)
    b = TemporalConvNet(1, [8, 16, 8], 3, 0.0, fused=True)
    assert not a.fused and list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 1, 59)
    assert torch.equal(a(x), b(x))                          # CPU tensors: the torch composition either way
