"""``net_config.fused_segment_loss`` on the CPU (psd/litz.py, psd/znet.py, spconv.functional.segment_loss_kind): what the
key switches on LitZ / LitEZ, the criteria it covers, SingleEndedEZConv's batch-size hint and valid count over the CPU
restatement of spconv, and the two shipped configs.  The kernel and the captured step are in
tests/test_gpu_segment_map_loss.py and tests/test_gpu_segment_capture.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from test_host_mirror import _z_config
from test_segment_callers import ez_config, segment_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "fused_segment_loss"


def _build(cls_name, key, imports=("oracle.spconv",), **net):
    from waveformml_amd.psd import litz
    from waveformml_amd.psd.config import load_config
    cfg = _z_config(list(imports)) if cls_name == "LitZ" else ez_config(list(imports))
    cfg["net_config"].update(net)
    if key is not None:
        cfg["net_config"][KEY] = key
    return getattr(litz, cls_name)(load_config(cfg))


@pytest.mark.parametrize("cls_name", ["LitZ", "LitEZ"])
def test_without_the_key_nothing_changes(cls_name):
    for key in (None, False):
        m = _build(cls_name, key)
        assert m.fused_segment_loss is False and m.segment_loss_kind is None
        assert m.per_row_targets is False and m.flat_optimizer is False and m.captured_validation is True
        flat = torch.zeros(sum(p.numel() for p in m.model.parameters()), requires_grad=True)
        m.optimizer_parameters = [flat]
        got = [p for g in m.configure_optimizers().param_groups for p in g["params"]]
        model = list(m.model.parameters())
        assert len(got) == len(model) and all(a is b for a, b in zip(got, model))     # optimizer_parameters ignored


@pytest.mark.parametrize("cls_name", ["LitZ", "LitEZ"])
def test_with_the_key_the_attributes_flip_and_a_flat_parameter_is_taken(cls_name):
    from waveformml_amd import _lib
    m = _build(cls_name, True)
    assert m.fused_segment_loss is True and m.segment_loss_kind == _lib.WFS_LOSS_L1
    assert m.per_row_targets is True and m.flat_optimizer is True and m.captured_validation is False
    flat = torch.zeros(sum(p.numel() for p in m.model.parameters()), requires_grad=True)
    m.optimizer_parameters = [flat]
    got = [p for g in m.configure_optimizers().param_groups for p in g["params"]]
    assert len(got) == 1 and got[0] is flat
    # the class attributes other modules read stay what they were
    assert type(m).per_row_targets is False and type(m).flat_optimizer is False
    assert _build(cls_name, True, criterion_class="MSELoss").segment_loss_kind == _lib.WFS_LOSS_MSE


def test_cpu_tensors_keep_the_composition_and_the_named_refusal():
    """The oracle route: with the key a CPU batch is scored by the torch composition, the same value as without; a padded
    CPU batch is refused as before."""
    rng = np.random.default_rng(2)
    rows, c, f = segment_rows(rng, 5, 3, 40)
    z = torch.from_numpy(rng.standard_normal(len(rows)).astype(np.float32))
    losses = []
    for key in (True, None):
        torch.manual_seed(0)
        m = _build("LitZ", key)
        losses.append(float(m.training_step(([c, f.clone()], z), 0).detach()))
        with pytest.raises(ValueError, match="do not take a capacity-padded batch"):
            m.training_step(([c, f.clone(), torch.tensor([len(rows)])], z), 0)
    assert losses[0] == losses[1] and np.isfinite(losses[0])


@pytest.mark.parametrize("cls_name", ["LitZ", "LitEZ"])
def test_a_criterion_the_kernel_does_not_cover_raises_at_construction(cls_name):
    with pytest.raises(ValueError) as err:
        _build(cls_name, True, criterion_class="SmoothL1Loss")
    assert "SmoothL1Loss" in str(err.value) and KEY in str(err.value)
    assert _build(cls_name, None, criterion_class="SmoothL1Loss").fused_segment_loss is False      # fine without the key


def test_segment_loss_kind():
    from waveformml_amd import _lib
    from waveformml_amd.spconv.functional import regression_loss_kind, segment_loss_kind
    nn = torch.nn
    assert segment_loss_kind(nn.L1Loss(reduction="sum")) == _lib.WFS_LOSS_L1
    assert segment_loss_kind(nn.MSELoss(reduction="sum")) == _lib.WFS_LOSS_MSE
    for criterion in (nn.L1Loss(), nn.MSELoss(), nn.L1Loss(reduction="none"), nn.SmoothL1Loss(reduction="sum"),
                      nn.HuberLoss(reduction="sum"), object()):
        assert segment_loss_kind(criterion) is None, criterion

    class MyL1(nn.L1Loss):                                        # a subclass may compute anything
        pass
    assert segment_loss_kind(MyL1(reduction="sum")) is None
    # the mean-reduced twin of the masked regression loss answers the other way round
    assert regression_loss_kind(nn.L1Loss(reduction="sum")) is None and regression_loss_kind(nn.L1Loss()) == _lib.WFS_LOSS_L1


@pytest.mark.parametrize("with_z_model", [False, True], ids=["two-planes", "frozen-z"])
def test_ez_net_takes_a_hint_and_a_valid_count(with_z_model, tmp_path):
    """SingleEndedEZConv.forward([coords, feats, n_valid]) with ``batch_size_hint`` over oracle.spconv: the map of the
    unpadded call on the batch's own events, zeros on the events the hint adds -- also through a frozen LitZ model."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitEZ, LitZ
    cfg = ez_config(["oracle.spconv"])
    if with_z_model:
        zcfg = _z_config(["oracle.spconv"])
        torch.manual_seed(1)
        torch.save({"state_dict": LitZ(load_config(copy.deepcopy(zcfg))).state_dict()}, str(tmp_path / "z.ckpt"))
        with open(str(tmp_path / "z.json"), "w") as fh:
            json.dump(zcfg, fh)
        cfg["net_config"].update(z_weights=str(tmp_path / "z.ckpt"), z_config=str(tmp_path / "z.json"))
    torch.manual_seed(3)
    net = LitEZ(load_config(cfg)).model.eval()
    assert net.batch_size_hint is None
    rng = np.random.default_rng(9)
    rows, c, f = segment_rows(rng, 6, 4, 40)
    with torch.no_grad():
        want = net([c, f])
        assert want.shape == (6, 2, 14, 11)
        net.batch_size_hint = 9
        got = net([c, f, torch.tensor([len(rows)])])
        assert torch.equal(net([c, f], batch_size=6), want)        # an explicit batch size wins over the hint
        net.batch_size_hint = None
    assert got.shape == (9, 2, 14, 11)
    assert torch.equal(got[:6], want) and (got[6:] == 0).all()
    # the batch-first columns a captured runner hands over are taken when they belong to these very coordinates
    net.batch_first_indices = (c, c[:, [2, 0, 1]].contiguous())
    with torch.no_grad():
        assert torch.equal(net([c, f]), want)
    net.batch_first_indices = None


@pytest.mark.parametrize("name,cls_name,planes", [("segment_z", "LitZ", 1), ("segment_ez", "LitEZ", 2)])
def test_shipped_configs_load_and_build(name, cls_name, planes):
    from waveformml_amd.psd.config import ModuleUtility, load_config
    path = os.path.join(ROOT, "config", name + ".json")
    raw = json.load(open(path))
    assert raw["net_config"][KEY] is True and "waveformml_amd.spconv" in raw["net_config"]["imports"]
    config = load_config(path)
    cls = ModuleUtility(config.run_config.imports).retrieve_class(config.run_config.run_class)
    assert cls.__name__ == cls_name
    m = cls(config)
    assert m.fused_segment_loss and m.per_row_targets and m.flat_optimizer and not m.captured_validation
    assert m.model.model.plan[-1][1] == planes
    (opt,), (sched,) = m.configure_optimizers()
    assert type(opt) is torch.optim.SGD and type(sched).__name__ == "ExponentialLR"


def test_litez_scales_features_out_of_place_on_request():
    """``algorithm == "features"`` with ``e_factor != 1``: in place as the reference does it on the dense-map route; the
    fused training route asks for a copy (a captured step's static buffer is read again by every warm-up replay), so the
    factor cannot compound."""
    m = _build("LitEZ", True, algorithm="features", escale=24.0)
    assert m.phys_coord and m.e_factor == 2.0
    f = torch.rand(5, 20)
    want = f.clone()
    assert m._scaled_features(want, in_place=True) is want
    assert torch.equal(want[:, [0, 2, 3]], 2.0 * f[:, [0, 2, 3]]) and torch.equal(want[:, [1] + list(range(4, 20))],
                                                                                  f[:, [1] + list(range(4, 20))])
    static = f.clone()
    for _ in range(3):                                            # warm-up replays: the same buffer every time
        got = m._scaled_features(static, in_place=False)
        assert got is not static and torch.equal(static, f) and torch.equal(got, want)


@pytest.mark.parametrize("cls_name", ["LitZ", "LitEZ"])
def test_dense_map_route_ignores_a_captured_steps_hint(cls_name):
    """A captured training step leaves its row capacity as ``batch_size_hint`` on the net; validation_step and test_step
    build their dense maps over the batch's own events all the same, with the values they have without a hint."""
    rng = np.random.default_rng(4)
    rows, c, f = segment_rows(rng, 5, 3, 40)
    y = torch.from_numpy(rng.random((len(rows), 2) if cls_name == "LitEZ" else len(rows)).astype(np.float32))
    torch.manual_seed(0)
    m = _build(cls_name, True).eval()
    with torch.no_grad():
        want_val = m.validation_step(([c, f.clone()], y), 0)
        want_test = float(m.test_step(([c, f.clone()], y), 0)["test_loss"])
        m.model.batch_size_hint = 16
        got_val = m.validation_step(([c, f.clone()], y), 0)
        got_test = float(m.test_step(([c, f.clone()], y), 0)["test_loss"])
    val = (lambda r: float(r["val_loss"]) if isinstance(r, dict) else float(r))
    assert val(got_val) == val(want_val) and got_test == want_test and np.isfinite(got_test)
    assert m.last_test_outputs[0].shape == (5, 2 if cls_name == "LitEZ" else 1, 14, 11)


def test_trainer_validate_takes_litz_bare_validation_loss():
    """LitZ.validation_step returns the loss itself, as the reference's does; Trainer.validate reads it as val_loss."""
    from waveformml_amd.psd.trainer import Trainer
    rng = np.random.default_rng(6)
    rows, c, f = segment_rows(rng, 5, 3, 40)
    y = torch.from_numpy(rng.random(len(rows)).astype(np.float32))
    torch.manual_seed(0)
    m = _build("LitZ", None).eval()
    with torch.no_grad():
        want = float(m.validation_step(([c, f.clone()], y), 0))
    got = Trainer(device="cpu").validate(m, [([c, f.clone()], y)])
    assert got["val_loss"] == want and np.isnan(got["val_acc"])
