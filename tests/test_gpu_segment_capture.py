"""LitZ and LitEZ through ``Trainer(capture=True)`` with ``net_config.fused_segment_loss`` (psd/litz.py, the fused loss of
csrc/segloss.hip), after test_gpu_masked_loss.test_seg_quantifier_trains_through_the_captured_step: two batches of 44
and 38 events, SGD with momentum (or Adam) under an ExponentialLR, 3 epochs, three runs from one seed --

  key off, eager     torch's optimizer on ``model.parameters()``, the torch composition of the loss
  key on, eager      FlatSGD / FlatAdam on the flat parameter, the fused loss
  key on, captured   the same inside the replayed graph, rows and targets padded to the step's capacity

-- whose epoch losses agree within 1e-4 relative: the parity test of the flat optimizers for these modules that DESIGN.md
("A preserved gap") asks for.  Without the key a captured step still refuses the padded batch by name."""
import copy

import numpy as np
import pytest
import torch

from test_host_mirror import _z_config
from test_segment_callers import ez_config, segment_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _config(which, optimizer="optim.SGD"):
    if which == "LitEZ":
        cfg = ez_config(["waveformml_amd.spconv"])
    else:
        cfg = _z_config(["waveformml_amd.spconv"])
        if which == "LitZ-SELoss":
            cfg["net_config"]["SELoss"] = True
    oc = cfg["optimize_config"]
    oc.update(imports=["torch.optim", "torch.optim.lr_scheduler"], optimizer_class=optimizer,
              scheduler_class="lr_scheduler.ExponentialLR", scheduler_params={"gamma": 0.9})
    if optimizer == "optim.SGD":
        oc.update(lr=0.01, optimizer_params={"momentum": 0.9})
    else:
        oc.update(lr=0.001, optimizer_params={})
    return cfg


def _batches(which, seed):
    rng = np.random.default_rng(seed)
    batches = []
    for B in (44, 38):                                            # the capture sizes itself on its first batch
        rows, c, f = segment_rows(rng, B, 5, 40)
        shape = (len(rows), 2) if which == "LitEZ" else (len(rows),)
        batches.append(([c, f], torch.from_numpy(rng.random(shape).astype(np.float32))))
    assert batches[0][0][0].shape[0] > batches[1][0][0].shape[0]
    return batches


def _fit(which, cfg, batches, key, capture, val=None, keep=None):
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitEZ, LitZ
    from waveformml_amd.psd.trainer import Trainer
    cfg = copy.deepcopy(cfg)
    if key:
        cfg["net_config"]["fused_segment_loss"] = True
    torch.manual_seed(7)
    mod = (LitEZ if which == "LitEZ" else LitZ)(load_config(cfg))
    made, configure = [], mod.configure_optimizers

    def recording():
        made.append(configure())
        return made[-1]
    mod.configure_optimizers = recording
    tr = Trainer(max_epochs=3, device=DEV, capture=capture, check_every=2)
    hist = tr.fit(mod, [([c.clone(), f.clone()], y.clone()) for (c, f), y in batches],
                  [([c.clone(), f.clone()], y.clone()) for (c, f), y in val] if val is not None else None)
    torch.cuda.synchronize()
    (optimizers, _schedulers), = made
    if keep is not None:
        keep.append((mod, hist))
    return [h["train_loss"] for h in hist], tr.eager_fallbacks, optimizers[0]


@pytest.mark.parametrize("which,optimizer", [("LitZ", "optim.SGD"), ("LitZ-SELoss", "optim.SGD"), ("LitEZ", "optim.SGD"),
                                             ("LitZ", "optim.Adam")])
def test_segment_modules_train_through_the_captured_step(which, optimizer):
    from waveformml_amd.psd.graph import GraphedTrainStep
    from waveformml_amd.psd.optim import FlatAdam, FlatSGD
    cfg, batches = _config(which, optimizer), _batches(which, 12)
    n0 = batches[0][0][0].shape[0]
    assert GraphedTrainStep.capacity_for(n0, n0) > n0           # padding rows behind every batch
    off, _, opt_off = _fit(which, cfg, batches, key=False, capture=False)
    eager, _, opt_eager = _fit(which, cfg, batches, key=True, capture=False)
    captured, fallbacks, opt_captured = _fit(which, cfg, batches, key=True, capture=True)
    print(which, optimizer, "epoch losses: key off", off, "key on", eager, "captured", captured)
    flat = FlatSGD if optimizer == "optim.SGD" else FlatAdam
    assert type(opt_off) is (torch.optim.SGD if optimizer == "optim.SGD" else torch.optim.Adam)
    assert type(opt_eager) is flat and type(opt_captured) is flat
    assert fallbacks == 0 and len(off) == 3
    for a, b, c in zip(off, eager, captured):
        assert np.isfinite(a) and abs(a - b) <= 1e-4 * abs(a) and abs(a - c) <= 1e-4 * abs(a), (off, eager, captured)


@pytest.mark.parametrize("which", ["LitZ", "LitEZ"])
def test_captured_fit_validates_and_tests_on_the_batchs_own_events(which):
    """``Trainer(capture=True).fit(module, train, val)`` with the key, then ``test_step``: the captured step leaves its row
    capacity as ``batch_size_hint`` on the net, and the dense-map route of validation_step / test_step must not take it
    for the number of events.  The eager keyed run is the reference: ``val_loss`` of every epoch and the ``test_loss``
    afterwards within 1e-4 relative (the two runs' weights differ by the rounding of their training steps)."""
    cfg, batches = _config(which), _batches(which, 12)
    val = _batches(which, 13)[1:]
    runs = []
    for capture in (False, True):
        keep = []
        _fit(which, cfg, batches, key=True, capture=capture, val=val, keep=keep)
        mod, hist = keep[0]
        if capture:
            assert mod.model.batch_size_hint is not None and mod.model.batch_size_hint > val[0][1].shape[0]
        (c, f), y = val[0]
        mod.eval()
        with torch.no_grad():
            out = mod.test_step(([c.to(DEV), f.to(DEV)], y.to(DEV)), 0)
        predictions = mod.last_test_outputs[0]
        assert predictions.shape[0] == int(c[-1, -1]) + 1 and predictions.shape[2:] == (14, 11)
        runs.append(([h["val_loss"] for h in hist], float(out["test_loss"])))
    (v0, t0), (v1, t1) = runs
    print(which, "val_loss eager", v0, "captured", v1, "test_loss", t0, t1)
    assert len(v0) == 3
    for a, b in zip(v0 + [t0], v1 + [t1]):
        assert np.isfinite(a) and abs(a - b) <= 1e-4 * abs(a), (runs,)


def test_without_the_key_a_captured_step_still_refuses_the_padded_batch():
    cfg, batches = _config("LitZ"), _batches("LitZ", 12)
    with pytest.raises(ValueError, match="do not take a capacity-padded batch"):
        _fit("LitZ", cfg, batches, key=False, capture=True)
