"""The hybrid 3-D net (BASELINE configs[4] "C5": feat [n, 1, 2T] -> TCN -> voxelise -> SubM3d head;
config/psd_c5_hybrid3d.json) on the GPU against a CPU twin assembled here: the torch TemporalConvNet on CPU tensors, a
test-local torch voxeliser (nonzero on the mask, gather) and the 3-D head bound to oracle.spconv, with the same
state_dict -- then the captured step against the eager one, the voxel capacity of a captured step, and the whole
LitPSD + Trainer surface."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch

from test_gpu_fullsize import GRAD_REL_L2, _one_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _config(T=1024, dropout=0.0):
    with open(os.path.join(ROOT, "config", "psd_c5_hybrid3d.json")) as f:
        cfg = json.load(f)
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["hparams"]["wf_params"]["dropout"] = dropout
    cfg["optimize_config"].pop("scheduler_class", None)
    return cfg


def _twin_forward(self, x, batch_size=None):
    """The CPU twin: torch TCN, torch voxeliser, oracle.spconv head through SPConvNet's own tail."""
    coords, feats = x[0], x[1]
    if batch_size is None:
        batch_size = int(coords[-1, -1]) + 1
    T = feats.shape[1] // 2
    y = self.waveformLayer(feats.unsqueeze(1)).squeeze(1)
    thr = self.voxelizer.threshold
    r, t = torch.nonzero((feats[:, :T] > thr) | (feats[:, T:] > thr), as_tuple=True)
    c = coords.long()
    indices = torch.stack([c[r, 2], c[r, 0], c[r, 1], t], 1).int()
    vox = torch.stack([y[r, t], y[r, T + t]], 1)
    st = self.spconv.SparseConvTensor(vox, indices, self.spatial_size, batch_size)
    return self._head(st)


def _cpu_module(cfg):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    ref = copy.deepcopy(cfg)
    ref["net_config"]["imports"] = ["oracle.spconv" if m == "waveformml_amd.spconv" else m
                                    for m in ref["net_config"]["imports"]]
    m = LitPSD(DictionaryUtility.to_object(ref))
    m.model.forward = types.MethodType(_twin_forward, m.model)
    return m


def _pair(cfg):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    gpu = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
    with torch.no_grad():
        for p in gpu.model.waveformLayer.parameters():        # N(0, 0.01) taps would leave the front end almost linear
            p.copy_(torch.randn_like(p) * 0.5)
    cpu = _cpu_module(cfg)
    cpu.load_state_dict(gpu.state_dict())
    cpu.make_twin = lambda: _cpu_module(cfg)
    gpu = gpu.to(DEV)
    gpu.train(), cpu.train()
    return gpu, cpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_one_training_step_against_the_cpu_twin(dtype):
    from waveformml_amd.psd import synthetic
    torch.manual_seed(31)
    gpu, cpu = _pair(_config())
    c, f, y = synthetic.generate(64, 1024, 3, seed=4, layout="2d")
    if dtype == torch.float32:
        _one_step(gpu, cpu, c, f, y, dtype, 1e-5, 1e-5)
    else:
        # 7.7e-3 measured: C2's 5e-3 bar plus the TCN's output rows, rounded to bf16 before the head
        _one_step(gpu, cpu, c, f, y, dtype, 1e-2, GRAD_REL_L2[dtype])


def _batches(E, T, seeds, dtype=torch.float32):
    from waveformml_amd.psd import synthetic
    out = []
    for s in seeds:
        c, f, y = synthetic.generate(E, T, 3, seed=s, layout="2d")
        out.append(([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV).to(dtype)], torch.from_numpy(y).to(DEV)))
    return out


def _module(cfg, seed=7):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(seed)
    mod = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg))).to(DEV)
    red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
    mod.optimizer_parameters = red.optimizer_parameters()
    opt = mod.configure_optimizers()
    return mod, red, opt


def _eager_step(mod, red, opt, batch):
    red.reset()
    loss = mod.training_step(batch, 0)
    loss.backward()
    red.finish()
    opt.step()
    return float(loss)


def test_captured_step_matches_the_eager_step():
    from waveformml_amd.psd.graph import GraphedTrainStep
    E, T = 32, 1024
    cfg = _config(T)
    batches = _batches(E, T, (41, 42, 43, 44))
    counts = [int(((b[0][1][:, :T] > 0) | (b[0][1][:, T:] > 0)).sum()) for b in batches]
    assert len(set(counts)) == len(counts)                  # different voxel counts per batch
    mod_g, red_g, opt_g = _module(cfg)
    mod_e, red_e, opt_e = _module(cfg)
    assert torch.equal(red_g.flat_param, red_e.flat_param)
    step = GraphedTrainStep(mod_g, opt_g, red_g, batches[0], warmup=2)
    assert mod_g.model.voxelizer.out_capacity >= counts[0]
    for _ in range(3):                                       # the calibration step and the two warm-up steps
        _eager_step(mod_e, red_e, opt_e, batches[0])
    scale = float(red_e.flat_param.abs().max())
    assert float((red_g.flat_param - red_e.flat_param).abs().max()) <= 2e-5 * scale
    for b in batches[1:]:
        lg = float(step(b))
        le = _eager_step(mod_e, red_e, opt_e, b)
        assert abs(lg - le) <= 1e-5 * abs(le), (lg, le)
        assert float((red_g.flat_param - red_e.flat_param).abs().max()) <= 2e-5 * scale
    step.check()
    with torch.no_grad():                                    # logits of the updated nets on the last batch
        mod_g.eval(), mod_e.eval()
        (c, f), _y = batches[-1]
        assert torch.allclose(mod_g.model([c, f]), mod_e.model([c, f]), rtol=0, atol=1e-4)


def test_voxel_overflow_of_a_captured_step_raises():
    from waveformml_amd.psd.graph import GraphedTrainStep
    E, T = 32, 1024
    cfg = _config(T)
    good = _batches(E, T, (51,))[0]
    (c, f), y = good
    # the same rows with more samples above threshold: the voxel count grows, the row count does not
    more = f.clone()
    more[:, : T // 2] += 0.001
    busy = ([c, more], y)
    mod, red, opt = _module(cfg)
    mod_e, red_e, opt_e = _module(cfg)
    step = GraphedTrainStep(mod, opt, red, good)
    for _ in range(3):
        _eager_step(mod_e, red_e, opt_e, good)
    lg, le = float(step(good)), _eager_step(mod_e, red_e, opt_e, good)
    assert abs(lg - le) <= 1e-5 * abs(le)
    step.check()
    assert step.fits(busy)
    step(busy)                                               # its results are invalid: check() must say so
    flags = mod.model.voxelizer.sticky_flags()
    assert len(flags) == 1 and int(flags[0].item()) == 1     # the VOXELISER's flag, not only a strided layer's
    with pytest.raises(RuntimeError, match="voxel capacity"):
        step.check()
    step.check()                                             # read and cleared


def _busier(batch, T):
    """The same rows with more samples above threshold: more voxels, the same rows and labels."""
    (c, f), y = batch
    more = f.clone()
    more[:, : T // 2] += 0.001
    return ([c, more], y)


def test_eval_graph_has_its_own_voxel_capacity_and_flag():
    """A captured eval forward (GraphedEvalStep) calibrates the voxeliser on its own batch and reads its own flag: a
    busier batch through the eval graph raises in ITS check(), the training step's check() stays silent."""
    from waveformml_amd.psd.graph import GraphedEvalStep, GraphedTrainStep
    E, T = 32, 1024
    good = _batches(E, T, (61,))[0]
    val = _batches(E, T, (62,))[0]
    mod, red, opt = _module(_config(T))
    step = GraphedTrainStep(mod, opt, red, good)
    train_flag = mod.model.voxelizer.sticky_flags()[0]
    ev = GraphedEvalStep(mod, val)
    assert mod.model.voxelizer.sticky_flags()[0] is not train_flag
    n_val = int(((val[0][1][:, :T] > 0) | (val[0][1][:, T:] > 0)).sum())
    assert mod.model.voxelizer.out_capacity >= n_val
    logits = ev(val).clone()
    ev.check()
    with torch.no_grad():
        mod.eval()
        want = mod.model([val[0][0], val[0][1]]).float()
        mod.train()
    assert torch.allclose(logits, want, rtol=0, atol=1e-4)
    ev(_busier(val, T))
    with pytest.raises(RuntimeError, match="voxel capacity"):
        ev.check()
    step(good)
    step.check()                                             # the eval graph's overflow is not the training step's


def _spread(batch, T, seed):
    """The same rows, features and labels, every event's rows moved to distinct random cells of the whole 14 x 11 x T grid
    (ascending in row order): far fewer rows share a strided layer's output cell, so its outputs outgrow the capacity a
    compact batch calibrated, while the rows still fit."""
    (c, f), y = batch
    cc = c.cpu().numpy().copy()
    rng = np.random.default_rng(seed)
    for e in np.unique(cc[:, -1]):
        rows = np.nonzero(cc[:, -1] == e)[0]
        cells = np.sort(rng.choice(14 * 11 * T, size=len(rows), replace=False))
        cc[rows, 0], cc[rows, 1], cc[rows, 2] = cells // (11 * T), cells // T % 11, cells % T
    return ([torch.from_numpy(cc).to(c.device), f], y)


def test_train_and_eval_graphs_keep_their_own_conv_overflow_flags():
    """A GraphedTrainStep and a GraphedEvalStep captured on one C2 module at the same batch size: a batch that fits the
    rows but overflows the strided layers raises in the check() of the runner that replayed it and never in the other's,
    in both directions -- the strided layers' flags are per runner, as the voxeliser's."""
    from test_gpu_event_conv import _batch, _cfg, _module, _train_step
    from waveformml_amd.psd.graph import GraphedEvalStep
    T, B = 64, 32
    mod = _module(_cfg(T))
    good = _batch(B, T, 71)
    spread = _spread(good, T, 72)
    step, _red, _opt = _train_step(mod, good)
    ev = GraphedEvalStep(mod, good)
    assert step.fits(spread) and ev.fits(spread)
    assert np.isfinite(float(step(good))) and bool(torch.isfinite(ev(good)).all())
    step.check()
    ev.check()
    ev(spread)
    step.check()                                             # the eval graph's overflow is not the training step's
    with pytest.raises(RuntimeError, match="sparse conv output exceeded its captured capacity"):
        ev.check()
    step(spread)
    ev.check()                                               # ... nor the training step's the eval graph's
    with pytest.raises(RuntimeError, match="sparse conv output exceeded its captured capacity"):
        step.check()
    ev(good)
    step(good)
    ev.check()
    step.check()
    ev.close()
    step.close()


def test_trainer_validation_on_a_busier_batch_raises():
    """Trainer(capture=True).fit with a validation loader: a validation batch with more voxels than the eval graph's
    capacity raises instead of giving wrong metrics."""
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.data import SyntheticPulseDataset
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.trainer import Trainer
    T = 1024
    ds = SyntheticPulseDataset(3, 16, T, layout="2d", seed=9)
    train = sorted((ds[i] for i in range(len(ds))), key=lambda b: -int((b[0][1] > 0).sum()))
    val = [train[0], _busier(train[0], T)]
    torch.manual_seed(3)
    m = LitPSD(DictionaryUtility.to_object(_config(T)))
    tr = Trainer(max_epochs=1, device=DEV, feature_dtype=torch.bfloat16, capture=True)
    with pytest.raises(RuntimeError, match="voxel capacity"):
        tr.fit(m, train, val_loader=val)


def test_litpsd_and_trainer_from_the_config():
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.data import SyntheticPulseDataset
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.trainer import Trainer
    cfg = _config(1024, dropout=0.2)
    ds = SyntheticPulseDataset(3, 16, 1024, layout="2d", seed=5)
    # the capture is calibrated on the first batch; the voxel count of a 16-event batch varies far more than its row
    # count, so the busiest batch goes first (a later, larger one would raise -- test_voxel_overflow_...)
    batches = sorted((ds[i] for i in range(len(ds))), key=lambda b: -int((b[0][1] > 0).sum()))
    for capture in (False, True):
        torch.manual_seed(3)
        m = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
        tr = Trainer(max_epochs=2, device=DEV, feature_dtype=torch.bfloat16, capture=capture)
        hist = tr.fit(m, batches)
        assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) for h in hist), hist
        assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
