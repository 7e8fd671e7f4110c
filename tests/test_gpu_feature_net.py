"""``ExtractedFeatureConvNet`` (psd/featurenet.py) on the GPU operators against the same module on the CPU oracle path,
with the bars of tests/test_gpu_segment_callers.py: fp32 loss 1e-5 relative, gradients 1e-4 of each tensor's maximum; and
two epochs through ``Trainer(capture=True)`` on the fixture files against the eager trainer to 1e-4.

bf16 rows: the bound is 1.5 x the largest logit error measured on this very case against the fp32 CPU path, relative to
the largest logit."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_segment_callers import _close, _compare_step, _pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BF16_LOGIT_ERROR = 6.3e-3           # measured on an MI355X (6.292e-3); the assertion is 1.5 x this


def config_dict():
    with open(os.path.join(ROOT, "config", "psd_features_det.json")) as fh:
        cfg = json.load(fh)
    cfg["dataset_config"]["base_path"] = os.path.join(HERE, "golden", "h5", "det")
    return cfg


def feature_rows(seed, events=8):
    """`events` events of 1 to 7 distinct segments each (about 30 rows), seven quantities in [0, 1)."""
    rng = np.random.default_rng(seed)
    coords, feats = [], []
    for e in range(events):
        n = int(rng.integers(1, 8))
        for k in rng.choice(14 * 11, size=n, replace=False):
            coords.append((k // 11, k % 11, e))
            feats.append(rng.uniform(0.02, 0.95, 7))
    return (torch.tensor(coords, dtype=torch.int32), torch.tensor(np.array(feats), dtype=torch.float32),
            torch.from_numpy(rng.integers(0, 2, events)))


def test_fp32_forward_loss_and_gradients_match_the_cpu_path():
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(3)
    gpu, cpu = _pair(LitPSD, config_dict())
    c, f, y = feature_rows(5)
    assert 20 <= len(c) <= 45
    with torch.no_grad():
        gpu.eval(), cpu.eval()
        _close(gpu.model([c.to(DEV), f.to(DEV)]).cpu().numpy(), cpu.model([c, f]).numpy(), 1e-5, "logits (eval mode)")
        gpu.train(), cpu.train()
    _compare_step(gpu, cpu, c, f, y)


def test_bf16_forward_against_the_fp32_cpu_path():
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(3)
    gpu, cpu = _pair(LitPSD, config_dict())
    c, f, _y = feature_rows(5)
    with torch.no_grad():
        want = cpu.model([c, f]).double().numpy()
        got = gpu.model([c.to(DEV), f.to(DEV).to(torch.bfloat16)]).double().cpu().numpy()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("bf16 logit error / largest logit: %.4g" % err)
    assert err <= 1.5 * BF16_LOGIT_ERROR, err


def test_two_epochs_through_the_captured_trainer_follow_the_eager_trainer():
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    from waveformml_amd.psd.trainer import Trainer
    cfg = config_dict()
    cfg["dataset_config"]["dataloader_params"]["pin_memory"] = False
    dm = PSDDataModule(load_config(copy.deepcopy(cfg)), DEV)
    dm.setup("fit")
    loader = torch.utils.data.DataLoader(dm.train_dataset, batch_size=2, shuffle=False,
                                         collate_fn=dm._collate(dm.train_dataset))
    batches = sorted(list(loader), key=lambda b: -b[0][0].shape[0])          # the capture sizes itself on its first batch
    assert len(batches) == 2 and batches[0][0][1].shape[1] == 7
    runs = []
    for capture in (False, True):
        torch.manual_seed(7)
        mod = LitPSD(load_config(copy.deepcopy(cfg)))
        tr = Trainer(max_epochs=2, device=DEV, capture=capture, check_every=2)
        hist = tr.fit(mod, [([c.clone(), f.clone()], y.clone()) for (c, f), y in batches])
        torch.cuda.synchronize()
        runs.append((hist, torch.cat([p.detach().reshape(-1).cpu() for p in mod.model.parameters()]), tr.eager_fallbacks))
    (h0, p0, _), (h1, p1, fb) = runs
    assert fb == 0 and np.isfinite(h0[-1]["train_loss"])
    for a, b in zip(h0, h1):
        assert abs(a["train_loss"] - b["train_loss"]) <= 1e-4 * abs(a["train_loss"]), (a, b)
    _close(p1.numpy(), p0.numpy(), 1e-4, "parameters after two epochs")
