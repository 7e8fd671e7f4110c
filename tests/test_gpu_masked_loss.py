"""GPU checks of the fused masked regression loss (csrc/segloss.hip, spconv.functional.MaskedRegressionLossFunction)
against a float64 torch composition over the same counted rows, and of LitSegQuantifier through the captured step.

Bounds: loss and mse within 1e-5 relative (measured near 1e-7: fp64 sums, one rounding to fp32 at the end); dpred of fp32
rows within 1e-6 of the gradient's scale; dpred of 16-bit rows within one correctly rounded store of the value -- 2^-8
(bf16) / 2^-11 (fp16) of it, the convention of tests/conv32_cases.py -- on top of that fp32 bar, and for fp16 half the
spacing of its subnormals (2^-25) where the value lies below its normal range.

Row counts: 1, 65, 1000, and 1023 / 1024 / 1025 around the forward's chunk of 1024 rows (csrc/wfs_lossfold.h)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from test_segment_callers import segment_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "config", "segment_quantifier_z.json")
U_ROUND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
WORST = {"loss": 0.0, "mse": 0.0, "dpred_f32": 0.0}
PAD = -100.0                                                   # the captured step's fill value for per-row targets


def _mask():
    from waveformml_amd.psd.segments import segment_status, single_ended_mask
    return single_ended_mask(segment_status()).to(DEV)


def _inputs(n, dtype, column, seed, n_valid=None, poison=False, mask=None):
    """pred [n], target [n, 8] or [n], coords [n, 3] on single-ended and other segments; ``poison``: NaN / Inf / the
    padding value in every row that is not counted."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(n, generator=g).to(dtype)
    target = (torch.rand((n, 8), generator=g) if column else torch.rand(n, generator=g)).to(dtype)
    c = torch.stack([torch.randint(0, 14, (n,), generator=g), torch.randint(0, 11, (n,), generator=g),
                     torch.arange(n) // 5], dim=1).to(torch.int32)
    if n > 2:
        pred[1] = (target[1, 4] if column else target[1])       # d = 0: sign(0) = 0
    counted = torch.ones(n, dtype=torch.bool)
    if n_valid is not None:
        counted &= torch.arange(n) < n_valid
    if mask is not None:
        counted &= mask.cpu()[0, 0, c[:, 0].long(), c[:, 1].long()] == 1.0
    if poison:
        bad = ~counted
        vals = torch.tensor([float("nan"), float("inf"), -float("inf"), PAD])[torch.arange(n) % 4].to(dtype)
        pred = torch.where(bad, vals, pred)
        target = torch.where(bad.reshape(-1, *([1] * (target.dim() - 1))), vals.roll(1).reshape(-1, *([1] * (target.dim() - 1))),
                             target)
        if n_valid is not None:
            c[n_valid:] = torch.tensor([-7, 400, 9], dtype=torch.int32)     # beyond the valid rows: never read
    return pred, target, c, counted


def _reference(pred, target, column, counted, kind):
    d = pred.double() - (target[:, 4] if column else target).double()
    d = d[counted]
    cnt = int(counted.sum())
    per = d.abs() if kind == 0 else d * d
    loss = per.sum() / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)
    mse = (d * d).sum() / cnt if cnt else torch.tensor(float("nan"), dtype=torch.float64)
    s = torch.sign(d) if kind == 0 else 2 * d
    grad = torch.zeros(pred.shape[0], dtype=torch.float64)
    if cnt:
        grad[counted] = s / cnt
    return float(loss), float(mse), grad, cnt


def _run(pred, target, c, kind, column, mask, n_valid, max_blocks=0, g=1.0):
    from waveformml_amd.spconv import functional as Fsp
    p = pred.to(DEV).requires_grad_(True)
    nv = torch.tensor([n_valid], dtype=torch.int64, device=DEV) if n_valid is not None else None
    loss, mse = Fsp.masked_regression_loss(p, target.to(DEV), kind, col=4 if column else 0, coords=c.to(DEV),
                                           se_mask=mask, n_valid=nv, max_blocks=max_blocks)
    assert loss.dtype == torch.float32 and loss.shape == () and not mse.requires_grad
    (loss * g).backward()
    return loss.detach(), mse.detach(), p.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [1, 65, 1000, 1023, 1024, 1025])
@pytest.mark.parametrize("kind", [0, 1], ids=["L1", "MSE"])
def test_loss_and_gradient_against_the_float64_composition(kind, n, dtype):
    mask = _mask()
    for use_mask, use_nv in ((True, False), (False, True), (True, True)):
        for column in (True, False):
            n_valid = max(1, (2 * n) // 3) if use_nv else None
            pred, target, c, counted = _inputs(n, dtype, column, 100 * n + kind, n_valid, poison=True,
                                               mask=mask if use_mask else None)
            if n == 1 and use_mask and not counted.any():
                c[0, 0], c[0, 1] = 1, 0                        # segment 1 is single-ended
                counted[:] = True
                pred[0], target.reshape(-1)[4 if column else 0] = 0.25, 0.75
            want_loss, want_mse, want_grad, cnt = _reference(pred, target, column, counted, kind)
            assert cnt > 0
            loss, mse, grad = _run(pred, target, c, kind, column, mask if use_mask else None, n_valid, g=3.0)
            what = (use_mask, use_nv, column)
            for key, got, want in (("loss", float(loss), want_loss), ("mse", float(mse), want_mse)):
                rel = abs(got - want) / abs(want)
                WORST[key] = max(WORST[key], rel)
                assert rel <= 1e-5, (what, key, got, want)
            want_grad = 3.0 * want_grad
            got = grad.double().cpu()
            assert grad.dtype == dtype and torch.isfinite(got).all()
            assert (got[~counted] == 0).all(), what                # exactly 0, whatever the row held
            scale = float(want_grad.abs().max())
            err = (got - want_grad).abs()
            bound = U_ROUND[dtype] * want_grad.abs() + 1e-6 * scale + (2.0 ** -25 if dtype == torch.float16 else 0.0)
            assert (err <= bound).all(), (what, float((err - bound).max()))
            if dtype == torch.float32:
                WORST["dpred_f32"] = max(WORST["dpred_f32"], float(err.max()) / scale)
            if kind == 0 and n > 2 and counted[1]:
                assert got[1] == 0                               # d = 0 under L1
    print("largest relative error of loss / mse, largest dpred error / scale (fp32):", WORST)


@pytest.mark.parametrize("kind", [0, 1], ids=["L1", "MSE"])
def test_no_counted_row_gives_nan_loss_and_zero_gradient(kind):
    pred, target, c, _counted = _inputs(65, torch.float32, True, 7)
    loss, mse, grad = _run(pred, target, c, kind, True, None, 0)
    assert torch.isnan(loss).item() and torch.isnan(mse).item() and (grad == 0).all().item()
    c[:, 0], c[:, 1] = 0, 0                                    # segment 0 is dead, not single-ended
    loss, _mse, grad = _run(pred, target, c, kind, True, _mask(), None)
    assert torch.isnan(loss).item() and (grad == 0).all().item()


@pytest.mark.parametrize("n", [1000, 5000])
def test_result_repeats_bit_for_bit_and_does_not_depend_on_the_launch_shape(n):
    mask = _mask()
    pred, target, c, _counted = _inputs(n, torch.float32, True, 11, n - 37, poison=True, mask=mask)
    runs = [_run(pred, target, c, 1, True, mask, n - 37, max_blocks=mb) for mb in (0, 0, 1, 2, 3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # nor on the rows' capacity: the same rows in a longer, padded buffer
    extra = 3000
    pred2 = torch.cat([pred, torch.full((extra,), float("nan"))])
    target2 = torch.cat([target, torch.full((extra, 8), PAD)])
    c2 = torch.cat([c, torch.zeros((extra, 3), dtype=torch.int32)])
    padded = _run(pred2, target2, c2, 1, True, mask, n - 37)
    assert torch.equal(padded[0], runs[0][0]) and torch.equal(padded[1], runs[0][1])
    assert torch.equal(padded[2][:n], runs[0][2]) and (padded[2][n:] == 0).all().item()


def test_fusion_decision_and_module_loss_match_torch():
    """can_fuse_regression_loss on GPU tensors; LitSegQuantifier's fused loss against its own torch composition (the path
    every other criterion takes), gradients into the net included."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litsegq import LitSegQuantifier
    from waveformml_amd.spconv import functional as Fsp
    p, t = torch.zeros(4, device=DEV), torch.zeros(4, 8, device=DEV)
    assert Fsp.can_fuse_regression_loss(torch.nn.L1Loss(), p, t) and Fsp.can_fuse_regression_loss(torch.nn.MSELoss(), p, t[:, 0])
    assert not Fsp.can_fuse_regression_loss(torch.nn.SmoothL1Loss(), p, t)
    assert not Fsp.can_fuse_regression_loss(torch.nn.L1Loss(reduction="sum"), p, t)
    cfg = json.load(open(CONFIG))
    rng = np.random.default_rng(31)
    rows, c, f = segment_rows(rng, 10, 6, 130)
    tg = torch.from_numpy(rng.random((len(rows), 8)).astype(np.float32))
    grads = []
    for fused in (True, False):
        torch.manual_seed(3)
        mod = LitSegQuantifier(load_config(copy.deepcopy(cfg))).to(DEV)
        if not fused:
            class L1Composition(torch.nn.L1Loss):                 # a subclass: not fused, same arithmetic
                pass
            mod.criterion, mod.criterion_none = L1Composition(), L1Composition(reduction="none")
            assert not Fsp.can_fuse_regression_loss(mod.criterion, p, t)
        out = mod.validation_step(([c.to(DEV), f.to(DEV)], tg.to(DEV)), 0)
        loss = mod.training_step(([c.to(DEV), f.to(DEV)], tg.to(DEV)), 0)
        loss.backward()
        grads.append((float(loss), float(out["val_mse"]),
                      torch.cat([q.grad.reshape(-1) for q in mod.model.parameters()]).cpu()))
    (l0, m0, g0), (l1, m1, g1) = grads
    assert abs(l0 - l1) <= 1e-5 * abs(l1) and abs(m0 - m1) <= 1e-5 * abs(m1)
    assert float((g0 - g1).abs().max()) <= 1e-4 * float(g1.abs().max())


def test_seg_quantifier_trains_through_the_captured_step():
    """Trainer eager against capture=True on config/segment_quantifier_z.json: the captured step pads rows and targets
    to its capacity (the padding targets hold the fill value, the padding rows exist: n_cap > rows) and follows the eager
    trainer: the same three losses, no eager fallback."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litsegq import LitSegQuantifier
    from waveformml_amd.psd.trainer import Trainer
    cfg = json.load(open(CONFIG))
    cfg["optimize_config"].update(lr=0.01, optimizer_params={"momentum": 0.9, "nesterov": True})
    rng = np.random.default_rng(12)
    batches = []
    for B in (44, 38):                                            # the capture sizes itself on its first batch
        rows, c, f = segment_rows(rng, B, 5, 130)
        batches.append(([c, f], torch.from_numpy(rng.random((len(rows), 8)).astype(np.float32))))
    assert batches[0][0][0].shape[0] > batches[1][0][0].shape[0]
    from waveformml_amd.psd.graph import GraphedTrainStep
    n0 = batches[0][0][0].shape[0]
    assert GraphedTrainStep.capacity_for(n0, n0) > n0           # padding rows behind every batch
    runs = []
    for capture in (False, True):
        torch.manual_seed(7)
        mod = LitSegQuantifier(load_config(copy.deepcopy(cfg)))
        tr = Trainer(max_epochs=3, device=DEV, capture=capture, check_every=2)
        hist = tr.fit(mod, [([c.clone(), f.clone()], y.clone()) for (c, f), y in batches])
        torch.cuda.synchronize()
        runs.append(([h["train_loss"] for h in hist], tr.eager_fallbacks))
    (h0, _), (h1, fb) = runs
    assert fb == 0 and len(h0) == 3
    for a, b in zip(h0, h1):
        assert np.isfinite(a) and abs(a - b) <= 1e-4 * abs(a), (h0, h1)
