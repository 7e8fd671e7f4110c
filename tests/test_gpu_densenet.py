"""The Conv2d + BatchNorm2d + ReLU (+ Dropout) stack kernels (wfs_conv2d_*, csrc/conv2d.hip) behind
Conv2DBlock(fused=True), the densify launch (wfs_densify_rows) and DenseConvNet under LitPSD on the GPU: forward, dX,
every parameter gradient and the running statistics against the torch composition in float64 on the CPU on the same
rounded inputs (training and eval mode), dropout with the masks rebuilt from the documented counter, determinism, the
fallbacks, one LitPSD step against the CPU module, the captured step against eager steps on capacity-padded batches, and
one forward + backward at the committed C1 shape.

The bars are the project's (waveform_cases.TOL): 1e-5 (fp32), 2e-2 (bf16), 3e-3 (fp16) of each tensor's max.  The
gradient of a conv bias in front of a training-mode BatchNorm is exactly zero (tests/test_gpu_convnet.py's docstring):
for exactly those tensors the same relative bars are taken against the summed |dz| of the reference.

Measured on an MI355X.  fp32: every tensor of all ten plans inside 1e-5 (worst 1.4e-6; the committed C1 shape 1.9e-6;
dropout 6.3e-7).  16-bit rows hold 2e-2 / 3e-3 because the forward keeps its operands in several 16-bit pieces
(csrc/conv2d.hip): with one-piece operands z differs from the float64 run by about 1e-3 of its deviation, some ReLU
masks come out on the other side of zero, and each such element moves dX and the few-hundred-term dW sums by a whole
term -- measured then: 16 of the 21 16-bit cases missed, dX by 7e-2 .. 2.3e-1 of its max.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import waveform_cases as wc
from waveform_cases import DEV, TOL, max_err as _max_err

pytestmark = pytest.mark.gpu

ROOT = wc.ROOT
H, W = 14, 11

CASES = {  # name -> (nin, nout, n, Conv2DBlock keyword arguments, B)
    "three-3x3-pad": (20, 6, 3, dict(pad_factor=1.), 3),                         # built by hand: see _build
    "no-pad-shrinks": (20, 5, 3, dict(), 3),
    "stride-2": (20, 6, 3, dict(size_factor=3, pad_factor=1., stride_factor=2.), 3),
    "dil-2": (20, 6, 2, dict(size_factor=3, pad_factor=1., dil_factor=2.), 3),
    "pointwise-first": (20, 6, 3, dict(size_factor=3, pad_factor=1., pointwise_factor=0.5), 3),
    "clamped-2x2": (20, 6, 3, dict(size_factor=1), 3),
    "bias": (20, 6, 2, dict(size_factor=3, pad_factor=1., trainable_weights=True), 3),
    "tails-300-252": (300, 158, 2, dict(size_factor=3, pad_factor=1., pointwise_factor=0.34), 2),
    "one-channel-out": (21, 1, 2, dict(size_factor=3, pad_factor=1.), 3),
    "expand": (12, 6, 3, dict(size_factor=3, pad_factor=1., expansion_factor=1.5, n_expansion=1), 3),
}
SIXTEEN_BIT = ["three-3x3-pad", "stride-2", "dil-2", "tails-300-252", "bias"]


def _build(name, fused=True):
    """The case's block.  `three-3x3-pad` is three size-preserving 3 x 3 layers 20 -> 12 -> 6: the reference's plan
    shrinks its kernels towards the last layer, so the block is built and its module list replaced (the kernels read
    the plan off the live modules)."""
    from waveformml_amd.psd.convnet2d import Conv2DBlock
    nin, nout, n, kw, _B = CASES[name]
    if name != "three-3x3-pad":
        return Conv2DBlock(nin, nout, n, [H, W, nin], fused=fused, **kw)
    block = Conv2DBlock(nin, nout, 2, [H, W, nin], fused=fused, pad_factor=1.)
    chans, mods = [20, 20, 12, 6], []
    for i in range(3):
        mods += [nn.Conv2d(chans[i], chans[i + 1], (3, 3), (1, 1), 1, (1, 1), 1, False), nn.BatchNorm2d(chans[i + 1]),
                 nn.ReLU()]
    block.model = nn.Sequential(*mods)
    return block


def _randomise(block, seed):
    """Live parameters: taps of order 1 / sqrt(fan), BN scale in [0.5, 1.5] and shift ~ N(0, 0.3), running statistics
    away from their (0, 1) start."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in block.model:
            if isinstance(m, nn.Conv2d):
                fan = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _pair(name, seed=0, dropout=None):
    gpu = _build(name)
    if dropout:
        mods = []
        for m in gpu.model:
            mods.append(m)
            if isinstance(m, nn.ReLU):
                mods.append(nn.Dropout(dropout))
        gpu.model = nn.Sequential(*mods)
    _randomise(gpu, seed)
    ref = copy.deepcopy(gpu).double()
    return gpu.to(DEV), ref


def _reference(ref, x, dy, masks=None):
    """The float64 composition layer by layer: (y, dx, [gradient at each conv output], [each layer's activation]);
    ``masks``: the dropout multipliers per layer, applied where the Dropout modules stand."""
    xr = x.double().requires_grad_(True)
    h, zs, acts, layer = xr, [], [], -1
    for m in ref.model:
        if isinstance(m, nn.Conv2d):
            layer += 1
            h = m(h)
            h.retain_grad()
            zs.append(h)
        elif isinstance(m, nn.Dropout):
            if masks is not None:
                h = h * masks[layer]
        else:
            h = m(h)
            if isinstance(m, nn.ReLU):
                acts.append(h)
    h.backward(dy.double())
    return h, xr.grad, [z.grad for z in zs], acts


def _compare(gpu, ref, y, yr, dx, dxr, dzs, tol, training, label):
    pairs = [("y", y, yr, None)]
    if dx is not None:
        pairs.append(("dx", dx, dxr, None))
    convs = [m for m in ref.model if isinstance(m, nn.Conv2d)]
    bias_scale = {id(c.bias): float(dz.abs().sum((0, 2, 3)).max()) for c, dz in zip(convs, dzs) if c.bias is not None}
    for (n, a), b in zip(gpu.named_parameters(), ref.parameters()):
        # a conv bias under batch statistics: exact gradient zero, bar against the summed terms (module docstring)
        pairs.append((n, a.grad, b.grad, bias_scale[id(b)] if (training and id(b) in bias_scale) else None))
    for (n, a), b in zip(gpu.named_buffers(), ref.buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(a) == int(b), (n, int(a), int(b))
        else:
            pairs.append((n, a, b, None))
    missed = []
    for name, a, b, scale_override in pairs:
        err, scale = _max_err(a, b)
        if scale_override is not None:
            scale = scale_override
        print("%s %s: max err %.3e of scale %.3e (%.2e)" % (label, name, err, scale, err / max(scale, 1e-300)))
        if not (scale > 0 and err <= tol * scale):
            missed.append((name, "%.2e of the scale, bar %.0e" % (err / max(scale, 1e-300), tol)))
    assert not missed, (label, missed)


def _inputs(name, gpu, dtype, seed):
    nin, B = CASES[name][0], CASES[name][4]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        shape = gpu.cpu().eval()(torch.zeros(B, nin, H, W)).shape
    gpu.to(DEV)
    x = torch.randn(B, nin, H, W, generator=g).to(dtype)              # the rounded inputs both sides see
    dy = torch.randn(shape, generator=g).to(dtype)
    return x, dy


def _run(name, dtype, training, want_dx=True):
    from waveformml_amd.psd import convnet2d
    gpu, ref = _pair(name, seed=len(name))
    x, dy = _inputs(name, gpu, dtype, seed=len(name) + 3)
    gpu.train(training), ref.train(training)
    xg = x.to(DEV).requires_grad_(want_dx)
    before = convnet2d.CONV2D_CALLS[0]
    y = gpu(xg)
    assert convnet2d.CONV2D_CALLS[0] == before + 1 and y.dtype == dtype and y.shape == dy.shape and y.is_contiguous()
    y.backward(dy.to(DEV))
    yr, dxr, dzs, acts = _reference(ref, x, dy)
    for i, a in enumerate(acts):                                      # a live net: every layer has ReLUs on AND off
        frac = float((a > 0).double().mean())
        assert 0.05 < frac < 0.95, (i, frac)
    assert float(yr.abs().max()) > 0 and float(dxr.abs().max()) > 0
    _compare(gpu, ref, y, yr, xg.grad if want_dx else None, dxr, dzs, TOL[dtype], training,
             "%s %s %s" % (name, dtype, "train" if training else "eval"))
    return gpu, ref


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(CASES))
def test_stack_fp32_against_float64(name, training):
    _run(name, torch.float32, training)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", SIXTEEN_BIT)
def test_stack_16_bit_rows_against_float64(name, dtype, training):
    _run(name, dtype, training)


def test_the_cases_are_the_plans_they_are_named_for():
    plans = {name: _build(name)._plan()[0] for name in CASES}
    assert plans["three-3x3-pad"] == (20, (20, 12, 6), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1))
    assert plans["no-pad-shrinks"][4] == (0, 0, 0) and _build("no-pad-shrinks").out_size == [10, 7, 5]
    assert plans["stride-2"][3] == (1, 1, 2)
    assert plans["dil-2"][4:] == ((2, 0), (1, 2))                                # padding 2 on the dilation-1 layer
    assert plans["pointwise-first"][2] == (1, 3, 2)
    assert plans["clamped-2x2"][2] == (2, 2, 2)
    assert plans["tails-300-252"][:2] == (300, (252, 158))
    assert plans["one-channel-out"][1][-1] == 1 and max(plans["expand"][1]) > plans["expand"][0]


def test_no_input_gradient_when_none_is_asked():
    _run("three-3x3-pad", torch.float32, True, want_dx=False)


def _dropout_masks(gpu, shapes, seed, p):
    masks = []
    for layer, shape in enumerate(shapes):
        n = int(np.prod(shape))
        ctr = (np.uint64(layer) << np.uint64(44)) + np.arange(n, dtype=np.uint64)      # include/wfsparse.h
        masks.append(wc.hash_masks(seed, p, ctr).reshape(shape))
    return masks


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_dropout_masks_are_the_documented_ones(dtype):
    from waveformml_amd.psd import convnet2d
    name, p = "three-3x3-pad", 0.3
    gpu, ref = _pair(name, seed=4, dropout=p)
    assert [type(m).__name__ for m in gpu.model][:4] == ["Conv2d", "BatchNorm2d", "ReLU", "Dropout"]
    x, dy = _inputs(name, gpu, dtype, seed=9)
    gpu.train(), ref.train()
    seed = torch.tensor([123456789012345], dtype=torch.int64, device=DEV)
    xg = x.to(DEV).requires_grad_(True)
    before = convnet2d.CONV2D_CALLS[0]
    y = gpu(xg, seed=seed)
    assert convnet2d.CONV2D_CALLS[0] == before + 1
    y.backward(dy.to(DEV))
    shapes = [(3, c, H, W) for c in (20, 12, 6)]
    masks = _dropout_masks(gpu, shapes, int(seed), p)
    assert 0.2 < float((masks[0] == 0).double().mean()) < 0.4
    yr, dxr, dzs, _acts = _reference(ref, x, dy, masks)
    _compare(gpu, ref, y, yr, xg.grad, dxr, dzs, TOL[dtype], True, "dropout %s" % dtype)
    # another seed: other masks; eval mode: none
    with torch.no_grad():
        y2 = gpu(x.to(DEV), seed=seed + 1)
        y3 = gpu(x.to(DEV), seed=seed + 1)
        assert not torch.equal(y2, y) and torch.equal(y2, y3)
        torch.manual_seed(1)
        y4 = gpu(x.to(DEV))                                           # a drawn seed
        y5 = gpu(x.to(DEV))
        assert not torch.equal(y4, y5)
        gpu.eval(), ref.eval()
        # the four extra training calls above moved the GPU module's running statistics: the reference takes them
        ref.load_state_dict({k: (v.double() if v.is_floating_point() else v).cpu() for k, v in gpu.state_dict().items()})
        ye = gpu(x.to(DEV), seed=seed)
        err, scale = _max_err(ye, ref.model(x.double()))
        assert err <= TOL[dtype] * scale


def test_two_runs_are_bit_equal():
    outs = []
    for _ in range(2):
        gpu, _ref = _pair("tails-300-252", seed=2)
        x, dy = _inputs("tails-300-252", gpu, torch.bfloat16, seed=5)
        gpu.train()
        xg = x.to(DEV).requires_grad_(True)
        y = gpu(xg)
        y.backward(dy.to(DEV))
        outs.append([y.detach(), xg.grad] + [p.grad for p in gpu.parameters()] + [b.clone() for b in gpu.buffers()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _rows(B, n, C, dtype, seed, skip_event=None):
    g = torch.Generator().manual_seed(seed)
    cells = torch.randperm(B * H * W, generator=g)[:n].sort().values
    if skip_event is not None:
        cells = cells[(cells // (H * W)) != skip_event]
    coords = torch.stack([(cells % (H * W)) // W, cells % W, cells // (H * W)], 1).to(torch.int32)
    return coords, torch.randn(coords.shape[0], C, generator=g).to(dtype)


def _to_dense(coords, feats, B):
    idx = coords[:, [2, 0, 1]].long().t()
    return torch.sparse_coo_tensor(idx, feats.float(), size=[B, H, W, feats.shape[1]]).to_dense().to(feats.dtype).permute(0, 3, 1, 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_densify_is_to_dense_bit_for_bit(dtype):
    from waveformml_amd.psd.convnet2d import densify_rows
    B, C = 5, 37
    coords, feats = _rows(B, 200, C, dtype, seed=1, skip_event=2)          # event 2 has no rows
    assert 2 not in coords[:, 2].tolist() and {1, 3} <= set(coords[:, 2].tolist())
    want = _to_dense(coords, feats, B)
    got = densify_rows(feats.to(DEV), coords.to(DEV), B, H, W)
    assert got.shape == (B, C, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.cpu(), want) and float(want[2].abs().max()) == 0
    # a capacity-padded batch: rows beyond n_valid hold stale data and out-of-range coordinates
    n = coords.shape[0]
    pad_c = torch.tensor([[99, 3, 1], [3, -7, 1], [2, 2, 77], [-1, -1, -1], [1 << 30, 1 << 30, 1 << 30]], dtype=torch.int32)
    cc = torch.cat([coords, pad_c, coords[:7]])
    ff = torch.cat([feats, torch.full((12, C), 7.0).to(dtype)])
    for n_valid in (n, n - 31, 0):
        nv = torch.tensor([n_valid], dtype=torch.int64, device=DEV)
        got = densify_rows(ff.to(DEV), cc.to(DEV), B, H, W, nv)
        assert torch.equal(got.cpu(), _to_dense(coords[:n_valid], feats[:n_valid], B)), n_valid
    # out-of-range coordinates among the VALID rows are skipped too, and int64 coordinates are taken
    got = densify_rows(ff[: n + 5].to(DEV), cc[: n + 5].long().to(DEV), B, H, W)
    assert torch.equal(got.cpu(), want)
    # equal coordinates are summed, as to_dense sums them (fp32: two terms, order-free)
    if dtype == torch.float32:
        c2, f2 = torch.cat([coords, coords[:9]]), torch.cat([feats, feats[:9] * 0.5])
        got = densify_rows(f2.to(DEV), c2.to(DEV), B, H, W)
        assert torch.equal(got.cpu(), _to_dense(c2, f2, B))


def test_fallbacks_take_the_torch_path():
    from waveformml_amd.psd import convnet2d
    from waveformml_amd.psd.convnet2d import Conv2DBlock
    x = torch.randn(3, 20, H, W)
    before = convnet2d.CONV2D_CALLS[0]
    cpu = _build("stride-2")
    assert cpu.can_fuse(x) is None and cpu(x).shape == (3, 5, 6, 5)                 # a CPU tensor
    off = _build("stride-2", fused=False).to(DEV)
    assert off.can_fuse(x.to(DEV)) is None and off(x.to(DEV)).shape == (3, 5, 6, 5)  # the flag off
    big = Conv2DBlock(20, 6, 2, [H, W, 20], size_factor=7, pad_factor=1., fused=True).to(DEV)
    assert big._plan()[0][2][0] == 7 and big.can_fuse(x.to(DEV)) is None             # a 7 x 7 kernel: out of bounds
    assert big(x.to(DEV)).shape[1] == 6
    mom = _build("stride-2").to(DEV)
    mom.model[1].momentum = None                                                    # cumulative average: not the kernels'
    assert mom.can_fuse(x.to(DEV)) is None and mom(x.to(DEV)).shape == (3, 5, 6, 5)
    assert _build("stride-2").to(DEV).can_fuse(x.to(DEV).double()) is None
    assert convnet2d.CONV2D_CALLS[0] == before
    ok = _build("stride-2").to(DEV)
    assert ok.can_fuse(x.to(DEV)) is not None and ok(x.to(DEV)).shape == (3, 5, 6, 5)
    assert convnet2d.CONV2D_CALLS[0] == before + 1


def _c1_config(n_samples=10):
    with open(os.path.join(ROOT, "config", "psd_c1_dense.json")) as f:
        cfg = json.load(f)
    cfg["system_config"]["n_samples"] = n_samples
    cfg["optimize_config"].pop("scheduler_class", None)
    return cfg


def _lit(cfg, seed=7):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(seed)
    m = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
    _randomise(m.model.model, seed)
    return m


def _batch(n, B, C, seed, dev="cpu"):
    coords, feats = _rows(B, n, C, torch.float32, seed)
    coords[-1, 2] = B - 1
    g = torch.Generator().manual_seed(seed + 100)
    y = torch.randint(0, 2, (B,), generator=g)
    return ([coords.to(dev), feats.abs().to(dev)], y.to(dev))


def test_n_valid_with_a_call_the_kernels_do_not_take_raises():
    net = _lit(_c1_config()).model.to(DEV)
    b = _batch(30, 8, 20, seed=3, dev=DEV)
    net.batch_size_hint = 8
    nv = torch.tensor([30], dtype=torch.int64, device=DEV)
    assert net([b[0][0], b[0][1], nv]).shape == (8, 2)
    net.model.fused = False
    with pytest.raises(RuntimeError):
        net([b[0][0], b[0][1], nv])
    assert net([b[0][0], b[0][1]]).shape == (8, 2)


def test_one_lit_psd_training_step_against_the_cpu_module():
    from waveformml_amd.psd import convnet2d
    cfg = _c1_config()
    gpu, cpu = _lit(cfg), _lit(cfg)
    cpu.load_state_dict(gpu.state_dict())
    gpu = gpu.to(DEV).train()
    cpu.train()
    b = _batch(30, 8, 20, seed=3)
    before = convnet2d.CONV2D_CALLS[0]
    lg = gpu.training_step(([b[0][0].to(DEV), b[0][1].to(DEV)], b[1].to(DEV)), 0)
    assert convnet2d.CONV2D_CALLS[0] == before + 1
    lc = cpu.training_step(b, 0)
    print("loss gpu %.8f cpu %.8f" % (lg.item(), lc.item()))
    assert abs(lg.item() - lc.item()) <= 1e-5 * abs(lc.item())
    lg.backward()
    lc.backward()
    for (n, a), p in zip(gpu.model.named_parameters(), cpu.model.parameters()):
        err, scale = _max_err(a.grad, p.grad)
        print("%s: %.3e of %.3e" % (n, err, scale))
        assert err <= 1e-4 * scale, (n, err, scale)
    for (n, a), p in zip(gpu.model.named_buffers(), cpu.model.buffers()):
        err, scale = _max_err(a, p)
        assert err <= 1e-5 * max(scale, 1.0), (n, err, scale)


def test_captured_step_matches_eager_steps_on_padded_batches():
    from waveformml_amd.psd import convnet2d
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.graph import GraphedTrainStep
    cfg = _c1_config()
    batches = [_batch(n, 8, 20, seed=40 + n, dev=DEV) for n in (60, 41, 66, 52)]

    def make():
        mod = _lit(cfg).to(DEV)
        red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
        mod.optimizer_parameters = red.optimizer_parameters()
        return mod, red, mod.configure_optimizers()

    mod_g, red_g, opt_g = make()
    mod_e, red_e, opt_e = make()
    assert torch.equal(red_g.flat_param, red_e.flat_param)
    start = red_g.flat_param.clone()
    calls = convnet2d.CONV2D_CALLS[0]
    step = GraphedTrainStep(mod_g, opt_g, red_g, batches[0], warmup=2)
    assert convnet2d.CONV2D_CALLS[0] > calls and step.n_cap > 66 and not step.per_row
    for _ in range(3):                                       # the calibration step and the two warm-up steps
        wc.eager_step(mod_e, red_e, opt_e, batches[0])
    scale = float(red_e.flat_param.abs().max())
    assert float((red_e.flat_param - start).abs().max()) > 0
    assert float((red_g.flat_param - red_e.flat_param).abs().max()) <= 2e-5 * scale
    for b in batches[1:]:
        lg = float(step(b))
        le = wc.eager_step(mod_e, red_e, opt_e, b)
        print("rows %d of %d: loss captured %.8f eager %.8f" % (b[0][0].shape[0], step.n_cap, lg, le))
        assert abs(lg - le) <= 1e-5 * abs(le), (lg, le)
        assert float((red_g.flat_param - red_e.flat_param).abs().max()) <= 2e-5 * scale
    step.check()
    step.close()


def test_full_c1_shape_forward_and_backward_fp32():
    """config/psd_c1_dense.json as committed: batch 32, 300 channels, the block 300 -> 221 -> 142 -> 63."""
    from waveformml_amd.psd import convnet2d
    from waveformml_amd.psd.convnet2d import Conv2DBlock
    with open(os.path.join(ROOT, "config", "psd_c1_dense.json")) as f:
        cfg = json.load(f)
    hp = cfg["net_config"]["hparams"]
    B, C = cfg["dataset_config"]["dataloader_params"]["batch_size"], 2 * cfg["system_config"]["n_samples"]
    gpu = Conv2DBlock(C, hp["out_planes"], hp["n_conv"], [H, W, C], fused=True, **hp["conv_params"])
    assert (B, C, gpu.nframes) == (32, 300, [300, 221, 142, 63])
    _randomise(gpu, 11)
    ref = copy.deepcopy(gpu).double()
    gpu = gpu.to(DEV).train()
    ref.train()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=g)
    dy = torch.randn(B, 63, 12, 9, generator=g)
    before = convnet2d.CONV2D_CALLS[0]
    y = gpu(x.to(DEV))
    assert convnet2d.CONV2D_CALLS[0] == before + 1
    y.backward(dy.to(DEV))
    yr, dxr, dzs, _acts = _reference(ref, x, dy)
    _compare(gpu, ref, y, yr, None, dxr, dzs, TOL[torch.float32], True, "C1 batch 32 fp32")
