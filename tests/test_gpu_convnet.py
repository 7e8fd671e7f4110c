"""The Conv1d + BatchNorm1d + ReLU stack kernels (wfs_conv1d_*, csrc/conv1d.hip) behind Conv1DNet(fused=True),
ConvWaveformNet, LinearWaveformNet and LitWaveform on the GPU: forward, dX, every parameter gradient and the running
statistics against the torch composition in float64 on the CPU (training and eval mode), the device-side valid-row
count, determinism, the bounds, one LitWaveform step against the CPU module, the captured step against the eager one on
padded batches, and Trainer(capture=True) from the r3 pulse fixture.

The gradient of a conv bias in front of a training-mode BatchNorm.  BatchNorm subtracts the batch mean, so the loss does
not depend on that bias: its exact gradient, sum(dz) over rows and samples with dz the gradient at the conv's output,
is ZERO, and what any implementation returns is the rounding residue of a sum of cancelling terms (float64: ~1e-16 of
the terms; fp32: ~1e-7).  A bar "relative to the tensor's max" compares residue with residue there.  For exactly these
tensors the checks below therefore scale the same relative bars by what the sum is made of -- max over channels of
sum |dz| of the reference -- instead of by the tensor's max.  Every other tensor, and the same biases in eval mode (where
the gradient is not zero), is held to the bar against its own max.
"""
import copy
import re

import pytest
import torch
from torch import nn

import waveform_cases as wc
from waveform_cases import DEV, TOL, max_err as _max_err

pytestmark = pytest.mark.gpu

COMMITTED = dict(num_channels=1, out_size=8, num_expand=2, num_contract=2, expand_factor=16, size_factor=5, pad_factor=1,
                 stride_factor=2, min_kernel=2)

CASES = {  # name -> (L, Conv1DNet arguments)
    "committed-59": (59, COMMITTED),
    "committed-62": (62, COMMITTED),          # ... with use_detector_number's three extra samples in the conv stack
    "one-layer": (59, dict(num_channels=1, out_size=4, num_expand=0, num_contract=1, expand_factor=1, size_factor=3,
                           pad_factor=1, stride_factor=0)),
    "stride-3": (62, dict(num_channels=2, out_size=5, num_expand=1, num_contract=2, expand_factor=4, size_factor=6,
                          pad_factor=1, stride_factor=3)),
    "min-kernel-no-pad": (59, dict(num_channels=1, out_size=3, num_expand=1, num_contract=1, expand_factor=6,
                                   size_factor=1, pad_factor=0, stride_factor=0, min_kernel=2)),
    "long-1024": (1024, dict(num_channels=1, out_size=4, num_expand=1, num_contract=1, expand_factor=12, size_factor=7,
                             pad_factor=1, stride_factor=2)),
    "bound-64ch-k16": (59, dict(num_channels=4, out_size=16, num_expand=1, num_contract=1, expand_factor=16,
                                size_factor=16, pad_factor=1, stride_factor=0)),
}


def _randomise(net, seed):
    """Live parameters: taps of order 1, BN scale in [0.5, 1.5] and shift ~ N(0, 0.3) (non-trivial), running statistics
    away from their (0, 1) start."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.network:
            if isinstance(m, nn.Conv1d):
                fan = m.in_channels * m.kernel_size[0]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / fan ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
            elif isinstance(m, nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


def _pair(L, kw, seed=0):
    from waveformml_amd.psd.convnet import Conv1DNet
    gpu = Conv1DNet(L, fused=True, **kw)
    _randomise(gpu, seed)
    ref = Conv1DNet(L, **kw).double()
    ref.load_state_dict({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in gpu.state_dict().items()})
    return gpu.to(DEV), ref


def _reference(ref, x, dy):
    """The float64 composition layer by layer: (y, dx, [gradient at each conv output], [each layer's activation])."""
    xr = x.double().requires_grad_(True)
    h, zs, acts = xr, [], []
    mods = list(ref.network)
    for i in range(0, len(mods), 3):
        z = mods[i](h)
        z.retain_grad()
        zs.append(z)
        h = mods[i + 2](mods[i + 1](z))
        acts.append(h)
    h.backward(dy.double())
    return h, xr.grad, [z.grad for z in zs], acts


def _compare(gpu, ref, y, yr, dx, dxr, dzs, tol, training, label):
    pairs = [("y", y, yr, None), ("dx", dx, dxr, None)]
    convs = [m for m in ref.network if isinstance(m, nn.Conv1d)]
    bias_scale = {id(c.bias): float(dz.abs().sum((0, 2)).max()) for c, dz in zip(convs, dzs)}
    for (n, a), b in zip(gpu.named_parameters(), ref.parameters()):
        # a conv bias under batch statistics: exact gradient zero, bar against the summed terms (module docstring)
        pairs.append((n, a.grad, b.grad, bias_scale[id(b)] if (training and id(b) in bias_scale) else None))
    for (n, a), b in zip(gpu.named_buffers(), ref.buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(a) == int(b), (n, int(a), int(b))
        else:
            pairs.append((n, a, b, None))
    for name, a, b, scale_override in pairs:
        err, scale = _max_err(a, b)
        if scale_override is not None:
            scale = scale_override
        print("%s %s: max err %.3e of scale %.3e (%.2e)" % (label, name, err, scale, err / max(scale, 1e-300)))
        assert scale > 0 and err <= tol * scale, (name, err, scale)


def _run(name, dtype, training, N=6):
    from waveformml_amd.psd import convnet
    L, kw = CASES[name]
    gpu, ref = _pair(L, kw, seed=L + len(name))
    gpu.train(training), ref.train(training)
    g = torch.Generator().manual_seed(L + 3)
    c0 = kw["num_channels"]
    lout, cout = gpu.out_size
    x = torch.randn(N, c0, L, generator=g).to(dtype)             # the rounded inputs both sides see
    dy = torch.randn(N, cout, lout, generator=g).to(dtype)
    xg = x.to(DEV).requires_grad_(True)
    before = convnet.CONV1D_CALLS[0]
    y = gpu(xg)
    assert convnet.CONV1D_CALLS[0] == before + 1 and y.dtype == dtype and y.shape == (N, cout, lout)
    y.backward(dy.to(DEV))
    yr, dxr, dzs, acts = _reference(ref, x, dy)
    for i, a in enumerate(acts):                                  # a live net: every layer has ReLUs on AND off
        frac = float((a > 0).double().mean())
        assert 0.05 < frac < 0.95, (i, frac)
    assert float(yr.abs().max()) > 0 and float(dxr.abs().max()) > 0
    _compare(gpu, ref, y, yr, xg.grad, dxr, dzs, TOL[dtype], training, "%s %s %s" % (name, dtype, "train" if training else "eval"))
    return gpu, ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_training_forward_dx_parameter_gradients_and_running_statistics_against_float64(name, dtype):
    gpu, _ref = _run(name, dtype, training=True)
    for m in gpu.network:
        if isinstance(m, nn.BatchNorm1d):
            assert int(m.num_batches_tracked) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", ["committed-59", "stride-3", "bound-64ch-k16"])
def test_eval_mode_uses_the_running_statistics_against_float64(name, dtype):
    gpu, _ref = _run(name, dtype, training=False)
    for m in gpu.network:
        if isinstance(m, nn.BatchNorm1d):
            assert int(m.num_batches_tracked) == 0                # ... and leaves them alone (compared in _run)


@pytest.mark.parametrize("name", ["committed-59", "stride-3"])
def test_rows_beyond_the_device_valid_count_take_no_part(name):
    """N rows padded with NaN / huge rows to N + P, n_valid = N on the device, against the unpadded N-row call on an
    identical net: Y[:N], dX[:N], every parameter gradient and the running statistics within the fp32 bar; dX[N:] exactly
    zero, Y[N:] zero."""
    from waveformml_amd.psd import convnet
    L, kw = CASES[name]
    N, P = 37, 11
    a, _ = _pair(L, kw, seed=5)
    b, ref = _pair(L, kw, seed=5)
    a.train(), b.train(), ref.train()
    g = torch.Generator().manual_seed(9)
    lout, cout = a.out_size
    x = torch.randn(N, kw["num_channels"], L, generator=g)
    dy = torch.randn(N, cout, lout, generator=g)
    junk = torch.full((P, kw["num_channels"], L), float("nan"))
    junk[::2] = 3e30
    xp = torch.cat([x, junk]).to(DEV).requires_grad_(True)
    dyp = torch.cat([dy, torch.full((P, cout, lout), float("nan"))]).to(DEV)
    n_valid = torch.tensor([N], dtype=torch.int64, device=DEV)
    before = convnet.CONV1D_CALLS[0]
    yp = a(xp, n_valid=n_valid)
    yp.backward(dyp)
    xb = x.to(DEV).requires_grad_(True)
    yb = b(xb)
    yb.backward(dy.to(DEV))
    assert convnet.CONV1D_CALLS[0] == before + 2
    assert torch.equal(xp.grad[N:], torch.zeros_like(xp.grad[N:])) and torch.equal(yp[N:], torch.zeros_like(yp[N:]))
    pairs = [("y", yp[:N], yb), ("dx", xp.grad[:N], xb.grad)]
    pairs += [(n, p.grad, q.grad) for (n, p), q in zip(a.named_parameters(), b.parameters())]
    pairs += [(n, p, q) for (n, p), q in zip(a.named_buffers(), b.buffers())]
    _yr, _dxr, dzs, _acts = _reference(ref, x, dy)
    summed = {"network.%d.bias" % (3 * i): float(dz.abs().sum((0, 2)).max()) for i, dz in enumerate(dzs)}
    for n, p, q in pairs:
        assert bool(torch.isfinite(p.double()).all()), n
        err, scale = _max_err(p, q)
        if n in summed:                     # a conv bias under batch statistics (module docstring): the summed |dz|
            scale = summed[n]
        print("n_valid %s %s: max err %.3e of scale %.3e" % (name, n, err, scale))
        assert err <= 1e-5 * scale, (n, err, scale)


def test_two_identical_calls_are_bit_identical():
    gpu, _ref = _pair(59, COMMITTED, seed=3)
    gpu.train()
    x = torch.randn(300, 1, 59, device=DEV)
    dy = torch.randn((300,) + tuple(reversed(gpu.out_size)), device=DEV)
    state = copy.deepcopy(gpu.state_dict())
    outs = []
    for _ in range(2):
        gpu.load_state_dict(state)
        gpu.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = gpu(xg)
        y.backward(dy)
        outs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in gpu.parameters()]
                    + [b.clone() for b in gpu.buffers()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_bounds_take_the_torch_composition_and_the_flag_off_never_calls_the_kernels():
    from waveformml_amd import _lib
    from waveformml_amd.psd import convnet
    lib = _lib.load()
    i32 = _lib.i32_array

    def ok(c0, ch, fs, st, pd, L):
        return lib.wfs_conv1d_ok(c0, i32(ch), i32(fs), i32(st), i32(pd), len(ch), L, _lib.WFS_F32)
    assert ok(64, [64] * 8, [16] * 8, [1] * 8, [15] * 8, 4096) == _lib.WFS_OK
    assert ok(1, [8], [3], [8], [1], 59) == _lib.WFS_OK
    assert ok(1, [65], [3], [1], [1], 59) == _lib.WFS_EINVAL
    assert ok(65, [8], [3], [1], [1], 59) == _lib.WFS_EINVAL
    assert ok(1, [8], [17], [1], [1], 59) == _lib.WFS_EINVAL
    assert ok(1, [8], [3], [9], [1], 59) == _lib.WFS_EINVAL
    assert ok(1, [8], [3], [1], [3], 59) == _lib.WFS_EINVAL          # pd < fs
    assert ok(1, [8] * 9, [3] * 9, [1] * 9, [1] * 9, 59) == _lib.WFS_EINVAL
    assert ok(1, [8], [3], [1], [1], 4097) == _lib.WFS_EINVAL
    assert ok(1, [8, 8], [8, 8], [1, 1], [0, 0], 10) == _lib.WFS_EINVAL   # second layer: 3 samples under a kernel of 8
    outside = [
        (59, dict(num_channels=1, out_size=8, num_expand=1, num_contract=1, expand_factor=65)),                  # channels
        (59, dict(num_channels=1, out_size=4, num_expand=1, num_contract=1, expand_factor=4, size_factor=17)),   # fs
        (200, dict(num_channels=1, out_size=4, num_expand=1, num_contract=1, expand_factor=4, stride_factor=9)),  # st
        (4100, dict(num_channels=1, out_size=4, num_expand=1, num_contract=1, expand_factor=4)),                 # L
        (59, dict(num_channels=1, out_size=4, num_expand=4, num_contract=5, expand_factor=4, size_factor=3)),    # layers
    ]
    for L, kw in outside:
        gpu, ref = _pair(L, kw, seed=9)
        gpu.eval(), ref.eval()
        x = torch.randn(3, 1, L)
        before = convnet.CONV1D_CALLS[0]
        with torch.no_grad():
            y = gpu(x.to(DEV))
            with pytest.raises(RuntimeError):                      # a valid-row count needs the kernels
                gpu(x.to(DEV), n_valid=torch.tensor([2], dtype=torch.int64, device=DEV))
        assert convnet.CONV1D_CALLS[0] == before                   # the torch composition ran
        err, scale = _max_err(y, ref(x.double()))
        assert err <= 1e-5 * scale
    # a BatchNorm the kernels do not compute: no momentum (cumulative average), no affine parameters
    for edit in ("momentum", "affine"):
        gpu, _ = _pair(59, COMMITTED)
        if edit == "momentum":
            gpu.network[1].momentum = None
        else:
            gpu.network[1] = nn.BatchNorm1d(8, affine=False).to(DEV)
        before = convnet.CONV1D_CALLS[0]
        gpu(torch.randn(4, 1, 59, device=DEV))
        assert convnet.CONV1D_CALLS[0] == before
    gpu, _ = _pair(59, COMMITTED)
    before = convnet.CONV1D_CALLS[0]
    gpu(torch.randn(4, 1, 59, device=DEV))
    assert convnet.CONV1D_CALLS[0] == before + 1
    gpu.fused = False
    gpu(torch.randn(4, 1, 59, device=DEV))
    assert convnet.CONV1D_CALLS[0] == before + 1
    # ConvWaveformNet turns the flag on, a plain Conv1DNet leaves it off
    assert not convnet.Conv1DNet(59, **COMMITTED).fused


# ---- LitWaveform on config/waveform_cnn_z.json

def _reinit(m, _cfg, seed):
    net = m.model.model if hasattr(m.model, "model") else None
    if net is not None:
        _randomise(net, seed)
    else:                                   # LinearWaveformNet ends in a ReLU: keep its outputs on
        with torch.no_grad():
            for mod in m.model.modules():
                if isinstance(mod, nn.Linear):
                    mod.bias.abs_().add_(0.2)


def _conv1d_calls():
    from waveformml_amd.psd import convnet
    return convnet.CONV1D_CALLS[0]


LIT = wc.LitCase("waveform_cnn_z.json", _conv1d_calls, _reinit)
LIT_LINEAR = wc.LitCase("waveform_cnn_z.json", lambda: 0, _reinit)


def _one_training_step_against_the_cpu_module(case, cfg, criterion, kernel_calls):
    """waveform_cases.check_one_training_step_against_the_cpu_module with one amendment: one LitWaveform.training_step on
    the GPU (exactly ``kernel_calls`` calls into the conv-stack kernels) against the same module on the CPU, the loss
    within 1e-5, every parameter gradient within 1e-4 of its max -- except the conv biases in front of the training-mode
    BatchNorms, whose exact gradient is zero (module docstring): there both sides hold rounding residue, the shared
    body's bar would compare residue with 1e-4 of residue, and the bar is 1e-4 of the summed |dz| the CPU module's
    backward saw at that conv's output instead."""
    gpu = wc.make_lit(case, cfg)
    cpu = wc.make_lit(case, cfg)
    cpu.load_state_dict(gpu.state_dict())
    gpu = gpu.to(DEV).train()
    cpu.train()
    summed = {}
    for name, mod in cpu.model.named_modules():
        if isinstance(mod, nn.Conv1d):
            mod.register_full_backward_hook(
                lambda _m, _gi, go, key=name + ".bias": summed.__setitem__(key, float(go[0].abs().sum((0, 2)).max())))
    b = wc.make_batch(500, 59, criterion, seed=3)
    before = case.calls()
    lg = gpu.training_step(([b[0][0].to(DEV), b[0][1].to(DEV)], b[1].to(DEV)), 0)
    assert case.calls() == before + kernel_calls
    lc = cpu.training_step(b, 0)
    print("%s: loss gpu %.8f cpu %.8f" % (criterion, lg.item(), lc.item()))
    assert abs(lg.item() - lc.item()) <= 1e-5 * abs(lc.item())
    lg.backward()
    lc.backward()
    live = 0
    for (n, a), p in zip(gpu.model.named_parameters(), cpu.model.parameters()):
        err, scale = _max_err(a.grad, p.grad)
        if n in summed:
            scale = summed[n]
        print("%s %s: max err %.3e of scale %.3e" % (criterion, n, err, scale))
        assert err <= 1e-4 * scale, (n, err, scale)
        live += scale > 0
    assert live == len(list(gpu.model.parameters()))
    return gpu


@pytest.mark.parametrize("detector", [False, True], ids=["rows", "detector"])
@pytest.mark.parametrize("criterion", ["L1Loss", "CrossEntropyLoss"])
def test_lit_waveform_one_training_step_against_the_cpu_module(criterion, detector):
    cfg = wc.lit_config(LIT, criterion, detector)
    gpu = _one_training_step_against_the_cpu_module(LIT, cfg, criterion, kernel_calls=1)
    assert gpu.model.nsamples == (62 if detector else 59)
    widths = [m.in_features for m in gpu.model.linear.net if isinstance(m, nn.Linear)]
    assert widths[0] == (227 if detector else 224)
    for m in gpu.model.model.network:
        if isinstance(m, nn.BatchNorm1d):
            assert int(m.num_batches_tracked) == 1


@pytest.mark.parametrize("criterion", ["L1Loss", "CrossEntropyLoss"])
def test_captured_step_matches_the_eager_step_on_padded_batches(criterion):
    """The eager side normalises over each batch's own rows; the captured side sees the same rows inside a padded buffer
    whose tail holds earlier batches' rows: only statistics that stop at the device-side count agree."""
    wc.check_captured_step_matches_the_eager_step_on_padded_batches(LIT, criterion)


@pytest.mark.parametrize("label_index", [0, 1, 2])
def test_trainer_captured_from_files_and_resume(label_index, tmp_path):
    ck, moms = wc.check_trainer_captured_from_files_and_resume(LIT, label_index, tmp_path)
    assert any(float(t.abs().sum()) > 0 for t in moms)
    means = [k for k in ck["state_dict"] if re.search(r"network\.\d+\.running_mean$", k)]
    assert len(means) == 4
    for k in means:                                   # the BatchNorm buffers travelled through the checkpoint
        assert float(ck["state_dict"][k].abs().max()) > 0, k
        assert int(ck["state_dict"][k.replace("running_mean", "num_batches_tracked")]) > 0


def test_linear_waveform_net_one_training_step_against_the_cpu_module():
    cfg = wc.lit_config(LIT_LINEAR, "L1Loss")
    cfg["net_config"]["net_class"] = "WaveformModels.LinearWaveformNet"
    cfg["net_config"]["net_type"] = "Linear"
    cfg["net_config"]["hparams"] = {"n_expand": 1, "expansion_factor": 2, "n_contract": 2, "n_lin": 3, "out_size": 1}
    gpu = _one_training_step_against_the_cpu_module(LIT_LINEAR, cfg, "L1Loss", kernel_calls=0)
    widths = [m.in_features for m in gpu.model.linear.net if isinstance(m, nn.Linear)]
    assert widths == [59, 118, 60]
