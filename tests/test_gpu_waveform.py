"""The multi-channel TCN kernels (wfs_tcnc_*, csrc/tcnc.hip) behind TemporalConvNet(fused=True), TemporalWaveformNet and
LitWaveform on the GPU: forward, dX and every parameter gradient against the torch composition in float64 on the CPU,
dropout masks, determinism, the bounds, one LitWaveform step against the CPU module, the captured step against the
eager one on a padded batch, and Trainer(capture=True) from the r3 pulse fixture."""
import math

import pytest
import torch

import waveform_cases as wc
from seq_cases import make_tcn, tcn_hash_masks as _hash_masks, tcn_masked_reference as _masked_reference
from waveform_cases import DEV, TOL, max_err as _max_err

pytestmark = pytest.mark.gpu


def _tcn_pair(c0, channels, k, dropout=0.0, seed=0):
    """The fused module on the GPU with the live-parameter recipe of tests/seq_cases.py, and its float64 twin."""
    gpu, ref = make_tcn(c0, channels, k, dropout=dropout, seed=seed)
    return gpu.to(DEV), ref


CASES = [  # (c0, channels, k, L)
    (1, [8, 16, 8], 3, 59),          # the committed plan (config/waveform_tcn_z.json)
    (1, [8, 16, 8], 3, 62),          # ... with use_detector_number
    (1, [1, 6, 6, 3], 2, 59),        # a one-channel first level, Cin == Cout and Cin != Cout levels, 4 levels
    (1, [4], 5, 1024),               # one level, long rows
    (1, [12, 32, 20, 2], 5, 1024),   # up to 32 channels, 4 levels, long rows
    (1, [3, 3], 2, 62),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, [c[0]] + c[1] + [c[2], c[3]])) for c in CASES])
def test_forward_dx_and_parameter_gradients_against_float64(case, dtype):
    from waveformml_amd.psd import tcn
    c0, channels, k, L = case
    gpu, ref = _tcn_pair(c0, channels, k, seed=len(channels) * 100 + k + L)
    gpu.train(), ref.train()
    N = 6
    g = torch.Generator().manual_seed(L + k)
    x = torch.randn(N, c0, L, generator=g).to(dtype)             # the rounded inputs both sides see
    dy = torch.randn(N, channels[-1], L, generator=g).to(dtype)
    xg = x.to(DEV).requires_grad_(True)
    before = tcn.TCNC_CALLS[0]
    y = gpu(xg)
    assert tcn.TCNC_CALLS[0] == before + 1 and y.dtype == dtype and y.shape == (N, channels[-1], L)
    y.backward(dy.to(DEV))
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.double())
    assert float(yr.abs().max()) > 0 and float(xr.grad.abs().max()) > 0       # a live net, not a dead one
    tol = TOL[dtype]
    pairs = [("y", y, yr), ("dx", xg.grad, xr.grad)]
    pairs += [(n, a.grad, b.grad) for (n, a), b in zip(gpu.named_parameters(), ref.parameters())]
    for name, a, b in pairs:
        err, scale = _max_err(a, b)
        print("%s %s: max err %.3e of max %.3e (%.2e)" % (dtype, name, err, scale, err / max(scale, 1e-30)))
        assert err <= tol * scale, (name, err, scale)


def _check_with_dropout(channels, k, N, L, p, seed_state):
    """Forward, dX and every parameter gradient of the fused TCN in training mode against the float64 composition run
    with the SAME masks, rebuilt here from the seed the module draws; fp32 bar 1e-5 of each tensor's max."""
    from waveformml_amd.psd import tcn
    gpu, ref = _tcn_pair(1, channels, k, dropout=p, seed=N + L)
    gpu.train(), ref.train()
    g = torch.Generator().manual_seed(N + k)
    x = torch.randn(N, 1, L, generator=g)
    dy = torch.randn(N, channels[-1], L, generator=g)
    torch.manual_seed(seed_state)
    seed = int(torch.randint(-2 ** 62, 2 ** 62, (1,), dtype=torch.int64, device=DEV).item())   # what forward draws
    torch.manual_seed(seed_state)
    xg = x.to(DEV).requires_grad_(True)
    before = tcn.TCNC_CALLS[0]
    y = gpu(xg)
    assert tcn.TCNC_CALLS[0] == before + 1
    y.backward(dy.to(DEV))
    masks = [_hash_masks(seed, p, N, channels[lv // 2], L, lv) for lv in range(2 * len(channels))]
    xr = x.double().requires_grad_(True)
    yr = _masked_reference(ref, xr, masks)
    yr.backward(dy.double())
    pairs = [("y", y, yr), ("dx", xg.grad, xr.grad)]
    pairs += [(n, a.grad, b.grad) for (n, a), b in zip(gpu.named_parameters(), ref.parameters())]
    for name, a, b in pairs:
        err, scale = _max_err(a, b)
        print("dropout %.2f N=%d %s: max err %.3e of max %.3e (%.2e)" % (p, N, name, err, scale, err / max(scale, 1e-30)))
        assert scale > 0 and err <= 1e-5 * scale, (name, err, scale)
    return masks


def test_dropout_masks_rebuilt_in_the_backward_match_a_reference_with_the_same_masks():
    """Both convolutions' masks of every level, every channel: the kernels' forward AND backward (which rebuilds the
    masks from the seed) against the float64 composition with those masks.  Each mask's kept fraction over >= 10^6
    elements lies within (1-p) +- 6 sqrt(p (1-p) / n) (the binomial bound), and channels get different masks."""
    p, N, L = 0.3, 256, 512
    masks = _check_with_dropout([16, 8], 3, N, L, p, seed_state=11)
    for ci, m in enumerate(masks):
        kept = (m > 0).double()
        n = kept.numel()
        frac = float(kept.mean())
        bound = 6 * math.sqrt(p * (1 - p) / n)
        print("conv %d: kept fraction %.6f over %d elements, expected %.3f +- %.6f" % (ci, frac, n, 1 - p, bound))
        assert n >= 10 ** 6 and abs(frac - (1 - p)) <= bound
        assert not torch.equal(m[:, 0], m[:, 1])
    assert not torch.equal(masks[0], masks[1])                 # conv1 and conv2 of a level draw different masks


def test_production_size_with_dropout_against_float64():
    """The committed plan at 16384 rows of 59 samples: the conv passes run their grid-stride loop (> 4096 blocks) and
    every dW block sums many tiles (its tile loop), with dropout on."""
    _check_with_dropout([8, 16, 8], 3, 16384, 59, 0.2, seed_state=5)


def test_two_identical_calls_are_bit_identical():
    gpu, _ref = _tcn_pair(1, [8, 16, 8], 3, dropout=0.2, seed=3)
    gpu.train()
    x = torch.randn(300, 1, 59, device=DEV)
    dy = torch.randn(300, 8, 59, device=DEV)
    outs = []
    for _ in range(2):
        gpu.zero_grad(set_to_none=True)
        torch.manual_seed(1234)                   # the same dropout seed for both calls
        xg = x.clone().requires_grad_(True)
        y = gpu(xg)
        y.backward(dy)
        outs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in gpu.parameters()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_bounds_take_the_torch_composition_and_the_flag_off_never_calls_the_kernels():
    from waveformml_amd import _lib
    from waveformml_amd.psd import tcn
    lib = _lib.load()
    assert lib.wfs_tcnc_ok(1, _lib.i32_array([8, 33]), 2, 3, 59, _lib.WFS_F32) == _lib.WFS_EINVAL
    assert lib.wfs_tcnc_ok(1, _lib.i32_array([8]), 1, 9, 59, _lib.WFS_F32) == _lib.WFS_EINVAL
    assert lib.wfs_tcnc_ok(1, _lib.i32_array([8]), 1, 1, 59, _lib.WFS_F32) == _lib.WFS_EINVAL    # no causal padding
    assert lib.wfs_tcnc_ok(1, _lib.i32_array([8]), 1, 3, 4097, _lib.WFS_F32) == _lib.WFS_EINVAL
    assert lib.wfs_tcnc_ok(1, _lib.i32_array([8] * 9), 9, 3, 59, _lib.WFS_F32) == _lib.WFS_EINVAL
    assert lib.wfs_tcnc_ok(1, _lib.i32_array([32] * 8), 8, 8, 4096, _lib.WFS_F32) == _lib.WFS_OK
    for c0, channels, k, L in [(1, [8, 33], 3, 59), (1, [4], 3, 4100)]:
        gpu, ref = _tcn_pair(c0, channels, k, seed=9)
        x = torch.randn(3, c0, L)
        before = tcn.TCNC_CALLS[0]
        with torch.no_grad():
            y = gpu(x.to(DEV))
        assert tcn.TCNC_CALLS[0] == before                      # the torch composition ran
        err, scale = _max_err(y, ref(x.double()))
        assert err <= 1e-5 * scale
    gpu, _ = _tcn_pair(1, [8, 16, 8], 3)
    gpu.fused = False
    before = tcn.TCNC_CALLS[0]
    with torch.no_grad():
        gpu(torch.randn(4, 1, 59, device=DEV))
    assert tcn.TCNC_CALLS[0] == before
    # the whole net with its flag off: TemporalWaveformNet turns it on, a plain TemporalConvNet leaves it off
    assert not tcn.TemporalConvNet(1, [8, 16], 3).fused


def _reinit(m, _cfg, _seed):
    with torch.no_grad():
        for p in m.model.model.parameters():
            p.copy_(torch.randn_like(p) * 0.5)


def _tcnc_calls():
    from waveformml_amd.psd import tcn
    return tcn.TCNC_CALLS[0]


LIT = wc.LitCase("waveform_tcn_z.json", _tcnc_calls, _reinit)


@pytest.mark.parametrize("detector", [False, True], ids=["rows", "detector"])
@pytest.mark.parametrize("criterion", ["L1Loss", "CrossEntropyLoss"])
def test_lit_waveform_one_training_step_against_the_cpu_module(criterion, detector):
    wc.check_one_training_step_against_the_cpu_module(LIT, criterion, detector)


@pytest.mark.parametrize("criterion", ["L1Loss", "CrossEntropyLoss"])
def test_captured_step_matches_the_eager_step_on_padded_batches(criterion):
    wc.check_captured_step_matches_the_eager_step_on_padded_batches(LIT, criterion)


@pytest.mark.parametrize("label_index", [0, 1, 2])
def test_trainer_captured_from_files_and_resume(label_index, tmp_path):
    _ck, moms = wc.check_trainer_captured_from_files_and_resume(LIT, label_index, tmp_path)
    assert any(float(t.abs().sum()) > 0 for t in moms)
