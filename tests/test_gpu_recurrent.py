"""The Elman-RNN scan kernels (wfs_rnn_*, csrc/rnn.hip) behind RecurrentBlock(fused=True), RecurrentWaveformNet and
LitWaveform on the GPU: forward, dX and every parameter gradient against torch.nn.RNN in float64 on the CPU, dropout
masks, the production size, determinism, the bounds, one LitWaveform step against the CPU module, the captured step
against the eager one on padded batches, and Trainer(capture=True) from the r3 pulse fixture.

Measured on an MI355X (worst tensor of a case, error over the tensor's max): fp32 2.5e-7 .. 6.6e-6 (the largest on
1024-1-16-3-2-relu, where torch's own fp32 CPU run is 1.2e-5 from float64), bf16 <= 3.6e-3, fp16 <= 4.4e-4, dropout case
5.6e-7, 16384 rows 4.2e-7 (the table is in DESIGN.md section 4, "Elman RNN").
"""
import copy
import math

import pytest
import torch

import waveform_cases as wc
from recurrent_cases import CASES, assert_live, case_id, make_inputs, make_rnn, run_torch
from seq_cases import elman as _elman, rnn_hash_masks as _hash_masks
from waveform_cases import DEV, TOL, max_err as _err

pytestmark = pytest.mark.gpu


def _block(rnn, case, dropout=0.0):
    """RecurrentBlock(fused=True) on the GPU holding rnn's parameters."""
    from waveformml_amd.psd.recurrent import RecurrentBlock
    _T, I, H, layers, dirs, nonlin, bias = case
    blk = RecurrentBlock(I, H, layers, nonlinearity=nonlin, bias=bias, dropout=dropout, bidirectional=dirs == 2, fused=True)
    blk.rnn.load_state_dict(rnn.state_dict())
    return blk.to(DEV)


def _run_fused(blk, x, dy):
    from waveformml_amd.psd import recurrent
    blk.zero_grad(set_to_none=True)
    xg = x.detach().to(DEV).requires_grad_(True)
    before = recurrent.RNN_CALLS[0]
    y, hidden = blk(xg)
    assert recurrent.RNN_CALLS[0] == before + 1                      # the kernels ran, exactly once
    y.backward(dy.to(DEV))
    return [("y", y.detach()), ("dx", xg.grad)] + [(n, p.grad) for n, p in blk.rnn.named_parameters()], hidden


def _compare(tag, got, ref, r32, dtype):
    """Each tensor within the bar of its float64 value: 16-bit rows the project's bars; fp32 rows max(1e-5, 2 e_torch32)
    where e_torch32 is torch's own fp32 CPU nn.RNN against the same float64 run (a long recurrence is where fp32
    itself leaves 1e-5; factor 2: another summation order of the same length, not a looser algorithm)."""
    worst = 0.0
    for (name, a), (_n, b), (_m, c) in zip(got, ref, r32):
        err, scale = _err(a, b)
        e32 = _err(c, b)[0] / scale
        bar = max(TOL[dtype], 2 * e32) if dtype == torch.float32 else TOL[dtype]
        print("%s %s: err %.3e of max %.3e = %.2e; e_torch32 %.2e; bar %.2e" % (tag, name, err, scale, err / scale, e32, bar))
        worst = max(worst, err / scale)
        assert a.shape == b.shape and err <= bar * scale, (tag, name, err / scale, bar)
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_forward_dx_and_parameter_gradients_against_float64(case, dtype):
    i = CASES.index(case)
    T, _I, H, layers, dirs, _nl, _b = case
    N = 6
    rnn = make_rnn(case, seed=i)
    x, dy = make_inputs(case, N, dtype, seed=i)                      # the rounded inputs both sides see
    ref = run_torch(rnn, x, dy, torch.float64)
    zeros, ymax = assert_live(ref)                                   # live inputs are a condition, asserted first
    print("%s: %.3f of Y exactly zero, max|Y| %.3g" % (case_id(case), zeros, ymax))
    r32 = run_torch(rnn, x, dy, torch.float32)
    blk = _block(rnn, case).train()
    got, hidden = _run_fused(blk, x, dy)
    assert got[0][1].dtype == dtype and got[0][1].shape == (N, T, dirs * H)
    _compare("%s %s" % (case_id(case), dtype), got, ref, r32, dtype)
    # hidden: [layers dirs, N, H], the last state of every chain (the same bar, e_torch32 of the hidden state itself)
    with torch.no_grad():
        _y, href = copy.deepcopy(rnn).double()(x.double())
        _y, h32 = rnn(x.float())
    assert hidden.shape == (layers * dirs, N, H) and hidden.dtype == dtype
    _compare("%s %s" % (case_id(case), dtype), [("hidden", hidden)], [("hidden", href)], [("hidden", h32)], dtype)


def test_dropout_masks_rebuilt_in_the_backward_match_a_reference_with_the_same_masks():
    """p = 0.3, training mode, 3 layers, 2 directions: forward, dX and all gradients against the float64 recurrence with
    the masks rebuilt from the documented counter scheme; each mask's kept fraction over >= 10^6 elements within
    (1-p) +- 6 sqrt(p (1-p) / n); no mask on the last layer's output; eval mode equals p = 0."""
    from waveformml_amd.psd import recurrent
    p, N = 0.3, 4096
    case = (64, 1, 8, 3, 2, "relu", True)
    T, _I, H, layers, dirs, _nl, _b = case
    rnn = make_rnn(case, dropout=p, seed=21)
    x, dy = make_inputs(case, N, torch.float32, seed=21)
    blk = _block(rnn, case, dropout=p).train()
    torch.manual_seed(11)
    seed = int(torch.randint(-2 ** 62, 2 ** 62, (1,), dtype=torch.int64, device=DEV).item())   # what forward draws
    torch.manual_seed(11)
    got, _hidden = _run_fused(blk, x, dy)
    masks = [_hash_masks(seed, p, N, dirs * H, T, l) for l in range(layers - 1)] + [None]
    for l, m in enumerate(masks[:-1]):
        kept = (m > 0).double()
        n, frac = kept.numel(), float(kept.mean())
        bound = 6 * math.sqrt(p * (1 - p) / n)
        print("layer %d: kept fraction %.6f over %d elements, expected %.3f +- %.6f" % (l, frac, n, 1 - p, bound))
        assert n >= 10 ** 6 and abs(frac - (1 - p)) <= bound
        assert not torch.equal(m[:, :, 0], m[:, :, 1])
    assert not torch.equal(masks[0], masks[1])
    xr = x.double().requires_grad_(True)
    yr, leaves = _elman(rnn, xr, masks)
    yr.backward(dy.double())
    ref = [("y", yr.detach()), ("dx", xr.grad)] + [(n, q.grad) for (n, _), q in zip(rnn.named_parameters(), leaves)]
    assert_live(ref)
    x32 = x.clone().requires_grad_(True)
    y32, leaves32 = _elman(rnn, x32, masks, torch.float32)
    y32.backward(dy)
    r32 = [("y", y32.detach()), ("dx", x32.grad)] + [(n, q.grad) for (n, _), q in zip(rnn.named_parameters(), leaves32)]
    _compare("dropout %.1f" % p, got, ref, r32, torch.float32)
    # eval mode: no mask anywhere = the module with p = 0 (and the last layer's output was never masked above: yr has it)
    blk.eval()
    plain = _block(rnn, case, dropout=0.0).eval()
    before = recurrent.RNN_CALLS[0]
    with torch.no_grad():
        ye, _ = blk(x.to(DEV))
        y0, _ = plain(x.to(DEV))
    assert recurrent.RNN_CALLS[0] == before + 2 and torch.equal(ye, y0)
    _yn, _ = _elman(rnn, x.double(), [None] * layers)
    err, scale = _err(ye, _yn)
    assert err <= 1e-5 * scale


def test_production_size_against_float64():
    """The committed shape at 16384 rows: the transposes' row loop and the dW blocks' tile loop run (30 tiles per
    block)."""
    case = CASES[0]
    rnn = make_rnn(case, seed=0)                      # the parameters of the first parametrised case
    x, dy = make_inputs(case, 16384, torch.float32, seed=5)
    ref = run_torch(rnn, x, dy, torch.float64)
    assert_live(ref)
    r32 = run_torch(rnn, x, dy, torch.float32)
    got, _hidden = _run_fused(_block(rnn, case).train(), x, dy)
    _compare("16384 rows", got, ref, r32, torch.float32)


def test_two_identical_calls_are_bit_identical():
    case = (59, 1, 4, 4, 2, "relu", True)
    rnn = make_rnn(case, dropout=0.2, seed=3)
    blk = _block(rnn, case, dropout=0.2).train()
    x, dy = make_inputs(case, 300, torch.float32, seed=3)
    outs = []
    for _ in range(2):
        torch.manual_seed(1234)                   # the same dropout seed for both calls
        got, hidden = _run_fused(blk, x, dy)
        outs.append([t.clone() for _n, t in got] + [hidden.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][0].abs().max()) > 0 and float(outs[0][2].abs().max()) > 0


def test_bounds_take_the_torch_module_and_the_flag_off_never_calls_the_kernels():
    from waveformml_amd.psd import recurrent
    for case in [(20, 1, 33, 2, 1, "tanh", True), (4100, 1, 4, 1, 1, "tanh", True)]:
        rnn = make_rnn(case, seed=9)
        blk = _block(rnn, case)
        x, _dy = make_inputs(case, 3, torch.float32, seed=9)
        before = recurrent.RNN_CALLS[0]
        with torch.no_grad():
            y, _h = blk(x.to(DEV))
            yr, _ = copy.deepcopy(rnn).double()(x.double())
            y32, _ = rnn(x)
        assert recurrent.RNN_CALLS[0] == before                      # self.rnn ran
        _compare("%s through nn.RNN on the GPU" % case_id(case), [("y", y)], [("y", yr)], [("y", y32)], torch.float32)
    case = CASES[0]
    blk = _block(make_rnn(case), case)
    blk.fused = False
    before = recurrent.RNN_CALLS[0]
    with torch.no_grad():
        blk(torch.rand(4, 59, 1, device=DEV))
    assert recurrent.RNN_CALLS[0] == before
    assert not recurrent.RecurrentBlock(1, 4, 4).fused and not recurrent.RecurrentNet(59, 1, 4, 4, 4, 1).rnn_block.fused


def _reinit(m, cfg, seed):
    """Live parameters: the RNN by the cases' recipe (the default init of a 4-unit bias-free ReLU net can be dead), the
    head N(0, 0.5^2) scaled by its fan-in."""
    hp = cfg["net_config"]["hparams"]
    src = make_rnn((m.model.nsamples, 1, hp["n_hidden"], hp["n_layers"], 1, "relu", False), seed=seed)
    m.model.model.rnn_block.rnn.load_state_dict(src.state_dict())
    with torch.no_grad():
        for p in m.model.model.linear.parameters():
            p.copy_(torch.randn_like(p) * (0.5 / math.sqrt(p.shape[-1]) if p.dim() > 1 else 0.5))


def _rnn_calls():
    from waveformml_amd.psd import recurrent
    return recurrent.RNN_CALLS[0]


LIT = wc.LitCase("waveform_rnn_z.json", _rnn_calls, _reinit)


@pytest.mark.parametrize("detector", [False, True], ids=["rows", "detector"])
@pytest.mark.parametrize("criterion", ["L1Loss", "CrossEntropyLoss"])
def test_lit_waveform_one_training_step_against_the_cpu_module(criterion, detector):
    gpu, errs = wc.check_one_training_step_against_the_cpu_module(LIT, criterion, detector)
    assert gpu.squeeze_index == 2
    for n, _err_n, scale in errs:
        assert scale > 0, n


@pytest.mark.parametrize("criterion", ["L1Loss", "CrossEntropyLoss"])
def test_captured_step_matches_the_eager_step_on_padded_batches(criterion):
    wc.check_captured_step_matches_the_eager_step_on_padded_batches(LIT, criterion)


@pytest.mark.parametrize("label_index", [0, 1, 2])
def test_trainer_captured_from_files_and_resume(label_index, tmp_path):
    ck, _moms = wc.check_trainer_captured_from_files_and_resume(LIT, label_index, tmp_path)
    assert "model.model.rnn_block.rnn.weight_hh_l3" in ck["state_dict"]
