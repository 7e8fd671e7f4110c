"""The row kernels of the two waveform front ends at every dispatch arm against float64: the multi-channel TCN
(wfs_tcnc_taps_fwd / wfs_tcnc_fwd / wfs_tcnc_bwd, csrc/tcnc.hip) and the Elman RNN (wfs_rnn_fwd / wfs_rnn_bwd,
csrc/rnn.hip), through ctypes on raw device tensors, for fp32, bf16 and fp16 rows.

Cases, inputs, arms and the float64 references: tests/seq_cases.py; tests/test_seq_cases_host.py proves every case live,
conditioned (torch's fp32 run within 3e-6 of float64) and ReLU-safe on the CPU, and that it reaches the arm it is
there for.  Every call gets `saved`, the effective taps and the workspace exactly wfs_*_floats long and filled with NaN,
Y / dX / hidden filled with a sentinel, every gradient slot filled with NaN, and a few trailing elements behind every
output that must keep their fill.  The RNN's padding lanes (N .. Npad of every [t][c] row of `saved` and the
workspace) are therefore NaN wherever k_rnn_tin has not zeroed them: a kernel that reads one without its n < N guard
poisons its result.  Bars, the project's own:
  RNN   |got - want| <= bar max|want|, bar = max(1e-5, 2 e_torch32) for fp32 rows (e_torch32: torch's own fp32 CPU run
        against the same float64 run), 2e-2 / 3e-3 for bf16 / fp16 rows; the last hidden states likewise
  TCN   |got - want| <= 1e-5 / 2e-2 / 3e-3 of max|want|; the dropout cases (fp32 rows, masks rebuilt from the seed) the same
  a reference that is identically zero (dW_hh at T = 1; the partial sums of a tap that falls off the row) is met exactly
  every output is finite
The TCN's partial sums of d effective taps (the tail of the workspace, [block][cout][cin k + 1] per convolution) are
added up here and held to the float64 gradient of the weight-normed taps with the same bar.
One case per family also runs through the module (RecurrentBlock / TemporalConvNet), which sizes the buffers itself.

The worst error / bar of every (family, case, row type) is printed when the module ends and written to
$WFS_SEQ_EDGES_REPORT when that is set (the table of DESIGN.md section 4).
"""
import os
import time

import pytest
import torch

import seq_cases as sc
from waveform_cases import DEV, TOL, max_err

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1, "f16": 2}
SENT = -768.0                      # exactly representable in bf16 and fp16
PAD = 5                            # trailing elements behind every output
NAN = float("nan")
WORST = {}                         # (family, case, kind) -> worst error / bar over the case's tensors


def _L():
    from waveformml_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    t0 = time.time()
    yield
    lines = ["# worst |got - want| / (bar max|want|) over the tensors of a case (<= 1 passes): family, case, row type"]
    lines += ["%-4s %-40s %-5s %.4f" % (fam, cid, kind, r) for (fam, cid, kind), r in sorted(WORST.items())]
    text = "\n".join(lines)
    print("\n" + text + "\n# module wall time %.1f s" % (time.time() - t0))
    path = os.environ.get("WFS_SEQ_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


class _Out:
    """An output of `shape` with PAD trailing elements, all filled with `fill`; `.t` is the output itself."""

    def __init__(self, shape, dtype, fill):
        n = 1
        for s in shape:
            n *= s
        self.flat = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
        self.t = self.flat[:n].view(shape)
        self.fill = fill

    def check_tail(self, what):
        tail = self.flat[self.t.numel():].float()
        kept = torch.isnan(tail) if self.fill != self.fill else tail == self.fill
        assert bool(kept.all()), "%s: an element behind the output was written" % what


def _nan(n):
    assert n > 0
    return torch.full((int(n),), NAN, dtype=torch.float32, device=DEV)


def _tables(params, width):
    """The forward's and the backward's pointer tables of the kernels' parameter list (None: absent), and the gradient
    slots (NaN-filled, with a tail) the backward's table points to."""
    from waveformml_amd.psd import _fused
    grads = [None if q is None else _Out(tuple(q.shape), torch.float32, NAN) for q in params]
    fwd = _fused.fwd_rows(params, width)
    slots = _fused.fwd_rows([None if g is None else g.t for g in grads], width)
    bwd = [a[:width] + b[:width] for a, b in zip(fwd, slots)]
    return _fused.ptr_table({}, "fwd", fwd, DEV), _fused.ptr_table({}, "bwd", bwd, DEV), grads


def _seed(c):
    return (sc.DROP_P, torch.tensor([sc.DROP_SEED], dtype=torch.int64, device=DEV)) if c.dropout else (0.0, None)


def _check(family, cid, kind, got, ref, r32):
    """Every tensor of `ref` ([(name, float64 tensor)]) against got[name], with the bars of the module docstring."""
    dtype = sc.KINDS[kind]
    worst = 0.0
    for (name, b), (_n, c) in zip(ref, r32):
        a = got[name]
        assert tuple(a.shape) == tuple(b.shape), name
        assert bool(torch.isfinite(a.float()).all()), "%s %s %s is not finite" % (cid, kind, name)
        err, scale = max_err(a, b)
        if scale == 0:
            assert err == 0, "%s %s %s: identically zero in float64, %.3e here" % (cid, kind, name, err)
            continue
        bar = TOL[dtype]
        if family == "rnn" and dtype == torch.float32:
            bar = max(bar, 2 * max_err(c, b)[0] / scale)
        print("%s %s %s: err %.3e of max %.3e = %.2e; bar %.2e" % (cid, kind, name, err, scale, err / scale, bar))
        worst = max(worst, err / (bar * scale))
    key = (family, cid, kind)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    assert worst <= 1.0, "%s %s: worst error is %.4g of its bar" % (cid, kind, worst)


# ---------------------------------------------------------------------------------------------------------- RNN
def _rnn_param_list(p, c):
    """(weight_ih, weight_hh, bias_ih, bias_hh) per (layer, direction) on the device, None without bias; and the names."""
    _T, _I, _H, layers, dirs, _nl, bias = c.case
    dev = {n: q.detach().to(DEV).contiguous() for n, q in p.net.named_parameters()}
    params, names = [], []
    for l in range(layers):
        for sfx in ("", "_reverse")[:dirs]:
            for stem in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                n = "%s_l%d%s" % (stem, l, sfx)
                params.append(dev.get(n) if bias or stem.startswith("weight") else None)
                names.append(n)
    assert sum(q is not None for q in params) == len(dev)
    return params, names


def run_rnn(i, kind, dx=True):
    """One wfs_rnn_fwd and one wfs_rnn_bwd through the C ABI.  Returns ({name: device tensor}, hidden)."""
    L = _L()
    lib = L.load()
    c, p = sc.RNN_CASES[i], sc.rnn_problem(i, kind)
    T, I, H, layers, dirs, nonlin, _b = c.case
    N, dt, code = c.N, sc.KINDS[kind], {"relu": L.WFS_RNN_RELU, "tanh": L.WFS_RNN_TANH}[c.case[5]]
    Npad, C = (N + 63) // 64 * 64, dirs * H
    params, names = _rnn_param_list(p, c)
    tab_f, tab_b, grads = _tables(params, 4)
    X, dY = p.x.to(DEV), p.dy.to(DEV)
    drop, seed = _seed(c)
    n_saved = int(lib.wfs_rnn_saved_floats(N, T, I, H, layers, dirs))
    assert n_saved == Npad * T * (I + layers * C)
    saved = _nan(n_saved)
    Y, hidden = _Out((N, T, C), dt, SENT), _Out((layers * dirs, N, H), dt, SENT)
    L.check(lib.wfs_rnn_fwd(L.ptr(X), N, T, I, H, layers, dirs, code, L.ptr(tab_f), L.ptr(saved), L.ptr(Y.t),
                            L.ptr(hidden.t), DT[kind], drop, L.ptr(seed), L.stream_ptr()))
    ws = _nan(lib.wfs_rnn_bwd_workspace_floats(N, T, I, H, layers, dirs))
    dX = _Out((N, T, I), dt, SENT) if dx else None
    L.check(lib.wfs_rnn_bwd(L.ptr(dY), N, T, I, H, layers, dirs, code, L.ptr(tab_b), L.ptr(saved),
                            L.ptr(dX.t) if dx else None, L.ptr(ws), DT[kind], drop, L.ptr(seed), L.stream_ptr()))
    torch.cuda.synchronize()
    for what, o in [("y", Y), ("hidden", hidden)] + ([("dx", dX)] if dx else []) + [(n, g) for n, g in zip(names, grads) if g]:
        o.check_tail(what)
    # the padding lanes of `saved`: zeros under X (k_rnn_tin), untouched under every layer's outputs
    lanes = saved.view(T * (I + layers * C), Npad)
    if Npad > N:
        assert bool((lanes[:T * I, N:] == 0).all()) and bool(torch.isnan(lanes[T * I:, N:]).all())
    assert bool(torch.isfinite(lanes[:, :N]).all())
    got = {n: g.t for n, g in zip(names, grads) if g is not None}
    got["y"] = Y.t
    if dx:
        got["dx"] = dX.t
    return got, hidden.t


def _rnn_params():
    return [pytest.param(i, kind, id="%s-%s" % (sc.rnn_id(c), kind)) for i, c in enumerate(sc.RNN_CASES) for kind in sc.kinds_of(c)]


@pytest.mark.parametrize("i,kind", _rnn_params())
def test_rnn_case_against_float64(i, kind):
    c, p = sc.RNN_CASES[i], sc.rnn_problem(i, kind)
    got, hidden = run_rnn(i, kind, dx=c.dx)
    ref, r32 = p.ref, p.r32
    if not c.dx:
        # the twin: without dX the backward skips layer 0's mix; no parameter gradient may notice
        full, hidden_full = run_rnn(i, kind, dx=True)
        for n, t in got.items():
            assert torch.equal(t.view(torch.uint8), full[n].view(torch.uint8)), n
        assert torch.equal(hidden.view(torch.uint8), hidden_full.view(torch.uint8))
        keep = [j for j, (n, _t) in enumerate(ref) if n != "dx"]
        ref, r32 = [ref[j] for j in keep], [r32[j] for j in keep]
    _check("rnn", sc.rnn_id(c), kind, got, ref, r32)
    _check("rnn", sc.rnn_id(c), kind, {"hidden": hidden}, [("hidden", p.hidden)], [("hidden", p.h32)])


def test_rnn_through_the_module_at_the_widest_case():
    """RecurrentBlock(fused=True) sizes `saved`, the workspace and the outputs itself: I = 32, C = 64, N = 257."""
    from waveformml_amd.psd import recurrent
    i = 6
    c, p = sc.RNN_CASES[i], sc.rnn_problem(i, "f32")
    _T, I, H, layers, dirs, nonlin, bias = c.case
    assert (I, dirs * H, c.N) == (32, 64, 257)
    blk = recurrent.RecurrentBlock(I, H, layers, nonlinearity=nonlin, bias=bias, bidirectional=dirs == 2, fused=True)
    blk.rnn.load_state_dict(p.net.state_dict())
    blk = blk.to(DEV).train()
    xg = p.x.to(DEV).requires_grad_(True)
    before = recurrent.RNN_CALLS[0]
    y, hidden = blk(xg)
    assert recurrent.RNN_CALLS[0] == before + 1
    y.backward(p.dy.to(DEV))
    got = {n: q.grad for n, q in blk.rnn.named_parameters()}
    got.update(y=y.detach(), dx=xg.grad)
    _check("rnn", sc.rnn_id(c) + " module", "f32", got, p.ref, p.r32)
    _check("rnn", sc.rnn_id(c) + " module", "f32", {"hidden": hidden}, [("hidden", p.hidden)], [("hidden", p.h32)])


# ---------------------------------------------------------------------------------------------------------- TCN
def _tcn_param_list(net):
    """(weight_v, weight_g, bias) per convolution in the kernels' order on the device -- the downsample as
    (weight, None, bias) -- and the parameters' names."""
    name_of = {id(q): n for n, q in net.named_parameters()}
    trips = []
    for blk in net.network:
        for conv in blk.convs:
            trips += [conv.weight_v, conv.weight_g, conv.bias]
        if blk.downsample is not None:
            trips += [blk.downsample.weight, None, blk.downsample.bias]
    assert sum(q is not None for q in trips) == len(name_of)
    return ([None if q is None else q.detach().to(DEV).contiguous() for q in trips],
            [None if q is None else name_of[id(q)] for q in trips])


def run_tcn(i, kind):
    """wfs_tcnc_taps_fwd, wfs_tcnc_fwd and wfs_tcnc_bwd through the C ABI.  Returns ({name: device tensor}, the summed
    partial sums [cout, cin, k] of d effective taps of conv1 and conv2 of every level)."""
    L = _L()
    lib = L.load()
    c, p = sc.TCN_CASES[i], sc.tcn_problem(i, kind)
    c0, channels, k, Lr = c.case
    N, dt, levels, ch = c.N, sc.KINDS[kind], len(channels), L.i32_array(channels)
    params, names = _tcn_param_list(p.net)
    tab_f, tab_b, grads = _tables(params, 3)
    X, dY = p.x.to(DEV), p.dy.to(DEV)
    drop, seed = _seed(c)
    wts = _nan(lib.wfs_tcnc_weights_floats(c0, ch, levels, k))
    saved = _nan(lib.wfs_tcnc_saved_floats(N, Lr, c0, ch, levels))
    assert saved.numel() == 3 * N * Lr * sum(channels)
    Y = _Out((N, channels[-1], Lr), dt, SENT)
    L.check(lib.wfs_tcnc_taps_fwd(L.ptr(tab_f), c0, ch, levels, k, L.ptr(wts), L.stream_ptr()))
    L.check(lib.wfs_tcnc_fwd(L.ptr(X), N, Lr, c0, ch, levels, k, L.ptr(wts), L.ptr(saved), L.ptr(Y.t), DT[kind], drop,
                             L.ptr(seed), L.stream_ptr()))
    ws = _nan(lib.wfs_tcnc_bwd_workspace_floats(N, Lr, c0, ch, levels, k))
    dX = _Out((N, c0, Lr), dt, SENT)
    L.check(lib.wfs_tcnc_bwd(L.ptr(X), L.ptr(dY), N, Lr, c0, ch, levels, k, L.ptr(wts), L.ptr(saved), L.ptr(dX.t),
                             L.ptr(ws), L.ptr(tab_b), DT[kind], drop, L.ptr(seed), L.stream_ptr()))
    torch.cuda.synchronize()
    for what, o in [("y", Y), ("dx", dX)] + [(n, g) for n, g in zip(names, grads) if g]:
        o.check_tail(what)
    assert bool(torch.isfinite(wts).all()) and bool(torch.isfinite(saved).all())     # every slot has a writer
    # the partial sums behind the five activation buffers: [block][cout][cin k + 1] per convolution, plan order
    cm, nl = max([c0] + list(channels)), N * Lr
    nblk = min(nl // 32 + 1, 1024)
    part = ws[5 * cm * nl:]
    convs = sc.tcn_convs(c.case)
    assert part.numel() == nblk * sum(cout * (cin * kk + 1) for _lv, cin, cout, kk, _d in convs)
    assert bool(torch.isfinite(part).all())
    dw, off = [], 0
    for _lv, cin, cout, kk, _d in convs:
        n = nblk * cout * (cin * kk + 1)
        if kk == k and _d:                                           # conv1 / conv2 (the downsample has d = 0)
            s = part[off:off + n].view(nblk, cout, cin * kk + 1).double().sum(0)
            dw.append(s[:, :-1].reshape(cout, cin, kk))
        off += n
    got = {n: g.t for n, g in zip(names, grads) if g is not None}
    got.update(y=Y.t, dx=dX.t)
    return got, dw


def _tcn_params():
    return [pytest.param(i, kind, id="%s-%s" % (sc.tcn_id(c), kind)) for i, c in enumerate(sc.TCN_CASES) for kind in sc.kinds_of(c)]


@pytest.mark.parametrize("i,kind", _tcn_params())
def test_tcn_case_against_float64(i, kind):
    c, p = sc.TCN_CASES[i], sc.tcn_problem(i, kind)
    got, dw = run_tcn(i, kind)
    _check("tcn", sc.tcn_id(c), kind, got, p.ref, p.r32)
    want = p.extra[1]
    assert len(dw) == len(want) == 2 * len(c.case[1])
    taps = {"taps%d" % ci: g for ci, g in enumerate(dw)}
    for ci, w in enumerate(want):                                    # a tap that falls off the row: exactly zero
        assert not bool(taps["taps%d" % ci].cpu()[w == 0].any()), "conv %d: zero exactly where float64 is" % ci
    ref = [("taps%d" % ci, w) for ci, w in enumerate(want)]
    _check("tcn", sc.tcn_id(c), kind, taps, ref, ref)


def test_tcn_through_the_module_at_the_widest_case():
    """TemporalConvNet(fused=True) sizes the taps, `saved` and the workspace itself: ncol = 257 on three convolutions."""
    from waveformml_amd.psd import tcn
    i = 0
    c, p = sc.TCN_CASES[i], sc.tcn_problem(i, "f32")
    c0, channels, k, _Lr = c.case
    assert any(a[2] for a in c.arms)
    net, _ref = sc.make_tcn(c0, channels, k, seed=sc.seed_of(c, "f32"))
    net = net.to(DEV).train()
    xg = p.x.to(DEV).requires_grad_(True)
    before = tcn.TCNC_CALLS[0]
    y = net(xg)
    assert tcn.TCNC_CALLS[0] == before + 1
    y.backward(p.dy.to(DEV))
    got = {n: q.grad for n, q in net.named_parameters()}
    got.update(y=y.detach(), dx=xg.grad)
    _check("tcn", sc.tcn_id(c) + " module", "f32", got, p.ref, p.r32)
