"""The dense Conv1d + BatchNorm1d + ReLU stack kernels (wfs_conv1d_fwd / wfs_conv1d_bwd, csrc/conv1d.hip) at every
planning edge against float64, through ctypes on raw device tensors with the 14-word pointer records of
include/wfsparse.h, for fp32, bf16 and fp16 rows.

Cases, inputs, arms and the float64 reference: tests/conv1d_cases.py; tests/test_conv1d_cases_host.py proves on the CPU
that every case is well-posed (no pre-ReLU value within 1e-5 of its layer's largest, 5 .. 95 % of the ReLUs on),
conditioned (torch's fp32 run within 3e-6 of float64), inside the bounds and on the arm it is there for.

Every call gets `saved` and the workspace exactly wfs_conv1d_saved_floats / wfs_conv1d_bwd_workspace_floats long and
filled with NaN, Y and dX filled with the sentinel -768 (Y is a ReLU output: a negative value is an unwritten cell),
every gradient slot filled with NaN, num_batches_tracked preset to 41, and five trailing elements behind `saved`, the
workspace, Y, dX, every gradient slot and the running statistics, which must keep their fill.  Rows of X and dY at or
beyond a device-side count alternate NaN and 3e30.  A kernel that reads a cell no kernel wrote (a statistics partial
past the block count, a dW partial past the dW blocks, a padding row) poisons its result with NaN.

Bars, derived and not measured.  The arithmetic of csrc/conv1d.hip is fp32 for every row type: only X and dY (on load)
and Y and dX (on store) are 16-bit, and the backward reads the saved fp32 z, not Y.  So
  * every fp32 output -- the four gradients of every layer, running_mean, running_var -- is within 1e-5 of its tensor's
    largest float64 magnitude in all three row types (d conv.bias in front of a training-mode BatchNorm and d conv.weight
    of a one-tap one-channel layer against what they are summed from: tests/conv1d_cases.py);
  * Y and dX are held element by element: |got - want| <= (1 + u) 1e-5 scale + u |want|, u = 0 / 2^-8 / 2^-11 (half an
    ulp of bf16 / fp16: one rounding of a value that was within 1e-5 scale), for fp16 plus 2^-25 (half the subnormal
    spacing);
  * where float64 is exactly zero (Y with the ReLU off, dX at samples no tap reads, rows at or beyond the count) the
    kernels' value is exactly zero; every output is finite;
  * num_batches_tracked is 42 after a training call and 41 after an eval call, which leaves the running statistics
    bit-identical.

An empty batch (n_valid <= 0, case `nv`): Y, dX and every gradient are exactly zero; as include/wfsparse.h says, a
training call then folds mean 0 and variance 0 into the running statistics and counts a batch (torch raises there).

Measured on an MI355X (profiles/conv1d_edges_errors.txt): worst error / bar 0.235 for fp32 rows
(st-exact: d conv.weight), 0.334 / 0.182 for the fp32 outputs of bf16 / fp16 runs (eight in eval mode: d bn.weight;
ew-over: d conv.weight) and 0.987 / 0.959 for their Y and dX (dw-8193: dX; ew-over: Y -- near 1 by construction: the
u |want| term is the worst case of one rounding); the 100 tests take 4.6 s.  Nothing here is tuned to these figures.

The worst error / bar of every (case, row type, mode, tensor group) is printed when the module ends and written to
$WFS_CONV1D_EDGES_REPORT when that is set (profiles/conv1d_edges_errors.txt, summarised in DESIGN.md).
"""
import collections
import ctypes

import pytest
import torch
from torch import nn

import conv1d_cases as cc
from edge_harness import NAN, SENT, Buf, bits_equal, error_report
from waveform_cases import DEV, TOL

pytestmark = pytest.mark.gpu

BAR32 = TOL[torch.float32]                                     # 1e-5, the bar of every fp32 quantity
U_ROUND = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}   # half an ulp of the stored value
FLOOR = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -25}           # half the fp16 subnormal spacing
GROUPS = ("y", "dx", "dw", "db", "dbn", "running")
WORST = {}                         # (case, kind, mode) -> {group: worst error / bar}
STEMS = ("conv.weight", "conv.bias", "bn.weight", "bn.bias")

_error_report = error_report(WORST, GROUPS, "WFS_CONV1D_EDGES_REPORT", "%-22s %-5s %-5s")


def _L():
    from waveformml_amd import _lib
    return _lib


def _group(name):
    if name in ("y", "dx"):
        return name
    return {"conv.weight": "dw", "conv.bias": "db", "bn.weight": "dbn", "bn.bias": "dbn", "running_mean": "running",
            "running_var": "running"}[name.split(".", 1)[1]]


def _padded(t, cap, dt):
    """`t` [rows, ...] at capacity `cap`: the rows behind it alternate NaN and 3e30."""
    rows = t.shape[0]
    out = torch.full((cap,) + tuple(t.shape[1:]), NAN, dtype=torch.float32)
    out[rows:][1::2] = 3e30
    out = out.to(dt)
    out[:rows] = t
    return out.contiguous().to(DEV)


Run = collections.namedtuple("Run", "got nbts before keep")        # keep: what the outputs' addresses live in


def run_case(i, kind, mode, nv=None, dx=True, no_grads=(), rows=None):
    """One wfs_conv1d_fwd and one wfs_conv1d_bwd through the C ABI on freshly poisoned buffers at the case's capacity.
    `nv`: the device-side row count (None: NULL); `dx`: whether dX is given; `no_grads`: the layers whose four gradient
    addresses are 0; `rows`: the rows of X and dY that hold the problem (default: those that count).  Returns the
    outputs {name: device tensor} at full capacity and checks every tail, sentinel and counter on the way."""
    L = _L()
    lib = L.load()
    c = cc.CASES[i]
    rows = cc.rows_of(c, nv) if rows is None else rows
    p = cc.problem(i, kind, mode, rows if rows > 0 else None)
    training, dt, code = mode == "train", cc.KINDS[kind], list(cc.KINDS).index(kind)
    n, N = len(c.layers), c.N
    arrays = [L.i32_array(v) for v in cc.plan_arrays(c)]
    shape_args = (N, c.L, c.c0) + tuple(arrays) + (n,)
    assert lib.wfs_conv1d_ok(c.c0, *arrays, n, c.L, code) == L.WFS_OK
    keep, table_rows, grads, stats, nbts = [], [], {}, {}, []
    for li, (conv, bn) in enumerate(p.net):
        par = [conv.weight, conv.bias, bn.weight, bn.bias]
        dev = [None if q is None else q.detach().to(DEV).contiguous() for q in par]
        rm, rv = Buf(bn.running_mean.shape, torch.float32, 0.0, SENT), Buf(bn.running_var.shape, torch.float32, 0.0, SENT)
        rm.t.copy_(bn.running_mean)
        rv.t.copy_(bn.running_var)
        nbt = None if li in c.nbt0 else torch.tensor([cc.NBT0], dtype=torch.int64, device=DEV)
        slots = [None if (q is None or li in no_grads) else Buf(tuple(q.shape), torch.float32, NAN) for q in par]
        keep += dev + [nbt]
        nbts.append(nbt)
        stats["L%d.running_mean" % li], stats["L%d.running_var" % li] = rm, rv
        for stem, s in zip(STEMS, slots):
            if s is not None:
                grads["L%d.%s" % (li, stem)] = s
        addr = lambda t: 0 if t is None else t.data_ptr()
        table_rows.append([addr(q) for q in dev] + [rm.t.data_ptr(), rv.t.data_ptr(), addr(nbt)]
                          + [0 if s is None else s.t.data_ptr() for s in slots] + [0, 0, 0])
    table = torch.tensor(table_rows, dtype=torch.int64, device=DEV)
    assert table.shape == (n, 14)
    X, dY = _padded(p.x[:rows], N, dt), _padded(p.dy[:rows], N, dt)
    assert X.shape == (N, c.c0, c.L) and X.dtype == dt
    mom = (ctypes.c_float * n)(*[ly.mom for ly in c.layers])
    eps = (ctypes.c_float * n)(*[ly.eps for ly in c.layers])
    n_dev = None if nv is None else torch.tensor([nv], dtype=torch.int64, device=DEV)
    before = {k: b.t.clone() for k, b in stats.items()}
    saved = Buf((int(lib.wfs_conv1d_saved_floats(*shape_args)),), torch.float32, NAN, SENT)
    Y = Buf(tuple(dY.shape), dt, SENT)
    L.check(lib.wfs_conv1d_fwd(L.ptr(X), *shape_args, L.ptr(table), mom, eps, int(training), L.ptr(saved.t), L.ptr(Y.t),
                               code, L.ptr(n_dev), L.stream_ptr()))
    ws = Buf((int(lib.wfs_conv1d_bwd_workspace_floats(*shape_args)),), torch.float32, NAN, SENT)
    dX = Buf(tuple(X.shape), dt, SENT) if dx else None
    L.check(lib.wfs_conv1d_bwd(L.ptr(X), L.ptr(dY), *shape_args, L.ptr(table), int(training), L.ptr(saved.t),
                               L.ptr(dX.t) if dx else None, L.ptr(ws.t), code, L.ptr(n_dev), L.stream_ptr()))
    torch.cuda.synchronize()
    tag = cc.run_id(i, kind, mode, nv)
    for what, b in [("saved", saved), ("workspace", ws), ("y", Y)] + ([("dx", dX)] if dx else []) + list(grads.items()) + list(stats.items()):
        b.check_tail("%s %s" % (tag, what))
    assert bool((Y.t.float() >= 0).all()), "%s: a cell of Y was not written" % tag
    if dx:
        assert not bool((dX.t.float() == SENT).any()), "%s: a cell of dX was not written" % tag
    got = {k: b.t for k, b in list(grads.items()) + list(stats.items())}
    got["y"] = Y.t
    if dx:
        got["dx"] = dX.t
    return Run(got, nbts, before, (keep, table, X, dY, saved, ws, n_dev))


def check(i, kind, mode, run, nv=None, label=None, skip=()):
    """Every tensor of the float64 reference over the rows that count against run.got[name] with the bars of the module
    docstring; the rows behind them exactly zero; the counters and, in eval mode, the running statistics untouched.
    Names in `skip` are not expected."""
    c = cc.CASES[i]
    rows = cc.rows_of(c, nv)
    p = cc.problem(i, kind, mode, rows)
    training, u, floor = mode == "train", U_ROUND[kind], FLOOR[kind]
    tag = label or cc.run_id(i, kind, mode, nv)
    got, worst = run.got, {}
    for li, nbt in enumerate(run.nbts):
        assert (nbt is None) == (li in c.nbt0)
        if nbt is not None:
            assert int(nbt) == cc.NBT0 + int(training), (tag, li, int(nbt))
    if not training:
        for k, b in run.before.items():
            assert torch.equal(got[k].view(torch.int32), b.view(torch.int32)), "%s: eval moved %s" % (tag, k)
    for name, b in p.ref:
        if name in skip:
            assert name not in got
            continue
        a = got[name].detach().double().cpu()
        assert bool(torch.isfinite(a).all()), "%s %s is not finite" % (tag, name)
        if name in ("y", "dx"):
            assert a.shape[0] == c.N and not bool(a[rows:].any()), "%s %s: a row behind the count is not zero" % (tag, name)
            a = a[:rows]
        assert tuple(a.shape) == tuple(b.shape), name
        special = training and name in p.summed
        if not special:
            assert not bool(a[b == 0].any()), "%s %s: not zero where float64 is exactly zero" % (tag, name)
        scale = cc.scale_of(name, b, p.summed, training)
        assert scale > 0, name
        err = (a - b).abs()
        if name in ("y", "dx"):
            ratio = float((err / ((1 + u) * BAR32 * scale + u * b.abs() + floor)).max())
        else:
            ratio = float(err.max()) / (BAR32 * scale)
        print("%s %s: err %.3e of scale %.3e = %.2e; over its bar %.3f" % (tag, name, float(err.max()), scale,
                                                                           float(err.max()) / scale, ratio))
        g = _group(name)
        worst[g] = max(worst.get(g, 0.0), ratio)
    key = (label or c.name + ("" if nv is None else " nv%d" % nv), kind, mode)
    old = WORST.setdefault(key, {})
    for g, w in worst.items():
        old[g] = max(old.get(g, 0.0), w)
    missed = {g: "%.4g" % w for g, w in worst.items() if not w <= 1.0}
    assert not missed, "%s: worst error over its bar: %s" % (tag, missed)


@pytest.mark.parametrize("i,kind,mode,nv", [pytest.param(i, k, m, nv, id=cc.run_id(i, k, m, nv))
                                            for i, k, m, nv in cc.case_params()])
def test_case_against_float64(i, kind, mode, nv):
    c = cc.CASES[i]
    r = run_case(i, kind, mode, nv)
    check(i, kind, mode, r, nv)
    if "unread samples" in c.arm:
        ly, lout = c.layers[0], cc.shapes(c)[0][2]
        read = torch.zeros(c.L, dtype=torch.bool)
        for t in range(lout):
            read[t * ly.st: t * ly.st + ly.fs] = True
        dx = r.got["dx"].float().cpu()
        assert int((~read).sum()) >= 3 and not bool(dx[:, :, ~read].any()) and bool(dx[:, :, read].any())


def test_a_count_above_the_capacity_is_the_capacity():
    """n_valid = 12 at capacity 9 gives the bits of n_valid = 9 and of NULL."""
    i = cc.BY_NAME["nv"]
    a, b, c = (run_case(i, "bf16", "train", nv) for nv in (None, 9, 12))
    bits_equal(a.got, b.got, list(a.got))
    bits_equal(a.got, c.got, list(a.got))


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nv", [0, -3])
def test_an_empty_batch_gives_zeros_folds_zero_statistics_and_counts_a_batch(nv, kind):
    """include/wfsparse.h: "An empty batch (n_valid <= 0) in a training call folds mean 0 and variance 0 into the
    running statistics and counts a batch; torch raises there."  Every row of X and dY is a padding row."""
    i = cc.BY_NAME["nv"]
    c = cc.CASES[i]
    r = run_case(i, kind, "train", nv, rows=0)
    for name, t in r.got.items():
        assert bool(torch.isfinite(t.float()).all()), name
        if "running" not in name:
            assert not bool(t.any()), "%s is not exactly zero" % name
    assert sorted(n for n in r.got if "running" not in n) == sorted(
        ["y", "dx"] + ["L%d.%s" % (li, s) for li in range(len(c.layers)) for s in STEMS])
    for li, ly in enumerate(c.layers):
        assert int(r.nbts[li]) == cc.NBT0 + 1
        keepf = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(ly.mom, dtype=torch.float32)
        for s in ("running_mean", "running_var"):
            k = "L%d.%s" % (li, s)
            assert torch.equal(r.got[k].cpu(), keepf * r.before[k].cpu()), k


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["g2-127", "co-32-64"])
def test_without_dx_every_other_output_is_bit_equal(name, kind):
    i = cc.BY_NAME[name]
    full = run_case(i, kind, "train")
    part = run_case(i, kind, "train", dx=False)
    assert sorted(set(full.got) - set(part.got)) == ["dx"]
    bits_equal(full.got, part.got, list(part.got))
    check(i, kind, "train", part, label=name + " -dx", skip=("dx",))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("name,layer", [("g2-127", 0), ("co-32-64", 1)])
def test_gradient_addresses_of_one_layer_zero_leave_every_other_output_bit_equal(name, layer, kind):
    i = cc.BY_NAME[name]
    full = run_case(i, kind, "train")
    part = run_case(i, kind, "train", no_grads=(layer,))
    gone = ["L%d.%s" % (layer, s) for s in STEMS]
    assert sorted(set(full.got) - set(part.got)) == sorted(gone)
    bits_equal(full.got, part.got, list(part.got))
    check(i, kind, "train", part, label="%s -L%d slots" % (name, layer), skip=gone)


@pytest.mark.parametrize("name,kind", [("st-over", "bf16"), ("dw-8193", "f32")])
def test_a_second_forward_and_backward_gives_the_same_bits(name, kind):
    i = cc.BY_NAME[name]
    a, b = run_case(i, kind, "train"), run_case(i, kind, "train")
    bits_equal(a.got, b.got, list(a.got))


def test_one_16_bit_case_through_the_module():
    """Conv1DNet(fused=True) builds the records and sizes the buffers itself: case `module` (bf16), the plan the
    constructor gives for `stride-3` of tests/test_gpu_convnet.py, with the case's parameters loaded."""
    from waveformml_amd.psd import convnet
    i, kind, mode = cc.BY_NAME["module"], "bf16", "train"
    c, p = cc.CASES[i], cc.problem(i, kind, mode)
    net = convnet.Conv1DNet(c.L, fused=True, **cc.MODULE_KW)
    state = {}
    for li, (conv, bn) in enumerate(p.net):
        state.update({"network.%d.%s" % (3 * li, k): v for k, v in conv.state_dict().items()})
        state.update({"network.%d.%s" % (3 * li + 1, k): v for k, v in bn.state_dict().items()})
    net.load_state_dict(state)
    net = net.to(DEV).train()
    xg = p.x.to(DEV).requires_grad_(True)
    before = convnet.CONV1D_CALLS[0]
    y = net(xg)
    assert convnet.CONV1D_CALLS[0] == before + 1
    y.backward(p.dy.to(DEV))
    got, nbts, start = {"y": y.detach(), "dx": xg.grad}, [], {}
    for li in range(len(c.layers)):
        conv, bn = net.network[3 * li], net.network[3 * li + 1]
        assert isinstance(conv, nn.Conv1d) and isinstance(bn, nn.BatchNorm1d)
        got.update({"L%d.conv.weight" % li: conv.weight.grad, "L%d.conv.bias" % li: conv.bias.grad,
                    "L%d.bn.weight" % li: bn.weight.grad, "L%d.bn.bias" % li: bn.bias.grad,
                    "L%d.running_mean" % li: bn.running_mean, "L%d.running_var" % li: bn.running_var})
        nbts.append(bn.num_batches_tracked)
    check(i, kind, mode, Run(got, nbts, start, None), label=c.name + " module")
    # and the ctypes harness computes the same bits as the module route
    bits_equal(got, run_case(i, kind, mode).got, list(got))
