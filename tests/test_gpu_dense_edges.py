"""The dense Conv2d + BatchNorm2d + ReLU (+ Dropout) stack kernels (wfs_conv2d_fwd / wfs_conv2d_bwd, csrc/conv2d.hip)
and wfs_densify_rows at every planning edge against float64, through ctypes on raw device tensors with the 14-word
pointer records of include/wfsparse.h, for fp32, bf16 and fp16 rows.

Cases, inputs, arms and the float64 reference: tests/dense_cases.py; tests/test_dense_cases_host.py proves on the CPU
that every case is well-posed (no pre-ReLU value within 1e-5 of its layer's largest, 5 .. 95 % of the ReLUs on),
conditioned (torch's fp32 run within 3e-6 of float64; for 16-bit rows the float64 run with the backward's documented
16-bit operands within half the row type's bar), inside the bounds and on the arm it is there for.

Every call gets `saved` and the workspace exactly wfs_conv2d_saved_floats / wfs_conv2d_bwd_workspace_floats long and
filled with NaN, Y and dX filled with the sentinel -768 (Y is a ReLU output: a negative value is an unwritten cell),
every gradient slot filled with NaN, num_batches_tracked preset to 41, and five trailing elements behind `saved`, the
workspace, Y, dX and every gradient slot, which must keep their fill.  A kernel that reads a granule no kernel wrote
(the padding of an odd 16-bit activation, a statistics partial past the block count, a dW slice past the slice count)
poisons its result with NaN.

Bars, the project's own (waveform_cases.TOL): Y, dX, d conv.weight, d bn.weight, d bn.bias, running_mean and
running_var within 1e-5 / 2e-2 / 3e-3 (fp32 / bf16 / fp16) of each tensor's largest float64 magnitude; d conv.bias in
front of a training-mode BatchNorm (exactly zero) with the same bar against the summed |dz| of the reference, in eval
mode against its own magnitude.  Where the float64 reference is exactly zero (dX at input cells no tap reads, Y where
the ReLU is off or the element dropped) the kernels' value is exactly zero.  Every output is finite.
num_batches_tracked is 42 after a training call and 41 after an eval call, which leaves the running statistics
bit-identical.

Measured on an MI355X (profiles/dense_edges_errors.txt): worst error / bar 0.20 for fp32 rows
(k12800: Y; eight in eval mode: d bn.weight), 0.48 for bf16 (eight, training: d bn.weight -- the 16-bit operand model
of tests/dense_cases.py predicts 0.483), 0.37 for fp16 (col-32x1: the BN gradients); the 89 tests take 4.2 s.

The worst error / bar of every (case, row type, mode, tensor group) is printed when the module ends and written to
$WFS_DENSE_EDGES_REPORT when that is set (the table of DESIGN.md section 4).
"""
import collections
import ctypes

import pytest
import torch
from torch import nn

import dense_cases as dc
from edge_harness import NAN, SENT, Buf as _Buf, bits_equal as _bits_equal, error_report
from waveform_cases import DEV, TOL

pytestmark = pytest.mark.gpu

NBT0 = 41
GROUPS = ("y", "dx", "dw", "db", "dbn", "running")
WORST = {}                         # (case, kind, mode) -> {group: worst error / bar}


def _L():
    from waveformml_amd import _lib
    return _lib


_error_report = error_report(WORST, GROUPS, "WFS_DENSE_EDGES_REPORT")


def _group(name):
    if name in ("y", "dx"):
        return name
    return {"conv.weight": "dw", "conv.bias": "db", "bn.weight": "dbn", "bn.bias": "dbn", "running_mean": "running",
            "running_var": "running"}[name.split(".", 1)[1]]


Run = collections.namedtuple("Run", "got keep")        # keep: what the outputs' addresses live in


def run_case(i, kind, mode, dx=None, no_grads=()):
    """One wfs_conv2d_fwd and one wfs_conv2d_bwd through the C ABI on freshly poisoned buffers.  `dx`: whether dX is
    given (default: the case's); `no_grads`: the layers whose four gradient addresses are 0.  Returns the outputs
    {name: device tensor} (dx as NCHW) and checks every tail, sentinel and counter on the way."""
    L = _L()
    lib = L.load()
    c, p = dc.CASES[i], dc.problem(i, kind, mode)
    training, dt, code = mode == "train", dc.KINDS[kind], list(dc.KINDS).index(kind)
    dx = c.dx if dx is None else dx
    n = len(c.layers)
    arrays = [L.i32_array(v) for v in dc.plan_arrays(c)]
    shape_args = (c.B, c.H, c.W, c.c0) + tuple(arrays) + (n,)
    assert lib.wfs_conv2d_ok(c.c0, *arrays, n, c.B, c.H, c.W, int(training), code) == L.WFS_OK
    keep, rows, grads, stats, nbts = [], [], {}, {}, []
    for li, (conv, bn) in enumerate(p.net):
        par = [conv.weight, conv.bias, bn.weight, bn.bias]
        dev = [None if q is None else q.detach().to(DEV).contiguous() for q in par]
        rm, rv = _Buf(bn.running_mean.shape, torch.float32, 0.0, SENT), _Buf(bn.running_var.shape, torch.float32, 0.0, SENT)
        rm.t.copy_(bn.running_mean)
        rv.t.copy_(bn.running_var)
        nbt = None if li in c.nbt0 else torch.tensor([NBT0], dtype=torch.int64, device=DEV)
        slots = [None if (q is None or li in no_grads) else _Buf(tuple(q.shape), torch.float32, NAN) for q in par]
        keep += dev + [nbt]
        nbts.append(nbt)
        stats["L%d.running_mean" % li], stats["L%d.running_var" % li] = rm, rv
        for stem, s in zip(("conv.weight", "conv.bias", "bn.weight", "bn.bias"), slots):
            if s is not None:
                grads["L%d.%s" % (li, stem)] = s
        addr = lambda t: 0 if t is None else t.data_ptr()
        rows.append([addr(q) for q in dev] + [rm.t.data_ptr(), rv.t.data_ptr(), addr(nbt)]
                    + [0 if s is None else s.t.data_ptr() for s in slots] + [0, 0, 0])
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    assert table.shape == (n, 14)
    X = p.x.permute(0, 2, 3, 1).contiguous().to(DEV)                  # channels-last, as the header says
    dY = p.dy.contiguous().to(DEV)
    mom = (ctypes.c_float * n)(*[ly.mom for ly in c.layers])
    eps = (ctypes.c_float * n)(*[ly.eps for ly in c.layers])
    drop = None if c.drop is None else (ctypes.c_float * n)(*c.drop)
    seed = None if c.drop is None else torch.tensor([dc.DROP_SEED], dtype=torch.int64, device=DEV)
    before = {k: b.t.clone() for k, b in stats.items()}
    saved = _Buf((int(lib.wfs_conv2d_saved_floats(*shape_args, code)),), torch.float32, NAN, SENT)
    Y = _Buf(tuple(p.dy.shape), dt, SENT)
    L.check(lib.wfs_conv2d_fwd(L.ptr(X), *shape_args, L.ptr(table), mom, eps, drop, L.ptr(seed), int(training),
                               L.ptr(saved.t), L.ptr(Y.t), code, L.stream_ptr()))
    ws = _Buf((int(lib.wfs_conv2d_bwd_workspace_floats(*shape_args, code)),), torch.float32, NAN, SENT)
    dX = _Buf((c.B, c.H, c.W, c.c0), dt, SENT) if dx else None
    L.check(lib.wfs_conv2d_bwd(L.ptr(X), L.ptr(dY), *shape_args, L.ptr(table), drop, L.ptr(seed), int(training),
                               L.ptr(saved.t), L.ptr(dX.t) if dx else None, L.ptr(ws.t), code, L.stream_ptr()))
    torch.cuda.synchronize()
    tag = dc.run_id(i, kind, mode)
    for what, b in [("saved", saved), ("workspace", ws), ("y", Y)] + ([("dx", dX)] if dx else []) + list(grads.items()) + list(stats.items()):
        b.check_tail("%s %s" % (tag, what))
    assert bool((Y.t.float() >= 0).all()), "%s: a cell of Y was not written" % tag
    if dx:
        assert not bool((dX.t.float() == SENT).any()), "%s: a cell of dX was not written" % tag
    for li, nbt in enumerate(nbts):
        if nbt is not None:
            assert int(nbt) == NBT0 + int(training), (tag, li, int(nbt))
    if not training:
        for k, b in stats.items():
            assert torch.equal(b.t.view(torch.int32), before[k].view(torch.int32)), "%s: eval moved %s" % (tag, k)
    got = {k: b.t for k, b in list(grads.items()) + list(stats.items())}
    got["y"] = Y.t
    if dx:
        got["dx"] = dX.t.permute(0, 3, 1, 2)
    return Run(got, (keep, table, X, dY, saved, ws))


def check(i, kind, mode, got, label=None, skip=()):
    """Every tensor of the case's float64 reference against got[name] with the bars of the module docstring; names in
    `skip` are not expected."""
    c, p = dc.CASES[i], dc.problem(i, kind, mode)
    training, tol = mode == "train", TOL[dc.KINDS[kind]]
    worst = {}
    for name, b in p.ref:
        if name in skip:
            assert name not in got
            continue
        a = got[name].detach().double().cpu()
        assert tuple(a.shape) == tuple(b.shape), name
        assert bool(torch.isfinite(a).all()), "%s %s is not finite" % (label or dc.run_id(i, kind, mode), name)
        if not (training and name in p.bias_scale):
            assert not bool(a[b == 0].any()), "%s %s: not zero where float64 is exactly zero" % (label or c.name, name)
        err, scale = float((a - b).abs().max()), dc.scale_of(name, b, p.bias_scale, training)
        assert scale > 0, name
        print("%s %s: err %.3e of scale %.3e = %.2e; bar %.0e" % (label or dc.run_id(i, kind, mode), name, err, scale, err / scale, tol))
        g = _group(name)
        worst[g] = max(worst.get(g, 0.0), err / (tol * scale))
    key = (label or c.name, kind, mode)
    old = WORST.setdefault(key, {})
    for g, w in worst.items():
        old[g] = max(old.get(g, 0.0), w)
    missed = {g: "%.4g" % w for g, w in worst.items() if not w <= 1.0}
    assert not missed, "%s: worst error over its bar: %s" % (label or dc.run_id(i, kind, mode), missed)


@pytest.mark.parametrize("i,kind,mode", [pytest.param(i, k, m, id=dc.run_id(i, k, m)) for i, k, m in dc.case_params()])
def test_case_against_float64(i, kind, mode):
    c = dc.CASES[i]
    r = run_case(i, kind, mode)
    check(i, kind, mode, r.got, skip=() if c.dx else ("dx",))
    if not c.dx:
        # the twin with dX: no other output may notice
        full = run_case(i, kind, mode, dx=True)
        _bits_equal(r.got, full.got, list(r.got))
        check(i, kind, mode, full.got, label=c.name + " +dx")
    if "unread cells of dX" in c.arm:
        dx = r.got["dx"]
        assert not bool(dx[:, :, -1, :].any()) and not bool(dx[:, :, :, -1].any())


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gradient_addresses_of_one_layer_zero_leave_every_other_output_bit_equal(kind):
    i = dc.BY_NAME["chain-31-33"]
    full = run_case(i, kind, "train")
    part = run_case(i, kind, "train", no_grads=(1,))
    gone = [n for n in full.got if n.startswith("L1.") and "running" not in n]
    assert sorted(gone) == ["L1.bn.bias", "L1.bn.weight", "L1.conv.bias", "L1.conv.weight"]
    assert sorted(set(full.got) - set(part.got)) == sorted(gone)
    _bits_equal(full.got, part.got, list(part.got))
    check(i, kind, "train", part.got, label="chain-31-33 -L1 slots", skip=gone)


@pytest.mark.parametrize("name,kind", [("nrb-over", "bf16"), ("dw-2052", "bf16")])
def test_a_second_forward_and_backward_gives_the_same_bits(name, kind):
    i = dc.BY_NAME[name]
    a, b = run_case(i, kind, "train"), run_case(i, kind, "train")
    _bits_equal(a.got, b.got, list(a.got))


def test_one_16_bit_case_through_the_module():
    """Conv2DBlock(fused=True) builds the records and sizes the buffers itself: `g-d2-k5` in bf16 (the module list is
    replaced by the case's layers; the kernels read the plan off the live modules)."""
    from waveformml_amd.psd import convnet2d
    i, kind, mode = dc.BY_NAME["g-d2-k5"], "bf16", "train"
    c, p = dc.CASES[i], dc.problem(i, kind, mode)
    block = convnet2d.Conv2DBlock(c.c0, c.layers[-1].cout, len(c.layers), [c.H, c.W, c.c0], fused=True)
    mods = []
    for conv, bn in dc._twin(p.net, torch.float32, True):
        mods += [conv, bn, nn.ReLU()]
    block.model = nn.Sequential(*mods)
    block = block.to(DEV).train()
    xg = p.x.to(DEV).requires_grad_(True)
    before = convnet2d.CONV2D_CALLS[0]
    y = block(xg)
    assert convnet2d.CONV2D_CALLS[0] == before + 1
    y.backward(p.dy.to(DEV))
    got = {"y": y.detach(), "dx": xg.grad}
    for li in range(len(c.layers)):
        conv, bn = block.model[3 * li], block.model[3 * li + 1]
        got.update({"L%d.conv.weight" % li: conv.weight.grad, "L%d.bn.weight" % li: bn.weight.grad,
                    "L%d.bn.bias" % li: bn.bias.grad, "L%d.running_mean" % li: bn.running_mean,
                    "L%d.running_var" % li: bn.running_var})
        assert int(bn.num_batches_tracked) == NBT0 + 1
    check(i, kind, mode, got, label=c.name + " module")
    # and the ctypes harness computes the same bits as the module route
    _bits_equal(got, run_case(i, kind, mode).got, list(got))


@pytest.mark.parametrize("d", dc.DENSIFY_CASES, ids=[d.name for d in dc.DENSIFY_CASES])
def test_densify_rows_bit_for_bit(d):
    L = _L()
    lib = L.load()
    coords, rows, n_valid, want = dc.densify_problem(d)
    out = _Buf((d.B, d.H, d.W, d.C), dc.KINDS[d.kind], SENT)
    nv = torch.tensor([n_valid], dtype=torch.int64, device=DEV) if d.counted else None
    cg, rg = coords.to(DEV), rows.to(DEV)
    L.check(lib.wfs_densify_rows(L.ptr(rg), L.ptr(cg), rows.shape[0], d.C, d.B, d.H, d.W, L.ptr(nv), L.ptr(out.t),
                                 list(dc.KINDS).index(d.kind), L.stream_ptr()))
    torch.cuda.synchronize()
    out.check_tail(d.name)
    assert torch.equal(out.t.cpu().view(torch.uint8), want.contiguous().view(torch.uint8))
