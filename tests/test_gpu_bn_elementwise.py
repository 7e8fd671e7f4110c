"""The elementwise passes of the register-resident BatchNorm kernels (csrc/bn.hip: k_bn_apply_rr / k_bn_bwd_apply_rr)
at the edges of their row lanes, through wfs_bn_relu_fwd / wfs_bn_relu_bwd and ctypes on raw device tensors.

16-bit rows move in lanes of 8 channels when C % 8 == 0 and the row buffers are 16-byte aligned, in lanes of 4 otherwise
and for fp32 rows; the reduce launch, and with it arm, rows per thread and partial count (wfs_bn_plan), is the same for
both.  Inputs, the float64 reference and the bars are tests/bn_cases.py's (its _draw and reference, ratio_f32 /
ratio_rows at BAR32 and U_ROUND); nothing of them is restated here.

The product of
  channels   8 (one group), 24 (3 groups, 4 idle threads), 32, 64, and 12 (no lane of 8: the 4-channel lane)
  capacity   1, 65, and unit * p - 1, unit * p, unit * p + 1 for p = 2, 4, 8, 16 with unit = the rows a launch holds per
             unit of rows-per-thread (8192 at C = 32); 16 unit + 1 rows leave the register-resident arm
  count      n_dev = 0, 1, N - 1, N and no n_dev
  row type   bf16, fp16 (and one fp32 case per channel count)
each running the forward with and without ReLU and the backward with training 1 and 0 on one drawn problem.  The eval
backward is handed the batch statistics as its running ones, so that the ReLU margin the draw conditioned holds for it.
Asserted per case: (a) every output within its bar of float64, (b) rows at and beyond the count keep the sentinel in Y
and dX, (c) a second call on the same inputs gives the same bits, (d) wfs_bn_plan reports what bn_cases.expected_plan
derives from the dispatch constants.  A count of 0 has no float64 reference: no row is written, dgamma = dbeta = 0.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DT = {"f32": 0, "bf16": 1, "f16": 2}
SENT = -768.0                      # exactly representable in bf16 and fp16
CHANNELS = (8, 24, 32, 64, 12)


def _L():
    from waveformml_amd import _lib
    return _lib


def unit_rows(C):
    """Rows a register-resident launch holds per unit of rows-per-thread: blocks x row slots of the reduce kernel."""
    blocks = min(bc.FOLD_PER * (bc.TB // bc.fold_cp(C)), bc.RR_BLOCKS)
    return blocks * (bc.TB // (C // 4))


def capacities(C):
    u = unit_rows(C)
    return [1, 65] + [u * p + d for p in (2, 4, 8, 16) for d in (-1, 0, 1)]


def counts(N):
    """Device-side counts of a capacity, None = no n_dev."""
    return sorted({0, 1, N - 1, N}) + [None]


@functools.lru_cache(maxsize=2)
def problem(C, N, valid, kind):
    """bn_cases._draw for a case of this file (training, ReLU, affine, running statistics), redrawn as make_problem
    redraws; read-only and shared by the count N and the call without a count."""
    case = SimpleNamespace(name="lane-C%d-N%d-v%d" % (C, N, valid), tag="lane", C=C, N=N, valid=valid, kinds=(kind,),
                           relu=True, training=True, affine=True, running=True, special=None, seed=7 * C + N % 1009)
    for attempt in range(bc.ATTEMPTS):
        p = bc._draw(case, kind, attempt)
        if p.moved_share <= bc.MOVED_MAX:
            return p
    raise AssertionError("%s %s: no draw out of %d is well-posed" % (case.name, kind, bc.ATTEMPTS))


@functools.lru_cache(maxsize=2)
def references(C, N, valid, kind):
    """float64: training with ReLU (everything), training without ReLU (y), eval backward on the batch statistics."""
    p = problem(C, N, valid, kind)
    full = bc.reference(p.x, p.g, p.gamma, p.beta, p.rm, p.rv, p.valid, True, True)
    plain = bc.reference(p.x, p.g, p.gamma, p.beta, p.rm, p.rv, p.valid, False, True)
    frozen = bc.reference(p.x, p.g, p.gamma, p.beta, full.mean, full.var, p.valid, True, False)
    return full, plain, frozen


def _t(a, dtype=None):
    t = torch.tensor(a, device=DEV)                    # a copy: the problems are shared and read-only
    return t.to(dtype) if dtype is not None else t


def _rows(n, C, dt, offset=0):
    """[n, C] rows of sentinels; offset: the buffer starts that many elements behind a 16-byte boundary."""
    return torch.full((n * C + offset,), SENT, dtype=dt, device=DEV)[offset:].view(n, C)


def run(p, kind, n_dev_value, offset=0):
    """The four modes on one problem.  Returns {name: device tensor}."""
    L = _L()
    lib = L.load()
    cap, C, dt = p.cap, p.case.C, TORCH[kind]
    X, dY = _rows(cap, C, dt, offset), _rows(cap, C, dt, offset)
    X.copy_(_t(p.x, dt))
    dY.copy_(_t(p.g, dt))
    gamma, beta = _t(p.gamma), _t(p.beta)
    n_dev = None if n_dev_value is None else torch.tensor([n_dev_value], dtype=torch.int64, device=DEV)
    nbytes = int(lib.wfs_bn_workspace_bytes(cap, C))
    out = {}

    def ch():
        return torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)

    def ws():
        return torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)

    for relu, tag in ((1, ""), (0, "_plain")):
        Y, sm, si, rm, rv = _rows(cap, C, dt, offset), ch(), ch(), _t(p.rm), _t(p.rv)
        tracked = torch.tensor([bc.TRACKED0], dtype=torch.int64, device=DEV)
        w = ws()
        L.check(lib.wfs_bn_relu_fwd(L.ptr(X), cap, C, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(tracked),
                                    bc.MOMENTUM, bc.EPS, 1, relu, L.ptr(Y), L.ptr(sm), L.ptr(si), L.ptr(w), nbytes,
                                    DT[kind], L.ptr(n_dev), L.stream_ptr()))
        out.update({"y" + tag: Y, "save_mean" + tag: sm, "save_invstd" + tag: si, "running_mean" + tag: rm,
                    "running_var" + tag: rv, "tracked" + tag: tracked})
    for training, tag in ((1, ""), (0, "_frozen")):
        dX, dg, db = _rows(cap, C, dt, offset), ch(), ch()
        w = ws()
        L.check(lib.wfs_bn_relu_bwd(L.ptr(X), L.ptr(dY), cap, C, L.ptr(gamma), L.ptr(beta), L.ptr(out["save_mean"]),
                                    L.ptr(out["save_invstd"]), training, 1, L.ptr(dX), L.ptr(dg), L.ptr(db), L.ptr(w),
                                    nbytes, DT[kind], L.ptr(n_dev), L.stream_ptr()))
        out.update({"dX" + tag: dX, "dgamma" + tag: dg, "dbeta" + tag: db})
    torch.cuda.synchronize()
    return out


def same_bits(a, b):
    for t in a:
        assert torch.equal(a[t].contiguous().view(torch.uint8), b[t].contiguous().view(torch.uint8)), t


def plan(N, C, kind, training, backward):
    per, partials = ctypes.c_int32(-7), ctypes.c_int32(-7)
    fam = _L().load().wfs_bn_plan(N, C, DT[kind], training, backward, ctypes.byref(per), ctypes.byref(partials))
    return fam, per.value, partials.value


def check(C, N, kind, count):
    valid = N if count is None else count
    p = problem(C, N, max(valid, 1), kind)             # a count of 0 runs on the inputs of the count 1
    out = run(p, kind, count)
    print("C %d N %d %s count %s" % (C, N, kind, count))
    # (d) the plan: that of the reduce launch, whatever lane the elementwise kernels take
    for training, backward in ((1, 0), (1, 1), (0, 1)):
        assert plan(N, C, kind, training, backward) == bc.expected_plan(N, C, kind, training, backward)
    # (b) rows at and beyond the count
    for t in ("y", "y_plain", "dX", "dX_frozen"):
        assert bool((out[t][valid:] == SENT).all()), "%s: a row at or beyond the valid count was written" % t
    # (c) the same bits again
    same_bits(out, run(p, kind, count))
    if valid == 0:
        for t in ("dgamma", "dbeta", "dgamma_frozen", "dbeta_frozen"):
            assert bool((out[t] == 0).all()), t
        return
    # (a) float64
    full, plain, frozen = references(C, N, valid, kind)
    pairs = [(t, t, bc.wanted(full)[t]) for t in bc.wanted(full)]
    pairs += [("y_plain", "y", plain.y)] + [(t + "_plain", t, getattr(plain, t)) for t in bc.F32_TENSORS[:4]]
    pairs += [(t + "_frozen", t, getattr(frozen, t)) for t in ("dX", "dgamma", "dbeta")]
    worst = {}
    for name, t, want in pairs:
        got = out[name].float().cpu().numpy().astype(np.float64)
        if t in bc.ROW_TENSORS:
            assert np.isfinite(got[:valid]).all(), "%s is not finite" % name
            worst[name] = bc.ratio_rows(got[:valid], want[:valid], bc.U_ROUND[kind])
        else:
            worst[name] = bc.ratio_f32(got, want)
    print("  " + "  ".join("%s %.4f" % kv for kv in sorted(worst.items())))
    for name, r in sorted(worst.items()):
        assert r <= 1.0, "C %d N %d %s count %s, %s: worst error is %.4g of its bar" % (C, N, kind, count, name, r)
    y = out["y"].float().cpu().numpy()
    assert np.array_equal(y[:valid] == 0, full.y[:valid] == 0), "y is zero exactly where the reference is"
    assert int(out["tracked"].item()) == bc.TRACKED0 + 1 and int(out["tracked_plain"].item()) == bc.TRACKED0 + 1


def _params():
    out = []
    for C in CHANNELS:
        for N in capacities(C):
            for kind in ("bf16", "f16"):
                for count in counts(N):
                    out.append(pytest.param(C, N, kind, count,
                                            id="C%d-N%d-%s-%s" % (C, N, kind, "null" if count is None else "v%d" % count)))
    return out


@pytest.mark.parametrize("C,N,kind,count", _params())
def test_16_bit_rows(C, N, kind, count):
    check(C, N, kind, count)


@pytest.mark.parametrize("C", CHANNELS)
def test_fp32_rows_take_the_arm_they_took(C):
    """fp32 rows already move 16 bytes per lane: the forward stays register-resident up to PER 16, the backward up to 8."""
    N = unit_rows(C) * 8 + 1
    assert plan(N, C, "f32", 1, 0)[:2] == (bc.RR, 16) and plan(N, C, "f32", 1, 1)[0] == bc.LOOP4
    check(C, N, "f32", N - 1)


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_rows_off_a_16_byte_boundary_take_the_4_channel_lane(kind):
    """Row buffers that start 8 bytes behind a 16-byte boundary cannot move in 16-byte lanes; same bits either way."""
    C, N = 32, 2 * unit_rows(32) + 1
    p = problem(C, N, N - 1, kind)
    same_bits(run(p, kind, N - 1), run(p, kind, N - 1, offset=4))
