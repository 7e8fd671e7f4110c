"""The wide matrix-core products of csrc/wide.hip (k_gemm16 with its staging kernels and k_sum_rows) at every planning
arm against float64: conv forward and dX (wfs_wide_gather_conv), conv dW in both orientations (the wide arm of
wfs_gather_dw) and the dense head layer (wfs_wide_linear_fwd / _bwd: y, dX, dW, db), for fp32, bf16 and fp16 rows.

Cases, inputs and references: tests/wide_cases.py; tests/test_wide_cases_host.py proves on the CPU that every case
reaches the arm it is there for (wfs_wide_plan) and that its inputs are well-posed.  Calls go through
spconv/functional.py (gather_conv, gather_dw, wide_linear); the C entry points are called directly where the wrappers
cannot express the case: an output prefilled with a sentinel, a workspace prefilled with NaN, db of the linear layer.

Bars, EVERY element held to its own (scale = the element's sum of absolute terms):
  exact set   fp32 results (fp32 Y and dX, every dW, linear y, dW, db) equal float64 bit for bit; 16-bit results equal
              the float64 value converted to the row type by torch, bit for bit
  gauss set   fp32 results |err| <= 1e-5 scale; 16-bit results |err| <= u |want| + 1e-5 scale, u = 2^-8 (bf16),
              2^-11 (fp16); an element with no term must be exact
Rows of Y at or beyond a device-side count are prefilled with a sentinel and must come back bit for bit; source rows no
valid row reads, and S / G rows beyond the count of a dW, hold NaN: no NaN may reach a result.  The workspace of a dW
with a count is prefilled with NaN: every slab of an empty part must be written as zeros for the sum to stay finite.

The worst ratio per (product, arm, row type, tensor) of the gauss set is printed when the module ends and written to
$WFS_WIDE_EDGES_REPORT when that is set: profiles/wide_edges_errors.txt.
"""
import os

import numpy as np
import pytest
import torch

import wide_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENT = -768.0                      # exactly representable in bf16 and fp16
WORST = {}                         # (product, arm, kind, tensor) -> worst ratio of the gauss set
RAN = {}                           # (product, arm, kind) -> exact-set comparisons that were bit-equal


def _L():
    from waveformml_amd import _lib
    return _lib


def _fsp():
    from waveformml_amd.spconv import functional as Fsp
    return Fsp


def _t(a, kind=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)          # a copy: the problems are read-only
    return t.to(TORCH[kind]) if kind else t


def _f32(a):
    return _t(None if a is None else np.asarray(a, np.float32))


def _view_at(t, off):
    """The same values as a view ``off`` elements into a larger buffer (whose start is 256-byte aligned)."""
    big = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = big[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16 and v.is_contiguous()
    return v


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    text = _report_text()
    print("\n" + text)
    path = os.environ.get("WFS_WIDE_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


def _report_text():
    lines = ["# gauss set: worst |got - want| / bar per product, planning arm, row type and tensor (<= 1 passes)"]
    lines += ["%-9s %-12s %-5s %-3s %.4f" % (k + (r,)) for k, r in sorted(WORST.items())]
    lines.append("# exact set: comparisons that equalled float64 bit for bit, per product, arm and row type")
    lines += ["%-9s %-12s %-5s %d" % (k + (n,)) for k, n in sorted(RAN.items())]
    return "\n".join(lines)


def compare(product, arm, kind, which, what, got, want, scale, sixteen):
    """One result tensor against its float64 reference at the bar of its input set."""
    assert tuple(got.shape) == want.shape, (got.shape, want.shape)
    if which == "exact":
        if sixteen:
            expect = torch.from_numpy(np.array(want)).to(TORCH[kind])
            assert got.dtype == expect.dtype
        else:
            expect = torch.from_numpy(np.array(want)).to(torch.float32)
            assert got.dtype == torch.float32 and np.array_equal(expect.double().numpy(), want)
        same = torch.equal(got.cpu(), expect)
        if not same:
            g = got.double().cpu().numpy()
            bad = np.argwhere(g != expect.double().numpy())
            raise AssertionError("%s %s %s %s: %d of %d elements differ from float64, first at %s: got %r want %r" % (
                product, arm, kind, what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], want[tuple(bad[0])]))
        RAN[(product, arm, kind)] = RAN.get((product, arm, kind), 0) + 1
        return
    r = wc.ratio(got.double().cpu().numpy(), want, scale, wc.U_ROUND[kind] if sixteen else 0.0)
    print("%s %s %s %s ratio %.4f" % (product, arm, kind, what, r))
    key = (product, arm, kind, what)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, (product, arm, kind, what, r)


# ---------------------------------------------------------------------------------------------------------------- conv
def _raw_wide_conv(c, kind, tr, table, kmap, X, W, bias, r_dev, w16=None):
    """lib.wfs_wide_gather_conv as Fsp.gather_conv calls it, into a caller's Y prefilled with the sentinel."""
    L = _L()
    lib = L.load()
    Cw_in, Cw_out = int(W.shape[1]), int(W.shape[2])
    Cy = Cw_in if tr else Cw_out
    Y = torch.full((c.R, Cy), SENT, dtype=X.dtype, device=DEV)
    nbytes = int(lib.wfs_wide_conv_workspace_bytes(c.K, c.R, X.shape[0], c.Cx, Cy, 0 if table is None else 1, L.dtype_code(X)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    L.check(lib.wfs_wide_gather_conv(L.ptr(table), kmap, c.K, c.ik, c.R, L.ptr(X), X.shape[0], c.Cx, L.ptr(W), L.ptr(w16),
                                     Cw_in, Cw_out, 1 if tr else 0, L.ptr(bias), L.ptr(Y), L.dtype_code(X), L.ptr(r_dev),
                                     L.ptr(ws), ws.numel(), L.stream_ptr()))
    return Y


def run_conv(name, kind, which, tr, count=None, x_off=0, w_off=0, given_filters=False):
    """One conv product; returns (Y on the device, rows that are valid)."""
    L, Fsp = _L(), _fsp()
    p = wc.conv_problem(name, kind, which, tr)
    c = p.case
    assert L.load().wfs_wide_conv_ok(c.K, c.R, c.XR, c.Cx, c.Cy, wc.DT[kind]) == 1
    X, W, bias = _t(p.X, kind), _f32(p.W), _f32(p.bias)
    table = _t(p.table)
    kmap = None if p.kmap is None else L.i32_array(p.kmap)
    if x_off:
        X = _view_at(X, x_off)
    if w_off:
        W = _view_at(W, w_off)
    w16 = Fsp.filters16(W, X) if given_filters else None
    if count is None:
        Y = Fsp.gather_conv(table, kmap, c.K, c.ik, c.R, X, W, tr, bias, None, w16)
        torch.cuda.synchronize()
        return Y, c.R
    v = min(count, c.R)
    X[torch.from_numpy(~wc.conv_rows_needed(p, v)).to(DEV)] = float("nan")          # rows no valid row reads
    r_dev = torch.tensor([count], dtype=torch.int64, device=DEV)
    Y = _raw_wide_conv(c, kind, tr, table, kmap, X, W, bias, r_dev, w16)
    torch.cuda.synchronize()
    assert bool((Y[v:] == SENT).all()), "%s %s: a row at or beyond the device-side count %d was written" % (name, kind, count)
    return Y, v


def check_conv(name, kind, which, tr, Y, v):
    c = wc.CONV[name]
    want, scale = wc.conv_reference(name, kind, which, tr)
    compare("conv_dx" if tr else "conv_fwd", c.arm, kind, which, "Y", Y[:v], want[:v], scale[:v], kind != "f32")


def _ids(runs):
    return ["%s-v%s" % (n, "all" if v is None else v) for n, v in runs]


@pytest.mark.parametrize("which", wc.SETS)
@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dx"])
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name,count", wc.conv_runs(), ids=_ids(wc.conv_runs()))
def test_wide_conv(name, count, kind, tr, which):
    Y, v = run_conv(name, kind, which, tr, count)
    assert Y.dtype == TORCH[kind]
    check_conv(name, kind, which, tr, Y, v)


@pytest.mark.parametrize("which", wc.SETS)
@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dx"])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["split_1100", "dense_1028"])
def test_fp32_rows_and_filters_in_place_against_copied(name, off, tr, which):
    """fp32 X and W with channel counts that are multiples of 4: at a 16-byte address the product reads them in place; the
    same data 1, 2 and 3 elements into a larger buffer (4-byte aligned only) goes through the padded copies."""
    c = wc.CONV[name]
    assert c.Cx % 4 == 0 and c.Cy % 4 == 0
    Y, v = run_conv(name, "f32", which, tr, None, x_off=off or 4, w_off=off or 4)
    check_conv(name, "f32", which, tr, Y, v)


@pytest.mark.parametrize("which", wc.SETS)
@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dx"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["nseg2", "dense_1030"])
def test_16_bit_rows_at_an_odd_element_offset(name, kind, tr, which):
    """Rows that start on an odd element of a larger buffer (2-byte aligned only), gathered through a table."""
    assert wc.CONV[name].table
    Y, v = run_conv(name, kind, which, tr, None, x_off=1)
    check_conv(name, kind, which, tr, Y, v)


@pytest.mark.parametrize("tr", [False, True], ids=["fwd", "dx"])
@pytest.mark.parametrize("kind", wc.KINDS)
def test_given_filter_copy_equals_the_call_that_converts(kind, tr):
    """Wp from wfs_wide_filters against Wp = NULL: bit-equal results (129 and 1025 filter columns: fp32 filters are
    copied too)."""
    given, _ = run_conv("split_1025", kind, "gauss", tr, None, given_filters=True)
    own, v = run_conv("split_1025", kind, "gauss", tr, None)
    assert torch.equal(given, own)
    check_conv("split_1025", kind, "gauss", tr, given, v)


# ------------------------------------------------------------------------------------------------------------------ dW
def _raw_gather_dw(c, table, kmap, S, G, swap, r_dev):
    """lib.wfs_gather_dw as Fsp.gather_dw calls it, with dW and the whole workspace prefilled with NaN."""
    L = _L()
    lib = L.load()
    dW = torch.full((c.K, c.Cg, c.Cs) if swap else (c.K, c.Cs, c.Cg), float("nan"), dtype=torch.float32, device=DEV)
    nbytes = max(int(lib.wfs_gather_dw_workspace_bytes(c.K, c.R, c.Cs, c.Cg)), 4)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    L.check(lib.wfs_gather_dw(L.ptr(table), kmap, c.K, c.ik, c.R, L.ptr(S), c.Cs, L.ptr(G), G.shape[0], c.Cg, 1 if swap else 0,
                              L.ptr(dW), L.dtype_code(S), L.ptr(ws), ws.numel() * 4, L.ptr(r_dev), None, 0, L.stream_ptr()))
    return dW


@pytest.mark.parametrize("which", wc.SETS)
@pytest.mark.parametrize("swap", [False, True], ids=["dw", "dw_swapped"])
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name,count", wc.dw_runs(), ids=_ids(wc.dw_runs()))
def test_wide_dw(name, count, kind, swap, which):
    L, Fsp = _L(), _fsp()
    p = wc.dw_problem(name, kind, which)
    c = p.case
    taken, plan = wc.plan_of(L.load(), wc.PLAN_DW, kind, c.K, c.R, 0, c.Cs, c.Cg)
    assert taken == 1
    S, G, table = _t(p.S, kind), _t(p.G, kind), _t(p.table)
    kmap = None if p.kmap is None else L.i32_array(p.kmap)
    if count is None:
        v = c.R
        dW = Fsp.gather_dw(table, c.K, c.ik, c.R, S, G, swap, kmap, None)
    else:
        n = wc.dw_count(c, count, plan["kchunk"])
        v = min(max(n, 0), c.R)
        S[v:] = float("nan")
        need = np.zeros(c.GR, bool)
        if c.ik >= 0:
            need[:v] = True
        if p.table is not None:
            e = p.table[:, :v]
            need[e[e >= 0]] = True
        G[torch.from_numpy(~need).to(DEV)] = float("nan")
        dW = _raw_gather_dw(c, table, kmap, S, G, swap, torch.tensor([n], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    want, scale = wc.dw_reference(name, kind, which, v, swap)
    if v == 0:
        assert not want.any() and bool((dW == 0).all()), "dW over no row must be exactly zero"
    compare("conv_dw", c.arm, kind, which, "dW", dW, want, scale, False)


# -------------------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("which", wc.SETS)
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", list(wc.LIN))
def test_wide_linear(name, kind, which):
    L, Fsp = _L(), _fsp()
    lib = L.load()
    p = wc.lin_problem(name, kind, which)
    c = p.case
    ref = wc.lin_reference(name, kind, which)
    lin = torch.nn.Linear(c.I, c.O).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(_f32(p.W))
        lin.bias.copy_(_f32(p.b))
    x = _t(p.x, kind).requires_grad_(True)
    g = _f32(p.g)
    assert Fsp.can_use_wide_linear(lin, x)
    y = Fsp.wide_linear(x, lin)
    y.backward(g)
    db = torch.full((c.O,), float("nan"), dtype=torch.float32, device=DEV)          # the wrapper sums db elsewhere
    ws = torch.empty((int(lib.wfs_wide_linear_workspace_bytes(c.B, c.I, c.O, wc.DT[kind])),), dtype=torch.uint8, device=DEV)
    L.check(lib.wfs_wide_linear_bwd(L.ptr(x.detach()), L.ptr(g), c.B, c.I, L.ptr(lin.weight.detach()), c.O, None, None,
                                    L.ptr(db), wc.DT[kind], L.ptr(ws), ws.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and x.grad.dtype == TORCH[kind]
    for what, got, sixteen in (("y", y.detach(), False), ("dX", x.grad, kind != "f32"), ("dW", lin.weight.grad, False),
                               ("db", db, False)):
        compare("linear", c.arm, kind, which, what, got, ref[what][0], ref[what][1], sixteen)
