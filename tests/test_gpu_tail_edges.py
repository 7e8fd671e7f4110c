"""The classifier tail at its dispatch edges against float64: the sparse head (csrc/shead.hip), the streaming head and
the fused cross-entropy (csrc/head.hip) and the mapped dense() (csrc/dense.hip), through the C ABI -- or through the
autograd functions of spconv/functional.py where their dispatch is what is under test.

References and case tables: tests/tail_cases.py (NumPy float64, pinned by tests/test_tail_cases_host.py).  16-bit rows
are rounded once on the host and fed to both sides.  Bars (none taken from the code under test):
  fp32 values (Y, dW, dB, fp32 dX)   |got - want| <= 1e-5 |want| + 1e-5 max|want|   (BASELINE.json north star, in
                                     test_gpu_parity._assert_close's form); cross-entropy: the same form at 1e-6
  16-bit dX                          one round-to-nearest of an fp32 value: 2^-8 |want| (bf16) or 2^-11 |want| (fp16)
                                     + 1e-5 max|want|, every element.  2^-8 and 2^-11 are the unit roundoffs of the 8-
                                     and 11-bit significands, so a correctly rounded result comes close to the bar
                                     (measured 0.99 of it) and a truncated or twice-rounded one exceeds it
  data movement, untouched rows      bit-exact
Buffers a kernel must fill completely start as NaN; dX of the sparse head and of the mapped dense() starts as a sentinel,
and every row that no live cell references must come back as it went in.  The worst error / bar of every family is
printed when the module ends (and written to $WFS_TAIL_EDGES_REPORT when that is set): profiles/tail_edges_errors.txt.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import tail_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BITS = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}
SENT = -768.0                 # exactly representable in bf16 and fp16
BAR = 1e-5
NAN = float("nan")
WORST = {}


def _lib():
    from waveformml_amd import _lib as lib
    return lib


def _fsp():
    from waveformml_amd.spconv import functional as Fsp
    return Fsp


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    lines = ["# worst |got - want| / bar per family and tensor (<= 1 passes)"]
    lines += ["%-16s %-8s %.4f" % (fam, what, r) for (fam, what), r in sorted(WORST.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("WFS_TAIL_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _check(family, what, got, want, rel=BAR, rel_of_scale=BAR):
    if torch.is_tensor(got):
        got = got.detach().float().cpu().numpy()
    r = tc.err_ratio(got, want, rel, rel_of_scale)
    WORST[(family, what)] = max(WORST.get((family, what), 0.0), r)
    assert r <= 1.0, "%s %s: worst error is %.4g of its bar (rel %.3g, of scale %.3g)" % (family, what, r, rel, rel_of_scale)


def _check_dx(family, got, want, kind):
    _check(family, "dX_" + kind, got, want, max(BAR, tc.ROUND_REL[kind]), BAR)


def _t(a, kind=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(TORCH[kind]) if kind else t


def _full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _dev_map(cmap, V):
    """(ticket_ptr, slot_ptr, keepalive, V) as spconv/ops.py hands it on; the cell_row form passes one array twice."""
    if cmap.form == "cell_row":
        cr = _t(cmap.slot)
        return (cr.data_ptr(), cr.data_ptr(), cr, V)
    tk, sl = _t(cmap.ticket.view(np.int32)), _t(cmap.slot)
    return (tk.data_ptr(), sl.data_ptr(), (tk, sl), V)


# ------------------------------------------------------------------------------------------------------ sparse head
@functools.lru_cache(maxsize=None)
def _shead_case(B, V, C, O, kind, form, M=None, valid=None, x_fill=None):
    """The problem and its float64 reference, computed once.  x_fill: "nan" = every row NaN, "row0_inf" = row 0 +Inf."""
    cmap, M, X, W, bias, G = tc.make_shead_problem(B, V, C, O, kind, form, M)
    valid = M if valid is None else valid
    if x_fill == "nan":
        X[:] = np.nan
    elif x_fill == "row0_inf":
        X[0] = np.inf
    with np.errstate(invalid="ignore"):
        ref = tc.ref_sparse_head(X, cmap.row_of_cell, valid, B, V, C, W, bias, G)
        ref_nobias = tc.ref_sparse_head(X, cmap.row_of_cell, valid, B, V, C, W, None, G)[0]
    return cmap, M, valid, X, W, bias, G, ref, ref_nobias


def _shead_run(case, B, V, C, O, kind, use_mdev=False, with_bias=True, want_dx=True, want_dw=True, want_db=True,
               defer=False):
    lib, L = _lib().load(), _lib()
    cmap, M, valid, X, W, bias, G = case[:7]
    dm = _dev_map(cmap, V)
    Xd, Wd, Gd = _t(X, kind), _t(W), _t(G)
    bd = _t(bias) if with_bias else None
    m_dev = torch.tensor([valid], dtype=torch.int64, device=DEV) if use_mdev else None
    assert use_mdev or valid == M
    assert lib.wfs_sparse_head_ok(B, V, C, O, L.dtype_code(Xd)) == 1
    nbytes = int(lib.wfs_sparse_head_workspace_bytes(B, V, C, O))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    Y = _full((B, O), NAN)
    L.check(lib.wfs_sparse_head_fwd(L.ptr(Xd), dm[0], dm[1], M, L.ptr(m_dev), B, V, C, L.ptr(Wd), L.ptr(bd), O, L.ptr(Y),
                                    L.dtype_code(Xd), L.ptr(ws), nbytes, L.stream_ptr()))
    dX = _full((M, C), SENT, TORCH[kind]) if want_dx else None
    dW = _full((O, C * V), NAN) if want_dw else None
    dB = _full((O,), NAN) if (want_dw and want_db) else None
    job = L.DwJob() if defer else None
    L.check(lib.wfs_sparse_head_bwd(L.ptr(Xd), L.ptr(Gd), dm[0], dm[1], M, L.ptr(m_dev), B, V, C, L.ptr(Wd), O, L.ptr(dX),
                                    L.ptr(dW), L.ptr(dB), L.dtype_code(Xd), L.ptr(ws) if want_dw else None,
                                    nbytes if want_dw else 0, ctypes.byref(job) if defer else None, L.stream_ptr()))
    torch.cuda.synchronize()
    return dict(Y=Y, dX=dX, dW=dW, dB=dB, job=job, ws=ws, keep=(dm, Xd, Wd, Gd, bd, m_dev))


def _shead_compare(family, out, case, kind, with_bias=True, finite_y_only=False):
    ref_y, ref_dx, ref_dw, ref_db, touched = case[7]
    if not with_bias:
        ref_y = case[8]
    got_y = out["Y"].cpu().numpy().astype(np.float64)
    if finite_y_only:               # a non-finite row: the same events must be non-finite, NaN or Inf as the order has it
        assert np.array_equal(np.isfinite(got_y), np.isfinite(ref_y))
        got_y, ref_y = np.where(np.isfinite(got_y), got_y, np.nan), np.where(np.isfinite(ref_y), ref_y, np.nan)
    _check(family, "Y", got_y, ref_y)
    if out["dX"] is not None:
        dx = out["dX"].float().cpu().numpy()
        assert (dx[~touched] == SENT).all(), "dX rows beyond the valid count or without a cell must stay untouched"
        if touched.any():
            _check_dx(family, dx[touched], ref_dx[touched], kind)
    if out["dW"] is not None:
        _check(family, "dW", out["dW"], ref_dw)
    if out["dB"] is not None:
        _check(family, "dB", out["dB"], ref_db)


@pytest.mark.parametrize("shape", tc.SHEAD_GRID_A, ids=tc.SHEAD_GRID_A_IDS)
def test_sparse_head_every_output_and_wave_count(shape):
    """O = 1 .. 4 x C = 8 .. 64 (1, 2, 4, 8 waves per block), fp32, two tiles with a 6-cell tail and two slices with a
    1-event tail."""
    O, C, B, V = shape
    case = _shead_case(B, V, C, O, "f32", "ticket")
    _shead_compare("shead_grid_a", _shead_run(case, B, V, C, O, "f32"), case, "f32")


@pytest.mark.parametrize("form", ["ticket", "cell_row"])
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("bv", tc.SHEAD_GRID_B, ids=tc.SHEAD_GRID_B_IDS)
def test_sparse_head_tile_and_slice_edges(bv, kind, form):
    """One cell, V < 64, V = 64 with B = 16 (exactly one tile and one slice), one past both, full tiles over three
    slices, five tiles; with the (ticket, slot) map and with one cell_row array serving as both."""
    B, V = bv
    O, C = tc.SHEAD_B_OC
    case = _shead_case(B, V, C, O, kind, form)
    _shead_compare("shead_grid_b", _shead_run(case, B, V, C, O, kind), case, kind)


def _valid_case(name, kind):
    p = tc.SHEAD_VALID
    B, V, C, O = p["B"], p["V"], p["C"], p["O"]
    n = int(round(0.4 * B * V))
    if name == "all_valid":
        return (B, V, C, O), _shead_case(B, V, C, O, kind, "ticket", n + p["spare"]), False
    if name == "partial":
        return (B, V, C, O), _shead_case(B, V, C, O, kind, "ticket", n + p["spare"], n), True
    if name == "none_valid_nan_rows":
        return (B, V, C, O), _shead_case(B, V, C, O, kind, "ticket", p["spare"], 0, "nan"), True
    assert name == "row0_inf"
    return (B, V, C, O), _shead_case(B, V, C, O, kind, "ticket", n + p["spare"], n, "row0_inf"), True


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("name", tc.SHEAD_VALID_CASES)
def test_sparse_head_valid_count(name, kind):
    """Capacity rows with a device-side valid count: cells that point at rows >= the count are absent; rows >= the count
    and rows no cell references come back bit-identical.  With a count of 0 and NaN in every capacity row the result is
    Y == bias exactly, dW == 0, dB == sum G; with +Inf in row 0 only row 0's own cell of dW is non-finite (a missing
    row's registers hold row 0: the kernels must select the data, not multiply it by 0)."""
    (B, V, C, O), case, use_mdev = _valid_case(name, kind)
    cmap, M, valid, X, W, bias, G = case[:7]
    ref_y, ref_dx, ref_dw, ref_db, touched = case[7]
    if name == "partial":
        assert (cmap.row_of_cell >= valid).any() and not touched[valid:].any()
    if name != "none_valid_nan_rows":
        assert (~touched[:valid]).any(), "the case needs a valid row that no cell references"
    out = _shead_run(case, B, V, C, O, kind, use_mdev=use_mdev)
    if name == "none_valid_nan_rows":
        assert not touched.any()
        assert torch.equal(out["Y"].cpu(), torch.from_numpy(np.tile(bias, (B, 1))))
        assert torch.count_nonzero(out["dW"]).item() == 0 and torch.isfinite(out["dW"]).all()
    if name == "row0_inf":
        cell0 = int(np.flatnonzero(cmap.row_of_cell == 0)[0])
        bad = ~np.isfinite(ref_dw)
        want_bad = np.zeros((O, C, V), bool)
        want_bad[:, :, cell0 % V] = True
        assert np.array_equal(bad, want_bad.reshape(O, C * V))
        assert np.array_equal(~np.isfinite(out["dW"].cpu().numpy()), bad), "non-finite dW outside row 0's own cell"
    _shead_compare("shead_valid", out, case, kind, finite_y_only=(name == "row0_inf"))


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("mode", ["dx_only", "dw_db_only", "dw_without_db", "no_bias"])
def test_sparse_head_modes(mode, kind):
    """dX alone (dW = dB = NULL, no workspace), dW + dB alone, dW without dB, bias = NULL."""
    (B, V, C, O), case, use_mdev = _valid_case("partial", kind)
    kw = dict(dx_only=dict(want_dw=False), dw_db_only=dict(want_dx=False), dw_without_db=dict(want_dx=False, want_db=False),
              no_bias=dict(with_bias=False))[mode]
    out = _shead_run(case, B, V, C, O, kind, use_mdev=use_mdev, **kw)
    assert (out["dX"] is None) == (mode in ("dw_db_only", "dw_without_db")) and (out["dW"] is None) == (mode == "dx_only")
    _shead_compare("shead_modes", out, case, kind, with_bias=(mode != "no_bias"))


@pytest.mark.parametrize("kind", tc.KINDS)
def test_sparse_head_deferred_dw(kind):
    """defer: the call leaves ceil(B / 16) per-slice partials and does NOT write dW; wfs_dw_reduce_jobs finishes it."""
    L = _lib()
    (B, V, C, O), case, use_mdev = _valid_case("partial", kind)
    out = _shead_run(case, B, V, C, O, kind, use_mdev=use_mdev, defer=True)
    job = out["job"]
    assert job.nslabs == -(-B // 16) and job.per == O * C * V and job.dW == out["dW"].data_ptr()
    assert job.part == out["ws"].data_ptr() and job.transpose == 0
    assert torch.isnan(out["dW"]).all(), "dW must not be written before the deferred reduction"
    L.check(L.load().wfs_dw_reduce_jobs(ctypes.byref(job), 1, L.stream_ptr()))
    torch.cuda.synchronize()
    _shead_compare("shead_defer", out, case, kind)


@pytest.mark.parametrize("kind", tc.KINDS)
def test_sparse_head_is_reproducible(kind):
    """Fixed summation orders, no atomics: two calls give bit-identical Y, dX and dW."""
    B, V = 17, 65
    O, C = tc.SHEAD_B_OC
    case = _shead_case(B, V, C, O, kind, "ticket")
    a, b = _shead_run(case, B, V, C, O, kind), _shead_run(case, B, V, C, O, kind)
    for k in ("Y", "dX", "dW", "dB"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_sparse_head_ok_truth_table():
    """wfs_sparse_head_ok at its edges; a refused shape makes the entry points return WFS_EINVAL before any launch."""
    L = _lib()
    lib = L.load()
    for name, B, V, C, O in tc.SHEAD_ACCEPTED:
        assert lib.wfs_sparse_head_ok(B, V, C, O, L.WFS_F32) == 1, name
    X, W, G = _full((8, 128), 1.0), _full((8, 1024), 1.0), _full((4, 8), 1.0)
    cells = torch.zeros((64,), dtype=torch.int32, device=DEV)
    ws = torch.empty((4096,), dtype=torch.uint8, device=DEV)
    for name, B, V, C, O in tc.SHEAD_REJECTED:
        assert lib.wfs_sparse_head_ok(B, V, C, O, L.WFS_F32) == 0, name
        Y, dX, dW = _full((4, 8), SENT), _full((8, 128), SENT), _full((8, 1024), SENT)
        rc = lib.wfs_sparse_head_fwd(L.ptr(X), L.ptr(cells), L.ptr(cells), 8, None, B, V, C, L.ptr(W), None, O, L.ptr(Y),
                                     L.WFS_F32, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert rc == L.WFS_EINVAL and "wfs_sparse_head_ok" in L.last_error(), name
        rc = lib.wfs_sparse_head_bwd(L.ptr(X), L.ptr(G), L.ptr(cells), L.ptr(cells), 8, None, B, V, C, L.ptr(W), O,
                                     L.ptr(dX), L.ptr(dW), None, L.WFS_F32, L.ptr(ws), ws.numel(), None, L.stream_ptr())
        assert rc == L.WFS_EINVAL, name
        torch.cuda.synchronize()
        for t in (Y, dX, dW):
            assert (t == SENT).all(), name
    assert lib.wfs_sparse_head_ok(2, 8, 32, 3, 3) == 0          # no such dtype
    with pytest.raises(RuntimeError):
        L.check(L.WFS_EINVAL)


def test_sparse_head_function_dispatch():
    """SparseHeadFunction: features without requires_grad take the dW-only call, a frozen weight the dX-only call with
    db = g.sum(0)."""
    Fsp = _fsp()
    (B, V, C, O), case, _m = _valid_case("all_valid", "f32")
    cmap, M, valid, X, W, bias, G = case[:7]
    ref_y, ref_dx, ref_dw, ref_db, touched = case[7]
    dm = _dev_map(cmap, V)
    for frozen in ("features", "weight"):
        f = _t(X).requires_grad_(frozen != "features")
        w = _t(W).requires_grad_(frozen != "weight")
        b = _t(bias).requires_grad_(True)
        y = Fsp.SparseHeadFunction.apply(f, w, b, dm, B, None)
        y.backward(_t(G))
        torch.cuda.synchronize()
        _check("shead_autograd", "Y", y, ref_y)
        _check("shead_autograd", "dB", b.grad, ref_db)
        if frozen == "features":
            assert f.grad is None
            _check("shead_autograd", "dW", w.grad, ref_dw)
        else:
            assert w.grad is None
            _check_dx("shead_autograd", f.grad.cpu().numpy()[touched], ref_dx[touched], "f32")


# --------------------------------------------------------------------------------------------------- streaming head
@functools.lru_cache(maxsize=None)
def _head_case(B, I, O, kind):
    X, W, bias, G = tc.make_linear_values(np.random.default_rng(131 * I + 7 * B + O), B, I, O, kind)
    return X, W, bias, G, tc.ref_linear(X, W, bias, G), tc.ref_linear(X, W, None, G)[0]


def _head_run(B, I, O, kind, with_bias=True, want_dx=True, want_dw=True, want_db=True, defer=False):
    L = _lib()
    lib = L.load()
    X, W, bias, G = _head_case(B, I, O, kind)[:4]
    Xd, Wd, Gd = _t(X, kind), _t(W), _t(G)
    bd = _t(bias) if with_bias else None
    Y = _full((B, O), NAN)
    L.check(lib.wfs_head_fwd(L.ptr(Xd), B, I, L.ptr(Wd), L.ptr(bd), O, L.ptr(Y), L.dtype_code(Xd), L.stream_ptr()))
    dX = _full((B, I), NAN, TORCH[kind]) if want_dx else None
    dW = _full((O, I), NAN) if want_dw else None
    dB = _full((O,), NAN) if (want_dw and want_db) else None
    nbytes = int(lib.wfs_head_workspace_bytes(B, I, O))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=DEV) if want_dw else None
    job = L.DwJob() if defer else None
    L.check(lib.wfs_head_bwd(L.ptr(Xd), L.ptr(Gd), B, I, L.ptr(Wd), O, L.ptr(dX), L.ptr(dW), L.ptr(dB), L.dtype_code(Xd),
                             L.ptr(ws), nbytes if want_dw else 0, ctypes.byref(job) if defer else None, L.stream_ptr()))
    torch.cuda.synchronize()
    return dict(Y=Y, dX=dX, dW=dW, dB=dB, job=job, ws=ws)


def _head_compare(family, out, B, I, O, kind, with_bias=True):
    case = _head_case(B, I, O, kind)
    ref_y, ref_dx, ref_dw, ref_db = case[4]
    _check(family, "Y", out["Y"], ref_y if with_bias else case[5])
    if out["dX"] is not None:
        _check_dx(family, out["dX"].float().cpu().numpy(), ref_dx, kind)
    if out["dW"] is not None:
        _check(family, "dW", out["dW"], ref_dw)
    if out["dB"] is not None:
        _check(family, "dB", out["dB"], ref_db)


@pytest.mark.parametrize("I", tc.HEAD_I_F32)
def test_streaming_head_row_lengths(I):
    """Scalar kernels (I < 1024 or I % 8 != 0, the bias column of k_head_dw_any at I % 16 = 15 and 0 among them), the
    256-thread kernel from I = 1024, the 1024-thread kernel from I = 8192, and both switch points."""
    B, O = tc.HEAD_DEFAULT["B"], tc.HEAD_DEFAULT["O"]
    _head_compare("head_rows", _head_run(B, I, O, "f32"), B, I, O, "f32")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("I", tc.HEAD_I_16BIT)
def test_streaming_head_row_lengths_16bit(I, kind):
    B, O = tc.HEAD_DEFAULT["B"], tc.HEAD_DEFAULT["O"]
    _head_compare("head_rows_16", _head_run(B, I, O, kind), B, I, O, kind)


@pytest.mark.parametrize("I", tc.HEAD_O_I)
@pytest.mark.parametrize("O", tc.HEAD_O)
def test_streaming_head_output_counts(O, I):
    B = tc.HEAD_DEFAULT["B"]
    _head_compare("head_outputs", _head_run(B, I, O, "f32"), B, I, O, "f32")


@pytest.mark.parametrize("defer", [False, True], ids=["direct", "defer"])
@pytest.mark.parametrize("B", tc.HEAD_B)
def test_streaming_head_chunk_edges(B, defer):
    """B around the chunk-count switches of head_chunks (ceil(B / 32) clamped to 16), fused dX + dW launch at I = 1024,
    the first length of the vector route: with defer it leaves exactly head_chunks(B) partials."""
    L = _lib()
    I, O = 1024, tc.HEAD_DEFAULT["O"]
    assert int(L.load().wfs_head_workspace_bytes(B, I, O)) == tc.head_chunks(B) * O * I * 4
    out = _head_run(B, I, O, "f32", defer=defer)
    if defer:
        assert out["job"].nslabs == tc.head_chunks(B) and torch.isnan(out["dW"]).all()
        L.check(L.load().wfs_dw_reduce_jobs(ctypes.byref(out["job"]), 1, L.stream_ptr()))
        torch.cuda.synchronize()
    _head_compare("head_chunks", out, B, I, O, "f32")


@pytest.mark.parametrize("I", tc.HEAD_MODE_I)
@pytest.mark.parametrize("mode", ["dx_only", "dw_db_only", "both", "no_bias", "defer"])
def test_streaming_head_modes(mode, I):
    """dX alone (k_head_dx / k_head_dx_any, no workspace), dW + dB alone (vector route: dB comes from k_head_dw_reduce),
    both, bias = NULL, and defer: the fused vector route leaves head_chunks(B) partials and an unwritten dW for
    wfs_dw_reduce_jobs (dB is final), the scalar route returns nslabs == 0 with dW written."""
    L = _lib()
    B, O = tc.HEAD_DEFAULT["B"], tc.HEAD_DEFAULT["O"]
    kw = dict(dx_only=dict(want_dw=False), dw_db_only=dict(want_dx=False), both={}, no_bias=dict(with_bias=False),
              defer=dict(defer=True))[mode]
    out = _head_run(B, I, O, "f32", **kw)
    if mode == "defer":
        job = out["job"]
        if tc.head_is_scalar(I):
            assert job.nslabs == 0
        else:
            assert job.nslabs == tc.head_chunks(B) and job.per == O * I and job.dW == out["dW"].data_ptr()
            assert torch.isnan(out["dW"]).all(), "dW must not be written before the deferred reduction"
            _check("head_modes", "dB", out["dB"], _head_case(B, I, O, "f32")[4][3])
            L.check(L.load().wfs_dw_reduce_jobs(ctypes.byref(job), 1, L.stream_ptr()))
            torch.cuda.synchronize()
    _head_compare("head_modes", out, B, I, O, "f32", with_bias=(mode != "no_bias"))


def test_streaming_head_empty_batch():
    """B == 0: the forward returns OK without a launch, the backward zero-fills dW."""
    L = _lib()
    lib = L.load()
    I, O = 1024, 3
    W, Y, dW = _full((O, I), 1.0), _full((1, O), SENT), _full((O, I), NAN)
    L.check(lib.wfs_head_fwd(None, 0, I, L.ptr(W), None, O, L.ptr(Y), L.WFS_F32, L.stream_ptr()))
    L.check(lib.wfs_head_bwd(None, None, 0, I, L.ptr(W), O, None, L.ptr(dW), None, L.WFS_F32, None, 0, None, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (Y == SENT).all() and torch.count_nonzero(dW).item() == 0 and torch.isfinite(dW).all()


@pytest.mark.parametrize("I", tc.HEAD_MODE_I)
@pytest.mark.parametrize("frozen", ["input", "weight"])
def test_skinny_linear_function_dispatch(frozen, I):
    """SkinnyLinearFunction: an input without requires_grad takes the dW-only route (dB from the reduce kernel on the
    vector route), a frozen weight the dX-only route with db = g.sum(0)."""
    Fsp = _fsp()
    B, O = tc.HEAD_DEFAULT["B"], tc.HEAD_DEFAULT["O"]
    X, W, bias, G, (ref_y, ref_dx, ref_dw, ref_db), _ = _head_case(B, I, O, "f32")
    lin = torch.nn.Linear(I, O).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(_t(W))
        lin.bias.copy_(_t(bias))
    lin.weight.requires_grad_(frozen != "weight")
    x = _t(X).requires_grad_(frozen != "input")
    assert Fsp.can_use_skinny_linear(lin, x)
    y = Fsp.skinny_linear(x, lin)
    y.backward(_t(G))
    torch.cuda.synchronize()
    _check("head_autograd", "Y", y, ref_y)
    _check("head_autograd", "dB", lin.bias.grad, ref_db)
    if frozen == "input":
        assert x.grad is None
        _check("head_autograd", "dW", lin.weight.grad, ref_dw)
    else:
        assert lin.weight.grad is None
        _check_dx("head_autograd", x.grad.cpu().numpy(), ref_dx, "f32")


def test_can_use_skinny_linear_agrees_with_the_kernels():
    """I = 4104 (> 4096, a multiple of 8): accepted, and the vector route computes it; I = 4097 and O = 9: refused (the
    library refuses O = 9 too)."""
    Fsp, L = _fsp(), _lib()
    B, O = 5, 3
    X, W, bias, G, (ref_y, ref_dx, ref_dw, ref_db), _ = _head_case(B, 4104, O, "f32")
    lin = torch.nn.Linear(4104, O).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(_t(W))
        lin.bias.copy_(_t(bias))
    x = _t(X).requires_grad_(True)
    assert Fsp.can_use_skinny_linear(lin, x)
    y = Fsp.skinny_linear(x, lin)
    y.backward(_t(G))
    _check("head_autograd", "Y", y, ref_y)
    _check_dx("head_autograd", x.grad.cpu().numpy(), ref_dx, "f32")
    _check("head_autograd", "dW", lin.weight.grad, ref_dw)
    _check("head_autograd", "dB", lin.bias.grad, ref_db)
    assert not Fsp.can_use_skinny_linear(torch.nn.Linear(4097, O).to(DEV), _full((B, 4097), 1.0))
    assert not Fsp.can_use_skinny_linear(torch.nn.Linear(1024, 9).to(DEV), _full((B, 1024), 1.0))
    Y = _full((B, 9), SENT)
    rc = L.load().wfs_head_fwd(L.ptr(_full((B, 1024), 1.0)), B, 1024, L.ptr(_full((9, 1024), 1.0)), None, 9, L.ptr(Y),
                               L.WFS_F32, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.WFS_EINVAL and (Y == SENT).all()


# ----------------------------------------------------------------------------------------------------- mapped dense
@pytest.mark.parametrize("form", ["ticket", "cell_row"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("cv", tc.DENSE_CASES, ids=tc.DENSE_IDS)
def test_mapped_dense_is_bit_exact(cv, kind, form):
    """wfs_to_dense_mapped / _bwd_mapped at C = 4 and 128, V = 2 (one word of 16-bit cells), 64 and 66: pure data
    movement, bit for bit; every cell of Y written (it starts as NaN); rows of dX without a live cell untouched; with all
    rows valid, with a device-side count, and with a count of 0 over NaN rows."""
    L = _lib()
    lib = L.load()
    C, V = cv
    B = tc.DENSE_B
    rng = np.random.default_rng(1000 * C + V)
    M = max(4, int(round(0.5 * B * V))) + 5
    cmap = tc.make_cell_map(rng, B, V, M, 0.5, form)
    dm = _dev_map(cmap, V)
    X = _t(rng.standard_normal((M, C)).astype(np.float32), kind)
    dY = _t(rng.standard_normal((B, C, V)).astype(np.float32), kind)
    for valid, use_mdev, nan_rows in ((M, False, False), (M // 2, True, False), (0, True, True)):
        Xv = torch.full_like(X, NAN) if nan_rows else X
        m_dev = torch.tensor([valid], dtype=torch.int64, device=DEV) if use_mdev else None
        Y = _full((B, C, V), NAN, TORCH[kind])
        dX = _full((M, C), SENT, TORCH[kind])
        L.check(lib.wfs_to_dense_mapped(L.ptr(Xv), dm[0], dm[1], M, L.ptr(m_dev), B, V, C, L.ptr(Y), L.dtype_code(Xv),
                                        L.stream_ptr()))
        L.check(lib.wfs_to_dense_bwd_mapped(L.ptr(dY), dm[0], dm[1], M, L.ptr(m_dev), B, V, C, L.ptr(dX),
                                            L.dtype_code(dY), L.stream_ptr()))
        torch.cuda.synchronize()
        bits = lambda t: t.view(BITS[kind]).cpu().numpy()
        want_y = tc.ref_dense_mapped(bits(Xv), cmap.row_of_cell, valid, B, V, C)
        want_dx = tc.ref_dense_mapped_bwd(bits(dY), cmap.row_of_cell, valid, B, V, C, bits(_full((M, C), SENT, TORCH[kind])))
        assert np.array_equal(bits(Y), want_y), "Y, valid = %d" % valid
        assert np.array_equal(bits(dX), want_dx), "dX, valid = %d" % valid
        if valid == 0:
            assert not bits(Y).any()


# ---------------------------------------------------------------------------------------------------- cross-entropy
XBAR = 1e-6


@pytest.mark.parametrize("scale", tc.XENT_SCALES, ids=["scale4", "scale60"])
@pytest.mark.parametrize("shape", tc.XENT_SHAPES, ids=tc.XENT_IDS)
def test_cross_entropy_shapes_and_large_logits(shape, scale):
    """B = 1, 1024, 1025 and 2049 around the single block's 1024-row stride, C = 1 and the C = 4096 cap, logits whose
    unshifted exp overflows fp32, ignored rows, an upstream gradient of 2.5."""
    Fsp = _fsp()
    B, C = shape
    z, t = tc.make_xent_values(np.random.default_rng(5), B, C, scale)
    loss, dz = tc.ref_xent_mean(z, t, -100)
    zg, tg = _t(z).requires_grad_(True), _t(t)
    assert Fsp.can_fuse_cross_entropy(torch.nn.CrossEntropyLoss(), zg, tg)
    lg = Fsp.cross_entropy_mean(zg, tg, -100)
    (2.5 * lg).backward()
    torch.cuda.synchronize()
    _check("xent", "loss", np.array([lg.item()]), np.array([loss]), XBAR, 0.0)
    _check("xent", "dlogits", zg.grad, 2.5 * dz, XBAR, XBAR)


def test_cross_entropy_every_row_ignored():
    """No counted row: the loss is NaN, as torch gives, and dlogits is all zero."""
    Fsp = _fsp()
    z, _t0 = tc.make_xent_values(np.random.default_rng(5), 1030, 3, 4.0)
    zg = _t(z).requires_grad_(True)
    lg = Fsp.cross_entropy_mean(zg, _full((1030,), -100, torch.int64), -100)
    lg.backward()
    torch.cuda.synchronize()
    assert torch.isnan(lg) and torch.count_nonzero(zg.grad).item() == 0 and torch.isfinite(zg.grad).all()


def test_cross_entropy_without_a_gradient_buffer():
    """dlogits == NULL: under no_grad, for logits without requires_grad, and through the C entry itself."""
    Fsp, L = _fsp(), _lib()
    B, C = 1025, 3
    z, t = tc.make_xent_values(np.random.default_rng(5), B, C, 60.0)
    loss, _dz = tc.ref_xent_mean(z, t, -100)
    zg, tg = _t(z), _t(t)
    with torch.no_grad():
        a = Fsp.cross_entropy_mean(_t(z).requires_grad_(True), tg, -100)
    b = Fsp.cross_entropy_mean(zg, tg, -100)
    assert not a.requires_grad and not b.requires_grad
    out = _full((1,), NAN)
    L.check(L.load().wfs_xent_mean_fwd_bwd(L.ptr(zg), L.ptr(tg), B, C, -100, L.ptr(out), None, L.stream_ptr()))
    torch.cuda.synchronize()
    for got in (a.item(), b.item(), out.item()):
        _check("xent", "loss", np.array([got]), np.array([loss]), XBAR, 0.0)
    assert a.item() == b.item() == out.item()
    assert not Fsp.can_fuse_cross_entropy(torch.nn.CrossEntropyLoss(), _full((2, 4097), 0.0), tg[:2])
    rc = L.load().wfs_xent_mean_fwd_bwd(L.ptr(_full((2, 4097), 0.0)), L.ptr(tg), 2, 4097, -100, L.ptr(out), None,
                                        L.stream_ptr())
    assert rc == L.WFS_EINVAL


def test_cross_entropy_unit_loss_grad_returns_the_buffer_itself():
    """A backward seeded with unit_loss_grad() hands on the kernel's dlogits unscaled and uncopied; any other seed
    multiplies into a new tensor."""
    Fsp = _fsp()
    B, C = 1025, 2
    z, t = tc.make_xent_values(np.random.default_rng(5), B, C, 4.0)
    _loss, dz = tc.ref_xent_mean(z, t, -100)
    for unit in (True, False):
        leaf = _t(z).requires_grad_(True)
        zg = leaf * 1.0
        seen = []
        zg.register_hook(seen.append)
        lg = Fsp.cross_entropy_mean(zg, _t(t), -100)
        buf = lg.grad_fn.dlogits
        seed = Fsp.unit_loss_grad(DEV) if unit else torch.ones((), device=DEV)
        torch.autograd.backward(lg, grad_tensors=seed)
        torch.cuda.synchronize()
        assert len(seen) == 1 and (seen[0].data_ptr() == buf.data_ptr()) == unit
        _check("xent", "dlogits", leaf.grad, dz, XBAR, XBAR)
