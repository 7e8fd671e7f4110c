"""Pins the float64 references of tests/tail_cases.py (no GPU): the loop-written sparse head against the linear reference
on the densified rows, the linear and cross-entropy references against torch in float64 on the CPU, the cell-map
generator's promises, and the value ranges the 16-bit bars of tests/test_gpu_tail_edges.py rely on."""
import numpy as np
import pytest
import torch

import tail_cases as tc

GRID = ([(B, V, C, O) for (O, C, B, V) in tc.SHEAD_GRID_A] +
        [(B, V, tc.SHEAD_B_OC[1], tc.SHEAD_B_OC[0]) for (B, V) in tc.SHEAD_GRID_B])
GRID_IDS = ["A_" + i for i in tc.SHEAD_GRID_A_IDS] + ["B_" + i for i in tc.SHEAD_GRID_B_IDS]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max(initial=0.0) <= tol * max(1.0, np.abs(b).max(initial=0.0))


@pytest.mark.parametrize("shape", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("partial", [False, True], ids=["all_rows", "valid_count"])
def test_sparse_head_reference_equals_linear_on_the_dense_tensor(shape, partial):
    """ref_sparse_head (loops over the map) == ref_linear(ref_dense_mapped(...).reshape(B, C V)) in both directions;
    dX is the gather of the dense gradient.  With a valid count, rows beyond it count as absent in both."""
    B, V, C, O = shape
    cmap, M, X, W, bias, G = tc.make_shead_problem(B, V, C, O, "f32")
    valid = M // 2 if partial else M
    Y, dX, dW, dB, touched = tc.ref_sparse_head(X, cmap.row_of_cell, valid, B, V, C, W, bias, G)
    dense = tc.ref_dense_mapped(X.astype(np.float64), cmap.row_of_cell, valid, B, V, C)
    y2, ddense, dW2, dB2 = tc.ref_linear(dense.reshape(B, C * V), W, bias, G)
    _close(Y, y2)
    _close(dW, dW2)
    _close(dB, dB2)
    gathered = tc.ref_dense_mapped_bwd(ddense, cmap.row_of_cell, valid, B, V, C, np.full((M, C), np.nan))
    assert np.array_equal(~np.isnan(gathered).any(axis=1), touched)
    _close(dX[touched], gathered[touched])
    assert not dX[~touched].any()
    live = tc.live_rows(cmap.row_of_cell, valid)
    assert touched.sum() == (live >= 0).sum()
    if partial and B * V > 8:
        assert (cmap.row_of_cell >= valid).any(), "the case must point some cells at rows beyond the valid count"


@pytest.mark.parametrize("shape", [(37, 269, 3), (5, 1024, 8), (1, 1, 1)], ids=lambda s: "B%d_I%d_O%d" % s)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
def test_linear_reference_equals_torch_float64(shape, with_bias):
    B, I, O = shape
    X, W, bias, G = tc.make_linear_values(np.random.default_rng(3), B, I, O, "f32")
    y, dx, dW, db = tc.ref_linear(X, W, bias if with_bias else None, G)
    xt = torch.from_numpy(X).double().requires_grad_(True)
    wt = torch.from_numpy(W).double().requires_grad_(True)
    bt = torch.from_numpy(bias).double().requires_grad_(True) if with_bias else None
    yt = torch.nn.functional.linear(xt, wt, bt)
    yt.backward(torch.from_numpy(G).double())
    _close(y, yt.detach().numpy())
    _close(dx, xt.grad.numpy())
    _close(dW, wt.grad.numpy())
    _close(db, bt.grad.numpy() if with_bias else G.astype(np.float64).sum(0))


@pytest.mark.parametrize("shape", tc.XENT_SHAPES, ids=tc.XENT_IDS)
@pytest.mark.parametrize("scale", tc.XENT_SCALES, ids=["scale4", "scale60"])
def test_cross_entropy_reference_equals_torch_float64(shape, scale):
    B, C = shape
    z, t = tc.make_xent_values(np.random.default_rng(5), B, C, scale)
    if B > 11:
        assert (t == -100).any()
    if B > 1 and C == 3:
        assert any(list(r) == [88.0, -88.0, 0.0] for r in z)
    loss, dz = tc.ref_xent_mean(z, t, -100)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    lt = torch.nn.functional.cross_entropy(zt, torch.from_numpy(t), ignore_index=-100)
    lt.backward()
    assert abs(loss - lt.item()) <= 1e-12 * max(1.0, abs(lt.item()))
    _close(dz, zt.grad.numpy())


def test_cross_entropy_reference_with_every_row_ignored():
    z, _t = tc.make_xent_values(np.random.default_rng(5), 9, 3, 4.0)
    loss, dz = tc.ref_xent_mean(z, np.full(9, -100), -100)
    assert np.isnan(loss) and not dz.any()
    lt = torch.nn.functional.cross_entropy(torch.from_numpy(z).double(), torch.full((9,), -100), ignore_index=-100)
    assert torch.isnan(lt)


@pytest.mark.parametrize("shape", GRID + [(tc.DENSE_B, V, C, 1) for (C, V) in tc.DENSE_CASES],
                         ids=GRID_IDS + ["D_" + i for i in tc.DENSE_IDS])
@pytest.mark.parametrize("form", ["ticket", "cell_row"])
def test_cell_map_invariants(shape, form):
    B, V, C, O = shape
    cmap, M, _X, _W, _b, _G = tc.make_shead_problem(B, V, C, O, "f32", form)
    r = cmap.row_of_cell
    assert r.shape == (B * V,) and r.min() >= -1 and r.max() < M
    act = r[r >= 0]
    assert len(np.unique(act)) == len(act), "injective"
    assert 0 in act, "row 0 is referenced"
    for cell in (0, V - 1, (B - 1) * V, B * V - 1):
        assert r[cell] >= 0, "corner cell %d" % cell
    per_event = (r.reshape(B, V) >= 0).sum(axis=1)
    if B >= 3:
        assert (per_event == 0).any(), "an event without rows"
    assert np.array_equal(tc.decode_cell_map(cmap.ticket, cmap.slot), r), "device form decodes to row_of_cell"
    assert cmap.ticket.dtype == np.uint32 and cmap.slot.dtype == np.int32
    if form == "cell_row":
        assert np.shares_memory(cmap.ticket, cmap.slot)
    else:
        empty = r < 0
        assert (cmap.ticket[empty] == tc.EMPTY).all() and (cmap.ticket[~empty] != tc.EMPTY).all()
        assert ((cmap.slot[empty] >= 0) & (cmap.slot[empty] < M)).all(), "empty cells carry an in-range row id"
    if V % 64 != 0 and B * V > 1:
        tail = r.reshape(B, V)[:, (V // 64) * 64:]
        assert (tail >= 0).any() and (tail < 0).any(), "tail tile: an active and an empty cell"
    other = tc.make_shead_problem(B, V, C, O, "f32", "cell_row" if form == "ticket" else "ticket")[0]
    assert other.row_of_cell.shape == r.shape


def test_rounding_helper_matches_torch():
    x = np.random.default_rng(1).standard_normal(4099).astype(np.float32) * 3
    x[:3] = (1.00390625, 1.01171875, -0.0)               # ties of bf16's 8-bit significand (to even: down, up)
    for kind, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
        assert np.array_equal(tc.round_to(x, kind), torch.from_numpy(x).to(dt).float().numpy())


@pytest.mark.parametrize("shape", GRID, ids=GRID_IDS)
def test_fp16_sparse_head_gradients_stay_normal(shape):
    B, V, C, O = shape
    cmap, M, X, W, bias, G = tc.make_shead_problem(B, V, C, O, "f16")
    _Y, dX, _dW, _dB, touched = tc.ref_sparse_head(X, cmap.row_of_cell, M, B, V, C, W, bias, G)
    a = np.abs(dX[touched])
    assert a.min() >= tc.F16_MIN_NORMAL and a.max() <= tc.F16_MAX


@pytest.mark.parametrize("I", tc.HEAD_I_16BIT + tc.HEAD_MODE_I)
def test_fp16_streaming_head_gradients_stay_normal(I):
    X, W, bias, G = tc.make_linear_values(np.random.default_rng(I), tc.HEAD_DEFAULT["B"], I, tc.HEAD_DEFAULT["O"], "f16")
    a = np.abs(tc.ref_linear(X, W, bias, G)[1])
    assert a.min() >= tc.F16_MIN_NORMAL and a.max() <= tc.F16_MAX


def test_error_ratio_helper():
    w = np.array([1.0, -2.0, 0.0, np.inf, np.nan])
    assert tc.err_ratio(w, w, 1e-5) == 0.0
    assert tc.err_ratio(w + np.array([0, 0, 2e-5, 0, 0]), w, 1e-5) == pytest.approx(1.0)
    assert tc.err_ratio(w + np.array([0, 1e-4, 0, 0, 0]), w, 1e-5) > 1.0
    assert tc.err_ratio(np.array([1.0, -2.0, 0.0, -np.inf, np.nan]), w, 1e-5) == float("inf")
    assert tc.err_ratio(np.array([1.0, -2.0, np.nan, np.inf, np.nan]), w, 1e-5) == float("inf")
    assert tc.err_ratio(np.zeros(3), np.zeros(3), 1e-5) == 0.0
    assert tc.err_ratio(np.array([0.0, 1e-30, 0.0]), np.zeros(3), 1e-5) == float("inf")
