"""SparseMaxPool2d / 3d on the GPU (csrc/pool.hip) against the restatement of spconv's pool arithmetic over the oracle's
rulebook (test_pool_host.py): output rows and their order bit for bit, values and gradients EXACTLY (a maximum rounds
nothing; gradients of small integers sum exactly in every dtype), through the Python surface and through the C ABI;
device-count mode, output capacities below the output count, the packed by-input table, and the captured training and
evaluation steps of config/psd_c2_pool.json."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from helpers import rand_coords
from test_pool_host import POOL_CASES, dense_max_pool, pool_backward, pool_forward, pool_rulebook

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# ndim, shape, ksize, stride, padding, dilation, subm
GEOMETRIES = [c + (False,) for c in POOL_CASES] + [(2, (9, 9), 3, 1, 2, 2, False), (3, (6, 7, 12), 3, 1, 0, 1, True)]
GEO_IDS = ["k3_s114", "k112_s112", "2d_k3_s2_p1", "2d_k2_s2", "2d_dilation2", "subm_k3"]
PSD_GEO = (3, (14, 11, 64), 3, (1, 1, 4), 0, 1, False)


def _events(rng, sizes, shape):
    """Index rows grouped by event, ``sizes[b]`` distinct sites in event b (0: an empty event)."""
    rows = []
    for b, n in enumerate(sizes):
        r = rand_coords(rng, 1, shape, n)
        r[:, 0] = b
        rows.append(r)
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, len(shape) + 1), np.int32)


def _features(rng, n, C, dtype, positive):
    """Values that every dtype holds exactly (multiples of 1/8 below 32); positive ones distinct per channel."""
    if positive and n <= 240:
        v = np.stack([rng.permutation(n) + 1 for _ in range(C)], 1).astype(np.float32) / 8.0
    else:
        v = rng.integers(1 if positive else -60, 61, size=(n, C)).astype(np.float32) / 8.0
    return torch.from_numpy(v).to(dtype)


def _module(geo):
    import waveformml_amd.spconv as sp
    ndim, _shape, k, s, p, d, subm = geo
    return sp.SparseMaxPool(ndim, k, s, p, d, subm)


def _run(geo, idx, X, dY, B):
    """The module on the GPU: (out_indices, Y, dX) as CPU tensors."""
    import waveformml_amd.spconv as sp
    xg = X.to(DEV).requires_grad_(True)
    out = _module(geo)(sp.SparseConvTensor(xg, torch.from_numpy(idx).to(DEV), list(geo[1]), B))
    assert out.features.dtype == X.dtype
    if dY is not None and out.features.shape[0]:
        out.features.backward(dY.to(DEV))
    dX = xg.grad.cpu() if xg.grad is not None else torch.zeros_like(X)
    return out, out.features.detach().cpu(), dX


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("positive", [True, False], ids=["positive", "signed"])
@pytest.mark.parametrize("C", [2, 32, 48, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
def test_pool_matches_the_restatement_exactly(geo, dtype, C, positive):
    """Batches with empty events (first, interior, last).  Output rows = the oracle's, in its order; values and
    gradients (dY small integers: every sum exact) bit-equal to the restatement on the same rounded inputs.  Signed
    features pin the zero start; positive ones are additionally the dense max pool's."""
    from oracle import ref
    ndim, shape, k, s, p, d, subm = geo
    rng = np.random.default_rng(7 + C)
    vol = int(np.prod(shape))
    sizes = [0, max(1, vol // 9), 0, max(1, vol // 5), max(1, vol // 20), 0]
    B = len(sizes)
    idx = _events(rng, sizes, shape)
    X = _features(rng, idx.shape[0], C, dtype, positive)
    out_idx, pairs, num = pool_rulebook(idx, B, shape, k, s, p, d, subm)
    M = out_idx.shape[0]
    dY = torch.from_numpy(rng.integers(-2, 3, size=(M, C)).astype(np.float32)).to(dtype)
    want_y = pool_forward(X, pairs, num, M)
    want_dx = pool_backward(X, want_y, dY, pairs, num).to(dtype)
    out, Y, dX = _run(geo, idx, X, dY, B)
    assert np.array_equal(out.indices.cpu().numpy(), out_idx)
    pool = _module(geo)
    assert out.spatial_shape == (list(shape) if subm else [int(v) for v in ref.conv_output_shape(
        list(shape), pool.kernel_size, pool.stride, pool.padding, pool.dilation)])
    assert out.indice_dict == {} and out.batch_size == B
    assert torch.equal(_bits(Y), _bits(want_y))
    assert torch.equal(dX, want_dx), float((dX.float() - want_dx.float()).abs().max())
    if positive and not subm and C <= 32:
        dense_y, _cells, dense_dx = dense_max_pool(idx, X, B, shape, out_idx, dY, k, s, p, d)
        assert torch.equal(Y.float(), dense_y)
        if idx.shape[0] <= 240:                 # distinct values: no ties for the dense pool to break its own way
            assert torch.equal(dX.float(), dense_dx)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_empty_input(dtype):
    import waveformml_amd.spconv as sp
    x = sp.SparseConvTensor(torch.zeros((0, 32), dtype=dtype, device=DEV, requires_grad=True),
                            torch.zeros((0, 4), dtype=torch.int32, device=DEV), [14, 11, 64], 2)
    out = sp.SparseMaxPool3d(3, [1, 1, 4])(x)
    assert tuple(out.features.shape) == (0, 32) and tuple(out.indices.shape) == (0, 4) and out.spatial_shape == [12, 9, 16]
    out.features.sum().backward()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_ties_all_receive_the_gradient(dtype):
    """A row's values copied into a neighbour of the same window (and raised above everything else): both rows receive
    the window's gradient."""
    geo = PSD_GEO
    ndim, shape, k, s, p, d, subm = geo
    rng = np.random.default_rng(21)
    B, C = 2, 32
    idx = _events(rng, [400, 300], shape)
    X = _features(rng, idx.shape[0], C, dtype, True)
    out_idx, pairs, num = pool_rulebook(idx, B, shape, k, s, p, d)
    by_out = np.full((pairs.shape[1], out_idx.shape[0]), -1, np.int64)
    for kk in range(pairs.shape[1]):
        by_out[kk, pairs[1, kk, :num[kk]]] = pairs[0, kk, :num[kk]]
    o = int(np.argmax((by_out >= 0).sum(0)))
    a, b = [int(v) for v in by_out[:, o][by_out[:, o] >= 0][:2]]
    X[a] = X[a] + 16.0                        # still exact in every dtype (< 64, multiples of 1/8)
    X[b] = X[a]
    dY = torch.ones((out_idx.shape[0], C), dtype=dtype)
    want_y = pool_forward(X, pairs, num, out_idx.shape[0])
    want_dx = pool_backward(X, want_y, dY, pairs, num).to(dtype)
    _out, Y, dX = _run(geo, idx, X, dY, B)
    assert torch.equal(_bits(Y), _bits(want_y)) and torch.equal(dX, want_dx)
    assert torch.equal(Y[o], X[a]) and bool((dX[a] >= 1).all()) and bool((dX[b] >= 1).all())


def test_real_gradients_against_float64():
    """fp32 rows, random real dY: dX against the float64 sums.  A sum of at most K terms accumulated in fp32 in any
    order is within K * 2^-24 * sum|terms| of the exact one (each of the < K additions and the final value round by at
    most 2^-24 of a partial sum that never exceeds sum|terms|) -- derived, not tuned."""
    geo = PSD_GEO
    ndim, shape, k, s, p, d, subm = geo
    rng = np.random.default_rng(22)
    B, C = 3, 32
    idx = _events(rng, [500, 0, 700], shape)
    X = torch.from_numpy(rng.integers(1, 9, size=(idx.shape[0], C)).astype(np.float32))          # many ties
    out_idx, pairs, num = pool_rulebook(idx, B, shape, k, s, p, d)
    M, K = out_idx.shape[0], pairs.shape[1]
    dY = torch.from_numpy(rng.standard_normal((M, C)).astype(np.float32))
    Yr = pool_forward(X, pairs, num, M)
    want = pool_backward(X, Yr, dY, pairs, num, torch.float64)
    mag = pool_backward(X, Yr, dY.abs(), pairs, num, torch.float64)
    _out, Y, dX = _run(geo, idx, X, dY, B)
    assert torch.equal(Y, Yr)
    err = (dX.double() - want).abs()
    bound = K * 2.0 ** -24 * mag
    print("max err %.3e, max bound %.3e" % (float(err.max()), float(bound.max())))
    assert bool((err <= bound).all()), float((err - bound).max())


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _tables(pairs, num, N, M):
    K = pairs.shape[1]
    by_in, by_out = np.full((K, N), -1, np.int32), np.full((K, M), -1, np.int32)
    for k in range(K):
        by_in[k, pairs[0, k, :num[k]]] = pairs[1, k, :num[k]]
        by_out[k, pairs[1, k, :num[k]]] = pairs[0, k, :num[k]]
    return by_in, by_out


@pytest.mark.parametrize("C", [2, 32, 48, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_c_abi_with_device_counts_leaves_the_spare_rows_alone(dtype, C):
    """wfs_maxpool_fwd / _bwd on the ORACLE's tables, with capacities above the valid counts: the valid rows equal the
    restatement bit for bit; rows past the count are neither read (their table entries are junk) nor written (they
    keep what they held), as wfs_gather_conv's; nothing is written around the buffers."""
    from waveformml_amd import _lib
    lib = _lib.load()
    ndim, shape, k, s, p, d, subm = PSD_GEO
    rng = np.random.default_rng(31 + C)
    B = 4
    idx = _events(rng, [300, 0, 450, 200], shape)
    N = idx.shape[0]
    X = _features(rng, N, C, dtype, False)
    out_idx, pairs, num = pool_rulebook(idx, B, shape, k, s, p, d)
    M, K = out_idx.shape[0], pairs.shape[1]
    by_in, by_out = _tables(pairs, num, N, M)
    dY = torch.from_numpy(rng.integers(-2, 3, size=(M, C)).astype(np.float32)).to(dtype)
    want_y = pool_forward(X, pairs, num, M)
    want_dx = pool_backward(X, want_y, dY, pairs, num).to(dtype)
    Ncap, Mcap, G = N + 37, M + 53, 8
    junk = 1 << 30

    def padded(t, cap, fill):
        big = torch.full((cap + 2 * G,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        big[G:G + t.shape[0]] = t
        return big.to(DEV)

    def table(t, cap):
        big = np.full((t.shape[0], cap), junk, np.int32)
        big[:, :t.shape[1]] = t
        return torch.from_numpy(big).to(DEV)

    Xb, dYb = padded(X, Ncap, 7.0), padded(dY, Mcap, 7.0)
    Yb, dXb = padded(torch.zeros((0, C), dtype=dtype), Mcap, 5.0), padded(torch.zeros((0, C), dtype=dtype), Ncap, 5.0)
    t_out, t_in = table(by_out, Mcap), table(by_in, Ncap)
    n_dev = torch.tensor([N], dtype=torch.int64, device=DEV)
    m_dev = torch.tensor([M], dtype=torch.int64, device=DEV)
    code = _lib.dtype_code(Xb)
    _lib.check(lib.wfs_maxpool_fwd(_lib.ptr(t_out), None, K, Mcap, _lib.ptr(Xb[G:G + Ncap]), Ncap, C, _lib.ptr(Yb[G:G + Mcap]),
                                   code, _lib.ptr(m_dev), _lib.stream_ptr()))
    _lib.check(lib.wfs_maxpool_bwd(_lib.ptr(t_in), K, 0, Ncap, _lib.ptr(Xb[G:G + Ncap]), _lib.ptr(Yb[G:G + Mcap]),
                                   _lib.ptr(dYb[G:G + Mcap]), Mcap, C, _lib.ptr(dXb[G:G + Ncap]), code, _lib.ptr(n_dev),
                                   _lib.stream_ptr()))
    torch.cuda.synchronize()
    Yc, dXc = Yb.cpu(), dXb.cpu()
    assert torch.equal(_bits(Yc[G:G + M]), _bits(want_y)) and torch.equal(dXc[G:G + N], want_dx)
    assert bool((Yc[:G] == 5.0).all()) and bool((Yc[G + M:] == 5.0).all())
    assert bool((dXc[:G] == 5.0).all()) and bool((dXc[G + N:] == 5.0).all())


def test_c_abi_rejects_bad_arguments():
    from waveformml_amd import _lib
    lib = _lib.load()
    t = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    x = torch.zeros((8, 4), device=DEV)
    bad_map = _lib.i32_array([0, 0, 1, 2])
    assert lib.wfs_maxpool_fwd(_lib.ptr(t), bad_map, 4, 8, _lib.ptr(x), 8, 4, _lib.ptr(x.clone()), 0, None,
                               _lib.stream_ptr()) == _lib.WFS_EINVAL
    assert lib.wfs_maxpool_fwd(_lib.ptr(t), None, 4, 8, _lib.ptr(x), 8, 4, _lib.ptr(x.clone()), 9, None,
                               _lib.stream_ptr()) == _lib.WFS_EINVAL
    assert lib.wfs_maxpool_bwd(_lib.ptr(t), 4, 3, 8, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 8, 4, _lib.ptr(x.clone()), 0, None,
                               _lib.stream_ptr()) == _lib.WFS_EINVAL          # 4 offsets in packs of 3
    assert lib.wfs_maxpool_packed_ok(3, 27, 32, 1) == 1 and lib.wfs_maxpool_packed_ok(3, 4, 32, 1) == 0
    assert lib.wfs_maxpool_packed_ok(0, 27, 32, 1) == 0 and lib.wfs_maxpool_packed_ok(9, 27, 32, 1) == 0


# ---------------------------------------------------------------------------------------------------- device-count mode
def _padded_tensor(idx, X, B, shape, n_pad=211):
    import waveformml_amd.spconv as sp
    N = idx.shape[0]
    junk = torch.full((n_pad, idx.shape[1]), 99999, dtype=torch.int32)
    junk[::3, 0] = 0
    ip = torch.cat([torch.from_numpy(idx), junk]).to(DEV)
    xp = torch.cat([X, torch.full((n_pad, X.shape[1]), 1000.0, dtype=X.dtype)]).to(DEV).requires_grad_(True)
    st = sp.SparseConvTensor(xp, ip, list(shape), B)
    st.n_valid = torch.tensor([N], dtype=torch.int64, device=DEV)
    return st, xp


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("geo", [PSD_GEO, GEOMETRIES[1], GEOMETRIES[5]], ids=["k3_s114", "k112_s112", "subm_k3"])
def test_device_count_mode_equals_exact_size_mode(geo, dtype):
    """The batch padded to a capacity with the count on the device (the event-local builds, the packed by-input table
    where the geometry has one): the valid rows equal the exact-size run bit for bit."""
    ndim, shape, k, s, p, d, subm = geo
    rng = np.random.default_rng(41)
    B, C = 5, 32
    vol = int(np.prod(shape))
    idx = _events(rng, [vol // 12, vol // 30, 0, vol // 8, vol // 16], shape)
    N = idx.shape[0]
    X = _features(rng, N, C, dtype, False)
    out_idx, pairs, num = pool_rulebook(idx, B, shape, k, s, p, d, subm)
    M = out_idx.shape[0]
    dY = torch.from_numpy(rng.integers(-2, 3, size=(M, C)).astype(np.float32)).to(dtype)
    _o, Y, dX = _run(geo, idx, X, dY, B)
    pool = _module(geo)
    st, xp = _padded_tensor(idx, X, B, shape)
    out = pool(st)
    m = int(out.n_valid)
    assert m == M and out.features.shape[0] >= M
    assert np.array_equal(out.indices[:M].cpu().numpy(), out_idx)
    g = torch.full(out.features.shape, 3.0, dtype=dtype)
    g[:M] = dY
    out.features.backward(g.to(DEV))
    assert torch.equal(_bits(out.features[:M].detach().cpu()), _bits(Y))
    assert torch.equal(xp.grad[:N].cpu(), dX)
    assert all(not f.any() for f in pool.sticky_flags())


def test_out_capacity_below_the_output_count_raises_the_flag_and_stays_in_bounds():
    """A sized buffer, not a provoked fault: with ``out_capacity`` below the true count the build raises the sticky
    overflow flag, every table entry names a row that exists, and forward and backward write their own rows only."""
    ndim, shape, k, s, p, d, subm = PSD_GEO
    rng = np.random.default_rng(43)
    B, C = 6, 32
    idx = _events(rng, [260, 410, 0, 330, 120, 500], shape)
    N = idx.shape[0]
    M = pool_rulebook(idx, B, shape, k, s, p, d)[0].shape[0]
    cap = M // 3
    pool = _module(PSD_GEO)
    pool.out_capacity = cap
    X = _features(rng, N, C, torch.bfloat16, True)
    st, xp = _padded_tensor(idx, X, B, shape)
    out = pool(st)
    rb = pool.last_rulebook
    torch.cuda.synchronize()
    assert tuple(out.features.shape) == (cap, C) and int(rb.m_dev) == cap
    assert int(pool._sticky_flags()["overflow"]) == 1
    t_in, t_out = rb.nbr_out[:, :N].cpu().numpy(), rb.nbr_in[:, :cap].cpu().numpy()
    assert t_in.min() >= -1 and t_in.max() < cap and t_out.min() >= -1 and t_out.max() < N
    out.features.backward(torch.ones_like(out.features))
    torch.cuda.synchronize()
    assert tuple(xp.grad.shape) == tuple(xp.shape) and bool(torch.isfinite(xp.grad[:N].float()).all())
    assert bool(torch.isfinite(out.features.float()).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [2, 32])
def test_packed_and_dense_by_input_tables_give_identical_gradients(dtype, C):
    from waveformml_amd.spconv import functional as Fsp
    from waveformml_amd.spconv import ops
    ndim, shape, k, s, p, d, subm = PSD_GEO
    assert ops.PACKED_TABLES and ops.EVENT_LOCAL_CONV
    rng = np.random.default_rng(47)
    B = 4
    idx = _events(rng, [350, 0, 280, 420], shape)
    N = idx.shape[0]
    X = _features(rng, N, C, dtype, True)
    st, xp = _padded_tensor(idx, X, B, shape)
    rb = ops.build_rulebook(st.indices, B, list(shape), [3] * 3, [1, 1, 4], [0] * 3, [1] * 3, False, n_dev=st.n_valid, flags={})
    assert rb.nbr_out_packed is not None and rb.packed_kl == 3
    x = xp.detach()
    Y = Fsp.maxpool_fwd(rb.nbr_in, None, rb.K, rb.M, x, rb.m_dev)
    dY = torch.from_numpy(rng.standard_normal((rb.M, C)).astype(np.float32)).to(dtype).to(DEV)
    a = Fsp.maxpool_bwd(rb.nbr_out_packed, rb.K, rb.packed_kl, rb.N, x, Y, dY, rb.n_dev)
    b = Fsp.maxpool_bwd(rb.nbr_out, rb.K, 0, rb.N, x, Y, dY, rb.n_dev)
    assert torch.equal(_bits(a[:N].cpu()), _bits(b[:N].cpu()))
    assert bool((a[:N].float().abs().sum(1) > 0).any())


# -------------------------------------------------------------------------------------------------- the captured steps
T_SMALL, B_SMALL = 64, 24


def _assert_close(got, want, rtol=1e-5, what=""):
    """|got - want| <= rtol * max|want| + rtol * |want|  (relative to the tensor's scale)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * max(scale, 1e-30), err_msg=what)


def _pool_cfg(T):
    with open(os.path.join(ROOT, "config", "psd_c2_pool.json")) as f:
        cfg = json.load(f)
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["algorithm"][-1] = [32 * 14 * 11 * (T // 16), 3]
    return cfg


def _pool_module(T):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(11)
    return LitPSD(DictionaryUtility.to_object(copy.deepcopy(_pool_cfg(T)))).to(DEV)


def _batches(seeds):
    from waveformml_amd.psd import synthetic
    out = []
    for sd in seeds:
        c, f, y = synthetic.generate(B_SMALL, T_SMALL, 3, seed=sd)
        out.append(([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV)], torch.from_numpy(y).to(DEV)))
    return out


def _make():
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    mod = _pool_module(T_SMALL)
    red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
    mod.optimizer_parameters = red.optimizer_parameters()
    opt = mod.configure_optimizers()[0][0]
    return mod, red, opt


def test_captured_pool_step_matches_eager_steps():
    """Replays of GraphedTrainStep on config/psd_c2_pool.json against the same steps run eagerly from the same state,
    compared as test_gpu_parity.test_graph_captured_step_matches_eager_steps compares C2 (and with its bounds: the loss
    to 1e-5, the six-step parameter update to 2e-3 of its size -- the padded step cuts its fp32 row reductions at other
    places than the exact-size one, fed back through six nesterov steps).  check() raises nothing; the head runs off
    the pool's cell map; an evaluation runner works beside the live train runner."""
    import waveformml_amd.spconv as sp
    from waveformml_amd.psd.graph import GraphedEvalStep, GraphedTrainStep
    batches = _batches((5, 6, 7))
    mod_e, red_e, opt_e = _make()
    mod_g, red_g, opt_g = _make()
    step = GraphedTrainStep(mod_g, opt_g, red_g, batches[0], warmup=2)
    pools = [m for m in mod_g.model.modules() if isinstance(m, sp.SparseMaxPool)]
    assert len(pools) == 2 and all(m.out_capacity >= m.calibration_count() for m in pools)
    assert mod_g.model.head_route == "sparse_head"
    for _ in range(3):
        red_e.reset()
        mod_e.training_step(batches[0], 0).backward()
        red_e.finish()
        opt_e.step()
    for b in batches:
        red_e.reset()
        le = mod_e.training_step(b, 0)
        le.backward()
        red_e.finish()
        opt_e.step()
        lg = step(b)
        step.check()
        print("loss captured %.8f eager %.8f" % (lg.item(), le.item()))
        assert abs(lg.item() - le.item()) <= 1e-5 * max(abs(le.item()), 1e-6), (lg.item(), le.item())
    ev = GraphedEvalStep(mod_g, batches[1])
    logits = ev(batches[1]).clone()
    ev.check()
    assert tuple(logits.shape) == (B_SMALL, 3) and bool(torch.isfinite(logits).all())
    step(batches[2])                          # the train graph replays beside the live evaluation graph
    step.check()
    assert bool(torch.isfinite(ev(batches[1])).all())
    ev.check()
    ev.close()
    step.close()


def test_captured_pool_updates_match_eager_updates():
    """The accumulated parameter update of six paired steps (three on the example batch, three more): 2e-3 of its size,
    the bound of test_graph_captured_step_matches_eager_steps."""
    from waveformml_amd.psd.graph import GraphedTrainStep
    batches = _batches((5, 6, 7))
    mod_e, red_e, opt_e = _make()
    mod_g, red_g, opt_g = _make()
    start = [p.detach().clone() for p in mod_e.model.parameters()]
    step = GraphedTrainStep(mod_g, opt_g, red_g, batches[0], warmup=2)
    for b in [batches[0]] * 3 + batches:
        red_e.reset()
        mod_e.training_step(b, 0).backward()
        red_e.finish()
        opt_e.step()
    for b in batches:
        step(b)
    step.check()
    for p0, a, b in zip(start, mod_e.model.parameters(), mod_g.model.parameters()):
        upd_e, upd_g = (a.detach() - p0).cpu().numpy(), (b.detach() - p0).cpu().numpy()
        _assert_close(upd_g, upd_e, 2e-3, "parameter update over 6 steps")
    step.close()


def test_captured_pool_runs_are_bit_identical():
    """Two captured runs from the same state: bit-identical losses and weights (the pool adds no atomics)."""
    from waveformml_amd.psd.graph import GraphedTrainStep
    batches = _batches((5, 6, 7))
    runs = []
    for _ in range(2):
        mod, red, opt = _make()
        step = GraphedTrainStep(mod, opt, red, batches[0], warmup=2)
        losses = [step(b).clone() for b in batches + batches]
        step.check()
        torch.cuda.synchronize()
        runs.append((losses, copy.deepcopy(mod.state_dict())))
        step.close()
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for name in runs[0][1]:
        assert torch.equal(runs[0][1][name], runs[1][1][name]), name


def test_pool_net_trains_through_the_capturing_trainer():
    """Trainer(capture=True) on the pool net: an epoch runs, the weights move, nothing is flagged."""
    from waveformml_amd.psd import data
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.trainer import Trainer
    ds = data.SyntheticPulseDataset(6, B_SMALL, T_SMALL, n_type=3, layout="3d", seed=77)
    loader = data.make_loader(ds, 1, shuffle=False, pin_memory=False)
    torch.manual_seed(11)
    mod = LitPSD(DictionaryUtility.to_object(copy.deepcopy(_pool_cfg(T_SMALL))))
    start = copy.deepcopy(mod.state_dict())
    tr = Trainer(max_epochs=1, device=DEV, capture=True)
    tr.fit(mod, loader)
    sd = mod.state_dict()
    assert all(bool(torch.isfinite(v.float()).all()) for v in sd.values())
    w = "model.sparseModel.0.weight"
    assert not torch.equal(sd[w].cpu(), start[w].cpu())
