"""SparseMaxPool2d / 3d on the host: the surface (signatures, geometry, config strings, no CPU path) and the
restatement of spconv 1.2.1's pool arithmetic over the oracle's rulebook, which the GPU tests (test_gpu_pool.py) compare
the HIP kernels with.  The restatement itself is pinned against ``torch.nn.functional.max_pool{2,3}d`` of the densified
input in the regime the nets use (positive, tie-free rows): values and input gradients exactly equal."""
import copy
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import densify, norm, rand_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------- restatement
def pool_rulebook(idx, B, shape, ksize, stride, padding, dilation, subm=False):
    """(out_indices [M, D+1], pairs [2, K, N], num [K]) of the oracle for a pool's geometry."""
    from oracle import ref
    ndim = len(shape)
    out, pairs, num = ref.get_indice_pairs(np.ascontiguousarray(idx, np.int32), B, list(shape), norm(ksize, ndim),
                                           norm(stride, ndim), norm(padding, ndim), norm(dilation, ndim), 0, subm)
    return np.asarray(out), np.asarray(pairs), np.asarray(num)


def pool_forward(X, pairs, num, M):
    """spconv's indice_maxpool: the output starts at ZERO; for every pair (in, out), in offset order,
    ``if X[in] > Y[out]: Y[out] = X[in]`` -- in X's own dtype (torch tensor [N, C])."""
    Y = torch.zeros((M, X.shape[1]), dtype=X.dtype)
    for k in range(pairs.shape[1]):
        i, o = torch.from_numpy(pairs[0, k, :num[k]]).long(), torch.from_numpy(pairs[1, k, :num[k]]).long()
        Y[o] = torch.where(X[i] > Y[o], X[i], Y[o])          # distinct sites: an output appears once per offset
    return Y


def pool_backward(X, Y, dY, pairs, num, acc=torch.float32):
    """spconv's indice_maxpool_backward: ``dX[in] += dY[out]`` where ``X[in] == Y[out]``, per channel, summed in ``acc``
    in offset order (returned in ``acc``: the caller rounds)."""
    dX = torch.zeros(X.shape, dtype=acc)
    for k in range(pairs.shape[1]):
        i, o = torch.from_numpy(pairs[0, k, :num[k]]).long(), torch.from_numpy(pairs[1, k, :num[k]]).long()
        dX[i] += torch.where(X[i] == Y[o], dY[o].to(acc), torch.zeros((), dtype=acc))
    return dX


def dense_max_pool(idx, X, B, shape, out, dY, ksize, stride, padding, dilation):
    """F.max_pool{2,3}d of the densified input: (values at ``out``, the set of non-zero pooled cells as index rows,
    gradient at the input sites for the dense gradient that holds ``dY`` at ``out`` and 0 elsewhere)."""
    ndim = len(shape)
    pool = {2: F.max_pool2d, 3: F.max_pool3d}[ndim]
    d = torch.from_numpy(densify(idx, X.float().numpy(), B, shape)).requires_grad_(True)
    # padded with the zeros of inactive cells (torch's own padding is limited to half a kernel; a dilated pool needs more)
    pad = [v for a in reversed(norm(padding, ndim)) for v in (a, a)]
    y = pool(F.pad(d, pad), norm(ksize, ndim), norm(stride, ndim), 0, norm(dilation, ndim))
    at = lambda t, rows: t[(torch.from_numpy(rows[:, 0]).long(), slice(None)) +          # noqa: E731
                           tuple(torch.from_numpy(rows[:, 1 + a]).long() for a in range(ndim))]
    g = torch.zeros_like(y)
    g[(torch.from_numpy(out[:, 0]).long(), slice(None)) + tuple(torch.from_numpy(out[:, 1 + a]).long() for a in range(ndim))] = dY.float()
    y.backward(g)
    cells = torch.nonzero(y.detach().amax(1))            # cells with a non-zero channel
    return at(y.detach(), out), cells.numpy().astype(np.int32), at(d.grad, idx)


POOL_CASES = [
    # ndim, shape, ksize, stride, padding, dilation
    (3, (14, 11, 64), 3, (1, 1, 4), 0, 1),
    (3, (14, 11, 64), (1, 1, 2), (1, 1, 2), 0, 1),
    (2, (13, 12), 3, 2, 1, 1),
    (2, (12, 10), 2, 2, 0, 1),
]


@pytest.mark.parametrize("case", POOL_CASES, ids=["k3_s114", "k112_s112", "2d_k3_s2_p1", "2d_k2_s2"])
def test_restatement_equals_dense_max_pool_on_positive_rows(case):
    """Positive tie-free features: the restatement's values and input gradients equal torch's dense max pool exactly;
    inactive cells are the zeros the output starts from; the non-zero pooled cells are the output set."""
    ndim, shape, k, s, p, d = case
    rng = np.random.default_rng(3)
    B, C = 3, 5
    n = int(0.12 * B * np.prod(shape))
    idx = rand_coords(rng, B, shape, n)
    X = torch.from_numpy((rng.permutation(n * C).reshape(n, C) + 1).astype(np.float32) / 8.0)       # distinct, > 0, exact
    out, pairs, num = pool_rulebook(idx, B, shape, k, s, p, d)
    Y = pool_forward(X, pairs, num, len(out))
    dY = torch.from_numpy(rng.integers(-2, 3, size=(len(out), C)).astype(np.float32))
    dX = pool_backward(X, Y, dY, pairs, num)
    want_y, cells, want_dx = dense_max_pool(idx, X, B, shape, out, dY, k, s, p, d)
    assert torch.equal(Y, want_y)
    assert torch.equal(dX, want_dx)
    key = lambda rows: sorted(map(tuple, rows.tolist()))          # noqa: E731
    assert key(cells) == key(out)


def test_restatement_starts_from_zero():
    """Rows with negative entries: max(0, neighbours), not the plain maximum; a 0 under an output that stayed 0 and
    tied inputs all receive the gradient."""
    idx = np.array([[0, 0, 0], [0, 0, 1], [0, 3, 3]], np.int32)
    X = torch.tensor([[-1.0, 2.0, 0.0], [-3.0, 2.0, -5.0], [4.0, -4.0, 1.0]])
    out, pairs, num = pool_rulebook(idx, 1, (4, 4), 2, 2, 0, 1)
    assert out.tolist() == [[0, 0, 0], [0, 1, 1]]
    Y = pool_forward(X, pairs, num, 2)
    assert Y.tolist() == [[0.0, 2.0, 0.0], [4.0, 0.0, 1.0]]
    dX = pool_backward(X, Y, torch.ones(2, 3), pairs, num)
    assert dX.tolist() == [[0.0, 1.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]]


# ------------------------------------------------------------------------------------------------------------- surface
def test_constructors_and_positional_signatures():
    import waveformml_amd.spconv as sp
    assert list(inspect.signature(sp.SparseMaxPool.__init__).parameters) == [
        "self", "ndim", "kernel_size", "stride", "padding", "dilation", "subm"]
    for cls in (sp.SparseMaxPool2d, sp.SparseMaxPool3d):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == ["self", "kernel_size", "stride", "padding", "dilation"]
        assert [sig.parameters[n].default for n in ("stride", "padding", "dilation")] == [1, 0, 1]
        assert issubclass(cls, sp.SparseMaxPool) and issubclass(cls, sp.SparseModule)
    sig = inspect.signature(sp.SparseMaxPool.__init__)
    assert [sig.parameters[n].default for n in ("stride", "padding", "dilation", "subm")] == [1, 0, 1, False]
    m = sp.SparseMaxPool3d([1, 1, 4], [1, 1, 4])
    assert (m.ndim, m.kernel_size, m.stride, m.padding, m.dilation, m.subm) == (3, [1, 1, 4], [1, 1, 4], [0] * 3, [1] * 3, False)
    m = sp.SparseMaxPool2d(3, 2, 1)
    assert (m.ndim, m.kernel_size, m.stride, m.padding, m.dilation) == (2, [3, 3], [2, 2], [1, 1], [1, 1])
    m = sp.SparseMaxPool(3, 3, subm=True)
    assert m.subm and m.calibration_count() is None
    assert not hasattr(m, "indice_key")
    with pytest.raises(AssertionError):
        sp.SparseMaxPool2d(3, 2, 0, 2)               # stride > 1 with dilation > 1, as the conv classes
    with pytest.raises(AssertionError):
        sp.SparseMaxPool3d([3, 3], 1)                # two values for three axes
    for name in ("SparseMaxPool", "SparseMaxPool2d", "SparseMaxPool3d"):
        assert name in sp.__all__


def test_pool_has_no_parameters_and_owns_sticky_flags():
    import waveformml_amd.spconv as sp
    m = sp.SparseMaxPool3d(3, [1, 1, 4])
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {}
    assert isinstance(m, sp.ops.StickyFlags) and m.sticky_flags() == []
    store = m._sticky_flags()
    m.fresh_sticky_flags()
    assert m._sticky_flags() is not store


@pytest.mark.parametrize("case", POOL_CASES + [(2, (9, 9), 3, 1, 2, 2), (3, (5, 6, 7), (2, 3, 3), (1, 2, 4), (0, 1, 0), 1)])
def test_output_shape_arithmetic(case):
    """The pool's output shape is ops.get_conv_output_size of its geometry = the oracle's regular-conv shape."""
    import waveformml_amd.spconv as sp
    from oracle import ref
    ndim, shape, k, s, p, d = case
    m = sp.SparseMaxPool(ndim, k, s, p, d)
    got = sp.ops.get_conv_output_size(list(shape), m.kernel_size, m.stride, m.padding, m.dilation)
    assert got == [int(v) for v in ref.conv_output_shape(list(shape), m.kernel_size, m.stride, m.padding, m.dilation)]
    want = [(shape[i] + 2 * m.padding[i] - m.dilation[i] * (m.kernel_size[i] - 1) - 1) // m.stride[i] + 1 for i in range(ndim)]
    assert got == want


def test_cpu_tensor_raises():
    import waveformml_amd.spconv as sp
    x = sp.SparseConvTensor(torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int32), [4, 4, 8], 1)
    with pytest.raises(RuntimeError):
        sp.SparseMaxPool3d(2, 2)(x)
    with pytest.raises(RuntimeError):
        sp.SparseSequential(sp.SparseMaxPool3d([1, 1, 4], [1, 1, 4]))(x)


def test_sequential_and_algorithm_list_build():
    import waveformml_amd.spconv as sp
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    seq = sp.SparseSequential(sp.SubMConv3d(2, 8, 3, indice_key="a"), torch.nn.ReLU(), sp.SparseMaxPool3d([1, 1, 4], [1, 1, 4]),
                              sp.ToDense())
    assert isinstance(seq[2], sp.SparseMaxPool3d) and len(seq) == 4
    with open(os.path.join(ROOT, "config", "psd_c2_pool.json")) as f:
        cfg = json.load(f)
    alg = cfg["net_config"]["algorithm"]
    assert alg.count("spconv.SparseMaxPool3d") == 2 and "spconv.SparseConv3d" not in alg
    assert alg[-1] == [14 * 11 * 16 * 32, 3]
    mod = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
    pools = [m for m in mod.model.sparseModel if isinstance(m, sp.SparseMaxPool3d)]
    assert len(pools) == 2 and all(m.kernel_size == [1, 1, 4] and m.stride == [1, 1, 4] for m in pools)
    # 14 x 11 stays, time 256 -> 64 -> 16: the Linear's inputs
    shape = [14, 11, cfg["system_config"]["n_samples"]]
    for m in pools:
        shape = sp.ops.get_conv_output_size(shape, m.kernel_size, m.stride, m.padding, m.dilation)
    assert shape == [14, 11, 16] and mod.model.linear[0].in_features == 32 * 14 * 11 * 16
