"""The float64 BatchNorm reference, the inputs and the case table of tests/bn_cases.py, checked on the CPU.

* The reference equals torch.nn.BatchNorm1d (+ relu) in float64 with autograd, to 1e-12.
* Every case, in every row type it runs in, is well-posed: the ReLU margin holds, few elements were moved to get it,
  the inputs are values of the row type, both sides of the ReLU are populated, no compared tensor is identically zero
  (but dX and dgamma of a single row, which are), and a plain fp32 restatement of the formulas stays within
  E32_MAX = 3e-6 of float64 for every tensor -- a third of the 1e-5 the kernels are held to.
* The arms the table claims are the ones wfs_bn_plan reports (csrc/bn.hip; host only, nothing is launched), with the
  partial counts derived from the dispatch constants; every family, direction, rows-per-thread value and both block
  sums occur; the channel-slice loops of the two entry points are unreachable.
"""
import ctypes

import numpy as np
import pytest

import bn_cases as bc

DT = {"f32": 0, "bf16": 1, "f16": 2}


def _plan(N, C, kind, training, backward):
    from waveformml_amd import _lib
    per, partials = ctypes.c_int32(-7), ctypes.c_int32(-7)
    fam = _lib.load().wfs_bn_plan(N, C, DT[kind] if isinstance(kind, str) else kind, 1 if training else 0,
                                  1 if backward else 0, ctypes.byref(per), ctypes.byref(partials))
    return fam, per.value, partials.value


# ------------------------------------------------------------------------------------------ reference against torch
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", [(2, 3, 2), (17, 5, 17), (40, 12, 29), (9, 130, 9)])
def test_reference_equals_torch_in_float64(shape, training, relu):
    import torch
    cap, C, n = shape
    rng = np.random.default_rng(cap * 7 + C)
    x, g = rng.standard_normal((cap, C)) * 2 + 1, rng.standard_normal((cap, C))
    x[n:], g[n:] = np.nan, np.nan
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
    rm, rv = rng.standard_normal(C), rng.uniform(0.5, 2.0, C)
    ref = bc.reference(x, g, gamma, beta, rm, rv, n, relu, training)
    bn = torch.nn.BatchNorm1d(C, eps=bc.EPS, momentum=bc.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm))
        bn.running_var.copy_(torch.from_numpy(rv))
    bn.train(training)
    xt = torch.from_numpy(x[:n].copy()).requires_grad_(True)
    y = bn(xt)
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(g[:n].copy()))

    def close(got, want, what):
        want = want.detach().numpy()
        assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max())), what

    close(ref.y[:n], y, "y")
    close(ref.dX[:n], xt.grad, "dX")
    close(ref.dgamma, bn.weight.grad, "dgamma")
    close(ref.dbeta, bn.bias.grad, "dbeta")
    close(ref.running_mean, bn.running_mean, "running_mean")
    close(ref.running_var, bn.running_var, "running_var")
    assert np.isnan(ref.y[n:]).all() and np.isnan(ref.dX[n:]).all(), "rows beyond the count are untouched"
    if training:
        close(ref.save_mean, xt.detach().mean(0), "mean")
        close(ref.var, xt.detach().var(0, unbiased=False), "var")
    else:
        assert np.array_equal(ref.running_mean, rm) and np.array_equal(ref.running_var, rv)
        assert np.array_equal(ref.save_mean, rm)
        close(ref.dX[:n], torch.from_numpy(gamma * ref.invstd * np.where(ref.pre > 0, g[:n], 0.0 if relu else g[:n])), "dX eval")


def test_one_row_keeps_the_biased_variance_in_the_running_statistics():
    """torch refuses a single row in training; the kernels take the factor n / (n - 1) as 1 there."""
    x, g = np.array([[1.5, -2.0]]), np.array([[1.0, 1.0]])
    rm, rv = np.array([0.5, 0.5]), np.array([2.0, 3.0])
    ref = bc.reference(x, g, None, None, rm, rv, 1, False, True)
    assert np.array_equal(ref.var, [0.0, 0.0]) and np.allclose(ref.running_var, 0.9 * rv, rtol=1e-15)
    assert np.allclose(ref.running_mean, 0.9 * rm + 0.1 * x[0], rtol=1e-15)
    assert not ref.y.any() and not ref.dX.any() and not ref.dgamma.any() and np.array_equal(ref.dbeta, [1.0, 1.0])


def test_the_blocked_fp32_sum_adds_in_the_order_it_says():
    rng = np.random.default_rng(2)
    a = rng.standard_normal((200, 3)).astype(np.float32)
    blocks = []
    for lo in range(0, 200, 64):
        s = np.zeros(3, np.float32)
        for row in a[lo:lo + 64]:
            s = s + row
        blocks.append(s)
    want = (blocks[0] + blocks[1]) + (blocks[2] + blocks[3])
    assert np.array_equal(bc._bsum32(a), want)
    assert np.array_equal(bc._bsum32(a[:1]), a[0])


def test_unit_steps_of_the_row_types():
    v = np.array([1.0, -1.0, 3.5, -0.0078125], np.float32)
    for kind, up in (("f32", 2.0 ** -23), ("bf16", 2.0 ** -7), ("f16", 2.0 ** -10)):
        s = bc.step_ulp(v, np.ones(4), kind)
        assert np.array_equal(bc.round_to(s, kind), s) and (s > v).all(), kind
        assert s[0] == np.float32(1.0 + up)
        d = bc.step_ulp(v, -np.ones(4), kind)
        assert np.array_equal(bc.round_to(d, kind), d) and (d < v).all(), kind
        assert np.array_equal(bc.step_ulp(d, np.ones(4), kind), v)


# ----------------------------------------------------------------------------------------------- every case, every kind
def _params():
    return [pytest.param(c.name, kind, id="%s-%s" % (c.name, kind)) for kind in bc.KINDS for c in bc.cases_for(kind)]


@pytest.mark.parametrize("name,kind", _params())
def test_case_is_well_posed(name, kind):
    p = bc.make_problem(name, kind)
    c, n = p.case, p.valid
    ref = bc.reference_of(name, kind)
    assert p.x.shape == p.g.shape == (c.N, c.C) and 1 <= n <= c.N
    # values of the row type; NaN beyond the count
    for a in (p.x, p.g):
        assert np.isfinite(a[:n]).all() and np.isnan(a[n:]).all()
        assert np.array_equal(bc.round_to(a[:n], kind), a[:n]), "inputs are rounded to the row type"
    assert (p.gamma is None) == (p.beta is None) == (not c.affine) and (p.rm is None) == (p.rv is None) == (not c.running)
    if c.affine:
        assert 0.5 <= p.gamma.min() and p.gamma.max() <= 1.5 and 0.02 <= np.abs(p.beta).min() and np.abs(p.beta).max() <= 0.5
    # the ReLU margin and what it cost
    top = float(np.abs(ref.pre).max())
    assert top > 0 and float(np.abs(ref.pre).min()) >= bc.MARGIN * top, "an element sits inside the ReLU margin"
    assert p.moved_share <= bc.MOVED_MAX, "%.2e of the elements were moved" % p.moved_share
    if c.relu and n >= 8:
        zero = ref.y[:n] == 0
        assert 0.2 <= float(zero.mean()) <= 0.8, float(zero.mean())
        assert zero.any(axis=0).all() and (~zero).any(axis=0).all(), "a channel is all live or all dead"
    # no compared tensor is identically zero, except what one row makes zero
    want = bc.wanted(ref)
    assert set(want) == set(bc.ROW_TENSORS + bc.F32_TENSORS) - (set() if c.running else {"running_mean", "running_var"})
    for t, w in want.items():
        w = w[:n] if t in bc.ROW_TENSORS else w
        assert np.isfinite(w).all(), t
        if n == 1 and c.training and t in ("dX", "dgamma"):
            assert not w.any(), t
        else:
            assert float(np.abs(w).max()) > 0, t
    if not c.training:
        assert np.array_equal(ref.running_mean, p.rm.astype(np.float64)) and np.array_equal(ref.save_mean, ref.running_mean)
    # what fp32 arithmetic of this shape costs on these inputs
    e32 = bc.e32_of(p, ref)
    print("%s %s: moved %.1e, replaced columns %d, e32 %s" % (name, kind, p.moved_share, p.replaced,
                                                             "  ".join("%s %.1e" % kv for kv in sorted(e32.items()))))
    for t, e in e32.items():
        assert e <= bc.E32_MAX, "%s: plain fp32 is %.2e of max|%s| away from float64" % (name, e, t)
    if c.special == "offset2000":
        assert abs(float(ref.mean.mean()) - 2000) < 1 and 0.15 < float(ref.var.mean()) < 0.35
        assert np.array_equal(ref.mean.astype(np.float32).astype(np.float64), ref.mean), "the exact means are fp32 numbers"
        x = p.x[:n].astype(np.float32)
        naive = (x * x).mean(axis=0, dtype=np.float32) - np.square(x.mean(axis=0, dtype=np.float32))
        assert float(np.abs(naive - ref.var).max()) > 0.1, "naive fp32 sums lose this variance"
    if c.special == "row0far":
        far = np.abs(p.x[0] - ref.mean) * ref.invstd
        assert 3.8 <= float(far.min()) and float(far.max()) <= 4.3, (far.min(), far.max())


# ------------------------------------------------------------------------------------------------------- coverage
def test_the_table_claims_what_the_library_plans():
    seen = set()
    for c in bc.CASES:
        for kind in c.kinds:
            for backward in (False, True):
                fam, per, partials = _plan(c.N, c.C, kind, c.training, backward)
                want = bc.expected_plan(c.N, c.C, kind, c.training, backward)
                assert (fam, per, partials) == want, (c.name, kind, backward, (fam, per, partials), want)
                assert (fam, per) == bc.claimed(c, kind, backward), (c.name, kind, backward, fam, per)
                if not backward and not c.training:
                    assert partials == 0 and fam != bc.RR          # the eval forward folds nothing
                else:
                    assert partials >= 1
                seen.add((fam, backward, per, bc.block_sum_path(c.C) if fam == bc.RR else None, kind,
                          "train" if c.training else "eval"))
    for backward in (False, True):
        for kind in bc.KINDS:
            for fam in (bc.COLUMN, bc.LOOP4, bc.LOOP1):
                for mode in ("train", "eval"):
                    assert (fam, backward, 0, None, kind, mode) in seen, (fam, backward, kind, mode)
            for path in ("serial", "lane-exchange"):
                pers = {s[2] for s in seen if s[0] == bc.RR and s[1] == backward and s[3] == path and s[4] == kind}
                top = 8 if backward and kind == "f32" else 16
                assert pers == {q for q in (2, 4, 8, 16) if q <= top}, (backward, kind, path, pers)
    assert any(s[0] == bc.RR and s[1] and s[5] == "eval" for s in seen), "the eval backward on the register-resident kernels"
    # the counts the table is there for
    assert bc.expected_plan(8193, 124, "f32", True, False) == (bc.LOOP4, 0, 64)
    assert bc.expected_plan(8192, 124, "f32", True, False) == (bc.RR, 16, 64)
    assert bc.expected_plan(8192, 124, "f32", True, True) == (bc.LOOP4, 0, 64)
    assert bc.expected_plan(8192, 124, "bf16", True, True) == (bc.RR, 16, 64)
    assert bc.expected_plan(32769, 64, "f16", True, True) == (bc.LOOP4, 0, 128)
    assert bc.expected_plan(16300, 516, "bf16", True, False) == (bc.LOOP4, 0, 32) and 516 * 16300 > 1 << 23
    assert bc.expected_plan(65537, 7, "f32", True, False) == (bc.LOOP1, 0, 1024)
    assert [bc.expected_plan(n, 33 if n == 64 else 46, "f32", True, False)[2] for n in (64, 65)] == [1, 2]
    assert [bc.expected_plan(n, 130, "f32", True, True)[2] for n in (32, 33, 8160, 8161, 8193)] == [1, 2, 255, 256, 256]
    assert bc.expected_plan(257, 32, "f32", False, False) == (bc.LOOP4, 0, 0)
    assert bc.expected_plan(33, 130, "f32", False, False) == (bc.COLUMN, 0, 0)


def test_device_counts_cover_every_family():
    fams = {}
    for c in bc.CASES:
        if c.valid is not None:
            fams.setdefault(c.fwd[0], set()).add((c.valid, c.N))
    assert set(fams) == {bc.COLUMN, bc.RR, bc.LOOP4, bc.LOOP1}
    for f, vs in fams.items():
        caps = {cap for _v, cap in vs}
        assert len(caps) == 1 and len(vs) == 3
        cap = caps.pop()
        assert {1, cap} <= {v for v, _c in vs} and any(1 < v < cap for v, _c in vs)


def test_plan_refuses_what_the_entry_points_refuse_and_never_slices():
    from waveformml_amd import _lib
    bad = -_lib.WFS_EINVAL
    assert _plan(10, 0, "f32", 1, 0)[0] == bad and _plan(10, -4, "f32", 1, 0)[0] == bad
    assert _plan(10, 32, 3, 1, 0)[0] == bad and _plan(10, 32, -1, 1, 1)[0] == bad
    assert _plan(-1, 32, "f32", 1, 0)[0] == bad
    assert _plan(10, 32, "f32", 1, 0) == (bc.RR, 2, 256)
    lib = _lib.load()
    assert lib.wfs_bn_plan(10, 32, 0, 1, 0, None, None) == bc.RR          # both pointers may be NULL
    # C > 1024 always takes the column-block family, so do odd widths from 128 on: the slice loops of wfs_bn_relu_fwd /
    # wfs_bn_relu_bwd are reached by no call that has rows
    widths = list(range(1, 1300)) + [1696, 1697, 2048, 2050, 4096, 4099, 65536]
    rows = (1, 2, 31, 32, 33, 255, 256, 257, 8191, 8192, 8193, 16257, 65537, 1 << 20, 1 << 24, (1 << 31) + 5)
    for C in widths:
        for N in rows:
            for kind in bc.KINDS:
                for training, backward in ((1, 0), (0, 0), (1, 1), (0, 1)):
                    fam, per, partials = _plan(N, C, kind, training, backward)
                    assert fam in (bc.COLUMN, bc.RR, bc.LOOP4, bc.LOOP1), (N, C, kind, training, backward, fam)
                    if N * C < 1 << 40:
                        assert (fam, per, partials) == bc.expected_plan(N, C, kind, training, backward), (N, C, kind)
    assert _plan(0, 2048, "f32", 1, 0)[0] == bc.SLICES                     # only the empty call passes the slice checks
