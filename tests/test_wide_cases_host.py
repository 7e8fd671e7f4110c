"""The references, inputs and claims of tests/wide_cases.py, checked on the CPU.

* The references equal a naive triple loop on tiny cases, and tests/test_gpu_wide.py's _ref_conv on one of that file's
  cases.
* Every case reports from wfs_wide_plan (csrc/wide.hip; host only, nothing is launched) exactly the plan the table claims,
  in every row type it runs in, and the arms the suite is there for are all reached (test_every_listed_arm_is_reached):
  a planner change that empties an arm fails here.
* The exact set is exact: every element's sum of absolute terms is below 2^24; it is not degenerate for 16-bit results:
  where a 16-bit result sums 1000 terms or more some expected value exceeds 256, so that a bf16 store has to round.
* The gauss set is well conditioned: a plain fp32 evaluation of the reference in index order stays within
  E32_MAX = 3e-6 of float64, per tensor, of the element's sum of absolute terms -- a third of the kernels' bar.  A case
  that misses gets other inputs, not a wider bar.  The figures are printed (pytest -s).
"""
import numpy as np
import pytest

import wide_cases as wc

E32_SEEN = {}


def _lib():
    from waveformml_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------ the references
def _naive_conv(t, kmap, ik, R, valid, X, W, tr, bias):
    K = W.shape[0]
    Cy = W.shape[1] if tr else W.shape[2]
    Y, A = np.zeros((R, Cy)), np.zeros((R, Cy))
    for r in range(valid):
        for c in range(Cy):
            v = a = 0.0
            if bias is not None:
                v, a = float(bias[c]), abs(float(bias[c]))
            for k in range(K):
                s = r if k == ik else int(t[kmap[k] if kmap is not None else k, r])
                if s < 0:
                    continue
                for j in range(X.shape[1]):
                    w = W[k, c, j] if tr else W[k, j, c]
                    v += X[s, j] * w
                    a += abs(X[s, j] * w)
            Y[r, c], A[r, c] = v, a
    return Y, A


@pytest.mark.parametrize("K,R,XR,Cx,Cy,ik,mirror,tr,valid", [(3, 5, 4, 3, 2, -1, False, False, 5), (3, 6, 6, 2, 3, 1, True, True, 4),
                                                             (1, 4, 4, 3, 3, 0, False, False, 4)])
def test_conv_reference_equals_a_naive_loop(K, R, XR, Cx, Cy, ik, mirror, tr, valid):
    rng = np.random.default_rng(K * 10 + R)
    t = wc.build_table(rng, K, R, XR, ik)
    X = rng.standard_normal((XR, Cx))
    W = rng.standard_normal((K, Cy, Cx) if tr else (K, Cx, Cy))
    bias = None if tr else rng.standard_normal(Cy)
    kmap = [K - 1 - k for k in range(K)] if mirror else None
    Y, A = wc.ref_gather_conv(t, kmap, K, ik, R, valid, X, W, tr, bias)
    Yn, An = _naive_conv(t, kmap, ik, R, valid, X, W, tr, bias)
    assert np.abs(Y - Yn).max() <= 1e-13 and np.abs(A - An).max() <= 1e-13
    assert (Y[valid:] == 0).all() and (A >= np.abs(Y) - 1e-13).all()
    # dW through the same table: dW[k, a, b] = sum_r S[r, a] G[src(k, r), b]
    S, G = rng.standard_normal((R, 2)), rng.standard_normal((XR, 3))
    for swap in (False, True):
        dW, dA = wc.ref_gather_dw(t, kmap, K, ik, R, valid, S, G, swap)
        n, na = np.zeros((K, 2, 3)), np.zeros((K, 2, 3))
        for k in range(K):
            for r in range(valid):
                s = r if k == ik else int(t[kmap[k] if kmap is not None else k, r])
                if s >= 0:
                    n[k] += np.outer(S[r], G[s])
                    na[k] += np.abs(np.outer(S[r], G[s]))
        if swap:
            n, na = n.transpose(0, 2, 1), na.transpose(0, 2, 1)
        assert np.abs(dW - n).max() <= 1e-13 and np.abs(dA - na).max() <= 1e-13


def test_linear_reference_equals_a_naive_loop():
    rng = np.random.default_rng(3)
    B, I, O = 3, 4, 2
    x, W, b, g = rng.standard_normal((B, I)), rng.standard_normal((O, I)), rng.standard_normal(O), rng.standard_normal((B, O))
    ref = wc.ref_linear(x, W, b, g)
    for r in range(B):
        for o in range(O):
            assert abs(ref["y"][0][r, o] - (sum(x[r, i] * W[o, i] for i in range(I)) + b[o])) <= 1e-13
            assert abs(ref["y"][1][r, o] - (sum(abs(x[r, i] * W[o, i]) for i in range(I)) + abs(b[o]))) <= 1e-13
        for i in range(I):
            assert abs(ref["dX"][0][r, i] - sum(g[r, o] * W[o, i] for o in range(O))) <= 1e-13
    for o in range(O):
        assert abs(ref["db"][0][o] - sum(g[r, o] for r in range(B))) <= 1e-13
        for i in range(I):
            assert abs(ref["dW"][0][o, i] - sum(g[r, o] * x[r, i] for r in range(B))) <= 1e-13
            assert abs(ref["dW"][1][o, i] - sum(abs(g[r, o] * x[r, i]) for r in range(B))) <= 1e-13


def test_conv_reference_equals_test_gpu_wide_ref_conv():
    """tests/test_gpu_wide.py's SubM case (9, 200, 200, 260, 264): mirrored column map, identity offset 4, 163 valid rows."""
    from test_gpu_wide import _ref_conv as ref_conv          # importing the module launches nothing
    K, R, XR, Cx, Cy, ik = 9, 200, 200, 260, 264, 4
    rng = np.random.default_rng(9200)
    t = rng.integers(0, XR, size=(K, R)).astype(np.int32)
    t[rng.random((K, R)) > 0.4] = -1
    X, W, bias = rng.standard_normal((XR, Cx)), rng.standard_normal((K, Cx, Cy)) * 0.05, rng.standard_normal(Cy)
    kmap = list(range(K - 1, -1, -1))
    for valid in (R, R - 37):
        theirs = ref_conv(t, kmap, ik, R, X, W, False, bias, valid)[:valid]
        ours = wc.ref_gather_conv(t, kmap, K, ik, R, valid, X, W, False, bias)[0][:valid]
        assert np.abs(ours - theirs).max() <= 1e-12 * np.abs(theirs).max()
    Wt = rng.standard_normal((K, 100, Cx)) * 0.05                                # dX: [K, Cy', Cx'] read transposed
    theirs = ref_conv(t, None, -1, R, X, Wt, True, None, R)
    ours = wc.ref_gather_conv(t, None, K, -1, R, R, X, Wt, True, None)[0]
    assert theirs.shape == ours.shape == (R, 100) and np.abs(ours - theirs).max() <= 1e-12 * np.abs(theirs).max()


# ------------------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", list(wc.CONV))
def test_conv_case_reaches_its_arm(name, kind):
    c = wc.CONV[name]
    taken, plan = wc.plan_of(_lib(), wc.PLAN_CONV, kind, c.K, c.R, c.XR, c.Cx, c.Cy, 1 if c.table else 0)
    assert taken == 1, "the wide path does not take %s" % name
    for field, want in c.plan[kind].items():
        assert plan[field] == want, (name, kind, field, plan)
    # forward and dX are one plan: the caller hands dX the same (K, R, X_rows) with the channel roles as they are
    assert _lib().wfs_wide_conv_ok(c.K, c.R, c.XR, c.Cx, c.Cy, wc.DT[kind]) == 1
    direct = plan["nz"] * plan["ksplit"] == 1 and not plan["dense_first"]
    assert (plan["slabs"] == 0) == direct
    if plan["dense_first"]:
        assert plan["slabs"] == c.K * plan["ksplit"] and plan["per_offset"] == plan["ksplit"] and c.XR < c.R
    elif not direct:
        assert plan["slabs"] == plan["nz"] * plan["ksplit"] and plan["per_offset"] == 1


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", list(wc.DW))
def test_dw_case_reaches_its_arm(name, kind):
    c = wc.DW[name]
    taken, plan = wc.plan_of(_lib(), wc.PLAN_DW, kind, c.K, c.R, 0, c.Cs, c.Cg)
    assert taken == 1
    for field, want in c.plan[kind].items():
        assert plan[field] == want, (name, kind, field, plan)
    assert plan["slabs"] == (plan["ksplit"] if plan["ksplit"] > 1 else 0)
    if kind != "f32":
        assert (plan["ksplit"] > 1) == (c.arm == "split")


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("name", list(wc.LIN))
def test_linear_case_reaches_its_arm(name, kind):
    c = wc.LIN[name]
    taken, fwd = wc.plan_of(_lib(), wc.PLAN_LIN_FWD, kind, 1, c.B, 0, c.I, c.O)
    taken2, dw = wc.plan_of(_lib(), wc.PLAN_LIN_DW, kind, 1, c.B, 0, c.I, c.O)
    assert taken == 1 and taken2 == 1
    assert (fwd["ksplit"], dw["ksplit"]) == c.plan[kind], (name, kind, fwd, dw)
    assert fwd["slabs"] == fwd["ksplit"] and dw["slabs"] == (dw["ksplit"] if dw["ksplit"] > 1 else 0)


def _steps(n, kind):
    gk = 32 if kind == "f32" else 64
    return -(-n // gk), n % gk


def test_every_listed_arm_is_reached():
    """The coverage the suite is there for, from wfs_wide_plan alone."""
    lib = _lib()

    def conv(name, kind):
        c = wc.CONV[name]
        return c, wc.plan_of(lib, wc.PLAN_CONV, kind, c.K, c.R, c.XR, c.Cx, c.Cy, 1 if c.table else 0)[1]

    for kind in wc.KINDS:
        h = kind != "f32"
        c, p = conv("direct", kind)                     # direct store, one partial step
        assert p["nz"] * p["ksplit"] == 1 and not p["dense_first"] and p["slabs"] == 0 and not c.table
        assert _steps(c.Cx, kind) == ((1, 40) if h else (2, 8))
        # smallest R, Cx, Cy, largest K
        assert wc.CONV["R1"].R == 1 and wc.CONV["R1"].Cx == 8 and wc.CONV["K128"].Cx == 8 and wc.CONV["Cy8"].Cy == 8
        assert wc.CONV["K128"].K == 128
        c, p = conv("nseg2", kind)                      # two offsets per block, last batch of one, partial last step
        assert (p["nseg"], p["nz"], p["ksplit"]) == (2, 14, 1) and c.K - (p["nz"] - 1) * p["nseg"] == 1
        assert _steps(c.Cx, kind) == ((2, 8) if h else (3, 8))
        c2, p2 = conv("nseg2_subm", kind)
        assert p2 == p and c2.kmap == "mirror" and c2.ik == 13 and c2.counts and c.counts
        c, p = conv("nseg3", kind)                      # three per block, no short batch, odd step count for 16-bit rows
        assert (p["nseg"], p["nz"]) == (3, 9) and c.K == 27 and _steps(c.Cx, kind)[0] == (1 if h else 2)
        c, p = conv("tails", kind)
        assert (p["nseg"], p["nz"]) == (2, 5) and c.K - 4 * 2 == 1 and c.R % 128 == 1 and c.Cy % 128 == 8
        for name, parts, last in (("split_1100", 9, 76), ("split_1025", 9, 1), ("split_1024", 8, 128)):
            c, p = conv(name, kind)
            assert not p["dense_first"] and p["ksplit"] == (parts if h else {9: 18, 8: 16}[parts] - (name == "split_1025"))
            assert c.Cx - (p["ksplit"] - 1) * p["kchunk"] == (last if h else {76: 12, 1: 1, 128: 64}[last])
        for name, slabs in (("dense_2050", 17), ("dense_1030", 9), ("dense_1030_map", 9)):
            c, p = conv(name, kind)
            assert p["dense_first"] and p["per_offset"] == (slabs if h else 2 * slabs - 1)
            assert p["per_offset"] >= 4 and p["per_offset"] % 4 != 0          # the four-at-a-time loop AND its tail
        assert wc.CONV["dense_1030_map"].kmap == "mirror" and wc.CONV["dense_1030_map"].counts
        # the three product orders of the device-count sweep
        kinds_of = [conv(n, kind)[1] for n in wc.COUNT_CASES]
        assert kinds_of[0]["slabs"] == 0 and kinds_of[1]["slabs"] > 0 and not kinds_of[1]["dense_first"] and kinds_of[2]["dense_first"]
        for n in wc.COUNT_CASES:
            R = wc.CONV[n].R
            assert {0, 1, 127, 128, 129, R - 1, R, R + 1} <= set(wc.CONV[n].counts) | ({127, 128, 129} if R < 129 else set())
        # in place against copy: Cx % 4 == 0 and Cy % 4 == 0 without a table, and dense-first
        assert wc.CONV["split_1100"].Cx % 4 == 0 and wc.CONV["split_1100"].Cy % 4 == 0 and not wc.CONV["split_1100"].table
        assert wc.CONV["dense_1028"].Cx % 4 == 0 and wc.CONV["dense_1028"].Cy % 4 == 0 and conv("dense_1028", kind)[1]["dense_first"]
        assert wc.CONV["direct"].Cy % 4 != 0

        def dw(name):
            c = wc.DW[name]
            return c, wc.plan_of(lib, wc.PLAN_DW, kind, c.K, c.R, 0, c.Cs, c.Cg)[1]

        if h:
            assert dw("R1024")[1]["ksplit"] == 8 and dw("R1023")[1]["ksplit"] == 1          # the 16-bit threshold
        for name, parts in (("split_9", 9), ("split_17", 17), ("split_9_K3", 9)):
            assert dw(name)[1]["ksplit"] == (parts if h else 2 * parts - (name == "split_17"))
        c, p = dw("odd_steps")
        if h:
            assert p["kchunk"] == 192 and p["kchunk"] // 64 == 3
        assert dw("R63")[1]["ksplit"] == 1 and dw("R64")[1]["ksplit"] == 1 and _steps(63, "bf16") == (1, 63)
        c, p = dw("split_9")
        assert p["ksplit"] > 1 and set(c.counts) == {"neg", 0, 1, "kchunk-1", "kchunk", "kchunk+1", c.R - 1, c.R}

        def lin(name):
            c = wc.LIN[name]
            return (wc.plan_of(lib, wc.PLAN_LIN_FWD, kind, 1, c.B, 0, c.I, c.O)[1],
                    wc.plan_of(lib, wc.PLAN_LIN_DW, kind, 1, c.B, 0, c.I, c.O)[1])

        assert (wc.LIN["smallest"].B, wc.LIN["smallest"].I, wc.LIN["smallest"].O) == (1, 256, 9)
        assert lin("dw_split")[1]["ksplit"] == (9 if h else 18)
        f = lin("fwd_split")[0]
        assert f["ksplit"] == (9 if h else 17) and wc.LIN["fwd_split"].B % 128 and wc.LIN["fwd_split"].O % 128
        f = lin("last_part_1")[0]
        assert wc.LIN["last_part_1"].I - (f["ksplit"] - 1) * f["kchunk"] == 1


def test_refused_shapes():
    lib = _lib()
    for kind in wc.KINDS:
        d = wc.DT[kind]
        assert lib.wfs_wide_linear_ok(4, 255, 9, d) == 0 and lib.wfs_wide_linear_ok(4, 256, 8, d) == 0
        assert lib.wfs_wide_linear_ok(1, 256, 9, d) == 1
        assert lib.wfs_wide_conv_ok(9, 100, 100, 7, 128, d) == 0 and lib.wfs_wide_conv_ok(129, 100, 100, 128, 128, d) == 0
        assert lib.wfs_wide_conv_ok(9, 100, 100, 127, 127, d) == 0 and lib.wfs_wide_conv_ok(9, 100, 100, 8, 128, d) == 1
        assert lib.wfs_wide_plan(wc.PLAN_CONV, 9, 100, 100, 7, 128, 1, d, None) == 0          # not taken; out may be NULL
        assert lib.wfs_wide_plan(wc.PLAN_CONV, 9, 100, 100, 127, 127, 1, d, None) == 0
        assert lib.wfs_wide_plan(wc.PLAN_LIN_FWD, 1, 4, 0, 255, 9, 0, d, None) == 0
        assert lib.wfs_wide_plan(wc.PLAN_DW, 9, 100, 0, 100, 100, 1, d, None) == 0
    EINVAL = -1
    for args in ((wc.PLAN_CONV, 129, 100, 100, 128, 128, 1, 0), (wc.PLAN_CONV, 0, 100, 100, 128, 128, 1, 0),
                 (wc.PLAN_CONV, 9, 100, 100, 128, 128, 0, 0), (wc.PLAN_CONV, 1, 100, 99, 128, 128, 0, 0),
                 (wc.PLAN_CONV, 9, 0, 100, 128, 128, 1, 0), (wc.PLAN_CONV, 9, 100, 0, 128, 128, 1, 0),
                 (wc.PLAN_CONV, 9, 100, 100, 128, 128, 1, 3), (4, 9, 100, 100, 128, 128, 1, 0), (-1, 9, 100, 100, 128, 128, 1, 0),
                 (wc.PLAN_DW, 129, 100, 0, 128, 128, 1, 0), (wc.PLAN_DW, 9, 100, 0, 0, 128, 1, 0),
                 (wc.PLAN_LIN_FWD, 1, 0, 0, 256, 9, 0, 0), (wc.PLAN_LIN_FWD, 1, 4, 0, 7, 9, 0, 0), (wc.PLAN_LIN_DW, 1, 4, 0, 256, 0, 0, 0)):
        assert lib.wfs_wide_plan(*args, None) == EINVAL, args


# ---------------------------------------------------------------------------------------------------------- the inputs
def _check_table(c, t, XR):
    assert t.shape == (c.K, c.R) and t.min() >= -1 and t.max() < XR
    live = t >= 0
    if c.ik < 0:
        assert (t == 0).any() and (t == XR - 1).any(), "row 0 and the last source row are read"
        assert live[:, 0].all(), "a destination row with every offset"
    else:
        assert not live[c.ik].any()
    if c.R > 1:
        assert (~live).all(axis=0).any(), "a destination row without a neighbour"


@pytest.mark.parametrize("name", list(wc.CONV))
def test_conv_inputs(name):
    c = wc.CONV[name]
    for kind in wc.KINDS:
        for tr in (False, True):
            p = wc.conv_problem(name, kind, "exact", tr)
            if c.table:
                _check_table(c, p.table, c.XR)
            want, scale = wc.conv_reference(name, kind, "exact", tr)
            assert scale.max() < 2 ** 24 and np.array_equal(want, np.rint(want))
            assert np.abs(p.X).max() <= 3 and np.abs(p.W).max() <= 2 and (p.bias is None or np.abs(p.bias).max() <= 3)
            if c.Cx * (c.K / 2 if c.table else c.K) >= 1000:          # terms of a row: half the table is live
                assert np.abs(want).max() > 256, "a bf16 store of this case never rounds"
            g = wc.conv_problem(name, kind, "gauss", tr)
            assert np.array_equal(g.X, wc.round_to(g.X, kind)) and np.array_equal(g.W, wc.round_to(g.W, kind))
            e = wc.conv_e32(name, kind, tr)
            E32_SEEN[("conv", name, kind, "dX" if tr else "Y")] = e
            assert e <= wc.E32_MAX, (name, kind, tr, e)


def test_the_exact_set_rounds_in_bf16_for_every_16_bit_result():
    """Per product with a 16-bit result (conv forward, conv dX, linear dX): some case's expected values leave the integers
    bf16 holds exactly (|v| > 256); fp16 holds integers to 2048, which the longest sums pass too."""
    for tr in (False, True):
        big = max(np.abs(wc.conv_reference(n, "bf16", "exact", tr)[0]).max() for n in wc.CONV)
        assert big > 256
        assert max(np.abs(wc.conv_reference(n, "f16", "exact", tr)[0]).max() for n in ("dense_2050", "nseg2", "tails")) > 600
    assert np.abs(wc.lin_reference("long_dx", "bf16", "exact")["dX"][0]).max() > 256


@pytest.mark.parametrize("name", list(wc.DW))
def test_dw_inputs(name):
    c = wc.DW[name]
    for kind in wc.KINDS:
        p = wc.dw_problem(name, kind, "exact")
        if c.table:
            _check_table(c, p.table, c.GR)
        for swap in (False, True):
            want, scale = wc.dw_reference(name, kind, "exact", c.R, swap)
            assert scale.max() < 2 ** 24 and np.array_equal(want, np.rint(want)) and np.abs(want).max() > 0
        zero, zs = wc.dw_reference(name, kind, "exact", 0, False)
        assert not zero.any() and not zs.any()
        assert not wc.dw_reference(name, kind, "exact", -5, False)[0].any()          # a negative count is 0 rows
        g = wc.dw_problem(name, kind, "gauss")
        assert np.array_equal(g.S, wc.round_to(g.S, kind)) and np.array_equal(g.G, wc.round_to(g.G, kind))
        e = wc.dw_e32(name, kind)
        E32_SEEN[("dw", name, kind, "dW")] = e
        assert e <= wc.E32_MAX, (name, kind, e)


@pytest.mark.parametrize("name", list(wc.LIN))
def test_linear_inputs(name):
    for kind in wc.KINDS:
        ref = wc.lin_reference(name, kind, "exact")
        for what, (want, scale) in ref.items():
            assert scale.max() < 2 ** 24 and np.array_equal(want, np.rint(want)), what
        g = wc.lin_problem(name, kind, "gauss")
        for a in (g.x, g.W, g.g):
            assert np.array_equal(a, wc.round_to(a, kind))
        for what, e in wc.lin_e32(name, kind).items():
            E32_SEEN[("linear", name, kind, what)] = e
            assert e <= wc.E32_MAX, (name, kind, what, e)


def test_print_e32():
    """The record: e32 per product, case, row type and tensor (pytest -s)."""
    for key, e in sorted(E32_SEEN.items()):
        print("%-7s %-16s %-5s %-3s e32 %.3e" % (key + (e,)))
    assert all(e <= wc.E32_MAX for e in E32_SEEN.values())
