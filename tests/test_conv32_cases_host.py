"""The float64 references, the packed-table encoder and the case table of tests/conv32_cases.py, checked on the CPU.

The references take a table as it is; here they meet the fp32 C oracle (oracle/spconv_ref.c) on rulebooks the oracle
builds for a SubM layer and for the strided (1, 1, 4) layer, in every form the kernels are called with: by-output and
by-input tables, the centre offset as identity_k with its entries wiped, the SubM mirror map, transposed filters, the
swapped 32 x 2 dW, and a valid-row count below a capacity padded with NaN rows.  Bar: the project's fp32 bar, 1e-5 of
each element's own sum of absolute terms.
"""
import numpy as np
import pytest

import conv32_cases as cc
from helpers import rand_coords

GEO = {"subm": dict(ksize=3, stride=1, subm=True), "strided": dict(ksize=3, stride=(1, 1, 4), subm=False)}
SHAPE, BATCH, SITES = (14, 11, 32), 3, 420


def _close(got, want32, scale, what):
    r = cc.ratio(np.asarray(want32, np.float64), got, scale)          # the fp32 oracle against float64
    assert r <= 1.0, "%s: the oracle is %.3g of the fp32 bar away from the float64 reference" % (what, r)


@pytest.fixture(scope="module", params=sorted(GEO))
def book(request):
    """A rulebook of the oracle and its two gather tables."""
    from oracle import ref
    g = GEO[request.param]
    rng = np.random.default_rng(31)
    idx = rand_coords(rng, BATCH, SHAPE, SITES)
    out, pairs, num = ref.get_indice_pairs(idx, BATCH, list(SHAPE), g["ksize"], g["stride"], 0, 1, 0, g["subm"])
    K, N, M = pairs.shape[1], idx.shape[0], len(out)
    by_in = np.full((K, N), -1, np.int32)
    by_out = np.full((K, M), -1, np.int32)
    for k in range(K):
        n = int(num[k])
        by_in[k, pairs[0, k, :n]] = pairs[1, k, :n]
        by_out[k, pairs[1, k, :n]] = pairs[0, k, :n]
    return dict(name=request.param, subm=g["subm"], pairs=pairs, num=num, K=K, N=N, M=M, by_in=by_in, by_out=by_out, rng=rng,
                centre=K // 2 if g["subm"] else -1)


def _values(rng, rows, cin, cout, K):
    X = rng.standard_normal((rows, cin)).astype(np.float32)
    W = (rng.standard_normal((K, cin, cout)) * 0.25).astype(np.float32)
    return X, W


def _wiped(table, k):
    t = table.copy()
    if k >= 0:
        t[k] = -1
    return t


@pytest.mark.parametrize("chan", [(32, 32), (2, 32)])
def test_forward_reference_agrees_with_the_oracle(book, chan):
    from oracle import ref
    b = book
    K, N, M, ik = b["K"], b["N"], b["M"], b["centre"]
    X, W = _values(np.random.default_rng(5), N, chan[0], chan[1], K)
    bias = np.random.default_rng(6).standard_normal(chan[1]).astype(np.float32)
    want = ref.indice_conv(X, W, b["pairs"], b["num"], M, subm=b["subm"])
    got, scale = cc.ref_gather_conv(b["by_out"], None, K, -1, M, M, X, W, False, None)
    assert float(np.abs(got).max()) > 0
    _close(got, want, scale, "by-output table")
    got_b, scale_b = cc.ref_gather_conv(b["by_out"], None, K, -1, M, M, X, W, False, bias)
    _close(got_b, want.astype(np.float64) + bias, scale_b, "with bias")
    assert np.allclose(scale_b, scale + np.abs(bias.astype(np.float64)), rtol=1e-13, atol=0)
    if b["subm"]:
        # the centre offset as identity_k, its entries wiped: the row itself must be taken
        got_i, scale_i = cc.ref_gather_conv(_wiped(b["by_out"], ik), None, K, ik, M, M, X, W, False, None)
        _close(got_i, want, scale_i, "identity_k with wiped entries")
        # the by-input table under the SubM mirror map is the by-output table
        mirror = [K - 1 - k for k in range(K)]
        got_m, scale_m = cc.ref_gather_conv(_wiped(b["by_in"], ik), mirror, K, ik, M, M, X, W, False, None)
        _close(got_m, want, scale_m, "mirror map")
        assert not np.array_equal(b["by_in"], b["by_out"])
    # a capacity above the valid rows: garbage columns point at NaN rows, X rows beyond the inputs are NaN
    cap = M + 37
    Xp = np.concatenate([X, np.full((5, chan[0]), np.nan, np.float32)])
    tp = np.concatenate([b["by_out"], np.full((K, cap - M), N + 2, np.int32)], axis=1)
    got_p, scale_p = cc.ref_gather_conv(tp, None, K, -1, cap, M, Xp, W, False, None)
    _close(got_p[:M], want, scale_p[:M], "valid rows of a padded table")
    assert not got_p[M:].any() and np.isfinite(got_p).all()


def test_backward_reference_agrees_with_the_oracle(book):
    from oracle import ref
    b = book
    K, N, M, ik = b["K"], b["N"], b["M"], b["centre"]
    rng = np.random.default_rng(8)
    X, W = _values(rng, N, 32, 32, K)
    dY = rng.standard_normal((M, 32)).astype(np.float32)
    want_dx, want_dw = ref.indice_conv_backward(X, W, dY, b["pairs"], b["num"], subm=b["subm"])
    dX, aX, dW, aW = cc.ref_conv_backward(_wiped(b["by_in"], ik), K, ik, N, N, X, dY, W)
    assert float(np.abs(dX).max()) > 0 and float(np.abs(dW).max()) > 0
    _close(dX, want_dx, aX, "dX")
    _close(dW, want_dw, aW, "dW")
    # the same dX as a transposed gather; the swapped dW is the transpose
    dX2, aX2 = cc.ref_gather_conv(_wiped(b["by_in"], ik), None, K, ik, N, N, dY, W, True, None)
    assert np.array_equal(dX2, dX) and np.array_equal(aX2, aX)
    dWs, aWs = cc.ref_gather_dw(_wiped(b["by_in"], ik), None, K, ik, N, N, X, dY, True)
    assert np.array_equal(dWs, dW.transpose(0, 2, 1)) and np.array_equal(aWs, aW.transpose(0, 2, 1))
    assert not np.allclose(dW, dW.transpose(0, 2, 1))
    # padded: X and dY rows beyond the valid ones are NaN, the garbage columns point at them
    cap = N + 21
    Xp = np.concatenate([X, np.full((cap - N, 32), np.nan, np.float32)])
    dYp = np.concatenate([dY, np.full((4, 32), np.nan, np.float32)])
    tp = np.concatenate([_wiped(b["by_in"], ik), np.full((K, cap - N), M + 1, np.int32)], axis=1)
    tp[ik if ik >= 0 else 0, N:] = -1
    dXp, aXp, dWp, aWp = cc.ref_conv_backward(tp, K, ik, cap, N, Xp, dYp, W)
    _close(dXp[:N], want_dx, aXp[:N], "dX, padded")
    _close(dWp, want_dw, aWp, "dW, padded")
    assert not dXp[N:].any()


def test_first_layer_dw_reference_agrees_with_the_oracle(book):
    """The 32 x 2 product as the first layer runs it: the 32-channel dY rows stationary, the 2-channel inputs gathered
    through the by-output table (SubM: the by-input one under the mirror map), swapped into [K, Cin, Cout]."""
    from oracle import ref
    b = book
    K, N, M, ik = b["K"], b["N"], b["M"], b["centre"]
    rng = np.random.default_rng(9)
    X, W = _values(rng, N, 2, 32, K)
    dY = rng.standard_normal((M, 32)).astype(np.float32)
    _dx, want_dw = ref.indice_conv_backward(X, W, dY, b["pairs"], b["num"], subm=b["subm"])
    dW, aW = cc.ref_gather_dw(_wiped(b["by_out"], ik), None, K, ik, M, M, dY, X, True)
    assert dW.shape == (K, 2, 32)
    _close(dW, want_dw, aW, "32 x 2 dW")
    if b["subm"]:
        mirror = [K - 1 - k for k in range(K)]
        dWm, aWm = cc.ref_gather_dw(_wiped(b["by_in"], ik), mirror, K, ik, M, M, dY, X, True)
        _close(dWm, want_dw, aWm, "32 x 2 dW, mirror map")


def test_a_column_map_names_the_table_column_of_an_offset():
    """kmap[k] is the table column that serves offset k: the reference on a table whose columns were moved to kmap[k]
    equals the reference on the original table without a map (a map applied the other way round differs)."""
    rng = np.random.default_rng(12)
    K, R, N = 9, 50, 40
    t = rng.integers(-1, N, (K, R)).astype(np.int32)
    X, W = _values(rng, N, 2, 32, K)
    perm = [int(v) for v in rng.permutation(K)]
    inverse = [perm.index(k) for k in range(K)]
    assert perm != inverse
    moved = np.empty_like(t)
    for k in range(K):
        moved[perm[k]] = t[k]
    want, _a = cc.ref_gather_conv(t, None, K, -1, R, R, X, W, False, None)
    got, _a = cc.ref_gather_conv(moved, perm, K, -1, R, R, X, W, False, None)
    assert np.array_equal(got, want)
    wrong, _a = cc.ref_gather_conv(moved, inverse, K, -1, R, R, X, W, False, None)
    assert not np.array_equal(wrong, want)
    S = rng.standard_normal((R, 32))
    want, _a = cc.ref_gather_dw(t, None, K, -1, R, R, S, X, False)
    got, _a = cc.ref_gather_dw(moved, perm, K, -1, R, R, S, X, False)
    assert np.array_equal(got, want)


def _decode_like_the_build_tests(packed, kl):
    """Dense [K, N] from the packed table: entry = row << 3 | offset along the last kernel dim (written out on its own)."""
    Kq, N = packed.shape
    dense = np.full((Kq * kl, N), -1, np.int32)
    for q in range(Kq):
        e = packed[q]
        for o in range(kl):
            hit = (e >= 0) & ((e & 7) == o)
            dense[q * kl + o, hit] = e[hit] >> 3
    return dense


def test_packed_encoder_round_trips(book):
    rng = np.random.default_rng(3)
    t, _facts = cc.build_table(rng, "random", 27, 500, 500, 400, -1, True)
    assert (t >= 0).any(axis=1).all(), "every offset is used"
    p = cc.encode_packed(t)
    assert p.shape == (9, 500) and p.dtype == np.int32
    assert np.array_equal(_decode_like_the_build_tests(p, 3), t) and np.array_equal(cc.decode_packed(p, 27), t)
    live = p >= 0
    assert set(np.unique(p[live] & 7).tolist()) == {0, 1, 2} and (p[~live] == -1).all()
    with pytest.raises(AssertionError):
        cc.encode_packed(np.zeros((27, 4), np.int32))          # three entries per leading offset
    if not book["subm"]:
        # the strided (1, 1, 4) layer's by-input table is packable: kernel 3 <= stride 4 along the last dimension
        pk = cc.encode_packed(book["by_in"])
        assert np.array_equal(_decode_like_the_build_tests(pk, 3), book["by_in"]) and (book["by_in"] >= 0).any()


def test_builders_reach_every_wanted_active_count():
    assert cc.active_counts_wanted(27) == [1, 2, 3, 4, 5, 6, 7, 27]
    assert cc.active_counts_wanted(3) == [1, 2, 3]


@pytest.mark.parametrize("kind", cc.KINDS)
def test_every_case_has_its_structure_and_is_live(kind):
    cases = cc.cases_for(kind)
    assert 40 <= len(cases), len(cases)
    for c in cases:
        p = cc.make_problem(c.name, kind)
        cc.check_structure(c, p)
        for a in (p.A, p.B, p.W):
            if a is not None and kind != "f32":
                fin = np.isfinite(a)
                assert np.array_equal(cc.round_to(np.where(fin, a, 0), kind)[fin], a[fin]), "inputs are rounded to the row type"
        for what, (want, scale) in cc.reference(c.name, kind).items():
            assert np.isfinite(want).all() and np.isfinite(scale).all(), (c.name, what)
            assert (scale >= np.abs(want) * (1 - 1e-12)).all()
            rows_out = what in ("Y", "dX")
            if rows_out:
                assert not want[p.valid:].any() and not scale[p.valid:].any()
            if c.all_zero_ok:
                assert p.valid == 0 and not want.any()
                continue
            assert float(np.abs(want).max()) > 0, (c.name, what)
            if c.builder != "dead" and what == "dW":
                # every offset with a source has a gradient
                t = cc.decode_packed(p.packed, c.K) if c.packed else p.table
                for k in range(c.K):
                    col = k if p.kmap is None else p.kmap[k]
                    used = k == c.identity_k or (t[col, :p.valid] >= 0).any()
                    assert used == bool(np.abs(want[k]).max() > 0), (c.name, k)
        if c.identity_k >= 0 and not c.all_zero_ok:
            # the identity offset carries weight: without it every tensor differs
            t, ref = p.table, cc.reference(c.name, kind)
            if c.op in ("conv32", "c2c32"):
                other = {"Y": cc.ref_gather_conv(t, p.kmap, c.K, -1, c.R, p.valid, p.B, p.W, c.transpose_w, p.bias)}
            elif c.op in ("dw32", "dw32x2"):
                other = {"dW": cc.ref_gather_dw(t, p.kmap, c.K, -1, c.R, p.valid, p.A, p.B, c.swap)}
            else:
                dX, aX, dW, aW = cc.ref_conv_backward(t, c.K, -1, c.R, p.valid, p.A, p.B, p.W)
                other = {"dX": (dX, aX), "dW": (dW, aW)}
            for what in ref:
                assert not np.array_equal(other[what][0], ref[what][0]), (c.name, what)


def test_case_table_covers_the_axes_the_launchers_branch_on():
    names = set(cc.BY_NAME)
    for R in (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 16385, cc.BIG32, cc.MID16, cc.BIG16):
        assert "conv32-R%d" % R in names
    for K in (1, 2, 3, 8, 9, 26, 28, 32):
        assert "conv32-K%d" % K in names
    f32 = {c.name for c in cc.cases_for("f32")}
    h16 = {c.name for c in cc.cases_for("bf16")}
    assert "conv32-R%d" % cc.BIG32 in f32 and "conv32-R%d" % cc.BIG16 not in f32
    assert "conv32-R%d" % cc.BIG16 in h16 and "conv32-R%d" % cc.MID16 in h16 and "conv32-R%d" % cc.MID16 not in f32
    assert (cc.BIG32 + 15) // 16 > 256 * 16 and (cc.BIG16 + 31) // 32 > 256 * 16 and (46112 + 31) // 32 > 1440
    assert (16385 + 15) // 16 > 1024 and (16385 + 31) // 32 > 64 * 8 and (cc.MID16 + 31) // 32 > 1024
    for c in cc.CASES:
        if c.R >= cc.BIG32:
            assert c.K == 27 and c.builder == "random" and not c.packed          # the largest cases stay sparse
