"""The cases of tests/seq_cases.py for the TCN and Elman-RNN row kernels (csrc/tcnc.hip, csrc/rnn.hip), checked on the
CPU, every case in every row dtype it runs in.

* Live: the three conditions of recurrent_cases.assert_live on the float64 run (for the TCN too, where every gradient
  must be non-zero as well), apart from the gradients a case names as identically zero, which are exactly zero.
* Conditioned: torch's own fp32 CPU run is within 3e-6 of float64 on every tensor (the bound of the BatchNorm host
  test; the kernels are held to 1e-5).
* ReLU-safe: in the float64 run no ReLU's pre-activation is smaller than 1e-5 of its layer's largest.  fp32 moves a
  pre-activation by about 1e-6 of the scale, so no ReLU of a case can fall on the other side in the kernels.  (Exact
  zeros apart: sums of exact zeros -- dropped or dead inputs -- which are zero in any precision; seq_cases.relu_margin.)
* On its arm: the plain-Python statement of the dispatch (seq_cases.rnn_arms / tcn_arms) gives what the table says, and
  across the table every arm that no other test reaches is reached (listed below, an explicit set comparison).
* In bounds: wfs_rnn_ok / wfs_tcnc_ok accept the case and refuse its neighbours just outside.

The arms.  tcnc.hip: the second column slot of k_tcnc_dw (ncol = 257, which also fills Ws and XS); groups == 1 at
ncol = 129 and groups = 2; a first level reading cin > 1 channels in the row dtype, an identity residual read in the row
dtype, a downsample over several 16-bit channels; 8 levels with a dilation longer than the row; L = 1 and L = 4096; the
dropout counter at conv = 15, channel = 31, t = 4095; one live channel in the last 8-channel chunk; cout = 8 | 9, 16 | 17.
rnn.hip: H = 1, 9, 17 and the top of every padded width; the register and the LDS-parked matvec; k_rnn_dw<8 / 16 / 32>;
C = 64 with ncol = 97; I = 32; T = 1, 2, 4096; more than one scan block (one live lane in the last), mix block and
transpose tile along the rows, N = Npad; no dX; two directions without bias; dropout at layer = 6, channel = 63,
t = 4095.
"""
import pytest
import torch

import seq_cases as sc
from recurrent_cases import assert_live


def _rnn_params():
    return [pytest.param(i, kind, id="%s-%s" % (sc.rnn_id(c), kind)) for i, c in enumerate(sc.RNN_CASES) for kind in sc.kinds_of(c)]


def _tcn_params():
    return [pytest.param(i, kind, id="%s-%s" % (sc.tcn_id(c), kind)) for i, c in enumerate(sc.TCN_CASES) for kind in sc.kinds_of(c)]


def _conditioned_and_relu_safe(tag, p, relus):
    e32 = sc.e32_of(p)
    margin = sc.relu_margin(relus)
    print("%s: worst e32 %.2e (%s), ReLU margin %.2e" % (tag, max(e32.values()), max(e32, key=e32.get), margin))
    for n, e in e32.items():
        assert e <= sc.E32_MAX, "%s: torch's fp32 run is %.2e of max|%s| away from float64" % (tag, e, n)
    assert margin >= sc.RELU_MARGIN, "%s: a ReLU pre-activation at %.2e of its layer's largest" % (tag, margin)


@pytest.mark.parametrize("i,kind", _rnn_params())
def test_rnn_case_is_live_conditioned_and_relu_safe(i, kind):
    c = sc.RNN_CASES[i]
    p = sc.rnn_problem(i, kind)
    assert p.x.dtype == p.dy.dtype == sc.KINDS[kind] and p.x.shape[0] == c.N
    zero = [(n, t) for n, t in p.ref if any(z in n for z in c.zero)]
    assert len(zero) == (c.case[3] * c.case[4] if c.zero else 0)
    for n, t in zero:
        assert not bool(t.any()), "%s is identically zero in float64" % n
    assert_live([(n, t) for n, t in p.ref if not any(z in n for z in c.zero)])
    assert float(p.hidden.abs().max()) > 0 and p.hidden.shape == p.h32.shape
    assert len(p.pre) == c.case[3] * c.case[4]
    _conditioned_and_relu_safe(sc.rnn_id(c) + " " + kind, p, [z for _l, _d, z in p.pre] if c.case[5] == "relu" else [])
    eh = float((p.h32.double() - p.hidden).abs().max()) / float(p.hidden.abs().max())
    assert eh <= sc.E32_MAX, eh


@pytest.mark.parametrize("i,kind", _tcn_params())
def test_tcn_case_is_live_conditioned_and_relu_safe(i, kind):
    c = sc.TCN_CASES[i]
    c0, channels, k, L = c.case
    p = sc.tcn_problem(i, kind)
    assert p.x.dtype == p.dy.dtype == sc.KINDS[kind] and p.x.shape == (c.N, c0, L)
    assert_live(p.ref)                                        # every gradient among them: none may be identically zero
    _masks, dw = p.extra
    assert len(dw) == 2 * len(channels)
    for ci, g in enumerate(dw):                                # [cout, cin, k]: tap j reads the sample (k - 1 - j) d back
        d = 1 << (ci // 2)
        for j in range(k):
            off = (k - 1 - j) * d >= L
            assert bool(g[:, :, j].any()) != off, "conv %d tap %d: zero exactly when it falls off the row" % (ci, j)
    if L == 1:
        assert all(not bool(g[:, :, :-1].any()) and bool(g[:, :, -1].any()) for g in dw)
    assert len(p.pre) == 3 * len(channels)
    _conditioned_and_relu_safe(sc.tcn_id(c) + " " + kind, p, [z for _lv, _n, z in p.pre])


def test_every_case_is_on_its_arm_and_every_untested_arm_is_reached():
    reached = set()
    for c in sc.RNN_CASES:
        assert sc.rnn_arms(c.case, c.N) == c.arms, (sc.rnn_id(c), sc.rnn_arms(c.case, c.N))
        reached |= sc.rnn_tags(c)
    assert sc.RNN_REQUIRED - reached == set() and reached - sc.RNN_REQUIRED == set()
    reached = set()
    for c in sc.TCN_CASES:
        assert sc.tcn_arms(c.case) == c.arms, (sc.tcn_id(c), sc.tcn_arms(c.case))
        reached |= sc.tcn_tags(c)
    assert sc.TCN_REQUIRED - reached == set() and reached - sc.TCN_REQUIRED == set()
    # the arms by the numbers the sources name
    by = {sc.rnn_id(c): c for c in sc.RNN_CASES}
    assert by["33-1-9-2-1-relu-True-N65"].arms["scan_blocks"] == 2 and 65 % sc.SCAN_TB == 1
    assert by["9-32-32-2-2-tanh-True-N257"].arms["ncol"] == [65, 97] and by["9-32-32-2-2-tanh-True-N257"].arms["mix_blocks"] == 2
    assert [c.arms["HP"] for c in sc.RNN_CASES[:10]] == [4, 4, 8, 16, 16, 32, 32, 32, 8, 4]
    slot1 = [sc.tcn_id(c) for c in sc.TCN_CASES if any(a[2] for a in c.arms)]
    assert slot1 == ["1-32-32-8-40-N3", "32-32-8-33-N2"]
    assert {a[3] for c in sc.TCN_CASES for a in c.arms} == {8, 16, 32}
    assert {a[4] for c in sc.TCN_CASES for a in c.arms} == {0, 1, 4, 5}


def test_the_library_accepts_every_case_and_refuses_its_neighbours():
    from waveformml_amd import _lib
    lib = _lib.load()
    OK, BAD = _lib.WFS_OK, _lib.WFS_EINVAL
    nl = {"relu": _lib.WFS_RNN_RELU, "tanh": _lib.WFS_RNN_TANH}
    for c in sc.RNN_CASES:
        T, I, H, layers, dirs, nonlin, _b = c.case
        for dt in (_lib.WFS_F32, _lib.WFS_BF16, _lib.WFS_F16):
            assert lib.wfs_rnn_ok(I, H, layers, dirs, nl[nonlin], T, dt) == OK, sc.rnn_id(c)
        assert lib.wfs_rnn_ok(I, 33, layers, dirs, nl[nonlin], T, 0) == BAD
        assert lib.wfs_rnn_ok(33, H, layers, dirs, nl[nonlin], T, 0) == BAD
        assert lib.wfs_rnn_ok(I, H, layers, dirs, nl[nonlin], 4097, 0) == BAD
        assert lib.wfs_rnn_ok(I, H, 9, dirs, nl[nonlin], T, 0) == BAD
        assert lib.wfs_rnn_saved_floats(c.N, T, I, H, layers, dirs) == (c.N + 63) // 64 * 64 * T * (I + layers * dirs * H)
    for c in sc.TCN_CASES:
        c0, channels, k, L = c.case
        ch, lv = _lib.i32_array(channels), len(channels)
        for dt in (_lib.WFS_F32, _lib.WFS_BF16, _lib.WFS_F16):
            assert lib.wfs_tcnc_ok(c0, ch, lv, k, L, dt) == OK, sc.tcn_id(c)
        assert lib.wfs_tcnc_ok(c0, ch, lv, 9, L, 0) == BAD
        assert lib.wfs_tcnc_ok(c0, ch, lv, k, 4097, 0) == BAD
        assert lib.wfs_tcnc_ok(33, ch, lv, k, L, 0) == BAD
        assert lib.wfs_tcnc_ok(c0, _lib.i32_array(channels[:-1] + [33]), lv, k, L, 0) == BAD
        assert lib.wfs_tcnc_ok(c0, _lib.i32_array((channels * 9)[:9]), 9, k, L, 0) == BAD
        assert lib.wfs_tcnc_n_conv(c0, ch, lv, k) == len(c.arms)
        assert lib.wfs_tcnc_saved_floats(c.N, L, c0, ch, lv) == 3 * c.N * L * sum(channels)


def test_the_moved_dropout_references_are_the_documented_counters():
    """One element of each mask by hand: the counter's fields at their edges land where the layouts say."""
    import numpy as np
    import waveform_cases as wc
    m = sc.rnn_hash_masks(sc.DROP_SEED, sc.DROP_P, 3, 64, 6, 6)
    ctr = np.array([(((2 << 3 | 6) << 6 | 63) << 12) | 5], dtype=np.uint64)
    assert m.shape == (3, 6, 64) and float(m[2, 5, 63]) == float(wc.hash_masks(sc.DROP_SEED, sc.DROP_P, ctr)[0])
    m = sc.tcn_hash_masks(sc.DROP_SEED, sc.DROP_P, 2, 32, 64, 15)
    ctr = np.array([(((1 << 4 | 15) << 5 | 31) << 12) | 63], dtype=np.uint64)
    assert m.shape == (2, 32, 64) and float(m[1, 31, 63]) == float(wc.hash_masks(sc.DROP_SEED, sc.DROP_P, ctr)[0])
    for m in (sc.rnn_hash_masks(sc.DROP_SEED, sc.DROP_P, 2, 4, 4096, 0), sc.tcn_hash_masks(sc.DROP_SEED, sc.DROP_P, 2, 4, 4096, 1)):
        kept = float((m > 0).double().mean())
        assert abs(kept - 0.7) < 0.02 and set(np.unique(m.numpy())) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.3)))}
