"""The cases of tests/dense_cases.py for the dense Conv2d + BatchNorm2d + ReLU stack kernels (csrc/conv2d.hip), checked
on the CPU, every case in every row type and mode it runs in.

* Well-posed: in the float64 run no pre-ReLU value of a layer lies within the case's margin (1e-5 unless the table
  says otherwise) of that layer's largest magnitude, and every layer has between 5 % and 95 % of its ReLUs on.
* Conditioned: torch's own fp32 CPU run is within 3e-6 of float64 on every tensor (the kernels are held to 1e-5); for
  16-bit rows the float64 run with the backward's documented 16-bit operands is within half the row type's bar
  (dense_cases.rounded_backward, itself held against autograd here).
* On its arm: wfs_conv2d_arms (host only) and its plain-Python restatement agree, and from its answer and plain
  arithmetic every case reaches the arm it is in the table for.
* In bounds: wfs_conv2d_ok accepts the case; each documented bound is refused one step outside, where both size
  queries return 0 and wfs_conv2d_arms returns WFS_EINVAL.

The arms (the planning constants of csrc/conv2d.hip): 16 rows per row block, at most NRB_MAX = 256 blocks in the
statistics / g-sum / dz passes (strided from M = 4097 on) and EW_MAXBLK = 1024 in the BN + ReLU pass (from M = 16385
on); 64 channels per block of those passes; dW slices of DW_CHUNK = 2048 positions; GEMM tiles 64 x 64 x 32 in all three
products; every bound of the header at its value.
"""
import ctypes

import pytest
import torch

import dense_cases as dc


def _params():
    return [pytest.param(i, kind, mode, id=dc.run_id(i, kind, mode)) for i, kind, mode in dc.case_params()]


def _lib():
    from waveformml_amd import _lib
    return _lib, _lib.load()


def _arms(c, dt=0):
    L, lib = _lib()
    arrays = [L.i32_array(v) for v in dc.plan_arrays(c)]
    out = (ctypes.c_int32 * (8 * len(c.layers)))()
    rc = lib.wfs_conv2d_arms(c.B, c.H, c.W, c.c0, *arrays, len(c.layers), dt, out)
    assert rc == L.WFS_OK, (c.name, rc)
    return [list(out[8 * i: 8 * i + 8]) for i in range(len(c.layers))]


@pytest.mark.parametrize("i,kind,mode", _params())
def test_case_is_well_posed_and_conditioned(i, kind, mode):
    c = dc.CASES[i]
    p = dc.problem(i, kind, mode)
    assert p.x.dtype == p.dy.dtype == dc.KINDS[kind] and p.x.shape == (c.B, c.c0, c.H, c.W)
    assert len(p.pre) == len(c.layers) and p.seed < dc.MAX_TRIES
    margin, lo, hi = dc.relu_state(p.pre)
    worst = max(p.e32, key=p.e32.get)
    print("%s: seed %d, ReLU margin %.2e, ReLUs on %.2f .. %.2f, worst e32 %.2e (%s)"
          % (dc.run_id(i, kind, mode), p.seed, margin, lo, hi, p.e32[worst], worst))
    assert margin >= c.margin >= dc.RELU_MARGIN
    assert 0.05 <= lo and hi <= 0.95
    for n, e in p.e32.items():
        assert e <= dc.E32_MAX, "torch's fp32 run is %.2e of the scale of %s away from float64" % (e, n)
    assert bool(p.e16) == (kind != "f32")
    for n, e in p.e16.items():
        assert e <= dc.E16_SHARE * dc.wc.TOL[dc.KINDS[kind]], "16-bit operands alone cost %.2e of the scale of %s" % (e, n)
    if p.e16:
        w16 = max(p.e16, key=p.e16.get)
        print("    16-bit operands alone: worst %.2e of the bar (%s)" % (p.e16[w16] / dc.wc.TOL[dc.KINDS[kind]], w16))
    for n, t in p.ref:                                   # a live problem: nothing is identically zero or not finite
        assert bool(torch.isfinite(t).all()), n
        if not (mode == "train" and n in p.bias_scale):
            assert float(t.abs().max()) > 0, n
    for n, s in p.bias_scale.items():
        assert s > 0, n
    if "unread cells of dX" in c.arm:                    # input row H - 1 and column W - 1: exactly zero in float64
        dx = dict(p.ref)["dx"]
        assert not bool(dx[:, :, -1, :].any()) and not bool(dx[:, :, :, -1].any()) and bool(dx[:, :, :-1, :-1].any())
    if c.drop is not None:
        assert [m is not None for m in p.masks] == [q > 0 for q in c.drop]
        kept = float((p.masks[1] > 0).double().mean())
        assert abs(kept - (1 - c.drop[1])) < 0.1


def test_the_library_plans_every_case_as_the_table_says():
    reached = set()
    for c in dc.CASES:
        for dt in (0, 1, 2):
            arms = _arms(c, dt)
            assert arms == dc.arms_py(c), (c.name, arms, dc.arms_py(c))
        tags = dc.tags_of(c, arms)
        assert c.arm <= tags, (c.name, c.arm - tags)
        reached |= tags
    assert reached == dc.REQUIRED
    by = {c.name: _arms(c) for c in dc.CASES}
    # the arms by the numbers the source names: [M, nrb, ew blocks, tiles M, tiles N, K steps, slices, last slice]
    assert by["m2"] == [[2, 1, 1, 1, 1, 1, 1, 2]]
    assert by["nrb-exact"] == [[4096, 256, 256, 64, 1, 1, 2, 2048]]
    assert by["nrb-over"] == [[5120, 256, 320, 80, 1, 1, 3, 1024], [5120, 256, 320, 80, 1, 2, 3, 1024]]
    assert by["ew-exact"][0][:3] == [16384, 256, 1024] and by["ew-over"][0][:3] == [17408, 256, 1024]
    assert by["b2048"][0][:4] == [2048, 128, 128, 32]
    assert by["chunk-64"][0][4] == 1 and by["chunk-65"][0][4] == 2
    assert by["dw-2048"][0][6:] == [1, 2048] and by["dw-2052"][0][6:] == [2, 4]
    assert [by["edge-%d" % m][0][3:6] for m in (63, 64, 65)] == [[1, 1, 2], [1, 1, 2], [2, 2, 3]]
    assert by["k1-n63"][0][5] == 1 and by["chain-31-33"][0][5] == 1 and by["chain-31-33"][2][5] == 2 and by["k32"][0][5] == 1
    assert by["maxc"][0][4:6] == [8, 16] and by["k12800"][0][5] == 400
    # the products of the tile-edge cases, by hand: (M, N, K) of forward, dX and dW
    assert dc.products(dc.CASES[dc.BY_NAME["edge-65"]]) == {"fwd": [(65, 65, 65)], "dx": [(65, 65, 65)], "dw": [(65, 65, 65)]}
    assert dc.products(dc.CASES[dc.BY_NAME["k32"]]) == {"fwd": [(48, 2, 32)], "dx": [(70, 2, 32)], "dw": [(2, 32, 48)]}
    assert dc.products(dc.CASES[dc.BY_NAME["k1-n63"]]) == {"fwd": [(60, 63, 1), (60, 1, 63)], "dx": [(60, 1, 63), (60, 63, 1)],
                                                           "dw": [(63, 1, 60), (1, 63, 60)]}
    # the geometry the issue lists is all there
    for f, vals in (("fs", range(1, 6)), ("st", range(1, 4)), ("dil", range(1, 5))):
        assert {getattr(ly, f) for c in dc.CASES if len(c.kinds) == 3 for ly in c.layers} == set(vals), f
    assert dc.shapes(dc.CASES[dc.BY_NAME["g-max"]]) == [(3, 32, 29, 16, 15), (4, 16, 15, 16, 15)]
    assert dc.shapes(dc.CASES[dc.BY_NAME["to-1x1"]])[-1][3:] == (1, 1)
    # 16-bit rows where the issue asks for them
    for name in ("dw-2052", "nrb-over", "maxc", "eight", "odd-act", "edge-63", "edge-64", "edge-65", "k1-n63", "chain-31-33",
                 "k32", "g-max", "g-st3-d3", "g-d2-k5", "to-1x1", "row-1x32", "col-32x1", "single-st2"):
        assert dc.CASES[dc.BY_NAME[name]].kinds == dc.ALL, name


def test_the_library_accepts_every_case_and_refuses_one_step_outside():
    L, lib = _lib()
    OK, BAD = L.WFS_OK, L.WFS_EINVAL

    def ask(B, H, W, c0, layers, training=0, dt=0):
        """(wfs_conv2d_ok, saved floats, workspace floats, wfs_conv2d_arms) of a plan [(cout, fs, st, pd, dil)]."""
        arrays = [L.i32_array([ly[j] for ly in layers]) for j in range(5)]
        n = len(layers)
        out = (ctypes.c_int32 * (8 * max(n, 1)))()
        return (lib.wfs_conv2d_ok(c0, *arrays, n, B, H, W, training, dt),
                int(lib.wfs_conv2d_saved_floats(B, H, W, c0, *arrays, n, dt)),
                int(lib.wfs_conv2d_bwd_workspace_floats(B, H, W, c0, *arrays, n, dt)),
                lib.wfs_conv2d_arms(B, H, W, c0, *arrays, n, dt, out))

    for c in dc.CASES:
        plan = [tuple(ly[:5]) for ly in c.layers]
        for kind in c.kinds:
            for mode in c.modes:
                ok, ns, nw, rc = ask(c.B, c.H, c.W, c.c0, plan, int(mode == "train"), list(dc.KINDS).index(kind))
                assert (ok, rc) == (OK, OK) and ns > 0 and nw > 0, c.name
    # the bounds at their values are taken ...
    inside = [
        (2, 9, 7, 3, [(4, 5, 1, 0, 1)]), (2, 9, 7, 3, [(4, 3, 3, 0, 1)]), (2, 9, 7, 3, [(4, 2, 1, 0, 4)]),
        (2, 9, 7, 3, [(4, 3, 1, 2, 1)]), (2, 32, 32, 3, [(4, 3, 1, 1, 1)]), (2, 6, 5, 3, [(4, 1, 1, 0, 1)] * 8),
        (2, 3, 3, 512, [(512, 1, 1, 0, 1)]), (2048, 1, 1, 3, [(4, 1, 1, 0, 1)]), (2, 1, 1, 3, [(4, 1, 1, 0, 1)]),
        (2, 5, 9, 3, [(4, 3, 1, 0, 2)]),
    ]
    for B, H, W, c0, layers in inside:
        assert ask(B, H, W, c0, layers, 1)[0::3] == (OK, OK), (B, H, W, c0, layers)
    # ... and refused one step outside: fs 6, stride 4, dilation 5, pd = dil (fs - 1) + 1, H or W 33, 9 layers, 513
    # channels (in and out), B 2049, B 0, a kernel reach that does not fit the map
    outside = [
        (2, 9, 7, 3, [(4, 6, 1, 0, 1)]), (2, 9, 7, 3, [(4, 3, 4, 0, 1)]), (2, 9, 7, 3, [(4, 2, 1, 0, 5)]),
        (2, 9, 7, 3, [(4, 3, 1, 3, 1)]), (2, 9, 7, 3, [(4, 3, 1, 5, 2)]), (2, 33, 32, 3, [(4, 3, 1, 1, 1)]),
        (2, 32, 33, 3, [(4, 3, 1, 1, 1)]), (2, 6, 5, 3, [(4, 1, 1, 0, 1)] * 9), (2, 3, 3, 513, [(4, 1, 1, 0, 1)]),
        (2, 3, 3, 4, [(513, 1, 1, 0, 1)]), (2049, 1, 1, 3, [(4, 1, 1, 0, 1)]), (0, 3, 3, 3, [(4, 1, 1, 0, 1)]),
        (2, 4, 9, 3, [(4, 3, 1, 0, 2)]), (2, 9, 4, 3, [(4, 3, 1, 0, 2)]), (2, 9, 7, 3, [(4, 3, 1, 0, 1), (4, 5, 1, 0, 2)]),
        (2, 9, 7, 3, [(4, 0, 1, 0, 1)]), (2, 9, 7, 3, [(4, 3, 0, 0, 1)]), (2, 9, 7, 3, [(4, 3, 1, -1, 1)]),
    ]
    for B, H, W, c0, layers in outside:
        for training in (0, 1):
            assert ask(B, H, W, c0, layers, training) == (BAD, 0, 0, BAD), (B, H, W, c0, layers)
    assert ask(2, 9, 7, 3, [(4, 3, 1, 0, 1)], 1, dt=3) == (BAD, 0, 0, BAD)
    # a training call with one value per channel is refused (torch raises there); the eval call of the same shape is
    # legal, and the size queries and wfs_conv2d_arms, which take no mode, answer for it
    for B, H, W, layers in ((1, 1, 1, [(4, 1, 1, 0, 1)]), (1, 3, 3, [(4, 1, 1, 0, 1), (4, 3, 1, 0, 1)])):
        assert ask(B, H, W, 3, layers, 1)[0] == BAD
        ok, ns, nw, rc = ask(B, H, W, 3, layers, 0)
        assert (ok, rc) == (OK, OK) and ns > 0 and nw > 0
    assert ask(2, 1, 1, 3, [(4, 1, 1, 0, 1)], 1)[0] == OK
    # NULL out
    arrays = [L.i32_array([v]) for v in (4, 1, 1, 0, 1)]
    assert lib.wfs_conv2d_arms(2, 3, 3, 3, *arrays, 1, 0, None) == BAD


@pytest.mark.parametrize("name,mode", [("eight", "train"), ("eight", "eval"), ("g-max", "train"), ("drop-0-p-0", "train"),
                                       ("bn-records", "eval")])
def test_the_written_out_backward_is_autograd(name, mode):
    """rounded_backward without rounding against the float64 reference: the model the 16-bit condition is taken on."""
    i = dc.BY_NAME[name]
    c, p = dc.CASES[i], dc.problem(i, "f32", mode)
    got = dc.rounded_backward(c, p.net, p.x, p.dy, p.masks, mode == "train", lambda t: t)
    for n, b in p.ref:
        if n in got:
            scale = dc.scale_of(n, b, p.bias_scale, mode == "train")
            assert float((got[n] - b).abs().max()) <= 1e-10 * scale, n
    assert {n for n, _b in p.ref} - set(got) == {"L%d.running_%s" % (l, s) for l in range(len(c.layers)) for s in ("mean", "var")}


def test_the_dropout_reference_is_the_documented_counter():
    """One element of a mask by hand: layer << 44 | ((b C + c) H' + y) W' + x."""
    import numpy as np
    import waveform_cases as wc
    c = dc.CASES[dc.BY_NAME["drop-0-p-0"]]
    m = dc.drop_masks(c)[1]
    assert m.shape == (3, 6, 7, 5)
    ctr = np.array([(1 << 44) | (((2 * 6 + 5) * 7 + 6) * 5 + 4)], dtype=np.uint64)
    assert float(m[2, 5, 6, 4]) == float(wc.hash_masks(dc.DROP_SEED, dc.DROP_P, ctr)[0])
    assert set(np.unique(m.numpy())) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.3)))}


def test_the_densify_references_are_to_dense():
    for d in dc.DENSIFY_CASES:
        coords, rows, n_valid, want = dc.densify_problem(d)
        assert want.shape == (d.B, d.H, d.W, d.C) and want.dtype == dc.KINDS[d.kind] and coords.dtype == torch.int32
        assert (rows.shape[0] > n_valid) == d.counted and bool(torch.isfinite(want.float()).all())
        if d.triple:
            x, y, b = coords[0].tolist()
            hits = [r for r in range(n_valid) if coords[r].tolist() == [x, y, b]]
            assert hits == [0, 3, n_valid - 1]
    assert {(d.H, d.W) for d in dc.DENSIFY_CASES} >= {(1, 32), (32, 1), (32, 32)}
    assert {d.C for d in dc.DENSIFY_CASES} >= {1, 512}
