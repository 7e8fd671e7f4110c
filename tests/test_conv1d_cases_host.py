"""The cases of tests/conv1d_cases.py for the dense Conv1d + BatchNorm1d + ReLU stack kernels (csrc/conv1d.hip), checked
on the CPU, every case in every row type, mode and row count it runs in.

* Well-posed: in the float64 run no pre-ReLU value of a layer lies within 1e-5 of that layer's largest magnitude, and
  every layer has between 5 % and 95 % of its ReLUs on.
* Conditioned: torch's own fp32 CPU run is within 3e-6 of float64 on every compared tensor (the kernels are held to
  1e-5), at a seed below 40; building a problem, seed search included, takes well under a second (asserted: 5 s).
* On its arm: wfs_conv1d_arms (host only) and its plain-Python restatement agree, and from its answer and plain
  arithmetic every case reaches the arm it is in the table for.
* In bounds: wfs_conv1d_ok accepts the case; each documented bound is refused one step outside, where both size queries
  return 0 and wfs_conv1d_arms returns WFS_EINVAL.

The arms (the planning constants of csrc/conv1d.hip): position blocks of 256, at most ST_MAXBLK = 512 of them in the
forward, head and role A passes (strided from 131073 positions on); EW_MAXBLK = 2048 blocks in the last forward launch
(from 524289 elements on); dW tiles of DW_TP = 32 positions on at most DW_MAXBLK = 256 blocks per chunk of 256 of the
cin fs + 1 columns; thread groups 256 / columns while the chunk has at most 128; accumulator widths 8 / 16 / 32 / 64;
channel chunks of 8; every bound of the header at its value.
"""
import ctypes
import time

import pytest
import torch

import conv1d_cases as cc


BUILD_SECONDS_MAX = 5.0              # what building one cached float64 problem may take


def _params():
    return [pytest.param(i, kind, mode, nv, id=cc.run_id(i, kind, mode, nv)) for i, kind, mode, nv in cc.case_params()]


def _lib():
    from waveformml_amd import _lib
    return _lib, _lib.load()


def _arms(c):
    L, lib = _lib()
    n = len(c.layers)
    arrays = [L.i32_array(v) for v in cc.plan_arrays(c)]
    out = (ctypes.c_int32 * (10 * n + 1))()
    rc = lib.wfs_conv1d_arms(c.N, c.L, c.c0, *arrays, n, out)
    assert rc == L.WFS_OK, (c.name, rc)
    return [list(out[10 * i: 10 * i + 10]) for i in range(n)] + [[out[10 * n]]]


@pytest.mark.parametrize("i,kind,mode,nv", _params())
def test_case_is_well_posed_and_conditioned(i, kind, mode, nv):
    c = cc.CASES[i]
    rows = cc.rows_of(c, nv)
    t0 = time.time()
    p = cc.problem(i, kind, mode, rows)
    took = time.time() - t0
    assert p.x.dtype == p.dy.dtype == cc.KINDS[kind] and p.x.shape == (rows, c.c0, c.L) and p.rows == rows
    assert len(p.pre) == len(c.layers) and p.seed < cc.MAX_TRIES
    margin, lo, hi = cc.relu_state(p.pre)
    worst = max(p.e32, key=p.e32.get)
    print("%s: seed %d in %.2f s, ReLU margin %.2e, ReLUs on %.2f .. %.2f, worst e32 %.2e (%s)"
          % (cc.run_id(i, kind, mode, nv), p.seed, took, margin, lo, hi, p.e32[worst], worst))
    # a cached problem is built in well under a second, its seed search included (the slowest, st-exact, takes about
    # 0.6 s); the bound is generous so that a loaded machine does not trip it, and a case grown tenfold does
    assert took <= BUILD_SECONDS_MAX, "building the problem took %.1f s" % took
    assert margin >= cc.RELU_MARGIN
    assert 0.05 <= lo and hi <= 0.95
    for n, e in p.e32.items():
        assert e <= cc.E32_MAX, "torch's fp32 run is %.2e of the scale of %s away from float64" % (e, n)
    for n, t in p.ref:                                   # a live problem: nothing is identically zero or not finite
        assert bool(torch.isfinite(t).all()), n
        if not (mode == "train" and n in p.summed):
            assert float(t.abs().max()) > 0, n
    for n, s in p.summed.items():
        assert s > 0, n
    if c.grid:                                           # the grid: exact in the row type, and wide
        assert torch.equal(p.x.double() * 16, (p.x.double() * 16).round()) and float(p.x.double().abs().max()) == 2.0
        assert all(ly.fs == 1 and ly.st == 1 for ly in c.layers) and c.c0 == 2
        first = p.pre[0].permute(0, 2, 1).reshape(-1, c.layers[0].cout)[:, 0]
        assert len(torch.unique(first)) <= 65 * 65
    if "unread samples" in c.arm:                        # exactly zero in float64 at the samples no tap reads
        ly = c.layers[0]
        lout = cc.shapes(c)[0][2]
        read = torch.zeros(c.L, dtype=torch.bool)
        for t in range(lout):
            read[t * ly.st: t * ly.st + ly.fs] = True
        dx = dict(p.ref)["dx"]
        assert int((~read).sum()) >= 3 and not bool(dx[:, :, ~read].any()) and bool(dx[:, :, read].all())


def test_the_two_tensors_that_are_zero_by_algebra_are_where_the_table_says():
    """Only layer 0 of `c1` has cin x fs = 1; there and for every conv bias the training-mode gradient is a residue of
    its terms in float64, in eval mode an ordinary tensor."""
    single = [(c.name, i) for c in cc.CASES for i, (ly, (cin, _l, _o)) in enumerate(zip(c.layers, cc.shapes(c)))
              if cin * ly.fs == 1]
    assert single == [("c1", 0)]
    p = cc.problem(cc.BY_NAME["c1"], "f32", "train")
    assert set(p.summed) == {"L0.conv.weight", "L0.conv.bias", "L1.conv.bias"}
    ref = dict(p.ref)
    assert float(ref["L0.conv.bias"].abs().max()) <= 1e-12 * p.summed["L0.conv.bias"]
    assert float(ref["L0.conv.weight"].abs().max()) <= 1e-3 * p.summed["L0.conv.weight"]
    p = cc.problem(cc.BY_NAME["co-32-64"], "f32", "eval")
    ref = dict(p.ref)
    assert float(ref["L1.conv.bias"].abs().max()) == cc.scale_of("L1.conv.bias", ref["L1.conv.bias"], p.summed, False) > 0


def test_the_library_plans_every_case_as_the_table_says():
    reached = set()
    for c in cc.CASES:
        arms = _arms(c)
        assert arms == cc.arms_py(c), (c.name, arms, cc.arms_py(c))
        tags = cc.tags_of(c, arms)
        assert c.arm <= tags, (c.name, c.arm - tags)
        reached |= tags
    assert reached == cc.REQUIRED
    by = {c.name: _arms(c) for c in cc.CASES}
    # the arms by the numbers the source names:
    # [L_in, L_out, position blocks, role A blocks, cin chunks, dW blocks, column chunks, last chunk, groups, CO], [ew blocks]
    assert by["st-exact"] == [[4096, 4096, 512, 512, 1, 256, 1, 3, 85, 8], [1024]]
    assert by["st-over"] == [[4096, 4096, 512, 512, 1, 256, 1, 3, 85, 8], [4096, 4096, 512, 512, 1, 256, 1, 4, 64, 8], [1056]]
    assert by["ew-exact"][-1] == [2048] and by["ew-over"][-1] == [2048]
    assert by["dw-8160"][0][1:6] == [2720, 32, 32, 1, 256] and by["dw-8192"][0][1:6] == [4096, 32, 32, 1, 256]
    assert by["dw-8193"][0][1:6] == [2731, 33, 33, 1, 256] and by["dw-8193"][1][1:6] == [2730, 32, 33, 1, 256]
    assert by["nv-dw"][0][1:6] == [2731, 43, 43, 1, 256]
    assert by["c1"] == [[40, 40, 1, 1, 1, 8, 1, 2, 128, 8], [40, 40, 1, 1, 1, 8, 1, 4, 64, 8], [1]]
    assert by["g3-85"][0][4:] == [2, 2, 1, 85, 3, 8] and by["g2-86"][0][4:] == [3, 2, 1, 86, 2, 8]
    assert by["g2-127"][0][4:] == [2, 4, 1, 127, 2, 16] and by["g1-129"][0][4:] == [2, 2, 1, 129, 1, 32]
    assert by["one-256"][0][4:] == [7, 2, 1, 256, 1, 16] and by["two-257"][0][4:] == [8, 2, 2, 1, 256, 64]
    assert by["max-1025"][0] == [4, 19, 1, 1, 8, 2, 5, 1, 256, 64]
    assert [a[6:] for a in by["co-32-64"][:3]] == [[1, 10, 25, 32], [1, 65, 3, 64], [1, 65, 3, 8]]
    assert [a[:2] for a in by["st8-k16"][:2]] == [[59, 6], [6, 1]] and by["st-gt-fs"][0][:2] == [30, 6]
    assert [a[:2] for a in by["pd-max"][:2]] == [[4, 19], [19, 5]] and [a[:2] for a in by["L1"][:2]] == [[1, 1], [1, 1]]
    assert [a[1] for a in by["eight"][:8]] == [200, 100, 104, 104, 54, 54, 55, 18]
    assert [a[9] for a in by["eight"][:8]] == [8, 16, 8, 32, 16, 64, 8, 8]
    assert [a[:2] for a in by["nv"][:2]] == [[37, 19], [19, 20]] and by["m2"][0][:3] == [1, 1, 1]
    # 16-bit rows and both modes where the issue asks for them
    for name in ("st-over", "ew-over", "dw-8193", "g2-127", "g1-129", "two-257", "max-1025", "co-32-64", "st8-k16", "st-gt-fs",
                 "pd-max", "L1", "eight", "odd-16", "nv"):
        assert cc.CASES[cc.BY_NAME[name]].kinds == cc.ALL, name
    for name in ("st-over", "max-1025", "co-32-64", "pd-max", "eight", "bn-records"):
        assert cc.CASES[cc.BY_NAME[name]].modes == cc.BOTH, name
    for name in ("st-exact", "st-over", "ew-exact", "ew-over"):
        assert cc.CASES[cc.BY_NAME[name]].grid, name
    # the module case is the plan Conv1DNet builds for `stride-3`
    from waveformml_amd.psd.convnet import conv1d_plan
    c = cc.CASES[cc.BY_NAME["module"]]
    planes, layers, out_size = conv1d_plan(c.L, **cc.MODULE_KW)
    assert planes == [c.c0] + [ly.cout for ly in c.layers]
    assert [l[:3] for l in layers] == [(ly.fs, ly.st, ly.pd) for ly in c.layers]
    assert list(out_size) == [cc.shapes(c)[-1][2], c.layers[-1].cout]


def test_the_library_accepts_every_case_and_refuses_one_step_outside():
    L, lib = _lib()
    OK, BAD = L.WFS_OK, L.WFS_EINVAL

    def ask(N, Lr, c0, layers, dt=0):
        """(wfs_conv1d_ok, saved floats, workspace floats, wfs_conv1d_arms) of a plan [(cout, fs, st, pd)]."""
        arrays = [L.i32_array([ly[j] for ly in layers]) for j in range(4)]
        n = len(layers)
        out = (ctypes.c_int32 * (10 * max(n, 1) + 1))()
        return (lib.wfs_conv1d_ok(c0, *arrays, n, Lr, dt), int(lib.wfs_conv1d_saved_floats(N, Lr, c0, *arrays, n)),
                int(lib.wfs_conv1d_bwd_workspace_floats(N, Lr, c0, *arrays, n)),
                lib.wfs_conv1d_arms(N, Lr, c0, *arrays, n, out))

    for c in cc.CASES:
        plan = [tuple(ly[:4]) for ly in c.layers]
        for kind in c.kinds:
            ok, ns, nw, rc = ask(c.N, c.L, c.c0, plan, list(cc.KINDS).index(kind))
            assert (ok, rc) == (OK, OK) and ns > 0 and nw > 0, c.name
    # the bounds at their values are taken ...
    inside = [
        (2, 59, 64, [(64, 16, 8, 15)]), (2, 4096, 1, [(1, 1, 1, 0)]), (2, 1, 1, [(1, 1, 1, 0)]), (2, 59, 3, [(4, 1, 1, 0)] * 8),
        (2, 14, 3, [(4, 16, 1, 1)]), (2, 59, 3, [(4, 3, 8, 2)]),
    ]
    for N, Lr, c0, layers in inside:
        assert ask(N, Lr, c0, layers)[0::3] == (OK, OK), (N, Lr, c0, layers)
    # ... and refused one step outside: 65 channels (in and out), fs 17 and 0, stride 9 and 0, pd = fs and -1, 9 and 0
    # layers, L 4097 and 0, a kernel that does not fit the row, in the first layer and in the second
    outside = [
        (2, 59, 65, [(4, 3, 1, 1)]), (2, 59, 3, [(65, 3, 1, 1)]), (2, 59, 0, [(4, 3, 1, 1)]), (2, 59, 3, [(0, 3, 1, 1)]),
        (2, 59, 3, [(4, 17, 1, 1)]), (2, 59, 3, [(4, 0, 1, 0)]), (2, 59, 3, [(4, 3, 9, 1)]), (2, 59, 3, [(4, 3, 0, 1)]),
        (2, 59, 3, [(4, 3, 1, 3)]), (2, 59, 3, [(4, 3, 1, -1)]), (2, 59, 3, [(4, 3, 1, 1)] * 9), (2, 59, 3, []),
        (2, 4097, 3, [(4, 3, 1, 1)]), (2, 0, 3, [(4, 1, 1, 0)]), (2, 13, 3, [(4, 16, 1, 1)]),
        (2, 10, 3, [(4, 8, 1, 0), (4, 8, 1, 0)]),
    ]
    for N, Lr, c0, layers in outside:
        assert ask(N, Lr, c0, layers) == (BAD, 0, 0, BAD), (N, Lr, c0, layers)
    # a row count the entry points refuse: wfs_conv1d_ok takes none; the size queries and wfs_conv1d_arms refuse it
    assert ask(-1, 59, 3, [(4, 3, 1, 1)]) == (OK, 0, 0, BAD)
    assert ask((1 << 40) // (4096 * 64) + 1, 59, 3, [(4, 3, 1, 1)]) == (OK, 0, 0, BAD)
    # a bad row type is wfs_conv1d_ok's alone to refuse: the other three take none
    ok, ns, nw, rc = ask(2, 59, 3, [(4, 3, 1, 1)], dt=3)
    assert (ok, rc) == (BAD, OK) and ns > 0 and nw > 0
    # NULL out
    arrays = [L.i32_array([v]) for v in (4, 3, 1, 1)]
    assert lib.wfs_conv1d_arms(2, 59, 3, *arrays, 1, None) == BAD
