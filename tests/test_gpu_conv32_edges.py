"""The 32-channel conv kernels of csrc/conv_mfma.hip at their dispatch edges against float64: the 32 -> 32 products
(k_gconv16_split / k_gconv16_f32 / k_gconv32_bf16, k_gdw32_split / k_gdw32 / k_gdw32_bf16, the one-launch backward
k_bwd32_split / k_bwd32_bf16), the 2 -> 32 forward (k_gconv_c2c32_f32 / _bf16 / k_gconv_c2c32) and the 32 x 2 dW
(k_gdw_c32c2_f32 / _bf16), with the slab reductions behind them, through spconv/functional.py's gather_conv, gather_dw
and conv_backward for fp32, bf16 and fp16 rows.

Cases, table builders and the float64 references: tests/conv32_cases.py (pinned on the CPU by
tests/test_conv32_cases_host.py).  Rows are rounded to the row type on the host and fed to both sides; for 16-bit rows
the filters are rounded too.  Bars, EVERY element held to its own (scale = the element's sum of absolute terms):
  fp32 outputs -- Y and dX of fp32 rows on either arithmetic, every dW --     |err| <= 1e-5 scale
  16-bit outputs -- Y and dX of 16-bit rows --                                 |err| <= u |want| + 1e-5 scale,
      u = 2^-8 (bf16), 2^-11 (fp16): one round-to-nearest of the stored value on top of the fp32 accumulation (the unit
      roundoff of 8 and 11 significant bits; half of it cannot be met by any kernel that stores in the row type)
  dW of the long sums (row counts above 10 000): max(1e-5, 2 e32) of the scale, e32 = the error of a plain fp32
  evaluation of the same reference on the CPU against float64 (recorded in the report)
  an element whose bar is 0 (no term at all: dW with no valid row, a row without a neighbour) must be exact
Rows at or beyond a device-side row count must come back as they went in, bit for bit.

The fp32-instruction kernels (WFS_SPLIT_BF16=0: k_gconv16_f32, k_gdw32<float>, the two-launch backward) run in ONE
child process, because the library reads the switch once: this file run as a script writes its worst ratios to a JSON
file and the parent asserts on it.

The worst ratio of every (family, row type, tensor) is printed when the module ends and written to
$WFS_CONV32_EDGES_REPORT when that is set: profiles/conv32_edges_errors.txt.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conv32_cases as cc          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENT = -768.0                      # exactly representable in bf16 and fp16
WORST = {}                         # (family, kind, tensor) -> worst ratio
E32 = {}                           # (case, kind) -> e32 of its dW


def _L():
    from waveformml_amd import _lib
    return _lib


def _fsp():
    from waveformml_amd.spconv import functional as Fsp
    return Fsp


def _t(a, kind=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(TORCH[kind]) if kind else t


def family(case, kind, split=True):
    """The kernel family the dispatchers of csrc/gather_conv.hip send a case to."""
    K, f32 = case.K, kind == "f32"
    known_map = case.kmap in (None, "ident", "mirror")
    if case.op == "conv32":
        if f32:
            return "gconv16_split" if (split and K <= 27) else "gconv16_f32"
        return "gconv32_h16" if K <= 27 else "gconv_generic"
    if case.op == "c2c32":
        fast = known_map and (K <= 27 if f32 else K <= 32)
        return "c2c32_mfma" if fast else "c2c32_any_map"
    if case.op == "dw32":
        return ("gdw32_split" if split else "gdw32_f32") if f32 else "gdw32_h16"
    if case.op == "dw32x2":
        return "gdw_c32c2" if K <= 27 else "gdw_generic"
    fused = K <= 27 and (split or not f32) and (not case.packed or K % 3 == 0)
    if fused:
        return "bwd32_split" if f32 else "bwd32_h16"
    return "bwd32_two_launch"


def _note(case, kind, what, r, split=True):
    key = (family(case, kind, split), kind, what)
    WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    text = _report_text(WORST, E32)
    print("\n" + text)
    path = os.environ.get("WFS_CONV32_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


def _report_text(worst, e32):
    lines = ["# worst |got - want| / bar per kernel family, row type and tensor (<= 1 passes)"]
    lines += ["%-24s %-5s %-3s %.4f" % (fam, kind, what, r) for (fam, kind, what), r in sorted(worst.items())]
    if e32:
        lines.append("# e32 of the long dW sums (plain fp32 on the CPU against float64, of the element's scale; bar 1e-5)")
        lines += ["%-28s %-5s %.3e" % (name, kind, v) for (name, kind), v in sorted(e32.items())]
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------ running
def _device_problem(p):
    c, kind = p.case, p.kind
    L = _L()
    d = dict(table=_t(p.packed if c.packed else p.table), A=_t(p.A, kind), B=_t(p.B, kind), W=_t(p.W), bias=_t(p.bias),
             kmap=L.i32_array(p.kmap) if p.kmap is not None else None,
             r_dev=torch.tensor([p.valid], dtype=torch.int64, device=DEV) if p.padded else None,
             pk=cc.PACKED_KL if c.packed else 0)
    return d


def _raw_gather_conv(p, d):
    """lib.wfs_gather_conv as Fsp.gather_conv calls it, into a caller's Y prefilled with a sentinel."""
    L = _L()
    lib = L.load()
    c = p.case
    Cw_in, Cw_out = int(d["W"].shape[1]), int(d["W"].shape[2])
    Cy = Cw_in if c.transpose_w else Cw_out
    Y = torch.full((c.R, Cy), SENT, dtype=TORCH[p.kind], device=DEV)
    L.check(lib.wfs_gather_conv(L.ptr(d["table"]), d["kmap"], c.K, c.identity_k, c.R, L.ptr(d["B"]), d["B"].shape[0],
                                d["B"].shape[1], L.ptr(d["W"]), Cw_in, Cw_out, 1 if c.transpose_w else 0, L.ptr(d["bias"]),
                                L.ptr(Y), L.dtype_code(d["B"]), L.ptr(d["r_dev"]), d["pk"], L.stream_ptr()))
    return Y


def _raw_conv_backward(p, d):
    """lib.wfs_conv_backward as Fsp.conv_backward calls it, into a caller's dX prefilled with a sentinel."""
    L = _L()
    lib = L.load()
    c = p.case
    dX = torch.full((c.R, 32), SENT, dtype=TORCH[p.kind], device=DEV)
    dW = torch.full((c.K, 32, 32), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty((max(int(lib.wfs_gather_dw_workspace_bytes(c.K, c.R, 32, 32)), 1),), dtype=torch.uint8, device=DEV)
    L.check(lib.wfs_conv_backward(L.ptr(d["table"]), c.K, c.identity_k, c.R, L.ptr(d["A"]), L.ptr(d["B"]), d["B"].shape[0],
                                  32, 32, L.ptr(d["W"]), L.ptr(dX), L.ptr(dW), L.dtype_code(d["A"]), L.ptr(ws), ws.numel(),
                                  L.ptr(d["r_dev"]), None, d["pk"], L.stream_ptr()))
    return dX, dW


def _untouched(rows, what):
    assert bool((rows == SENT).all()), "%s: a row at or beyond the valid count was written" % what


def run_case(name, kind):
    """One case through spconv/functional.py (and, with a device-side count, through the C entry point into
    sentinel-filled rows).  Returns {tensor: numpy array} with the rows beyond the valid count cut off."""
    Fsp = _fsp()
    p = cc.make_problem(name, kind)
    c, V = p.case, p.valid
    d = _device_problem(p)
    out = {}
    if c.op in ("conv32", "c2c32"):
        Y = Fsp.gather_conv(d["table"], d["kmap"], c.K, c.identity_k, c.R, d["B"], d["W"], c.transpose_w, d["bias"], d["r_dev"],
                            None, d["pk"])
        if p.padded:
            Ys = _raw_gather_conv(p, d)
            torch.cuda.synchronize()
            _untouched(Ys[V:], name)
            assert torch.equal(Ys[:V], Y[:V]), "the same call twice"
        out["Y"] = Y[:V]
    elif c.op in ("dw32", "dw32x2"):
        out["dW"] = Fsp.gather_dw(d["table"], c.K, c.identity_k, c.R, d["A"], d["B"], c.swap, d["kmap"], d["r_dev"], None,
                                  d["pk"])
    else:
        dX, dW = Fsp.conv_backward(d["table"], c.K, c.identity_k, c.R, d["A"], d["B"], d["W"], d["r_dev"], None, d["pk"])
        if p.padded:
            dXs, dWs = _raw_conv_backward(p, d)
            torch.cuda.synchronize()
            _untouched(dXs[V:], name)
            assert torch.equal(dXs[:V], dX[:V]) and torch.equal(dWs, dW), "the same call twice"
        out["dX"], out["dW"] = dX[:V], dW
    torch.cuda.synchronize()
    return {k: v.float().cpu().numpy() for k, v in out.items()}


def ratios_of(name, kind, got):
    """{tensor: worst |err| / bar} of one case; the e32 clause for the dW of the long sums."""
    p = cc.make_problem(name, kind)
    ref = cc.reference(name, kind)
    res = {}
    for what, g in got.items():
        want, scale = ref[what]
        if what in ("Y", "dX"):
            want, scale = want[:p.valid], scale[:p.valid]
        u = cc.U_ROUND[kind] if what in ("Y", "dX") else 0.0
        r = cc.ratio(g, want, scale, u)
        if what == "dW" and p.case.long_sum:
            e32 = cc.e32_of(name, kind)
            E32[(name, kind)] = e32
            r = r / max(1.0, 2.0 * e32 / cc.BAR32)
        res[what] = r
    return res


def _params():
    return [pytest.param(c.name, kind, id="%s-%s" % (c.name, kind)) for kind in cc.KINDS for c in cc.cases_for(kind)]


RESULTS = {}                       # (case, kind) -> ratios, one GPU run per case and module


def _ratios_once(name, kind):
    if (name, kind) not in RESULTS:
        from waveformml_amd.spconv import functional as Fsp
        assert Fsp.SPLIT_BF16, "this suite runs the default arithmetic; the child process runs WFS_SPLIT_BF16=0"
        case = cc.BY_NAME[name]
        cc.check_structure(case, cc.make_problem(name, kind))
        res = ratios_of(name, kind, run_case(name, kind))
        print("%s %s [%s]: %s" % (name, kind, family(case, kind), "  ".join("%s %.4f" % kv for kv in sorted(res.items()))))
        for what, r in res.items():
            _note(case, kind, what, r)
        RESULTS[(name, kind)] = res
    return RESULTS[(name, kind)]


@pytest.mark.parametrize("name,kind", _params())
def test_case_against_float64(name, kind):
    for what, r in _ratios_once(name, kind).items():
        assert r <= 1.0, "%s %s %s: worst error is %.4g of its bar" % (name, kind, what, r)


# -------------------------------------------------------------------------------------------------- filter rounding
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_16bit_kernels_round_the_filters_to_nearest_even(kind):
    """Filters handed over unrounded: the 32 -> 32 and 2 -> 32 kernels must stage them as round-to-nearest-even does
    (the reference rounds them so).  A truncating conversion is off by up to 2^-8 (bf16) of every term."""
    Fsp = _fsp()
    for name in ("conv32-ik13", "conv32-tr", "c2c32-mirror_ik13"):
        p = cc.make_problem(name, kind)
        c = p.case
        rng = np.random.default_rng(99)
        W = (rng.standard_normal(p.W.shape) * 0.25).astype(np.float32)
        assert not np.array_equal(cc.round_to(W, kind), W)
        d = _device_problem(p)
        Y = Fsp.gather_conv(d["table"], d["kmap"], c.K, c.identity_k, c.R, d["B"], _t(W), c.transpose_w, d["bias"])
        want, scale = cc.ref_gather_conv(p.table, p.kmap, c.K, c.identity_k, c.R, p.valid, p.B, cc.round_to(W, kind),
                                         c.transpose_w, p.bias)
        r = cc.ratio(Y.float().cpu().numpy(), want, scale, cc.U_ROUND[kind])
        print("%s %s, unrounded filters: %.4f" % (name, kind, r))
        WORST[("filters_rne:" + c.op, kind, "Y")] = max(WORST.get(("filters_rne:" + c.op, kind, "Y"), 0.0), r)
        assert r <= 1.0, "%s %s: %.4g of the bar with filters rounded to nearest even" % (name, kind, r)


# ------------------------------------------------------------------------------------------------- non-finite inputs
def _inf_problem(K):
    """A small fp32 case with one gathered row = +Inf in channel 5 and zero elsewhere, referenced by a few output rows
    through ONE offset each (so that an fp32 product gives one signed Inf, not Inf - Inf)."""
    p = cc.make_problem("conv32-K%d" % K if K != 27 else "conv32-R129", "f32")
    c = p.case
    table = p.table.copy()
    j, ch = 7, 5
    table[table == j] = -1
    rows = np.arange(3, c.R, 17)
    ks = (np.arange(len(rows)) * 5) % K
    table[ks, rows] = j
    X = p.B.copy()
    X[j] = 0.0
    X[j, ch] = np.inf
    sign = np.sign(p.W[ks, ch, :].astype(np.float64))            # [rows, 32]
    assert (sign != 0).all()
    return p, table, X, rows, sign


def _inf_run(K):
    Fsp = _fsp()
    p, table, X, rows, sign = _inf_problem(K)
    c = p.case
    Y = Fsp.gather_conv(_t(table), None, c.K, -1, c.R, _t(X), _t(p.W), False, _t(p.bias)).cpu().numpy().astype(np.float64)
    Xz = X.copy()
    Xz[7] = 0.0                                                   # the other rows: as if the Inf row were zero
    want, scale = cc.ref_gather_conv(table, None, c.K, -1, c.R, p.valid, Xz, p.W, False, p.bias)
    others = np.setdiff1d(np.arange(c.R), rows)
    r = cc.ratio(Y[others], want[others], scale[others])
    return Y[rows], sign, r


def test_an_inf_input_on_the_three_piece_path():
    """include/wfsparse.h: non-finite inputs give NaN on the three-piece path; every other row is unharmed."""
    hit, _sign, r = _inf_run(27)
    assert not np.isfinite(hit).any(), "every element of a row that gathers the Inf row is non-finite"
    assert r <= 1.0, "rows that do not gather the Inf row: %.4g of the bar" % r


@pytest.mark.parametrize("K", [28, 32])
def test_fp32_rows_with_more_than_27_offsets_take_the_fp32_instructions(K):
    """K = 28 and 32 do not fit the three-piece kernel's LDS: the dispatcher must send fp32 rows to k_gconv16_f32 even
    with the split on -- seen from outside by an Inf input giving exactly +-Inf with the filter element's sign."""
    hit, sign, r = _inf_run(K)
    assert np.array_equal(hit, sign * np.inf)
    assert r <= 1.0


# ----------------------------------------------------------------------------------------------------- deferred dW
def test_deferred_dw_of_two_jobs_in_one_reduction():
    """A 32 x 32 job (13 slabs) and a 32 x 2 job (65 slabs: the 32-slice form) queued together and reduced by ONE
    k_slab_reduce_multi4 launch: float64 bars, and bit-identical to the undeferred results."""
    Fsp = _fsp()
    kind = "f32"
    names = ("dw32-R16385", "dw32x2-R16385")
    plain = {}
    for n in names:
        p = cc.make_problem(n, kind)
        d = _device_problem(p)
        plain[n] = Fsp.gather_dw(d["table"], p.case.K, -1, p.case.R, d["A"], d["B"], p.case.swap)
    sizes = [27 * 32 * 32, 27 * 32 * 2]
    flat_p = torch.zeros((sum(sizes),), device=DEV)
    flat_g = torch.full((sum(sizes),), float("nan"), device=DEV)
    likes = [flat_p[:sizes[0]].view(27, 32, 32), flat_p[sizes[0]:].view(27, 32, 2)]
    Fsp.register_grad_slots(flat_p, flat_g)
    Fsp.defer_dw(True)
    try:
        got, keep = {}, []
        for n, like in zip(names, likes):
            p = cc.make_problem(n, kind)
            d = _device_problem(p)
            keep.append(d)
            got[n] = Fsp.gather_dw(d["table"], p.case.K, -1, p.case.R, d["A"], d["B"], p.case.swap, None, None, like)
            assert got[n].data_ptr() >= flat_g.data_ptr() and got[n]._base is not None
        slabs = sorted(int(j.nslabs) for j, _ws in Fsp._DEFERRED_DW)
        assert len(slabs) == 2 and slabs[0] <= 64 < slabs[1], slabs
        torch.cuda.synchronize()
        assert bool(torch.isnan(flat_g).all()), "nothing is written before the flush"
        Fsp.flush_deferred_dw()
        torch.cuda.synchronize()
    finally:
        Fsp.defer_dw(False)
        Fsp.reset_grad_slots()
    for n in names:
        assert torch.equal(got[n], plain[n]), n
        res = ratios_of(n, kind, {"dW": got[n].cpu().numpy()})
        print("%s deferred: dW %.4f" % (n, res["dW"]))
        WORST[("slab_reduce_multi4", kind, "dW")] = max(WORST.get(("slab_reduce_multi4", kind, "dW"), 0.0), res["dW"])
        assert res["dW"] <= 1.0


# ------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("kind", cc.KINDS)
def test_two_identical_calls_are_bit_identical(kind):
    big = cc.BIG32 if kind == "f32" else cc.BIG16
    for name in ("conv32-R%d" % big, "bwd32-R%d" % big):
        a, b = run_case(name, kind), run_case(name, kind)
        for what in a:
            assert np.array_equal(a[what].view(np.int32), b[what].view(np.int32)), (name, what)


# ------------------------------------------------------------------------------------- the fp32-instruction kernels
CHILD_OPS = ("conv32", "dw32", "bwd32")


def _child_cases():
    return [c.name for c in cc.cases_for("f32") if c.op in CHILD_OPS]


def _child_main(out_path):
    """WFS_SPLIT_BF16=0: the fp32 cases of the 32 -> 32 products on the fp32 matrix instructions; conv_backward takes
    its two-launch route.  Writes the ratios; the parent asserts."""
    Fsp = _fsp()
    assert os.environ.get("WFS_SPLIT_BF16") == "0" and Fsp.SPLIT_BF16 is False
    assert not Fsp._one_launch_rows(torch.float32)
    res = {"split": Fsp.SPLIT_BF16, "cases": {}, "e32": {}}
    for name in _child_cases():
        cc.check_structure(cc.BY_NAME[name], cc.make_problem(name, "f32"))
        res["cases"][name] = ratios_of(name, "f32", run_case(name, "f32"))
    res["e32"] = {n: v for (n, _k), v in E32.items()}
    hit, sign, r = _inf_run(27)
    res["inf_exact"] = bool(np.array_equal(hit, sign * np.inf))
    res["inf_others"] = r
    a, b = run_case("bwd32-R%d" % cc.BIG32, "f32"), run_case("bwd32-R%d" % cc.BIG32, "f32")
    res["deterministic"] = all(np.array_equal(a[w].view(np.int32), b[w].view(np.int32)) for w in a)
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_fp32_instruction_kernels_in_a_child_process(tmp_path):
    """k_gconv16_f32, k_gdw32<float> and the two-launch fp32 backward (WFS_SPLIT_BF16=0), every fp32 case of the
    32 -> 32 products, in one fresh process; an Inf input must come out as exactly +-Inf there, which also shows that
    the child ran the fp32 instructions and not the three-piece kernels (those give NaN)."""
    out = tmp_path / "split_off.json"
    env = dict(os.environ)
    env["WFS_SPLIT_BF16"] = "0"
    env.pop("WFS_CONV32_EDGES_REPORT", None)
    done = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, cwd=ROOT, timeout=420,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    res = json.loads(out.read_text())
    assert res["split"] is False
    assert sorted(res["cases"]) == sorted(_child_cases()) and len(res["cases"]) >= 30
    for name, r in sorted(res["cases"].items()):
        print("%s f32 [split off]: %s" % (name, "  ".join("%s %.4f" % kv for kv in sorted(r.items()))))
        for what, v in r.items():
            _note(cc.BY_NAME[name], "f32", what, v, split=False)
    for name, v in res["e32"].items():
        E32[(name + " [split off]", "f32")] = v
    bad = {(n, w): v for n, r in res["cases"].items() for w, v in r.items() if not v <= 1.0}
    assert not bad, bad
    assert res["inf_exact"], "an Inf input must give exactly +-Inf with the filter element's sign on the fp32 instructions"
    assert res["inf_others"] <= 1.0 and res["deterministic"]


if __name__ == "__main__":
    _child_main(sys.argv[1])
