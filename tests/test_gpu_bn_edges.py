"""The sparse-row BatchNorm (+ ReLU) kernels of csrc/bn.hip at every dispatch arm against float64: the register-resident
kernels (k_bn_reduce_rr / k_bn_apply_rr / k_bn_bwd_apply_rr, 2 .. 16 rows per thread, both block sums), the loop
kernels (k_bn_reduce / k_bn_apply / k_bn_bwd_apply, VEC 4 and VEC 1) and the column-block kernels (k_bnw_*), through
wfs_bn_relu_fwd / wfs_bn_relu_bwd and ctypes on raw device tensors, for fp32, bf16 and fp16 rows.

Cases, inputs and the float64 reference: tests/bn_cases.py; tests/test_bn_cases_host.py proves every case well-posed
on the CPU (ReLU margin, fp32 conditioning e32 <= 3e-6) and that it reaches the arm it is there for (wfs_bn_plan).
Every call gets a workspace of exactly wfs_bn_workspace_bytes filled with NaN, outputs filled with a sentinel (rows)
or NaN (per-channel tensors) and num_batches_tracked preset to 41.  Bars:
  save_mean, save_invstd, running_mean, running_var, dgamma, dbeta (fp32 in every row type)
        |got - want| <= 1e-5 max|want|          the project's fp32 bar; the host test keeps plain fp32 3x below it
  y, dX   |got - want| <= 1e-5 max|want| + u |want| per element, u = 0 / 2^-8 / 2^-11 (fp32 / bf16 / fp16): fp32
        arithmetic and ONE round to nearest on the store
  a reference that is identically zero (dX and dgamma of a single row) must be met exactly
Structure: y == 0 exactly where the reference is 0 (ReLU); rows at and beyond a device-side count keep the sentinel;
every output is finite; num_batches_tracked grows by one in training and not at all in eval; eval leaves the running
statistics as they were.

The worst ratio of every (family, direction, row type) is printed when the module ends and written to
$WFS_BN_EDGES_REPORT when that is set (the table of DESIGN.md section 4).
"""
import os

import numpy as np
import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DT = {"f32": 0, "bf16": 1, "f16": 2}
SENT = -768.0                      # exactly representable in bf16 and fp16
FWD_TENSORS = ("save_mean", "save_invstd", "running_mean", "running_var", "y")
WORST = {}                         # (family, direction, kind) -> [worst ratio of the per-channel tensors, of the rows]


def _L():
    from waveformml_amd import _lib
    return _lib


def _t(a, dtype=None):
    if a is None:
        return None
    t = torch.tensor(a, device=DEV)                    # a copy: the problems are shared and read-only
    return t.to(dtype) if dtype is not None else t


def _family(c, kind, backward):
    fam = _L().load().wfs_bn_plan(c.N, c.C, DT[kind], 1 if c.training else 0, 1 if backward else 0, None, None)
    assert fam in bc.FAMILY_NAMES, fam
    return bc.FAMILY_NAMES[fam]


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    lines = ["# worst |got - want| / bar per kernel family, direction and row type (<= 1 passes):",
             "# the fp32-held per-channel tensors, then the rows (y forward, dX backward)"]
    lines += ["%-18s %-8s %-5s %.4f %.4f" % (fam, d, kind, r[0], r[1]) for (fam, d, kind), r in sorted(WORST.items())]
    text = "\n".join(lines)
    print("\n" + text)
    path = os.environ.get("WFS_BN_EDGES_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


def _nan_ws(nbytes):
    assert nbytes % 4 == 0 and nbytes > 0
    return torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)


def run_case(name, kind):
    """One forward and one backward call through the C ABI.  Returns ({tensor: device tensor}, problem)."""
    L = _L()
    lib = L.load()
    p = bc.make_problem(name, kind)
    c = p.case
    cap, C, dt = c.N, c.C, TORCH[kind]
    X, dY = _t(p.x, dt), _t(p.g, dt)
    gamma, beta, rm, rv = _t(p.gamma), _t(p.beta), _t(p.rm), _t(p.rv)
    tracked = torch.tensor([bc.TRACKED0], dtype=torch.int64, device=DEV)
    n_dev = torch.tensor([p.valid], dtype=torch.int64, device=DEV) if p.padded else None
    nbytes = int(lib.wfs_bn_workspace_bytes(cap, C))
    Y = torch.full((cap, C), SENT, dtype=dt, device=DEV)
    dX = torch.full((cap, C), SENT, dtype=dt, device=DEV)
    ch = {t: torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
          for t in ("save_mean", "save_invstd", "dgamma", "dbeta")}
    training, relu = (1 if c.training else 0), (1 if c.relu else 0)
    ws = _nan_ws(nbytes)
    L.check(lib.wfs_bn_relu_fwd(L.ptr(X), cap, C, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(tracked),
                                bc.MOMENTUM, bc.EPS, training, relu, L.ptr(Y), L.ptr(ch["save_mean"]),
                                L.ptr(ch["save_invstd"]), L.ptr(ws), nbytes, DT[kind], L.ptr(n_dev), L.stream_ptr()))
    ws2 = _nan_ws(nbytes)
    L.check(lib.wfs_bn_relu_bwd(L.ptr(X), L.ptr(dY), cap, C, L.ptr(gamma), L.ptr(beta), L.ptr(ch["save_mean"]),
                                L.ptr(ch["save_invstd"]), training, relu, L.ptr(dX), L.ptr(ch["dgamma"]),
                                L.ptr(ch["dbeta"]), L.ptr(ws2), nbytes, DT[kind], L.ptr(n_dev), L.stream_ptr()))
    torch.cuda.synchronize()
    out = dict(ch, y=Y, dX=dX, tracked=tracked)
    if rm is not None:
        out["running_mean"], out["running_var"] = rm, rv
    return out, p


def check_case(name, kind, out, p):
    """Every assertion of the module docstring on one case; returns {tensor: ratio to its bar}."""
    c, n = p.case, p.valid
    ref = bc.reference_of(name, kind)
    want = bc.wanted(ref)
    got = {t: out[t].float().cpu().numpy().astype(np.float64) for t in want}
    for t in ("y", "dX"):
        assert bool((out[t][n:] == SENT).all()), "%s: a row at or beyond the valid count was written" % t
    res = {}
    for t, w in want.items():
        if t in bc.ROW_TENSORS:
            res[t] = bc.ratio_rows(got[t][:n], w[:n], bc.U_ROUND[kind])
        else:
            res[t] = bc.ratio_f32(got[t], w)
        assert np.isfinite(got[t][:n] if t in bc.ROW_TENSORS else got[t]).all(), "%s is not finite" % t
    print("%s %s [%s | %s]: %s" % (name, kind, _family(c, kind, False), _family(c, kind, True),
                                   "  ".join("%s %.4f" % kv for kv in sorted(res.items()))))
    for t, r in res.items():
        key = (_family(c, kind, t not in FWD_TENSORS), "forward" if t in FWD_TENSORS else "backward", kind)
        pair = WORST.setdefault(key, [0.0, 0.0])
        i = 1 if t in bc.ROW_TENSORS else 0
        pair[i] = max(pair[i], r)
    for t, r in sorted(res.items()):
        assert r <= 1.0, "%s %s %s: worst error is %.4g of its bar" % (name, kind, t, r)
    if c.relu:
        assert np.array_equal(got["y"][:n] == 0, want["y"][:n] == 0), "y is zero exactly where the reference is"
    assert int(out["tracked"].item()) == bc.TRACKED0 + (1 if c.training else 0)
    if not c.training:
        assert np.array_equal(out["running_mean"].cpu().numpy(), p.rm) and np.array_equal(out["running_var"].cpu().numpy(), p.rv)
    return res


def _params():
    return [pytest.param(c.name, kind, id="%s-%s" % (c.name, kind)) for kind in bc.KINDS for c in bc.cases_for(kind)]


@pytest.mark.parametrize("name,kind", _params())
def test_case_against_float64(name, kind):
    out, p = run_case(name, kind)
    check_case(name, kind, out, p)


# one case per family and direction: register-resident on either block sum, the fp32 backward that has left the
# registers while its forward stays, both loop kernels at their partial caps, the column blocks at their chunk cap
TWICE = ("rr_serial-C124-N1025", "rr_lanes-C64-N4097", "rr_serial-C124-N8192", "loop4-C124-N8193", "loop1-C7-N65537",
         "column-C130-N8193", "count-C124-N1100-v700", "eval-C130-N33")


@pytest.mark.parametrize("kind", bc.KINDS)
def test_two_identical_calls_are_bit_identical(kind):
    seen = set()
    for name in TWICE:
        c = bc.BY_NAME[name]
        seen |= {(_family(c, kind, False), "forward"), (_family(c, kind, True), "backward")}
        a, _p = run_case(name, kind)
        b, _p = run_case(name, kind)
        for t in a:
            assert torch.equal(a[t].view(torch.uint8), b[t].view(torch.uint8)), (name, t)
    names = [bc.FAMILY_NAMES[f] for f in (bc.COLUMN, bc.RR, bc.LOOP4, bc.LOOP1)]
    assert seen == {(f, d) for f in names for d in ("forward", "backward")}


def test_a_count_equal_to_the_capacity_is_the_call_without_a_count():
    """n_dev == capacity and n_dev == NULL run the same kernels on the same rows: the same bits."""
    L = _L()
    lib = L.load()
    for name in ("count-C124-N1100-v1100", "count-C124-N8193-v8193", "count-C7-N300-v300", "count-C130-N200-v200"):
        out, p = run_case(name, "bf16")
        c = p.case
        X = _t(p.x, torch.bfloat16)
        Y = torch.full((c.N, c.C), SENT, dtype=torch.bfloat16, device=DEV)
        sm, si = torch.empty(c.C, device=DEV), torch.empty(c.C, device=DEV)
        nbytes = int(lib.wfs_bn_workspace_bytes(c.N, c.C))
        ws, gamma, beta = _nan_ws(nbytes), _t(p.gamma), _t(p.beta)
        L.check(lib.wfs_bn_relu_fwd(L.ptr(X), c.N, c.C, L.ptr(gamma), L.ptr(beta), None, None, None, bc.MOMENTUM,
                                    bc.EPS, 1, 1, L.ptr(Y), L.ptr(sm), L.ptr(si), L.ptr(ws), nbytes, DT["bf16"], None,
                                    L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(Y.view(torch.int16), out["y"].view(torch.int16)), name
        assert torch.equal(sm, out["save_mean"]) and torch.equal(si, out["save_invstd"]), name
