"""First conv (2 -> 32) + BatchNorm (+ ReLU) backward without a dz tensor (include/wfsparse.h
wfs_first_conv_bn_backward; csrc/conv_mfma.hip k_gdw_bnapply_c32c2 behind bn.hip's reduce launch).

Kernel level: every case is compared with float64 computed from the same 16-bit inputs (the ReLU mask taken from the
kernels' fp32 expression, everything else in float64) and with the existing three-launch route (wfs_bn_relu_bwd +
wfs_gather_dw) on the same inputs.  The bars:
  * the new route's maximum error relative to the tensor's scale, on dW, dgamma and dbeta, is no larger than the
    existing route's in the same case;
  * dgamma / dbeta lie within fp32 summation-order distance of the existing route: that route adds at most 64 terms in
    one chain (16 rows per thread, an 8-step tree, 32 + 8 partials) and rounds xhat and the product once each, so its
    distance from the exact sum is at most (64 + 3) 2^-24 sum_r |g xhat|; the bar is 72 2^-24 sum_r |g xhat| (sum_r |g|);
  * and, since the new route is built to do the existing route's arithmetic in the existing route's order, its three
    results equal the existing route's bit for bit (which implies the two bars above).
Shapes: R in {1, 31, 32, 33, 257} (the tile edge, fewer tiles than waves, a second block, empty waves), a capacity above
the valid count with NaN / poisoned padding, K = 27 with the SubM mirror, K = 9, a strided conv's table
(identity_k = -1), ReLU on / off, affine parameters present / None, bf16 / fp16, a channel the ReLU masks entirely and a
channel whose mean is 30 sigma, 16 417 rows (65 slabs: the second stage's 32-slice form, and the reduce launch's
register-resident kernel with 4 rows per thread) and 131 105 rows: the smallest count at which a wave takes a second
tile (512 blocks of 8 waves).

Module level (a 4-event, 64-sample C2 net): a captured step and the same padded step run eagerly give bit-identical
gradients; gradients of fp16 rows against the CPU oracle stay within the bar test_gpu_parity.py's
test_c4_deep_stack_config_matches_the_cpu_path uses for 16-bit rows (relative L2 error of every parameter gradient below
0.15); the fused node and the separate launches SparseSequential issued before it give the same outputs, statistics and
gradients bit for bit, both for the layer it covers and for each it does not (conv bias, input requiring grad, fp32
rows, eval-mode BatchNorm)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}
EPS = 1e-5
MASKED_CH, FAR_CH = 3, 5


def _fsp():
    from waveformml_amd.spconv import functional as Fsp
    return Fsp


def _L():
    from waveformml_amd import _lib
    return _lib


def _round(a, kind):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH[kind]).float().numpy()


class Case(object):
    def __init__(self, name, R, cap=None, K=27, table="mirror", kind="bf16", relu=True, affine=True):
        self.name, self.R, self.cap, self.K, self.table = name, R, (R if cap is None else cap), K, table
        self.kind, self.relu, self.affine = kind, relu, affine


CASES = [Case("R1", 1), Case("R31", 31), Case("R32", 32), Case("R33", 33), Case("R257", 257),
         Case("padded", 257, cap=300), Case("padded-R33-f16", 33, cap=97, kind="f16"),
         Case("K9", 257, K=9), Case("strided", 257, table="plain"), Case("strided-padded", 100, cap=140, table="plain"),
         Case("norelu", 257, relu=False), Case("noaffine", 257, affine=False),
         Case("norelu-noaffine-f16", 257, relu=False, affine=False, kind="f16"), Case("f16", 257, kind="f16"),
         Case("K9-f16-norelu", 65, K=9, kind="f16", relu=False), Case("many-slabs", 16417),
         Case("two-tiles", 131105)]
_PROBLEMS = {}


def problem(case):
    """Inputs (numpy, already rounded to the row type), the float64 results and the device tensors of a case."""
    if case.name in _PROBLEMS:
        return _PROBLEMS[case.name]
    rng = np.random.default_rng(sum(map(ord, case.name)) * 7919 + case.R)
    R, cap, K = case.R, case.cap, case.K
    subm = case.table == "mirror"
    n_in = cap + 1 if subm else 3 * cap + 6             # the last input row is poison: only padding points at it
    X = _round(rng.standard_normal((n_in, 2)), case.kind)
    X[n_in - 1] = np.nan
    table = rng.integers(0, n_in - 1, size=(K, cap)).astype(np.int32)
    table[rng.random((K, cap)) < 0.3] = -1
    table[:, R:] = n_in - 1                              # padding rows of the table: the poison row
    ident = K // 2 if subm else -1
    mean_c = rng.uniform(-1.0, 1.0, 32)
    std_c = rng.uniform(0.5, 2.0, 32)
    mean_c[FAR_CH] = 30.0 * std_c[FAR_CH]
    z = _round(mean_c + std_c * rng.standard_normal((cap, 32)), case.kind)
    dY = _round(rng.standard_normal((cap, 32)), case.kind)
    z[R:], dY[R:] = np.nan, np.nan
    gamma = (rng.uniform(0.5, 1.5, 32) * np.where(rng.random(32) < 0.25, -1.0, 1.0)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(32)).astype(np.float32)
    gamma[MASKED_CH], beta[MASKED_CH] = 0.5, -50.0       # the ReLU masks this channel in every row
    zv = z[:R].astype(np.float64)
    mean = zv.mean(0).astype(np.float32)
    invstd = (1.0 / np.sqrt(zv.var(0) + EPS)).astype(np.float32)
    ga = gamma if case.affine else np.ones(32, np.float32)
    be = beta if case.affine else np.zeros(32, np.float32)
    # the mask as the kernels decide it: xhat in fp32, then the sign of the exactly evaluated fma (float64 holds the
    # product of two floats exactly, and rounding a sum never changes its sign)
    xh32 = ((z[:R] - mean) * invstd).astype(np.float32)
    keep = (ga.astype(np.float64) * xh32.astype(np.float64) + be.astype(np.float64) > 0) if case.relu else np.ones((R, 32), bool)
    xhat = (zv - mean.astype(np.float64)) * invstd.astype(np.float64)
    g = np.where(keep, dY[:R].astype(np.float64), 0.0)
    sg, sgx = g.sum(0), (g * xhat).sum(0)
    dz = ga.astype(np.float64) * invstd.astype(np.float64) * (g - sg / R - xhat * sgx / R)
    kmap = [K - 1 - k for k in range(K)] if subm else None
    xg = np.zeros((R, K, 2))
    for k in range(K):
        col = table[kmap[k] if kmap else k, :R]
        rows = np.where(col >= 0, col, 0)
        xg[:, k] = np.where((col >= 0)[:, None], X[rows].astype(np.float64), 0.0)
        if k == ident:
            xg[:, k] = X[:R].astype(np.float64)
    p = dict(case=case, ident=ident, kmap=kmap, n_in=n_in,
             dW=np.einsum("rkc,ro->kco", xg, dz), dgamma=sgx, dbeta=sg,
             abs_gx=np.abs(g * xhat).sum(0), abs_g=np.abs(g).sum(0))
    dt = TORCH[case.kind]
    p["dev"] = dict(X=torch.from_numpy(X).to(DEV).to(dt), z=torch.from_numpy(z).to(DEV).to(dt),
                    dY=torch.from_numpy(dY).to(DEV).to(dt), table=torch.from_numpy(table).to(DEV),
                    gamma=torch.from_numpy(gamma).to(DEV) if case.affine else None,
                    beta=torch.from_numpy(beta).to(DEV) if case.affine else None,
                    mean=torch.from_numpy(mean).to(DEV), invstd=torch.from_numpy(invstd).to(DEV),
                    r_dev=torch.tensor([R], dtype=torch.int64, device=DEV) if cap != R else None,
                    filters=torch.zeros((K, 2, 32), device=DEV))
    _PROBLEMS[case.name] = p
    return p


def run_new(p, filters=None, gamma=None, beta=None):
    Fsp, d, case = _fsp(), p["dev"], p["case"]
    kmap = _L().i32_array(p["kmap"]) if p["kmap"] else None
    return Fsp.first_conv_bn_backward(d["table"], kmap, case.K, p["ident"], case.cap, d["z"], d["dY"], d["X"],
                                      d["gamma"] if gamma is None else gamma, d["beta"] if beta is None else beta,
                                      d["mean"], d["invstd"], case.relu, d["r_dev"],
                                      d["filters"] if filters is None else filters)


def run_old(p):
    Fsp, d, case = _fsp(), p["dev"], p["case"]
    kmap = _L().i32_array(p["kmap"]) if p["kmap"] else None
    dz, dgamma, dbeta = Fsp.bn_relu_backward(d["z"], d["dY"], d["gamma"], d["beta"], d["mean"], d["invstd"], True,
                                             case.relu, d["r_dev"])
    dW = Fsp.gather_dw(d["table"], case.K, p["ident"], case.cap, dz, d["X"], True, kmap, d["r_dev"])
    return dW, dgamma, dbeta


def rel_err(got, ref):
    got = got.detach().double().cpu().numpy()
    assert np.isfinite(got).all(), "padding (NaN) reached a result"
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_against_float64_and_the_three_launch_route(case):
    p = problem(case)
    new, old = run_new(p), run_old(p)
    torch.cuda.synchronize()
    for name, n, o in zip(("dW", "dgamma", "dbeta"), new, old):
        if n is None:
            assert o is None and not case.affine
            continue
        e_new, e_old = rel_err(n, p[name]), rel_err(o, p[name])
        print("%s %s: new %.3e  three-launch %.3e" % (case.name, name, e_new, e_old))
        assert e_new <= e_old, (name, e_new, e_old)
        assert torch.equal(n, o), "%s differs from the three-launch route" % name
    if case.affine:
        for name, bound in (("dgamma", "abs_gx"), ("dbeta", "abs_g")):
            n, o = new[1 if name == "dgamma" else 2], old[1 if name == "dgamma" else 2]
            dist = (n.double() - o.double()).abs().cpu().numpy()
            bar = 72 * 2.0 ** -24 * p[bound] + 1e-30
            print("%s %s: max distance / bar %.3f" % (case.name, name, float((dist / bar).max())))
            assert (dist <= bar).all(), name
        assert float(new[1][MASKED_CH]) == 0.0 == float(new[2][MASKED_CH]) or not case.relu
        if case.relu:
            assert not bool(new[0][:, :, MASKED_CH].any()), "a channel the ReLU masks entirely has no gradient"


@pytest.mark.parametrize("name", ["R33", "padded", "many-slabs"])
def test_two_runs_are_bit_identical(name):
    p = problem([c for c in CASES if c.name == name][0])
    a, b = run_new(p), run_new(p)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["R1", "padded", "K9", "many-slabs"])
def test_deferred_second_stage_equals_the_immediate_one(name):
    """dW's slab reduction joins a pass's deferred ones (one k_slab_reduce_multi4 launch, here beside the three-launch
    route's dW job) when dW sits in a slot of a registered flat gradient buffer: dW is not written before the flush
    while dgamma and dbeta are written by the call itself, straight into their slots; the results are bitwise those of
    the immediate second stage."""
    Fsp = _fsp()
    p = problem([c for c in CASES if c.name == name][0])
    case, d = p["case"], p["dev"]
    plain = run_new(p)
    other = run_old(p)[0]
    n_w = case.K * 64
    flat_p = torch.zeros((2 * n_w + 64 + 3,), device=DEV)          # the +3: a slot at an odd 4-byte offset
    flat_g = torch.full_like(flat_p, float("nan"))
    with torch.no_grad():
        flat_p[3 + n_w:3 + n_w + 32] = d["gamma"]
        flat_p[3 + n_w + 32:3 + n_w + 64] = d["beta"]
    filters = flat_p[3:3 + n_w].view(case.K, 2, 32)
    gamma, beta = flat_p[3 + n_w:3 + n_w + 32], flat_p[3 + n_w + 32:3 + n_w + 64]
    filters2 = flat_p[3 + n_w + 64:].view(case.K, 2, 32)
    Fsp.register_grad_slots(flat_p, flat_g)
    Fsp.defer_dw(True)
    try:
        got = run_new(p, filters, gamma, beta)
        kmap = _L().i32_array(p["kmap"]) if p["kmap"] else None
        dz = Fsp.bn_relu_backward(d["z"], d["dY"], d["gamma"], d["beta"], d["mean"], d["invstd"], True, case.relu,
                                  d["r_dev"])[0]
        got2 = Fsp.gather_dw(d["table"], case.K, p["ident"], case.cap, dz, d["X"], True, kmap, d["r_dev"], filters2)
        assert len(Fsp._DEFERRED_DW) == 2 and all(t._base is not None for t in got + (got2,))
        torch.cuda.synchronize()
        assert bool(torch.isnan(flat_g[:3 + n_w]).all()) and bool(torch.isnan(flat_g[3 + n_w + 64:]).all()), \
            "no dW is written before the flush"
        assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
        Fsp.flush_deferred_dw()
        torch.cuda.synchronize()
        assert Fsp.was_deferred(got[0].data_ptr()) and Fsp.was_deferred(got2.data_ptr())
    finally:
        Fsp.defer_dw(False)
        Fsp.reset_grad_slots()
    for a, b in zip(got + (got2,), plain + (other,)):
        assert torch.equal(a, b)
    assert bool(torch.isnan(flat_g[:3]).all())


def test_an_empty_batch_and_bad_arguments():
    Fsp, L = _fsp(), _L()
    lib = L.load()
    p = problem(CASES[0])
    d = p["dev"]
    dW = torch.full((27, 2, 32), 7.0, device=DEV)
    dg, db = torch.full((32,), 7.0, device=DEV), torch.full((32,), 7.0, device=DEV)
    rc = lib.wfs_first_conv_bn_backward(None, None, 27, 13, 0, None, None, None, 0, None, None, None, None, 1, L.ptr(dW),
                                        L.ptr(dg), L.ptr(db), L.dtype_code(d["z"]), None, 0, None, None, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and not bool(dW.any()) and not bool(dg.any()) and not bool(db.any())
    ws = torch.empty((int(lib.wfs_first_conv_bn_backward_workspace_bytes(28, 1)),), dtype=torch.uint8, device=DEV)
    for K, dtype_code, nbytes in ((28, L.dtype_code(d["z"]), ws.numel()), (27, 0, ws.numel()), (27, L.dtype_code(d["z"]), 16)):
        rc = lib.wfs_first_conv_bn_backward(L.ptr(d["table"]), None, K, 13, 1, L.ptr(d["z"]), L.ptr(d["dY"]), L.ptr(d["X"]),
                                            2, None, None, L.ptr(d["mean"]), L.ptr(d["invstd"]), 1, L.ptr(dW), None, None,
                                            dtype_code, L.ptr(ws), nbytes, None, None, L.stream_ptr())
        assert rc != 0, (K, dtype_code, nbytes)


# ------------------------------------------------------------------------------------------------------ module level
def _count_calls(monkeypatch):
    Fsp = _fsp()
    calls = []
    real = Fsp.first_conv_bn_backward

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(Fsp, "first_conv_bn_backward", counted)
    return calls


def _c2_module(T, seed=11):
    import copy
    import json
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    cfg = json.load(open(os.path.join(os.path.dirname(HERE), "config", "psd_c2_3d.json")))
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["algorithm"][-1] = [32 * 10 * 7 * (T // 16), 3]
    torch.manual_seed(seed)
    return LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg))), cfg


def test_captured_step_and_the_same_step_run_eagerly_give_identical_gradients(monkeypatch):
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.graph import GraphedTrainStep
    calls = _count_calls(monkeypatch)
    T, B = 64, 4
    c, f, y = synthetic.generate(B, T, 3, seed=5)
    batch = ([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV).to(torch.bfloat16)], torch.from_numpy(y).to(DEV))
    grads = []
    for captured in (True, False):
        mod = _c2_module(T)[0].to(DEV)
        red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
        mod.optimizer_parameters = red.optimizer_parameters()
        opt = mod.configure_optimizers()[0][0]
        step = GraphedTrainStep(mod, opt, red, batch, warmup=1)
        n0 = len(calls)
        if captured:
            step(batch)
        else:
            step._load(batch)
            step._body()
            assert len(calls) == n0 + 1, "the eager step's first layer takes the one-pass backward"
        step.check()
        torch.cuda.synchronize()
        grads.append(red.flat_grad.detach().clone())
        step.close()
    assert len(calls) >= 5, "the calibration, warm-up and captured steps take it too"
    assert bool(torch.isfinite(grads[0]).all()) and bool(grads[0].any())
    assert torch.equal(grads[0], grads[1])


def test_fp16_net_gradients_against_the_cpu_oracle(monkeypatch):
    """Bar quoted from test_gpu_parity.py::test_c4_deep_stack_config_matches_the_cpu_path (16-bit rows): the relative L2
    error of every parameter gradient against the fp32 CPU path on the same fp16-rounded input is below 0.15."""
    import copy
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    calls = _count_calls(monkeypatch)
    T, B = 64, 4
    gpu, cfg = _c2_module(T, seed=21)
    cfg_ref = copy.deepcopy(cfg)
    cfg_ref["net_config"]["imports"] = ["oracle.spconv" if m == "waveformml_amd.spconv" else m
                                        for m in cfg_ref["net_config"]["imports"]]
    cpu = LitPSD(DictionaryUtility.to_object(cfg_ref))
    cpu.load_state_dict(gpu.state_dict())
    gpu = gpu.to(DEV)
    gpu.train(), cpu.train()
    c, f, y = synthetic.generate(B, T, 3, seed=99)
    fin = torch.from_numpy(f).to(torch.float16)
    loss_r = cpu.training_step(([torch.from_numpy(c), fin.float()], torch.from_numpy(y)), 0)
    loss_g = gpu.training_step(([torch.from_numpy(c).to(DEV), fin.to(DEV)], torch.from_numpy(y).to(DEV)), 0)
    loss_r.backward()
    loss_g.backward()
    assert len(calls) == 1
    for (name, a), b in zip(gpu.model.named_parameters(), cpu.model.parameters()):
        assert a.grad is not None and bool(torch.isfinite(a.grad).all()), name
        err = float((a.grad.float().cpu() - b.grad).norm() / b.grad.norm().clamp_min(1e-30))
        print("%s: relative L2 error %.4f" % (name, err))
        assert err < 0.15, (name, err)


def _first_layer(sp, bias, seed=3):
    torch.manual_seed(seed)
    return sp.SparseSequential(sp.SubMConv3d(2, 32, 3, 1, 0, 1, 1, bias, "k0"), torch.nn.BatchNorm1d(32),
                               torch.nn.ReLU()).to(DEV)


@pytest.mark.parametrize("why", ["eligible", "bias", "input_grad", "fp32_rows", "eval_bn"])
def test_layers_the_fused_node_does_not_cover_take_the_separate_launches(why, monkeypatch):
    import waveformml_amd.spconv as sp
    from waveformml_amd.psd import synthetic
    Fsp = _fsp()
    calls = _count_calls(monkeypatch)
    T, B = 64, 4
    c, f, _ = synthetic.generate(B, T, 3, seed=8)
    idx = torch.from_numpy(np.ascontiguousarray(c[:, [3, 0, 1, 2]])).to(DEV)
    dtype = torch.float32 if why == "fp32_rows" else torch.bfloat16
    feats = torch.from_numpy(f).to(DEV).to(dtype)
    gout = torch.from_numpy(np.random.default_rng(1).standard_normal((len(c), 32)).astype(np.float32)).to(DEV).to(dtype)
    res = []
    for fused in (True, False):
        net = _first_layer(sp, why == "bias")
        if why == "eval_bn":
            net[1].eval()
        x = feats.clone().requires_grad_(why == "input_grad")
        t = sp.SparseConvTensor(x, idx, [14, 11, T], B)
        if fused:
            out = net(t).features
        else:                           # the launches SparseSequential issued before the fused node existed
            mid = net[0](t)
            out = Fsp.batch_norm_relu(mid.features, net[1], True, mid.n_valid)
        out.backward(gout)
        torch.cuda.synchronize()
        res.append([out.detach()] + [q.grad.detach().clone() for q in net.parameters()] +
                   ([x.grad.detach().clone()] if why == "input_grad" else []) +
                   [b.detach().clone() for b in net.buffers()])
    assert len(calls) == (1 if why == "eligible" else 0)
    assert len(res[0]) == len(res[1])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
