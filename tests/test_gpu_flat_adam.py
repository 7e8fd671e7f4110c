"""Adam and AdamW in the captured training step: FlatAdam / FlatAdamW (psd/optim.py; their update is
csrc/optim.hip wfs_adam_step) against torch's Adam / AdamW, replayed inside a HIP graph, behind Trainer(capture=True),
in checkpoints; and an optimizer whose step cannot be captured (RMSprop) stepping after the replay (psd/graph.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
N = 70001                       # odd: the kernel's float4 rows end in a scalar tail
T = 64


def _assert_close(got, want, rtol, what=""):
    """|got - want| <= rtol * max|want| + rtol * |want|  (relative to the tensor's scale)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * max(scale, 1e-30), err_msg=what)


CASES = {
    "plain": (torch.optim.Adam, "FlatAdam", dict()),
    "weight_decay": (torch.optim.Adam, "FlatAdam", dict(weight_decay=1e-2)),
    "amsgrad": (torch.optim.Adam, "FlatAdam", dict(amsgrad=True)),
    "maximize": (torch.optim.Adam, "FlatAdam", dict(maximize=True)),
    "adamw": (torch.optim.AdamW, "FlatAdamW", dict(weight_decay=1e-2)),
    "unaligned": (torch.optim.Adam, "FlatAdam", dict(weight_decay=1e-3)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_flat_adam_matches_torch_adam(case):
    """Five steps of FlatAdam / FlatAdamW against torch's Adam / AdamW on the CPU in fp32: ExponentialLR steps after the
    second, betas[0] changes after the third.  Parameters and every moment within 1e-6 of scale, step == 5 on the
    device, no private keys in state_dict().  ``unaligned``: parameter and gradient 4 bytes off a 16-byte boundary (the
    kernel's scalar path)."""
    from waveformml_amd.psd import optim
    ref_cls, name, kw = CASES[case]
    rng = np.random.default_rng(17)
    w0 = rng.standard_normal(N).astype(np.float32)
    pr = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    if case == "unaligned":
        base = torch.zeros(N + 1, device=DEV)
        base[1:] = torch.from_numpy(w0)
        pg, gbase = base[1:], torch.zeros(N + 1, device=DEV)
        assert pg.data_ptr() % 16 != 0
    else:
        pg = torch.nn.Parameter(torch.from_numpy(w0.copy()).to(DEV))
    ref = ref_cls([pr], lr=0.01, **kw)
    opt = getattr(optim, name)([pg], lr=0.01, **kw)
    sr = torch.optim.lr_scheduler.ExponentialLR(ref, gamma=0.5)
    sg = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    for step in range(5):
        g = (rng.standard_normal(N) * (1.0 + step)).astype(np.float32)
        pr.grad = torch.from_numpy(g.copy())
        if case == "unaligned":
            gbase[1:] = torch.from_numpy(g)
            pg.grad = gbase[1:]
        else:
            pg.grad = torch.from_numpy(g.copy()).to(DEV)
        ref.step()
        opt.step()
        if step == 1:
            sr.step()
            sg.step()
        if step == 2:
            for o in (ref, opt):
                o.param_groups[0]["betas"] = (0.8, o.param_groups[0]["betas"][1])
    _assert_close(pg.detach().cpu().numpy(), pr.detach().numpy(), 1e-6, "parameters")
    names = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if kw.get("amsgrad") else [])
    for k in names:
        _assert_close(opt.state[pg][k].cpu().numpy(), ref.state[pr][k].numpy(), 1e-6, k)
    step_t = opt.state[pg]["step"]
    assert step_t.device == pg.device and float(step_t) == 5.0
    sd = opt.state_dict()
    assert not [k for g in sd["param_groups"] for k in g if k.startswith("_")]
    assert not [k for st in sd["state"].values() for k in st if k.startswith("_")]
    assert sorted(sd["state"][0]) == sorted(ref.state_dict()["state"][0])
    assert abs(sd["param_groups"][0]["lr"] - 0.005) < 1e-12


def test_flat_adam_step_replays_in_a_graph():
    """FlatAdam.step() captured once and replayed four times, the gradient refilled in place and lr changed between the
    replays (sync_hyperparameters, as GraphedTrainStep calls it): bit-identical to four eager steps on the same gradients;
    the step count advances on the device."""
    from waveformml_amd.psd.optim import FlatAdam
    rng = np.random.default_rng(23)
    w0 = rng.standard_normal(N).astype(np.float32)
    grads = [rng.standard_normal(N).astype(np.float32) for _ in range(5)]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        pa = torch.nn.Parameter(torch.from_numpy(w0.copy()).to(DEV))
        pb = torch.nn.Parameter(torch.from_numpy(w0.copy()).to(DEV))
        a = FlatAdam([pa], lr=1e-2, weight_decay=1e-3, amsgrad=True)
        b = FlatAdam([pb], lr=1e-2, weight_decay=1e-3, amsgrad=True)
        for p, o in ((pa, a), (pb, b)):           # the first step creates the state, outside the capture
            p.grad = torch.from_numpy(grads[0]).to(DEV)
            o.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            b.step()
        assert float(b.state[pb]["step"]) == 1.0           # captured, not run
        for i in range(1, 5):
            lr = 1e-2 * 0.7 ** i
            a.param_groups[0]["lr"] = b.param_groups[0]["lr"] = lr
            pa.grad = torch.from_numpy(grads[i]).to(DEV)
            a.step()
            pb.grad.copy_(torch.from_numpy(grads[i]))
            b.sync_hyperparameters()
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pa.detach(), pb.detach())
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.equal(a.state[pa][k], b.state[pb][k]), k
        assert float(a.state[pa]["step"]) == float(b.state[pb]["step"]) == 5.0
        graph.reset()
        torch.cuda.synchronize()


def _c2_cfg(opt_class, params, lr=1e-3):
    with open(os.path.join(os.path.dirname(HERE), "config", "psd_c2_3d.json")) as f:
        cfg = json.load(f)
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["algorithm"][-1] = [32 * 10 * 7 * 4, 3]
    oc = cfg["optimize_config"]
    oc["optimizer_class"], oc["optimizer_params"], oc["lr"] = opt_class, dict(params), lr
    return cfg


def _loader():
    from waveformml_amd.psd import data
    ds = data.SyntheticPulseDataset(6, 24, T, n_type=3, layout="3d", seed=77)
    return data.make_loader(ds, 1, shuffle=False, pin_memory=False)


def _fit(cfg, capture, loader, max_epochs=1, root=None, resume=None, val=None):
    """One Trainer.fit of the small C2 net (fp32 rows): (module, its initial state_dict, the optimizer, the trainer)."""
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.trainer import Trainer
    torch.manual_seed(11)
    mod = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
    start = copy.deepcopy(mod.state_dict())
    box, configure = {}, mod.configure_optimizers

    def keep():                                   # the optimizer the fit builds, for the test to inspect
        out = configure()
        box["opt"] = out[0][0] if isinstance(out, tuple) else out
        return out
    mod.configure_optimizers = keep
    tr = Trainer(max_epochs=max_epochs, device=DEV, capture=capture, default_root_dir=root, resume_from_checkpoint=resume)
    tr.fit(mod, loader, val_loader=val)
    return mod, start, box["opt"], tr


def _flat_state(opt):
    (p,) = [p for g in opt.param_groups for p in g["params"]]
    return p, opt.state[p]


def _updates_agree(mod_e, mod_g, start, rtol, few=0.0):
    """Update of every tensor of the captured run within ``rtol`` of the eager run's update scale; ``few``: the share of
    a tensor's elements that may miss that bar, by no more than 10 x (test_rmsprop_steps_after_the_replay says why).
    Every tensor is measured before anything is asserted; the report names them all."""
    sd_e, sd_g = mod_e.state_dict(), mod_g.state_dict()
    report, bad = [], []
    for name in sd_e:
        a, b, p0 = sd_e[name].double().cpu(), sd_g[name].double().cpu(), start[name].double().cpu()
        if a.numel() == 1 and "num_batches_tracked" in name:
            assert int(a) == int(b) == 6, (name, int(a), int(b))
            continue
        got, want = b - p0, a - p0
        scale = max(float(want.abs().max()), 1e-30)
        err = (got - want).abs() - rtol * want.abs()
        misses = int((err > rtol * scale).sum())
        worst = float(err.max()) / scale
        report.append("%-32s n %7d  misses %5d  worst %.2e of scale" % (name, want.numel(), misses, worst))
        if misses > few * want.numel() or worst > (10 * rtol if few else rtol):
            bad.append(name)
    print("\n".join(report))
    assert not bad, "updates off by more than %g of scale in %s:\n%s" % (rtol, bad, "\n".join(report))


@pytest.mark.parametrize("opt_class,params,flat", [("optim.Adam", {}, "FlatAdam"),
                                                   ("optim.AdamW", {"weight_decay": 1e-2}, "FlatAdamW")],
                         ids=["adam", "adamw"])
def test_trainer_captures_adam(opt_class, params, flat):
    """Trainer(capture=True) with optimizer_class optim.Adam / optim.AdamW (torch's step raises under capture): the fit
    finishes with the flat optimizer's HIP step inside the graph, no eager fallbacks, step == 6 after six batches (the
    capture's calibration and warm-up steps left no trace in the state), and the weights follow Trainer(capture=False)
    within 1e-3 of each tensor's update scale."""
    from waveformml_amd.psd.graph import steps_in_graph
    loader = _loader()
    cfg = _c2_cfg(opt_class, params)
    mod_e, start, opt_e, _ = _fit(cfg, False, loader)
    mod_g, start_g, opt_g, tr = _fit(cfg, True, loader)
    assert type(opt_g).__name__ == flat and steps_in_graph(opt_g)
    assert tr.last_capacity > 0 and tr.eager_fallbacks == 0
    for name in start:
        assert torch.equal(start[name], start_g[name])
    for opt in (opt_e, opt_g):
        p, st = _flat_state(opt)
        assert st["step"].device == p.device and float(st["step"]) == 6.0
    _updates_agree(mod_e, mod_g, start, 1e-3)


def test_adam_checkpoint_loads_into_torch_adam_and_resumes(tmp_path):
    """A checkpoint of a captured Adam run holds one optimizer entry per model parameter, the layout a reference
    Lightning run writes: it loads into torch.optim.Adam(model.parameters()) on the CPU, whose per-parameter state equals
    the flat state's slices.  resume_from_checkpoint with one more epoch continues from the saved step count."""
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.trainer import _offsets_in_flat
    loader = _loader()
    cfg = _c2_cfg("optim.Adam", {})
    mod, _, opt, tr = _fit(cfg, True, loader, root=str(tmp_path / "a"), val=loader)
    ck_path = tr.last_checkpoint
    assert ck_path is not None
    ck = torch.load(ck_path, map_location="cpu", weights_only=True)
    sd = ck["optimizer_states"][0]
    params = list(mod.model.parameters())
    assert len(sd["state"]) == len(params)
    cpu = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
    ref = torch.optim.Adam(cpu.model.parameters(), lr=1e-3)
    ref.load_state_dict(sd)
    flat, st = _flat_state(opt)
    offsets = _offsets_in_flat(flat, params)
    for i, (p, q) in enumerate(zip(params, cpu.model.parameters())):
        rs = ref.state[q]
        assert float(rs["step"]) == 6.0
        for k in ("exp_avg", "exp_avg_sq"):
            want = st[k].reshape(-1)[offsets[i]:offsets[i] + p.numel()].reshape(p.shape).cpu()
            assert rs[k].shape == q.shape and torch.equal(rs[k], want), (i, k)
    assert float(st["exp_avg_sq"].abs().max()) > 0
    mod2, _, opt2, tr2 = _fit(cfg, True, loader, max_epochs=2, root=str(tmp_path / "b"), resume=ck_path, val=loader)
    assert [h["epoch"] for h in tr2.history] == [1]
    p2, st2 = _flat_state(opt2)
    assert st2["step"].device == p2.device and float(st2["step"]) == 12.0
    ck2 = torch.load(tr2.last_checkpoint, map_location="cpu", weights_only=True)
    assert all(float(e["step"]) == 12.0 for e in ck2["optimizer_states"][0]["state"].values())


def test_rmsprop_steps_after_the_replay():
    """optimizer_class optim.RMSprop (capturable off: its step cannot go into the graph) under Trainer(capture=True): the
    graph ends with the gradient, the optimizer steps eagerly after each replay, and the weights follow
    Trainer(capture=False) within 1e-3 of each tensor's update scale -- all but at most 5 % of a tensor's elements (one
    of 32 is 3 %), which stay within 1e-2.  Both runs step with the same torch RMSprop, so what differs is the gradient: the captured step
    sums some reductions in another order, and the two runs' weights drift apart over the steps.  Adam averages those
    differences into its momentum before it divides by the RMS (test_trainer_captures_adam holds 1e-3 for every
    element); RMSprop divides each element's raw gradient by that element's running RMS -- its first update is
    10 x lr x sign(g) -- so a gradient difference that is small against the tensor's largest gradient is not small against
    that element's own.  Measured on one MI355X: 12 of 27 648 elements of the fourth layer's filters miss 1e-3 (worst
    3.6e-3), 69 of the seventh layer's (worst 7.3e-3), 1 of 32 of the BatchNorm bias after it (2.1e-3); every other
    tensor holds 1e-3."""
    from waveformml_amd.psd.graph import steps_in_graph
    loader = _loader()
    cfg = _c2_cfg("optim.RMSprop", {})
    mod_e, start, opt_e, _ = _fit(cfg, False, loader)
    mod_g, _, opt_g, tr = _fit(cfg, True, loader)
    assert type(opt_g) is torch.optim.RMSprop and not steps_in_graph(opt_g)
    assert tr.last_capacity > 0 and tr.eager_fallbacks == 0
    _, st = _flat_state(opt_g)
    assert float(st["step"]) == 6.0
    _updates_agree(mod_e, mod_g, start, 1e-3, few=0.05)


def test_captured_adam_runs_are_bit_identical():
    """Two identical captured Adam runs end with bit-identical weights and optimizer state."""
    loader = _loader()
    cfg = _c2_cfg("optim.Adam", {"amsgrad": True})
    runs = [_fit(cfg, True, loader) for _ in range(2)]
    sd0, sd1 = runs[0][0].state_dict(), runs[1][0].state_dict()
    for name in sd0:
        assert torch.equal(sd0[name], sd1[name]), name
    (_, s0), (_, s1) = _flat_state(runs[0][2]), _flat_state(runs[1][2])
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
