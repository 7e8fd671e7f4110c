"""GPU per-segment evaluators (csrc/segstats.hip, psd/segment_evaluator.py) against tables RECORDED from the reference's own
row walks (tests/golden/segment_evaluator_cases.npz, made by tests/golden/make_segment_evaluator_goldens.py).  Nothing here
reads the reference tree.

Bounds: integer tables exactly; float tables within 1e-5 of the recorded table's largest absolute entry (the recorded
tables are the reference's float32 running sums; the generator holds the float64 restatement to the same bound)."""
import copy

import numpy as np
import pytest
import torch

import segment_evaluator_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)
HIST = ("seg_sample_error",)


@pytest.fixture(scope="module")
def gold():
    return sc.load_golden()


def batch_of(gold, dt, b):
    """(coords, pred, targ) of a recorded batch on the device, maps in the case's dtype (plane 0 energy, plane 1 z)."""
    c, p, t = (torch.from_numpy(gold["%s_b%d_%s" % (dt, b, k)]).to(DEV) for k in ("coords", "pred", "targ"))
    p, t = p.to(TORCH_DTYPE[dt]), t.to(TORCH_DTYPE[dt])
    assert np.array_equal(p.float().cpu().numpy(), gold["%s_b%d_pred" % (dt, b)])     # the reference saw these very values
    return c, p, t


def state_of(ev):
    return [t.clone() for t in ev.state_tensors()]


def same_state(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def check_shapes(res, shapes):
    assert sorted(res) == sorted(shapes)
    for k, shape in shapes.items():
        if isinstance(res[k], tuple):
            assert res[k][0].dtype == np.float32 and res[k][1].dtype == np.int32 and res[k][0].shape == res[k][1].shape == shape, k
        else:
            assert res[k].dtype == np.int32 and res[k].shape == shape, k
        if k.endswith("_cal") or k.startswith("E_z_"):
            assert all(np.count_nonzero(a) == 0 for a in (res[k] if isinstance(res[k], tuple) else (res[k],))), k


@pytest.mark.parametrize("dt", sc.DTYPES)
def test_z_evaluator_matches_the_recorded_reference(gold, dt):
    from waveformml_amd.psd.segment_evaluator import ZEvaluator, z_result_shapes
    plain, with_E = ZEvaluator(DEV), ZEvaluator(DEV, use_energy=True)
    worst = 0.0
    for b in range(2):
        c, p, t = batch_of(gold, dt, b)
        before = (p.clone(), t.clone(), c.clone())
        # the reference's call: [B, 1, 14, 11] slices of the z plane, the energy target map as E
        plain.add(p[:, 1].unsqueeze(1), t[:, 1].unsqueeze(1), c, None, E=t[:, 0])
        with_E.add(p[:, 1].unsqueeze(1), t[:, 1].unsqueeze(1), c, None, E=t[:, 0])
        assert torch.equal(p, before[0]) and torch.equal(t, before[1]) and torch.equal(c, before[2])   # only read
        acc = "%s_after%d_" % (dt, b + 1)
        for ev, kind in ((plain, "z_"), (with_E, "zE_")):
            res = ev.results()
            check_shapes(res, z_result_shapes())
            worst = max(worst, sc.assert_tables_match(res, gold, acc + kind, sc.Z_PAIRS + HIST, kind))
    print(dt, "z tables: worst float error %.3g of scale" % worst)
    assert plain.has_true_E and plain.E_high == 9.0                                  # set_true_E, as the reference
    assert plain.results()["E_mult_mae_single"][1].sum() == 0 and with_E.results()["E_mult_mae_dual"][1].sum() > 0
    m = plain.retrieve_error_metrics()
    s, n = plain.results()["z_mult_mae_dual"]
    assert m["evaluation/dual_mae"] == float(np.sum(s) / np.sum(n) * 1200.) and len(m["evaluation/single_mae_mult"]) == 6
    assert m["evaluation/single_mae_cal"] == 0.0
    # no E: E_high stays 10 and nothing else changes
    no_E = ZEvaluator(DEV)
    for b in range(2):
        c, p, t = batch_of(gold, dt, b)
        no_E.add(p[:, 1:2], t[:, 1:2], c, None)
    assert not no_E.has_true_E and same_state(state_of(no_E), state_of(plain))


@pytest.mark.parametrize("dt", sc.DTYPES)
def test_energy_evaluator_matches_the_recorded_reference(gold, dt):
    from waveformml_amd.psd.segment_evaluator import EnergyEvaluator, energy_result_shapes
    ev = EnergyEvaluator(DEV)
    for b in range(2):
        c, p, t = batch_of(gold, dt, b)
        ev.add(p[:, 0].unsqueeze(1), t[:, 0].unsqueeze(1), c, None)
        res = ev.results()
        check_shapes(res, energy_result_shapes())
        worst = sc.assert_tables_match(res, gold, "%s_after%d_" % (dt, b + 1) + "e_", sc.E_PAIRS)
    print(dt, "energy tables: worst float error %.3g of scale" % worst)
    m = ev.retrieve_error_metrics()
    assert len(m["evaluation/single_E_MAPE"]) == 20 and len(m["evaluation/dual_E_MAPE"]) == 20


@pytest.mark.parametrize("planes", ["reference", "lit"])
@pytest.mark.parametrize("dt", sc.DTYPES)
def test_ez_evaluator_in_both_plane_orders(gold, dt, planes):
    """The recorded maps are in the order EZEvaluatorBase.add reads (plane 0 energy, plane 1 z); for ``planes="lit"`` the
    same maps are handed over in LitEZ's order (z, E) and must give the same tables."""
    from waveformml_amd.psd.segment_evaluator import EZEvaluator
    ev = EZEvaluator(DEV, planes=planes, use_energy=True)
    for b in range(2):
        c, p, t = batch_of(gold, dt, b)
        if planes == "lit":
            p, t = p.flip(1).contiguous(), t.flip(1).contiguous()
        ev.add(p, t, c, None)
    res = ev.results()
    assert sorted(res) == ["EnergyEvaluator", "ZEvaluator"]
    acc = dt + "_after2_"
    sc.assert_tables_match(res["ZEvaluator"], gold, acc + "zE_", sc.Z_PAIRS + HIST)
    sc.assert_tables_match(res["EnergyEvaluator"], gold, acc + "e_", sc.E_PAIRS)
    plain = EZEvaluator(DEV, planes=planes)                                          # the reference: E tables stay empty
    c, p, t = batch_of(gold, dt, 0)
    if planes == "lit":
        p, t = p.flip(1).contiguous(), t.flip(1).contiguous()
    plain.add(p, t, c, None)
    sc.assert_tables_match(plain.results()["ZEvaluator"], gold, dt + "_after1_z_", sc.Z_PAIRS + HIST)
    assert len(ev.state_tensors()) == 2 and set(ev.retrieve_error_metrics()) >= {"evaluation/dual_mae", "evaluation/dual_E_MAPE"}


def test_padding_determinism_reset(gold):
    from waveformml_amd.psd.segment_evaluator import EZEvaluator
    batches = [batch_of(gold, "f32", b) for b in range(2)]

    def run(ev):
        for c, p, t in batches:
            ev.add(p, t, c, None)
        return state_of(ev)
    ev = EZEvaluator(DEV, use_energy=True)
    first = run(ev)
    assert all(t.dtype == torch.int64 for t in first)
    # the same batches inside capacity-padded coordinate buffers, garbage beyond n_valid
    pad = EZEvaluator(DEV, use_energy=True)
    g = torch.Generator(device="cpu").manual_seed(3)
    for c, p, t in batches:
        n, cap = c.shape[0], c.shape[0] + 300
        pc = torch.randint(-5, 100, (cap, 3), generator=g, dtype=torch.int32).to(DEV)
        pc[:n] = c
        pad.add(p, t, pc, None, n_valid=torch.tensor([n], dtype=torch.int64, device=DEV))
    assert same_state(first, state_of(pad))
    pad.results()                                                                    # the garbage raised no flag
    assert same_state(first, run(EZEvaluator(DEV, use_energy=True)))                 # a second run: the same bits
    ev.reset()
    assert all(int(t.abs().sum()) == 0 for t in ev.state_tensors())
    empty = ev.results()["ZEvaluator"]
    assert all(np.count_nonzero(a) == 0 for v in empty.values() for a in (v if isinstance(v, tuple) else (v,)))
    assert same_state(first, run(ev))


def test_bad_batches_raise_from_results_with_their_own_message(gold):
    from waveformml_amd.psd.segment_evaluator import EnergyEvaluator, ZEvaluator
    c, p, t = batch_of(gold, "f32", 0)
    z = ZEvaluator(DEV)
    unsorted = c.clone()
    unsorted[[3, 20]] = unsorted[[20, 3]]
    z.add(p[:, 1:2], t[:, 1:2], unsorted, None)
    with pytest.raises(RuntimeError, match="not sorted"):
        z.results()
    z.reset()
    beyond = c.clone()
    beyond[-1, 2] = 10                                                               # an event outside the [10, ...] maps
    z.add(p[:, 1:2], t[:, 1:2], beyond, None)
    with pytest.raises(RuntimeError, match="not sorted or held an event outside"):
        z.results()
    z.reset()
    outside = c.clone()
    outside[5, 0], outside[9, 1], outside[11, 0] = 14, -1, 1 << 20
    z.add(p[:, 1:2], t[:, 1:2], outside, None)
    with pytest.raises(RuntimeError, match="outside the detector grid") as info:
        z.results()
    assert "sorted" not in str(info.value)
    assert int(z.tables[:14 * 11 * 7].sum()) == len(c) - 3                          # the three rows are left out, no more
    z.reset()
    z.add(p[:, 1:2], t[:, 1:2], c, None)
    z.results()                                                                      # reset() cleared the flag
    en = EnergyEvaluator(DEV)
    zero = t.clone()
    zero[int(c[7, 2]), 0, int(c[7, 0]), int(c[7, 1])] = 0
    en.add(p[:, 0:1], zero[:, 0:1], c, None)
    with pytest.raises(RuntimeError, match="energy target was zero") as info:
        en.results()
    assert "grid" not in str(info.value) and int(en.tables[:14 * 11 * 11].sum()) == len(c) - 1
    en.reset()
    nan = p.clone()
    nan[int(c[7, 2]), 0, int(c[7, 0]), int(c[7, 1])] = float("nan")
    en.add(nan[:, 0:1], t[:, 0:1], c, None)
    with pytest.raises(RuntimeError, match="not finite"):
        en.results()
    with pytest.raises(RuntimeError, match="no CPU path"):
        z.add(p[:, 1:2].cpu(), t[:, 1:2], c, None)
    with pytest.raises(RuntimeError, match="must be"):
        z.add(p[:, 1:2, :, :10], t[:, 1:2], c, None)


def test_segment_test_loop_hands_every_batch_to_the_evaluator():
    from test_host_mirror import _z_config
    from test_segment_callers import segment_rows
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litz import LitZ
    from waveformml_amd.psd.segment_evaluator import ZEvaluator
    torch.manual_seed(3)
    mod = LitZ(load_config(copy.deepcopy(_z_config(["waveformml_amd.spconv"])))).to(DEV)
    rng = np.random.default_rng(14)
    batches = []
    for B in (9, 6):
        rows, c, f = segment_rows(rng, B, 4, 40)
        batches.append(([c, f], torch.from_numpy(rng.random(len(rows)).astype(np.float32))))
    plain = segment_test_loop(mod, batches, DEV)
    assert "evaluation" not in plain and plain["rows"] == sum(len(b[0][0]) for b in batches)
    ev = mod.evaluator
    assert isinstance(ev, ZEvaluator) and mod.evaluator is ev
    out = segment_test_loop(mod, batches, DEV, evaluator=ev)
    assert out["test_loss"] == plain["test_loss"]
    direct = ZEvaluator(DEV)
    losses = []
    mod.eval()
    with torch.no_grad():
        for i, ((c, f), z) in enumerate(batches):
            res = mod.test_step(([c.to(DEV), f.to(DEV)], z.to(DEV)), i)
            direct.add(*mod.last_test_outputs)
            losses.append(float(res["test_loss"]) * len(c))
    assert abs(out["test_loss"] - sum(losses) / out["rows"]) <= 1e-6 * abs(out["test_loss"])
    assert same_state(state_of(ev), state_of(direct))
    want = direct.results()
    for k, v in out["evaluation"].items():
        for a, b in zip(v if isinstance(v, tuple) else (v,), want[k] if isinstance(want[k], tuple) else (want[k],)):
            assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert out["evaluation"]["seg_mult_mae"][1].sum() == out["rows"]
