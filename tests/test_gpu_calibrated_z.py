"""The calibrated z / E baseline on the GPU (csrc/calibz.hip, the ``calibration=`` route of psd/segment_evaluator.py)
against values RECORDED from the reference's own functions (tests/golden/calibrated_z_cases.npz, made by
tests/golden/make_calibrated_z_goldens.py; layout in tests/calibrated_z_cases.py).  Nothing here reads the reference tree.

Bounds: states, peak lists, counts and histograms exactly; z_cal, E_cal and the float tables within 1e-5 of the recorded
output's largest magnitude, the project's bar for recorded values."""
import copy

import numpy as np
import pytest
import torch

import calibrated_z_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TORCH_DTYPE = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)
HIST = ("seg_sample_error",)


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


@pytest.fixture(scope="module")
def curves(gold):
    return cc.curves_of(gold)


def n_valid_of(gold, key, n):
    nv = int(gold[key])
    return (n, None) if nv < 0 else (nv, torch.tensor([nv], dtype=torch.int64, device=DEV))


def rows_on_device(rows, dt):
    """Recorded rows in the case's dtype; the valid ones hold exactly the values the reference saw."""
    t = torch.from_numpy(rows).to(DEV).to(TORCH_DTYPE[dt])
    ok = np.isfinite(rows)
    assert np.array_equal(t.float().cpu().numpy()[ok], rows[ok])
    return t.contiguous()


@pytest.mark.parametrize("name", ["L150_f32", "L150_bf16", "L150_f16", "L64_f32", "L64_bf16", "L64_f16", "L40_f32",
                                  "L40_bf16", "L40_f16", "one_row", "padded"])
def test_reconstruction_matches_the_recorded_reference(gold, curves, name):
    from waveformml_amd.psd.calibration import CalibratedReconstruction
    k = "k_%s_" % name
    assert name in [str(n) for n in gold["kernel_names"]]
    L, dt = int(gold[k + "L"]), str(gold[k + "dtype"])
    rows, coo = rows_on_device(gold[k + "rows"], dt), torch.from_numpy(gold[k + "coords"]).to(DEV)
    nv, n_dev = n_valid_of(gold, k + "n_valid", len(coo))
    rec = CalibratedReconstruction(DEV, curves, n_samples=L, z_scale=float(gold["z_default_z_scale"]))
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    before = rows.clone()
    z, E = rec.run(rows, coo, flags, n_dev)
    torch.cuda.synchronize()
    assert int(flags.item()) == 0
    assert torch.equal(rows.view(torch.uint8), before.view(torch.uint8))            # only read, NaN padding included
    n = len(coo)
    z, E = z[:n].cpu().numpy(), E[:n].cpu().numpy()
    state, peaks = rec.state[:n].cpu().numpy(), rec.peaks[:n].cpu().numpy()
    assert np.array_equal(state[:nv], gold[k + "state"]), np.flatnonzero(state[:nv] != gold[k + "state"])
    assert np.array_equal(peaks[:nv], gold[k + "peaks"]), np.flatnonzero((peaks[:nv] != gold[k + "peaks"]).any(axis=(1, 2)))
    for got, key in ((z, "z"), (E, "E")):
        want = gold[k + key]
        scale = float(np.abs(want).max())
        err = float(np.abs(got[:nv] - want).max()) / scale if scale > 0 else float(np.abs(got[:nv]).max())
        print("%s %s_cal: worst error %.3g of the largest magnitude %.6g" % (name, key, err, scale))
        assert err <= cc.REL, (name, key, err, int(np.abs(got[:nv] - want).argmax()))
    # rows beyond the valid count: defined and empty
    assert not z[nv:].any() and not E[nv:].any() and not state[nv:].any() and (peaks[nv:] == -1).all()


def batches_of(gold, name):
    dt = str(gold["ev_%s_dtype" % name])
    out = []
    for b in range(int(gold["ev_%s_nb" % name])):
        t = "ev_%s_b%d_" % (name, b)
        c = torch.from_numpy(gold[t + "coords"]).to(DEV)
        p = torch.from_numpy(gold[t + "pred"]).to(DEV).to(TORCH_DTYPE[dt])
        g = torch.from_numpy(gold[t + "targ"]).to(DEV).to(TORCH_DTYPE[dt])
        assert np.array_equal(p.float().cpu().numpy(), gold[t + "pred"]) and np.array_equal(g.float().cpu().numpy(), gold[t + "targ"])
        _nv, n_dev = n_valid_of(gold, t + "n_valid", len(c))
        out.append((c, p, g, rows_on_device(gold[t + "feats"], dt), n_dev))
    return out


def feats_len(batches):
    return batches[0][3].shape[1] // 2


def state_of(ev):
    return [t.clone() for t in ev.state_tensors()]


def same_state(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


CASES = ["two_adds_f32", "bf16", "f16", "padded"]


@pytest.mark.parametrize("name", CASES)
def test_z_evaluator_with_a_calibration(gold, curves, name):
    """ZEvaluatorWF.add with a calibrator: with the true energy, without it (the calibrated energy is the axis), and with
    target_is_cal."""
    from waveformml_amd.psd.segment_evaluator import ZEvaluator, z_result_shapes
    batches = batches_of(gold, name)
    L = feats_len(batches)
    worst = 0.0
    for kind, with_E, tic in (("zE_", True, False), ("z0_", False, False), ("zT_", True, True)):
        ev = ZEvaluator(DEV, calibration=curves, n_samples=L)
        for c, p, t, f, n_dev in batches:
            ev.add(p[:, 1:2], t[:, 1:2], c, f, E=t[:, 0] if with_E else None, target_is_cal=tic, n_valid=n_dev)
        res = ev.results()
        shapes = z_result_shapes()
        assert sorted(res) == sorted(shapes) and all((res[k][0] if isinstance(res[k], tuple) else res[k]).shape == s
                                                     for k, s in shapes.items())
        worst = max(worst, cc.assert_tables_match(res, gold, "ev_%s_%s" % (name, kind), cc.Z_PAIRS, HIST))
        assert ev.has_true_E == with_E and ev.E_high == (9.0 if with_E else 10.0)
        m = ev.retrieve_error_metrics(res)
        s, n = res["z_mult_mae_dual_cal"]
        assert m["evaluation/dual_mae_cal"] == float(np.sum(s) / np.sum(n) * 1200.)
        # target_is_cal hands double-ended segments their own target: no error there, by construction
        assert (m["evaluation/dual_mae_cal"] == 0.0) if tic else (m["evaluation/dual_mae_cal"] > 0)
    print(name, "calibrated z tables: worst float error %.3g of scale" % worst)


@pytest.mark.parametrize("name", CASES)
def test_energy_evaluator_with_a_calibration(gold, curves, name):
    from waveformml_amd.psd.segment_evaluator import EnergyEvaluator, energy_result_shapes
    batches = batches_of(gold, name)
    ev = EnergyEvaluator(DEV, calibration=curves, n_samples=feats_len(batches))
    for c, p, t, f, n_dev in batches:
        ev.add(p[:, 0:1], t[:, 0:1], c, f, n_valid=n_dev)
    res = ev.results()
    shapes = energy_result_shapes()
    assert sorted(res) == sorted(shapes) and all(res[k][0].shape == res[k][1].shape == s for k, s in shapes.items())
    worst = cc.assert_tables_match(res, gold, "ev_%s_e_" % name, cc.E_PAIRS)
    print(name, "calibrated energy tables: worst float error %.3g of scale" % worst)
    m = ev.retrieve_error_metrics(res)
    assert len(m["evaluation/single_E_MAPE_cal"]) == 20 and len(m["evaluation/dual_E_MAPE"]) == 20


@pytest.mark.parametrize("planes", ["reference", "lit"])
@pytest.mark.parametrize("name", CASES)
def test_ez_evaluator_with_a_calibration_in_both_plane_orders(gold, curves, name, planes):
    """The recorded maps are in the order EZEvaluatorBase.add reads (plane 0 energy, plane 1 z); for ``planes="lit"`` the
    same maps go in in LitEZ's order (z, E) and must give the same tables."""
    from waveformml_amd.psd.segment_evaluator import EZEvaluator
    batches = batches_of(gold, name)
    ev = EZEvaluator(DEV, planes=planes, calibration=curves, n_samples=feats_len(batches))
    for c, p, t, f, n_dev in batches:
        if planes == "lit":
            p, t = p.flip(1).contiguous(), t.flip(1).contiguous()
        ev.add(p, t, c, f, n_valid=n_dev)
    res = ev.results()
    cc.assert_tables_match(res["EnergyEvaluator"], gold, "ev_%s_e_" % name, cc.E_PAIRS)
    cc.assert_tables_match(res["ZEvaluator"], gold, "ev_%s_zE_" % name, cc.Z_PAIRS, HIST)
    assert len(ev.state_tensors()) == 2 and all(t.dtype == torch.int64 for t in ev.state_tensors())
    assert "evaluation/dual_mae_cal" in ev.retrieve_error_metrics()


def test_adds_concatenate_runs_repeat_and_reset_clears(gold, curves):
    """Two add calls equal one over the concatenated batch; a second run is bit-identical; reset() empties the new tables;
    without a calibration nothing changes."""
    from waveformml_amd.psd.segment_evaluator import EZEvaluator, ZEvaluator
    batches = batches_of(gold, "two_adds_f32")
    L = feats_len(batches)

    def run(bts):
        ev = EZEvaluator(DEV, calibration=curves, n_samples=L)
        for c, p, t, f, n_dev in bts:
            ev.add(p, t, c, f, n_valid=n_dev)
        return ev
    two, again = run(batches), run(batches)
    assert same_state(state_of(two), state_of(again))
    (c0, p0, t0, f0, _), (c1, p1, t1, f1, _) = batches
    c1 = c1.clone()
    c1[:, 2] += p0.shape[0]
    one = run([(torch.cat([c0, c1]), torch.cat([p0, p1]), torch.cat([t0, t1]), torch.cat([f0, f1]), None)])
    assert same_state(state_of(one), state_of(two))
    n_ints = sum(int(t.numel()) for t in two.state_tensors())
    plain = EZEvaluator(DEV)
    assert n_ints > 2 * sum(int(t.numel()) for t in plain.state_tensors())
    assert all(int(t.abs().sum()) > 0 for t in two.state_tensors())
    two.reset()
    assert all(int(t.abs().sum()) == 0 for t in two.state_tensors())
    res = two.results()
    assert res["ZEvaluator"]["seg_mult_mae_cal"][1].sum() == 0 and res["EnergyEvaluator"]["E_z_dual_cal"][1].sum() == 0
    # calibration=None is what it was: f is ignored, *_cal stay zero
    z_plain, z_none = ZEvaluator(DEV), ZEvaluator(DEV, calibration=None)
    z_plain.add(p0[:, 1:2], t0[:, 1:2], c0, None, E=t0[:, 0])
    z_none.add(p0[:, 1:2], t0[:, 1:2], c0, f0, E=t0[:, 0], target_is_cal=True)
    assert same_state(state_of(z_plain), state_of(z_none)) and z_none.results()["seg_mult_mae_cal"][1].sum() == 0
    with pytest.raises(RuntimeError, match="n_samples"):
        ZEvaluator(DEV, calibration=curves, n_samples=L).add(p0[:, 1:2], t0[:, 1:2], c0, f0[:, :-2].contiguous())


def test_a_reconstruction_that_is_not_finite_is_left_out_and_reported(gold, curves):
    """A segment whose light_sum curve is zero makes E = PE / 0 (numba raises there): flag 16, the row in no table,
    results() raises.  The same rows with the curve intact fill the tables without a flag."""
    from waveformml_amd.psd.calibration import CalibrationCurves
    from waveformml_amd.psd.segment_evaluator import EZEvaluator
    c, p, t, f, n_dev = batches_of(gold, "two_adds_f32")[0]
    L = f.shape[1] // 2
    good = EZEvaluator(DEV, calibration=curves, n_samples=L)
    good.add(p, t, c, f)
    rec = good.EnergyEvaluator._recon
    state = rec.state[:len(c)].cpu().numpy()
    row = int(np.flatnonzero(state == 2)[0])
    x, y = int(c[row, 0]), int(c[row, 1])
    arrays = {k: gold["cal_" + k].copy() for k in cc.CURVES}
    arrays["light_sum_curves"][x, y, :, 1] = 0
    bad = EZEvaluator(DEV, calibration=CalibrationCurves(**arrays), n_samples=L)
    bad.add(p, t, c, f)
    torch.cuda.synchronize()
    hit = int((c[:, 0] == x).logical_and(c[:, 1] == y).logical_and(torch.from_numpy(state != 0).to(DEV)).sum())
    assert hit >= 1 and int(bad.EnergyEvaluator.flags.item()) == 16 and int(good.EnergyEvaluator.flags.item()) == 0
    assert not np.isfinite(bad.EnergyEvaluator._recon.E[:len(c)].cpu().numpy()[row])
    full = good.results()
    assert full["ZEvaluator"]["seg_mult_mae_cal"][1].sum() == full["EnergyEvaluator"]["seg_mult_Emape_cal"][1].sum() == len(c)
    # the counts of the flagged evaluator, read past the check: the row is absent from every table
    from waveformml_amd.psd.eval_common import read_back
    for ev_bad in (bad.ZEvaluator, bad.EnergyEvaluator):
        cur = read_back(ev_bad.tables)
        for name, shape, pair in ev_bad._layout:
            if pair:
                n, _s = cur.take_pair(shape)
                if name.startswith("seg_mult"):
                    assert int(n.sum()) == len(c) - hit, name
            else:
                cur.take(shape)
    with pytest.raises(RuntimeError, match="not finite"):
        bad.results()
    with pytest.raises(RuntimeError, match="not finite"):
        bad.EnergyEvaluator.results()


def _calibration_file(curves, tmp_path):
    path = str(tmp_path / "curves.npz")
    curves.save(path)
    return path


def test_litz_and_litez_from_a_config_with_a_calibration_file(gold, curves, tmp_path):
    """``dataset_config.calibration_file``: module.evaluator carries the curves, and segment_test_loop fills ``*_cal``."""
    from test_host_mirror import _z_config
    from test_segment_callers import ez_config, segment_rows
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litz import LitEZ, LitZ
    from waveformml_amd.psd.segment_evaluator import EZEvaluator, ZEvaluator
    path = _calibration_file(curves, tmp_path)
    rng = np.random.default_rng(23)
    pool = gold["k_L40_f32_rows"][gold["k_L40_f32_state"] >= 2]                 # L = 40 waveforms with peaks on both sides
    for cls, cfg, ev_cls, width in ((LitZ, _z_config(["waveformml_amd.spconv"]), ZEvaluator, 1),
                                    (LitEZ, ez_config(["waveformml_amd.spconv"]), EZEvaluator, 2)):
        cfg = copy.deepcopy(cfg)
        cfg["system_config"]["n_samples"] = 20
        cfg["dataset_config"]["calibration_file"] = path
        torch.manual_seed(5)
        mod = cls(load_config(cfg)).to(DEV)
        ev = mod.evaluator
        assert isinstance(ev, ev_cls) and ev.calibration is not None
        assert np.array_equal(ev.calibration.light_sum_curves, gold["cal_light_sum_curves"])
        zev = ev if width == 1 else ev.ZEvaluator
        assert zev._recon.n_samples == 20
        batches = []
        for B in (7, 5):
            rows, c, _f = segment_rows(rng, B, 4, 40)
            f = torch.from_numpy(pool[rng.integers(0, len(pool), len(rows))][:, list(range(20)) + list(range(40, 60))].copy())
            t = torch.from_numpy((0.1 + 0.8 * rng.random((len(rows), width))).astype(np.float32))
            batches.append(([c, f], t[:, 0] if width == 1 else t))
        out = segment_test_loop(mod, copy.deepcopy(batches), DEV, evaluator=ev)
        n = sum(len(b[0][0]) for b in batches)
        res = out["evaluation"] if width == 1 else out["evaluation"]["ZEvaluator"]
        assert out["rows"] == n and res["seg_mult_mae"][1].sum() == n and res["seg_mult_mae_cal"][1].sum() == n
        assert res["seg_mult_mae_cal"][0].sum() > 0
        if width == 2:
            e = out["evaluation"]["EnergyEvaluator"]
            assert e["seg_mult_Emape_cal"][1].sum() == n and (e["E_z_single"][1].sum() + e["E_z_dual"][1].sum()) == n
