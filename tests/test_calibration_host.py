"""CPU checks of the calibrated-baseline feature: the CalibrationCurves holder (psd/calibration.py), the messages that
still refuse ``calgroup=``, the layout of the recorded cases, and the new entry points in the header.  No kernel runs."""
import os
import re

import numpy as np
import pytest

import calibrated_z_cases as cc
from waveformml_amd.psd import calibration as cal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


def arrays(gold):
    return {k: gold["cal_" + k].copy() for k in cc.CURVES}


def test_save_load_round_trip(gold, tmp_path):
    curves = cc.curves_of(gold)
    path = str(tmp_path / "curves.npz")
    curves.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(cal.SHAPES)
    back = cal.CalibrationCurves.load(path)
    for k, shape in cal.SHAPES.items():
        a = getattr(back, k)
        assert a.dtype == np.float32 and a.shape == shape and np.array_equal(a, gold["cal_" + k]), k
    assert tuple(cc.CURVES) == tuple(cal.SHAPES)
    assert cal.SHAPES["t_interp_curves"] == (14, 11, 2, 50, 2) and cal.SHAPES["light_pos_curves"] == (14, 11, 51, 2)


def test_gain_factor_is_formed_in_float64(gold):
    curves = cc.curves_of(gold)
    g = curves.gain_factor
    assert g.dtype == np.float64 and g.shape == (14, 11, 2)
    # np.divide(np.full((nx, ny, 2), MAX_RANGE), gains) on the float32 gains: the quotient of the widened values
    assert np.array_equal(g, 16383.0 / gold["cal_gains"].astype(np.float64))
    assert not np.array_equal(g, (np.float32(16383.0) / gold["cal_gains"]).astype(np.float64))


@pytest.mark.parametrize("name", cc.CURVES)
def test_validation_names_the_offending_array(gold, name):
    a = arrays(gold)
    a[name] = a[name][..., :1]
    with pytest.raises(ValueError, match=name + " must have shape"):
        cal.CalibrationCurves(**a)
    for bad in (np.nan, np.inf):
        a = arrays(gold)
        a[name].flat[3] = bad
        with pytest.raises(ValueError, match=name + " holds a value that is not finite"):
            cal.CalibrationCurves(**a)


def test_validation_of_keys_gains_and_files(gold, tmp_path):
    a = arrays(gold)
    del a["eres"]
    with pytest.raises(ValueError, match="missing \\['eres'\\]"):
        cal.CalibrationCurves(**a)
    with pytest.raises(ValueError, match="unknown \\['psd_curves'\\]"):
        cal.CalibrationCurves(psd_curves=np.zeros(3), **arrays(gold))
    a = arrays(gold)
    a["gains"][2, 3, 1] = 0
    with pytest.raises(ValueError, match="gains holds a zero"):
        cal.CalibrationCurves(**a)
    a = arrays(gold)
    a["rel_times"] = a["rel_times"].astype(str)
    with pytest.raises(ValueError, match="rel_times must be numeric"):
        cal.CalibrationCurves(**a)
    path = str(tmp_path / "short.npz")
    np.savez(path, **{k: v for k, v in arrays(gold).items() if k != "sampletime"})
    with pytest.raises(ValueError, match="holds exactly"):
        cal.CalibrationCurves.load(path)
    with pytest.raises(RuntimeError, match="GPU only"):
        cc.curves_of(gold).to("cpu")
    with pytest.raises(TypeError, match="CalibrationCurves"):
        cal.CalibratedReconstruction("cuda:0", arrays(gold))


def test_calgroup_still_raises_and_names_calibration():
    """Every place that refused ``calgroup=`` before still does, on the CPU, before anything touches a device."""
    from waveformml_amd.psd.PredictionWriter import PredictionWriter
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    from waveformml_amd.psd.real_z_evaluator import ZEvaluatorRealWFNorm
    from waveformml_amd.psd.tensor_evaluator import TensorEvaluator
    for cls, exc in ((ZEvaluatorRealWFNorm, RuntimeError), (SegEvaluator, RuntimeError), (TensorEvaluator, RuntimeError)):
        with pytest.raises(exc, match="calgroup[^$]*calibration="):
            cls("cuda:0", calgroup="x")
    with pytest.raises(NotImplementedError, match="calgroup[^$]*calibration="):
        PredictionWriter("out.h5", "in.h5", object(), None, calgroup="x")
    assert "calibration=" in cal.CALGROUP_MESSAGE


def test_lit_modules_read_calibration_file(gold, tmp_path):
    from types import SimpleNamespace
    from waveformml_amd.psd.litz import calibration_from_config
    cfg = SimpleNamespace(dataset_config=SimpleNamespace(), system_config=SimpleNamespace(n_samples=20))
    assert calibration_from_config(cfg) == {}
    path = str(tmp_path / "c.npz")
    cc.curves_of(gold).save(path)
    cfg.dataset_config.calibration_file = path
    got = calibration_from_config(cfg)
    assert sorted(got) == ["calibration", "n_samples"] and got["n_samples"] == 20
    assert np.array_equal(got["calibration"].eres, gold["cal_eres"])


def test_golden_layout(gold):
    for k in cc.CURVES:
        assert gold["cal_" + k].dtype == np.float32 and gold["cal_" + k].shape == cal.SHAPES[k]
    has = gold["cal_t_interp_curves"][..., 10, 0] != 0
    assert has.any() and (~has).any() and ((gold["cal_sampletime"] != 0) == has).all()
    assert (np.diff(gold["cal_light_pos_curves"][..., 1], axis=2) > 0).all() and (gold["cal_light_sum_curves"][..., 1] > 0).all()
    names = [str(n) for n in gold["kernel_names"]]
    assert {"L150_f32", "L64_bf16", "L40_f16", "one_row", "padded"} <= set(names)
    states, lengths, dtypes, sizes = set(), set(), set(), []
    for n in names:
        k = "k_%s_" % n
        rows, coo, L = gold[k + "rows"], gold[k + "coords"], int(gold[k + "L"])
        nv = len(rows) if gold[k + "n_valid"] < 0 else int(gold[k + "n_valid"])
        assert rows.dtype == np.float32 and rows.shape == (len(coo), 2 * L) and coo.dtype == np.int32
        assert np.isfinite(rows[:nv]).all() and (nv == len(rows) or np.isnan(rows[nv:]).all())
        for key, shape, dt in (("z", (nv,), np.float64), ("E", (nv,), np.float64), ("state", (nv,), np.int32),
                               ("peaks", (nv, 2, 5), np.int32)):
            assert gold[k + key].shape == shape and gold[k + key].dtype == dt, (n, key)
        assert np.isfinite(gold[k + "z"]).all() and np.isfinite(gold[k + "E"]).all()
        skipped = gold[k + "state"] == 0
        assert not gold[k + "z"][skipped].any() and (gold[k + "z"][gold[k + "state"] == 1] == 0.5).all()
        # unique segments within an event, events in order
        assert (np.diff(coo[:nv, 2]) >= 0).all() and len({tuple(c) for c in coo[:nv]}) == nv
        states |= set(gold[k + "state"].tolist())
        lengths.add(L), dtypes.add(str(gold[k + "dtype"])), sizes.append(nv)
    assert states == {0, 1, 2, 3} and lengths == {150, 64, 40} and dtypes == {"f32", "bf16", "f16"}
    assert min(sizes) == 1 and 100 <= max(sizes) <= 125
    pk = gold["k_L150_f32_peaks"]
    n0, n1 = (pk[:, 0] >= 0).sum(axis=1), (pk[:, 1] >= 0).sum(axis=1)
    assert (n0 == 5).any() and ((n0 > 0) & (n0 < n1) & (n1 < 5)).any() and ((n1 > 0) & (n1 < n0) & (n0 < 5)).any()
    assert (pk[:, :, 0] == 1).any() and (pk.max(axis=(1, 2)) >= 125).any()      # a peak at sample 1, one in the last 25
    for n in (str(c) for c in gold["case_names"]):
        for b in range(int(gold["ev_%s_nb" % n])):
            t = "ev_%s_b%d_" % (n, b)
            B = gold[t + "pred"].shape[0]
            assert gold[t + "pred"].shape == gold[t + "targ"].shape == (B, 2, 14, 11) and gold[t + "feats"].dtype == np.float32
        for kind, pairs in (("zE_", cc.Z_PAIRS), ("z0_", cc.Z_PAIRS), ("zT_", cc.Z_PAIRS), ("e_", cc.E_PAIRS)):
            for k in pairs:
                for calx in ("", "_cal"):
                    s, cnt = gold["ev_%s_%s%s%s_sum" % (n, kind, k, calx)], gold["ev_%s_%s%s%s_n" % (n, kind, k, calx)]
                    assert s.shape == cnt.shape and s.dtype == np.float32 and cnt.dtype == np.int32
        assert gold["ev_%s_zE_seg_mult_mae_cal_n" % n].sum() > 0 and gold["ev_%s_e_E_z_dual_n" % n].sum() > 0
    assert int(gold["ev_padded_b0_n_valid"]) > 0


def test_header_declares_the_new_entry_points():
    from waveformml_amd import _lib
    text = open(os.path.join(ROOT, "include", "wfsparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("wfs_calib_z_E", "wfs_seg_z_accumulate_cal", "wfs_seg_energy_cal_table_ints",
                 "wfs_seg_energy_accumulate_cal"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES or name in _lib.SIGNATURES_CASED, name
    lib = _lib.load()
    assert hasattr(lib, "wfs_calib_z_E") and lib.wfs_abi_version() == _lib.WFS_ABI_VERSION
    for macro, value in (("WFS_CALIB_T_POINTS", cal.T_POINTS), ("WFS_CALIB_TIME_POINTS", cal.TIME_POINTS),
                         ("WFS_CALIB_LIGHT_POINTS", cal.LIGHT_POINTS), ("WFS_CALIB_SUM_POINTS", cal.SUM_POINTS),
                         ("WFS_CALIB_PEAKS", 5)):
        assert re.search(r"#define %s %d\b" % (macro, value), text), macro
    # every set of the calibrated energy tables: the plain set plus two [nE + 2, nz + 2] pairs, twice
    plain = lib.wfs_seg_energy_table_ints(14, 11, 10, 20)
    assert lib.wfs_seg_energy_cal_table_ints(14, 11, 10, 20, 20) == 2 * (plain + 4 * 22 * 22)
