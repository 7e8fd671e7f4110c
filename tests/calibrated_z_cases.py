"""What tests/test_gpu_calibrated_z.py and tests/test_calibration_host.py share: the recorded cases of
tests/golden/calibrated_z_cases.npz (made by tests/golden/make_calibrated_z_goldens.py from the reference's own
functions) and their layout.

Layout of the file
  cal_<name>                  the eight calibration arrays, float32, the shapes of psd/calibration.SHAPES
  seg_status, sample_segs, z_default_*, e_default_*   the reference evaluators' constants
  kernel_names                the cases of the reconstruction alone; per case k_<case>_:
      rows [n, 2 L] float32 (values already rounded to the case's dtype), coords int32 [n, 3], L, dtype, n_valid (-1: all
      rows; else the rows behind it are padding, NaN, never to be read), patterns (names of the leading crafted rows),
      z, E float64 [valid rows] (what calc_calib_z_E leaves in its maps), state int32 (0 skipped, 1 one side, 2 equal
      counts, 3 unequal counts), peaks int32 [valid rows, 2, 5] (the culled peak lists, -1 behind them)
  case_names                  the evaluator cases; per case ev_<case>_: nb batches b<i>_{coords, pred, targ, feats, n_valid}
      (pred, targ [B, 2, 14, 11] float32 in the order EZEvaluatorBase.add reads: plane 0 energy, plane 1 z), dtype, and the
      tables after all batches as <kind><table>[_cal]_{sum, n} / <kind>seg_sample_error[_cal], kinds zE_ (ZEvaluatorWF.add
      with the true energy), z0_ (without), zT_ (with it and target_is_cal), e_ (EnergyEvaluatorWF.add)
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calibrated_z_cases.npz")
CURVES = ("gains", "eres", "rel_times", "sampletime", "t_interp_curves", "time_pos_curves", "light_pos_curves",
          "light_sum_curves")
Z_PAIRS = ("seg_mult_mae", "z_mult_mae_single", "z_mult_mae_dual", "E_mult_mae_single", "E_mult_mae_dual")
E_PAIRS = ("seg_mult_Emape", "E_mult_single", "E_mult_dual", "E_z_single", "E_z_dual")
REL = 1e-5                                   # the project's bar for recorded values: of the largest recorded magnitude


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def curves_of(gold):
    from waveformml_amd.psd.calibration import CalibrationCurves
    return CalibrationCurves(**{k: gold["cal_" + k] for k in CURVES})


def assert_tables_match(res, gold, prefix, pairs, hists=()):
    """Counts and histograms exactly, float sums within REL of the recorded table's largest magnitude; the worst float
    error in units of that scale."""
    worst = 0.0
    for cal in ("", "_cal"):
        for k in pairs:
            s, n = res[k + cal]
            ws, wn = gold[prefix + k + cal + "_sum"], gold[prefix + k + cal + "_n"]
            assert np.array_equal(n, wn), (prefix, k + cal, int(np.abs(n.astype(np.int64) - wn).sum()))
            scale = float(np.abs(ws).max())
            if scale > 0:
                err = float(np.abs(s.astype(np.float64) - ws).max()) / scale
                worst = max(worst, err)
                assert err <= REL, (prefix, k + cal, err)
            else:
                assert not s.any(), (prefix, k + cal)
        for k in hists:
            assert np.array_equal(res[k + cal], gold[prefix + k + cal]), (prefix, k + cal)
    return worst
