"""Generates tests/golden/calibrated_z_cases.npz from the REFERENCE's own arithmetic (the reference tree, this container
only): waveform rows, synthetic calibration curves, and what the reference's classical reconstruction and its evaluators'
``hascal`` branches give for them.  No reference text is written anywhere; the npz holds arrays only.

How the reference is run (the method of make_z_real_evaluator_goldens.py)
  * numba is not installed here, so the functions are taken from the syntax trees IN MEMORY, their ``@nb.jit`` decorators
    dropped, and executed unmodified: calc_calib_z_E and everything under it, z_deviation_with_E, z_error,
    E_deviation_with_z, z_basic_prediction_dense, get_bin_index (src/utils/SparseUtils.py) and the sorts of
    src/utils/NumbaFunctions.py.  ``log`` is numba's (NaN for a negative argument, where math.log raises).
  * They get float64 arrays that hold the fp32 (or rounded 16-bit) values.  The bodies of ZEvaluatorWF.add / z_from_cal,
    EnergyEvaluatorWF.add / z_E_from_cal / calc_deviation_with_z and EZEvaluatorBase.add are repeated call for call; the
    per-row state and the culled peak lists are the first lines of calc_calib_z_E's loop, repeated.
  * The curves are synthetic but shaped like real ones: monotone light_pos / time_pos, positive light_sum, some PMTs with and
    some without a t_interp curve, sampletime nonzero where there is one.
  * The generator FAILS rather than records a case in which a maximum's value is exactly 0, a side has more than 41 maxima
    (the reference's sort stops sorting there), a divisor is zero (numpy raises), |z| lies within 1e-6 of 650 without
    being on it, a dRpos within 1e-12 of 0 without being 0, or a binned value lies within 1e-6 of its range of an
    interior edge that it is not exactly on.
  * find_peaks cannot return sample 0 (a maximum closes at a fall after a rise, so it sits at 1 or later): the "peak at the
    row's start" cases have their peak at sample 1, with sample 0 below and above half height.

Run:  python tests/golden/make_calibrated_z_goldens.py
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_pid_evaluator_goldens as mp                                   # noqa: E402
import make_segment_evaluator_goldens as sg                               # noqa: E402
from make_z_real_evaluator_goldens import check_clear                     # noqa: E402

SPARSE = ["calc_calib_z_E", "find_peaks", "cull_peaks", "remove_end_zeros", "match_peaks", "excluded_inds", "peak_to_z",
          "peak_to_dt", "z_dt_to_z", "z_from_total_light", "calc_arrival_from_peak", "calc_size", "get_residual",
          "sum_range", "sum1d", "lin_interp", "z_deviation_with_E", "z_error", "is_in_sample", "sample_index",
          "E_deviation_with_z", "z_basic_prediction_dense", "get_bin_index"]
SORTS = ["merge_numba", "merge_numba_two", "insertion_sort_numba", "insertion_sort_numba_two", "merge_sort_numba",
         "merge_sort_numba_two", "merge_sort_main_numba", "merge_sort_two"]
NX, NY = 14, 11
MAX_RANGE = 2 ** 14 - 1                      # src/datasets/HDF5Dataset.py


def numba_log(x):
    with np.errstate(all="ignore"):
        return float(np.log(np.float64(x)))


def checked_abs(x):
    if isinstance(x, (float, np.floating)):
        assert x == 0 or not abs(x) < 1e-12, "a dRpos within 1e-12 of 0: %r" % x
    return abs(x)


def reference():
    import ast
    ntree = mp._tree("src", "utils", "NumbaFunctions.py")
    small = [n for n in ntree.body if isinstance(n, ast.Assign) and n.targets[0].id == "SMALL_MERGESORT_NUMBA"][0]
    sorts = mp._functions(ntree, SORTS, dict(np=np, SMALL_MERGESORT_NUMBA=ast.literal_eval(small.value)))
    inner = sorts["merge_sort_two"]

    def merge_sort_two(A, C, sort="d"):
        assert len(A) <= 41, "more than 41 maxima on a side"
        assert len(A) == len(C) and not (np.asarray(A) == 0).any(), "a maximum whose value is exactly 0"
        return inner(A, C, sort)
    ns = dict(zeros=np.zeros, int32=np.int32, float32=np.float32, floor=math.floor, log=numba_log, sqrt=math.sqrt,
              MAX_RANGE=MAX_RANGE, abs=checked_abs, merge_sort_two=merge_sort_two,
              merge_sort_main_numba=sorts["merge_sort_main_numba"], print=print)
    raw = mp._functions(mp._tree("src", "utils", "SparseUtils.py"), SPARSE, ns)
    for name in ("peak_to_z", "z_from_total_light"):
        def wrap(f):
            def g(*a, **k):
                out = f(*a, **k)
                z = out[0]
                assert abs(z) == 650 or abs(abs(z) - 650) > 1e-6, "|z| within 1e-6 of 650: %r" % z
                return out
            return g
        raw[name] = wrap(raw[name])
    return raw


def synthetic_curves(rng):
    """float32, the shapes of Calibrator.__init__."""
    f = np.float32
    gains = rng.uniform(300., 600., (NX, NY, 2)).astype(f)
    eres = rng.uniform(80., 120., (NX, NY, 2)).astype(f)
    rel = rng.uniform(-2., 2., (NX, NY)).astype(f)
    st = np.zeros((NX, NY, 2), f)
    tint = np.zeros((NX, NY, 2, 50, 2), f)
    tpos = np.zeros((NX, NY, 50, 2), f)
    lpos = np.zeros((NX, NY, 51, 2), f)
    lsum = np.zeros((NX, NY, 50, 2), f)
    for x in range(NX):
        for y in range(NY):
            for r in range(2):
                if rng.random() < 0.6:
                    xs = np.linspace(0., 4., 50)
                    tint[x, y, r, :, 0] = xs
                    tint[x, y, r, :, 1] = xs + rng.uniform(0.1, 0.4) * np.sin(np.pi * xs / 4.)     # monotone
                    st[x, y, r] = round(max(xs))
            dts = np.linspace(-14., 14., 50)
            tpos[x, y, :, 0], tpos[x, y, :, 1] = dts, rng.uniform(55., 65.) * dts + rng.uniform(-10., 10.)
            R = np.linspace(-4., 4., 51)
            lpos[x, y, :, 0] = R
            lpos[x, y, :, 1] = rng.uniform(380., 420.) * R + rng.uniform(-5., 5.)                       # to beyond +-650
            zs = np.linspace(-600., 600., 50)
            lsum[x, y, :, 0] = zs
            lsum[x, y, :, 1] = rng.uniform(250., 350.) * (1. + 0.25 * (zs / 600.) ** 2)
    assert (np.diff(lpos[..., 1], axis=2) > 0).all() and (np.diff(tpos[..., 1], axis=2) > 0).all() and (lsum[..., 1] > 0).all()
    assert (np.diff(tint[..., 1], axis=3)[tint[..., 10, 0] != 0] > 0).all() and ((st != 0) == (tint[..., 10, 0] != 0)).all()
    return dict(gains=gains, eres=eres, rel_times=rel, sampletime=st, t_interp_curves=tint, time_pos_curves=tpos,
                light_pos_curves=lpos, light_sum_curves=lsum)


def pulses(L, spec):
    """A side as a sum of pulses (position, amplitude[, rise, decay]): a Gaussian rise, an exponential tail."""
    t = np.arange(L, dtype=np.float64)
    v = np.zeros(L)
    for p in spec:
        pos, amp = p[0], p[1]
        rise, decay = (p[2], p[3]) if len(p) > 2 else (1.6, 5.0)
        v += amp * np.where(t <= pos, np.exp(-0.5 * ((t - pos) / rise) ** 2), np.exp(-(t - pos) / decay))
    return v


def spread(rng, L, k, lo=4):
    """k pulse positions more than 21 samples apart in [lo, L - 3)."""
    while True:
        pos = np.sort(rng.integers(lo, max(lo + 1, L - 3), k))
        if k == 1 or np.diff(pos).min() > 21:
            return [int(p) for p in pos]


def random_side(rng, L, k, amp=(0.004, 0.07)):
    return pulses(L, [(p, rng.uniform(*amp), rng.uniform(1.0, 2.2), rng.uniform(3.0, 7.0)) for p in spread(rng, L, k)])


def crafted_rows(rng, L):
    """(name, side 0, side 1): the routes of calc_calib_z_E that random pulses do not reach by themselves."""
    Z, out = np.zeros(L), []
    tiny = pulses(L, [(L // 2, 0.0012)])                                   # below cull_peaks' 30 ADC counts
    one = lambda a=0.03, p=None: pulses(L, [(L // 3 if p is None else p, a)])
    out.append(("all_zero", Z, Z))                                        # state 0
    out.append(("both_tiny", tiny, tiny * 0.9))                           # maxima, none survives the cull
    out.append(("constant", np.full(L, 0.01), np.full(L, 0.02)))
    out.append(("left_only", one(), Z))                                   # state 1, r = 0
    out.append(("right_only", tiny, one(0.05)))                           # state 1, r = 1
    out.append(("peak_at_1_low_start", pulses(L, [(1, 0.04, 0.5, 4.0)]), one(0.03, 2)))    # sample 0 below half height
    out.append(("peak_at_1_high_start", pulses(L, [(1, 0.04, 3.0, 4.0)]), one(0.03, 3)))   # sample 0 above it
    out.append(("peak_near_end", one(0.03, L - 4), one(0.04, L - 9)))     # calc_size clamped at the end
    out.append(("peak_last_fall", one(0.03, L - 2), one(0.04, L - 2)))
    out.append(("bright_right", one(0.012), one(0.3)))                    # the light ratio beyond the clamp at +650
    out.append(("bright_left", one(0.3), one(0.012)))                     # and at -650
    v = Z.copy(); v[5], v[6], v[7] = 0.0, 0.01, -0.01                     # L[0] == 0: the window sums to exactly 0
    out.append(("zero_light_left", v, one(0.03, 7)))
    v = Z.copy(); v[6:12] = [0.0, 0.02, -0.01, -0.02, -0.02, -0.01]       # a negative sum: log of a negative ratio
    out.append(("invalid_ratio", v, one(0.03, 8)))
    eq = Z.copy(); eq[4:9] = [0.0, 0.02, 0.04, 0.02, 0.01]; eq[12:17] = [0.01, 0.02, 0.04, 0.02, 0.0]
    out.append(("equal_maxima_close", eq, one(0.03, 8)))                  # 6 and 14: the stable order keeps 6
    fl = Z.copy(); fl[4:11] = [0.0, 0.01, 0.03, 0.03, 0.03, 0.01, 0.0]
    out.append(("flat_top", fl, pulses(L, [(7, 0.05)])))
    if L >= 64:
        eq = Z.copy(); eq[5:8] = [0.02, 0.04, 0.02]; eq[40:43] = [0.02, 0.04, 0.02]
        out.append(("equal_maxima_apart", eq, pulses(L, [(7, 0.03), (42, 0.05)])))
        out.append(("two_two", pulses(L, [(8, 0.03), (40, 0.05)]), pulses(L, [(9, 0.04), (41, 0.02)])))
        out.append(("one_two", one(0.04, 30), pulses(L, [(10, 0.03), (40, 0.05)])))            # n0 < n1
        out.append(("two_one", pulses(L, [(10, 0.03), (40, 0.05)]), one(0.04, 20)))            # n0 > n1
    if L >= 120:
        v = Z.copy(); v[60:68] = [0.0, 0.01, 0.03, 0.05, 0.05, 0.05, 0.02, 0.0]
        out.append(("plateau_across_chunks", v, one(0.03, 62)))
        five = pulses(L, [(6 + 24 * i, 0.02 + 0.005 * i) for i in range(5)])
        out.append(("five_peaks", five, one()))                           # five survive: the side counts as having none
        out.append(("five_five", five, five[::1] * 1.1))                  # state 0 with ten peaks
        out.append(("four_three", pulses(L, [(6 + 30 * i, 0.02 + 0.004 * i) for i in range(4)]),
                    pulses(L, [(8 + 40 * i, 0.05 - 0.01 * i) for i in range(3)])))
        out.append(("three_three", pulses(L, [(10 + 40 * i, 0.02 + 0.01 * i) for i in range(3)]),
                    pulses(L, [(12 + 40 * i, 0.04 - 0.01 * i) for i in range(3)])))
        out.append(("one_four", one(0.05, 70), pulses(L, [(6 + 30 * i, 0.02 + 0.004 * i) for i in range(4)])))
        bumps = sum(pulses(L, [(int(p), 0.0009, 0.8, 0.8)]) for p in range(5, L - 5, 7))    # many small maxima
        out.append(("bumpy", bumps + pulses(L, [(30, 0.03), (90, 0.05)]), bumps * 0.8 + pulses(L, [(32, 0.04)])))
        six = pulses(L, [(4 + 23 * i, 0.03 - 0.002 * i, 1.0, 2.0) for i in range(6)])
        out.append(("six_maxima", six, pulses(L, [(20, 0.03), (80, 0.02)])))                  # the greedy stop at five
    return out


def kernel_rows(rng, L, n_random):
    named = crafted_rows(rng, L)
    rows = [np.concatenate([a, b]) for _n, a, b in named]
    kmax = 4 if L >= 120 else (2 if L >= 64 else 1)
    for _ in range(n_random):
        k0, k1 = rng.integers(0, kmax + 1), rng.integers(1, kmax + 1)
        a = random_side(rng, L, k0) if k0 else np.zeros(L)
        rows.append(np.concatenate([a, random_side(rng, L, k1)]))
    return np.array(rows), [n for n, _a, _b in named]


def events(rng, counts):
    co = []
    for e, n in enumerate(counts):
        cells = rng.permutation(NX * NY)[:n]
        co += [(c // NY, c % NY, e) for c in cells]
    return np.array(co, np.int32).reshape(-1, 3)


class Recon:
    """calc_calib_z_E with a Calibrator's arrays; per row what its maps hold, the state and the culled peaks."""

    def __init__(self, raw, curves, z_scale, sample_width=4):
        self.raw, self.c, self.z_scale, self.sw = raw, curves, float(z_scale), sample_width
        self.gain_factor = np.divide(np.full((NX, NY, 2), MAX_RANGE), curves["gains"])     # ZEvaluatorWF.__init__
        assert self.gain_factor.dtype == np.float64

    def maps(self, coo, f, B, dtype=np.float64):
        z, E = np.zeros((B, NX, NY), dtype), np.zeros((B, NX, NY), dtype)
        c = self.c
        with np.errstate(divide="raise", over="raise", invalid="raise"):
            self.raw["calc_calib_z_E"](coo, f, z, E, self.sw, c["t_interp_curves"], c["sampletime"], c["rel_times"],
                                       self.gain_factor, c["eres"], c["time_pos_curves"], c["light_pos_curves"],
                                       c["light_sum_curves"], self.z_scale, f.shape[1] // 2)
        return z, E

    def rows(self, coo, f):
        B = int(coo[:, 2].max()) + 1
        z, E = self.maps(coo, f, B)
        n = f.shape[1] // 2
        state, peaks = np.zeros(len(coo), np.int32), np.full((len(coo), 2, 5), -1, np.int32)
        for i, wf in enumerate(f):
            culled = []
            for s in range(2):                                              # the head of calc_calib_z_E's loop
                side = wf[s * n:(s + 1) * n]
                local, cul = np.full(5, -1, np.int32), np.full(5, -1, np.int32)
                maxloc = self.raw["find_peaks"](side, local, 10)
                self.raw["cull_peaks"](local, cul, side, maxloc)
                peaks[i, s] = cul
                culled.append(self.raw["remove_end_zeros"](cul, -1))
            a, b = culled
            state[i] = 0 if a is None and b is None else 1 if a is None or b is None else 2 if len(a) == len(b) else 3
        return z[coo[:, 2], coo[:, 0], coo[:, 1]], E[coo[:, 2], coo[:, 0], coo[:, 1]], state, peaks


def main():
    raw = reference()
    rng = np.random.default_rng(20250611)
    curves = synthetic_curves(rng)
    zd, seg, z_fresh = sg.z_reference_setup()
    ed, e_fresh = sg.energy_reference_setup()
    _res, sample_segs = z_fresh()
    sample_segs = np.asarray(sample_segs)
    out = {"cal_" + k: v for k, v in curves.items()}
    out["seg_status"], out["sample_segs"] = seg, sample_segs
    for k in ("nmult", "n_bins", "n_err_bins", "error_low", "error_high", "z_scale", "E_low", "E_high", "true_E_high",
              "E_scale"):
        out["z_default_" + k] = np.float64(zd[k])
    for k in ("n_mult", "n_E", "n_z", "E_scale", "z_scale"):
        out["e_default_" + k] = np.float64(ed[k])
    out["e_default_E_bounds"] = np.asarray(ed["E_bounds"], np.float64)
    recon = Recon(raw, curves, zd["z_scale"])
    assert ed["z_scale"] == zd["z_scale"]

    # ---- the kernel alone
    names, seen_states, seen_counts = [], set(), set()
    plans = [("L150_f32", 150, "f32", 92, 12, 0), ("L150_bf16", 150, "bf16", 6, 3, 0), ("L150_f16", 150, "f16", 6, 2, 0),
             ("L64_f32", 64, "f32", 10, 3, 0), ("L64_bf16", 64, "bf16", 4, 2, 0), ("L64_f16", 64, "f16", 4, 1, 0),
             ("L40_f32", 40, "f32", 9, 3, 0), ("L40_bf16", 40, "bf16", 4, 2, 0), ("L40_f16", 40, "f16", 4, 1, 7),
             ("one_row", 150, "f32", 1, 1, 0), ("padded", 150, "f32", 12, 3, 9)]
    for name, L, dt, n_random, n_events, pad in plans:
        if name == "one_row":
            rows, pat = np.concatenate([random_side(rng, L, 2), random_side(rng, L, 2)])[None], []
        elif name == "padded":
            rows, pat = kernel_rows(rng, L, n_random)
            rows, pat = rows[-n_random:], []
        else:
            rows, pat = kernel_rows(rng, L, n_random)
        cuts = np.sort(rng.choice(np.arange(1, len(rows)), n_events - 1, replace=False)) if n_events > 1 else []
        counts = np.diff(np.concatenate([[0], cuts, [len(rows)]])).astype(int)
        assert len(counts) == n_events and counts.min() >= 1 and len(rows) <= 125
        rows = mp.rounded(rows, dt)
        coo = events(rng, counts)
        z, E, state, peaks = recon.rows(coo, rows.astype(np.float64))
        seen_states |= set(state.tolist())
        seen_counts |= {((p[0] >= 0).sum(), (p[1] >= 0).sum()) for p in peaks}
        n_valid = -1
        if pad:                                  # rows beyond the valid count: never read
            n_valid = len(rows)
            rows = np.concatenate([rows, np.full((pad, 2 * L), np.nan, np.float32)])
            coo = np.concatenate([coo, np.tile(np.array([[-3, 50, 999]], np.int32), (pad, 1))])
        k = "k_" + name
        out[k + "_rows"], out[k + "_coords"], out[k + "_z"], out[k + "_E"] = rows.astype(np.float32), coo, z, E
        out[k + "_state"], out[k + "_peaks"], out[k + "_patterns"] = state, peaks, np.array(pat)
        out[k + "_L"], out[k + "_dtype"], out[k + "_n_valid"] = np.int64(L), np.array(dt), np.int64(n_valid)
        names.append(name)
        print("kernel case %s: %d rows, states %s" % (name, len(state), np.bincount(state, minlength=4)))
    out["kernel_names"] = np.array(names)
    assert seen_states == {0, 1, 2, 3}, seen_states
    assert any(a == 5 for a, _b in seen_counts) and any(0 < a < b for a, b in seen_counts) and \
        any(a > b > 0 for a, b in seen_counts), seen_counts
    s150 = {n: i for i, n in enumerate(out["k_L150_f32_patterns"].tolist())}
    st, zz = out["k_L150_f32_state"], (out["k_L150_f32_z"] - 0.5) * zd["z_scale"]
    assert st[s150["five_peaks"]] == 1 and st[s150["five_five"]] == 0 and st[s150["one_two"]] == 3 and st[s150["two_one"]] == 3
    # z * E / E / z_scale + 0.5 and back: the clamp's 650 to rounding
    assert abs(zz[s150["bright_right"]] - 650) < 1e-9 and abs(zz[s150["bright_left"]] + 650) < 1e-9, "the clamp was not reached"
    assert out["k_L150_f32_peaks"][s150["equal_maxima_close"], 0, 0] == 6 and st[s150["zero_light_left"]] == 2
    assert zz[s150["zero_light_left"]] == 0 and st[s150["invalid_ratio"]] == 2 and st[s150["five_peaks"]] == 1

    # ---- the evaluators: ZEvaluatorWF.add / z_from_cal, EnergyEvaluatorWF.add / calc_deviation_with_z, call for call
    nx, ny = NX, NY
    z_keys = ["seg_mult_mae", "z_mult_mae_single", "z_mult_mae_dual", "E_mult_mae_single", "E_mult_mae_dual"]
    e_keys = ["seg_mult_Emape", "E_mult_single", "E_mult_dual", "E_z_single", "E_z_dual"]
    out["z_pair_keys"], out["e_pair_keys"] = np.array(z_keys), np.array(e_keys)

    def z_walks(res, cal, coo, p, t, E, E_high):
        r = lambda k: res[k + cal]
        raw["z_deviation_with_E"](coo, p, t, r("seg_mult_mae")[0], r("seg_mult_mae")[1], r("z_mult_mae_dual")[0],
                                  r("z_mult_mae_dual")[1], r("z_mult_mae_single")[0], r("z_mult_mae_single")[1], seg, nx,
                                  ny, zd["nmult"], zd["n_bins"], zd["z_scale"], E, r("E_mult_mae_dual")[0],
                                  r("E_mult_mae_dual")[1], r("E_mult_mae_single")[0], r("E_mult_mae_single")[1],
                                  zd["E_low"], E_high)
        raw["z_error"](coo, p, t, res["seg_sample_error" + cal], zd["n_err_bins"], zd["error_low"], zd["error_high"],
                       zd["nmult"], sample_segs, zd["z_scale"])
        err = (p - t)[coo[:, 2], coo[:, 0], coo[:, 1]] * zd["z_scale"]
        check_clear("z error", err, zd["error_low"], zd["error_high"], zd["n_err_bins"])
        check_clear("E axis", E[coo[:, 2], coo[:, 0], coo[:, 1]], zd["E_low"], E_high, zd["n_bins"])

    def z_add(res, coo, pz, tz, f, E_map, target_is_cal):
        """ZEvaluatorWF.add with hascal; E_map: the float32 true-energy map or None."""
        B = pz.shape[0]
        E = None if E_map is None else (E_map * np.float32(zd["E_scale"])).astype(np.float64)
        E_high = zd["E_high"] if E_map is None else zd["true_E_high"]                          # set_true_E
        # z_from_cal
        pred, cal_E = recon.maps(coo, f, B)
        if target_is_cal:
            tz32 = tz.astype(np.float32)                                   # the target map as the module hands it over
            assert (tz32 == tz).all()
            pred = np.zeros((B, nx, ny), np.float32)                       # get_dense_matrix(torch.full(.., 0.5), c)
            pred[coo[:, 2], coo[:, 0], coo[:, 1]] = 0.5
            pred[:, seg != 0.5] = tz32[:, seg != 0.5]
            raw["z_basic_prediction_dense"](coo, pred, tz32, True)
            pred = pred.astype(np.float64)
        if E is None:
            E = cal_E
        z_walks(res, "_cal", coo, pred, tz, E, E_high)
        z_walks(res, "", coo, pz, tz, E, E_high)

    def e_add(res, coo, pe, te, f):
        """EnergyEvaluatorWF.add with hascal: z_E_from_cal's float32 maps, then calc_deviation_with_z."""
        Z, E = recon.maps(coo, f, pe.shape[0], np.float32)
        Z, E = Z.astype(np.float64), E.astype(np.float64)
        for cal, p in (("", pe), ("_cal", E)):
            r = lambda k: res[k + cal]
            raw["E_deviation_with_z"](coo, p, te, r("seg_mult_Emape")[0], r("seg_mult_Emape")[1], r("E_mult_dual")[0],
                                      r("E_mult_dual")[1], r("E_mult_single")[0], r("E_mult_single")[1], seg, nx, ny,
                                      ed["n_mult"], ed["n_E"], ed["E_bounds"][0], ed["E_bounds"][1], ed["E_scale"],
                                      ed["z_scale"], Z, r("E_z_dual")[0], r("E_z_dual")[1], r("E_z_single")[0],
                                      r("E_z_single")[1])
        at = (coo[:, 2], coo[:, 0], coo[:, 1])
        check_clear("E target", te[at] * ed["E_scale"], ed["E_bounds"][0], ed["E_bounds"][1], ed["n_E"])
        check_clear("cal z", (Z[at] - 0.5) * ed["z_scale"], -ed["z_scale"] / 2., ed["z_scale"] / 2., ed["n_E"])

    S = [tuple(int(v) for v in s) for s in sample_segs]
    single = [tuple(int(v) for v in c) for c in np.argwhere(seg == 0.5)]
    dead = [tuple(int(v) for v in c) for c in np.argwhere(seg == 1.0)]

    def batch(counts, forced, L, dt, pad=0):
        zd2 = dict(zd)
        coo, pred, targ = sg.build_batch(rng, counts, forced, dt, zd2, ed, [])
        rows, _pat = kernel_rows(rng, L, 0)
        pick = rng.permutation(len(rows))
        extra = len(coo) - len(rows)
        if extra > 0:
            more = kernel_rows(rng, L, extra)[0][-extra:]
            rows = np.concatenate([rows[pick], more])
        else:
            rows = rows[pick][:len(coo)]
        rows = rows[rng.permutation(len(rows))]
        return dict(coords=coo, pred=pred, targ=targ, feats=mp.rounded(rows, dt), pad=pad)

    ev_names = []

    def ev_case(name, batches):
        zE, z0, zT, en = z_fresh()[0], z_fresh()[0], z_fresh()[0], e_fresh()
        for b, bt in enumerate(batches):
            coo, pred, targ, f = bt["coords"], bt["pred"], bt["targ"], bt["feats"].astype(np.float64)
            p64, t64 = pred.astype(np.float64), targ.astype(np.float64)
            # EZEvaluatorBase.add: plane 0 to the energy evaluator, plane 1 to the z evaluator with E = target plane 0
            e_add(en, coo, p64[:, 0], t64[:, 0], f)
            z_add(zE, coo, p64[:, 1], t64[:, 1], f, targ[:, 0], False)
            z_add(z0, coo, p64[:, 1], t64[:, 1], f, None, False)           # ZEvaluatorWF.add without E
            z_add(zT, coo, p64[:, 1], t64[:, 1], f, targ[:, 0], True)      # target_is_cal
            check_clear("true z", (t64[:, 1][coo[:, 2], coo[:, 0], coo[:, 1]] - 0.5) * zd["z_scale"],
                        -zd["z_scale"] / 2., zd["z_scale"] / 2., zd["n_bins"])
            n_valid, feats = -1, bt["feats"]
            if bt["pad"]:
                n_valid = len(coo)
                coo = np.concatenate([coo, np.tile(np.array([[-3, 50, 999]], np.int32), (bt["pad"], 1))])
                feats = np.concatenate([feats, np.full((bt["pad"], feats.shape[1]), np.nan, np.float32)])
            tag = "ev_%s_b%d_" % (name, b)
            out[tag + "coords"], out[tag + "pred"], out[tag + "targ"], out[tag + "feats"] = coo, pred, targ, feats
            out[tag + "n_valid"] = np.int64(n_valid)
        for kind, res, keys in (("zE_", zE, z_keys), ("z0_", z0, z_keys), ("zT_", zT, z_keys), ("e_", en, e_keys)):
            for cal in ("", "_cal"):
                for k in keys:
                    out["ev_%s_%s%s%s_sum" % (name, kind, k, cal)] = res[k + cal][0].copy()
                    out["ev_%s_%s%s%s_n" % (name, kind, k, cal)] = res[k + cal][1].copy()
                if kind != "e_":
                    out["ev_%s_%sseg_sample_error%s" % (name, kind, cal)] = res["seg_sample_error" + cal].copy()
        out["ev_%s_nb" % name], out["ev_%s_dtype" % name] = np.int64(len(batches)), np.array(batches[0]["dtype"])
        assert zE["seg_mult_mae_cal"][1].sum() > 0 and en["E_z_single_cal"][1].sum() + en["E_z_dual_cal"][1].sum() > 0
        assert zE["seg_sample_error_cal"].sum() > 0 and z0["E_mult_mae_dual_cal"][1].sum() > 0
        ev_names.append(name)
        print("evaluator case %s done" % name)

    def with_dtype(dt, bts):
        for bt in bts:
            bt["dtype"] = dt
        return bts
    forced_a = {0: [S[0], single[0]], 1: [S[1], S[2], dead[0], single[1]], 2: [S[0], S[1], S[2], single[2], single[3]], 3: [S[2]]}
    forced_b = {0: [S[1], single[4]], 1: [S[0], S[2], single[0], dead[0]], 2: [S[1]]}
    ev_case("two_adds_f32", with_dtype("f32", [batch([6, 7, 12, 1], forced_a, 150, "f32"),
                                               batch([9, 11, 2], forced_b, 150, "f32")]))
    ev_case("bf16", with_dtype("bf16", [batch([5, 7, 8], forced_b, 64, "bf16")]))
    ev_case("f16", with_dtype("f16", [batch([7, 4, 6], forced_b, 40, "f16")]))
    ev_case("padded", with_dtype("f32", [batch([4, 6, 5], forced_b, 64, "f32", pad=10)]))
    out["case_names"] = np.array(ev_names)
    path = os.path.join(HERE, "calibrated_z_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote calibrated_z_cases.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
