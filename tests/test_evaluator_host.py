"""CPU checks around the GPU PSDEvaluator: the goldens recorded from the reference's helpers load, the NumPy restatement
in tests/evaluator_cases.py reproduces them, the constructor defaults / result keys / shapes of psd/evaluator.py match the
recorded ones, and the header and the ctypes table agree on the new symbols.  No kernel is launched here."""
import inspect
import os
import re

import numpy as np
import pytest

import evaluator_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["wfs_eval_table_ints", "wfs_event_pulse_stats", "wfs_eval_accumulate"]


@pytest.fixture(scope="module")
def gold():
    return ec.load_golden()


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300) + 0.0), (a, b)


def test_goldens_load(gold):
    for T in (20, 150):
        for dt in ("f32", "bf16", "f16"):
            tag = "stats_T%d_%s_" % (T, dt)
            assert gold[tag + "pulses"].shape == (93, 2 * T) and gold[tag + "pulses"].dtype == np.float32
            assert gold[tag + "coords"].shape == (93, 3) and gold[tag + "stats"].shape == (6, 7)
            assert list(gold[tag + "multiplicity"]) == [1, 2, 3, 5, 1, 17, 64]
    assert gold["tab0_labels"].shape == (37,) and gold["tab1_labels"].shape == (24,)
    assert not (np.concatenate([gold["tab0_labels"], gold["tab1_labels"], gold["tab0_predictions"],
                                gold["tab1_predictions"]]) == 2).any()          # the class that no event has
    assert gold["tab0_exact_energy"].sum() == 1


def test_restatement_reproduces_the_recorded_helpers(gold):
    hp = gold["h_pulses"]
    arr = ec.calc_arrival(hp)
    close(arr, gold["h_arrival"])
    close(ec.calc_psd(hp, gold["h_arrival"]), gold["h_psd"])
    close(ec.calc_time(hp), gold["h_time"])
    for k, (a, b) in enumerate(gold["h_ranges"]):
        got = ec.integrate_lininterp_range(hp, np.full(len(hp), a), np.full(len(hp), b))
        ref = gold["h_integ"][:, k]
        assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(hp).sum(axis=1).max()), (a, b)
    T = hp.shape[1]
    x, y, dt, E = gold["h_spread_args"]
    sc, sp = gold["h_spread_coords"], gold["h_spread_pulses"]
    close(ec.calc_spread(sc, sp, T, x, y, dt, E), gold["h_spread"])
    close(ec.calc_spread(sc[:1], sp[:1], T, x, y, dt, E), gold["h_spread_one"])
    close(ec.calc_spread(sc[:2], sp[:2] * 0, T, x, y, dt, E), gold["h_spread_zero"])
    times = np.arange(T) + 0.5
    for w, (tv, nv) in zip(gold["h_moment_weights"], gold["h_moment"]):
        close(ec.moment_variance(times, T, w), tv)
        close(ec.moment_variance(w, T), nv)
    for (tl, tr), ref in zip([(2.0, 3.0), (0.0, 3.0), (2.0, 0.0), (0.0, 0.0)], gold["h_normalize"]):
        coo, a, b, d = ec.normalize_coords([7.0, 9.0], tl, tr, 1.5, 0.6, 4.0)
        close([coo[0], coo[1], a, b, d], ref)
    vals = gold["h_bin_values"]
    for name, (lo, hi, nb) in dict(e=(0.0, 5.0, 100), p=(0.0, 0.6, 100), c=(0.0, 5.0, 10), s=(-0.5, 4.5, 5)).items():
        assert list(ec.metric_bin(vals, lo, hi, nb)) == list(gold["h_metric_bin_" + name]), name
        assert list(ec.confusion_bin(vals, lo, hi, nb)) == list(gold["h_confusion_bin_" + name]), name
    # exactly at `high` the two conventions part: overflow bin for the metric tables, bin 0 for the confusion tables
    at_high = list(vals).index(5.0)
    assert gold["h_metric_bin_c"][at_high] == 11 and gold["h_confusion_bin_c"][at_high] == 0
    assert gold["h_confusion_bin_c"][list(vals).index(7.0)] == -1 and gold["h_confusion_bin_c"][0] == -1


def test_restatement_reproduces_the_recorded_batches(gold):
    """average_pulse as a whole: the reference keeps fp32 running sums where the restatement rounds once, hence 1e-5 of
    each output's scale here (the helpers above agree to 1e-12)."""
    for T in (20, 150):
        for dt in ("f32", "bf16", "f16"):
            tag = "stats_T%d_%s_" % (T, dt)
            got = ec.average_pulse(gold[tag + "coords"], gold[tag + "pulses"], gold["gains"], gold["seg_status"], 7)
            for k in ("avg_coo", "summed", "psdl", "psdr", "energy"):
                ref = gold[tag + k].astype(np.float64)
                assert np.abs(got[k] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30), (tag, k)
            for k in range(6):
                ref = gold[tag + "stats"][k].astype(np.float64)
                assert np.abs(got["stats"][k] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-30), (tag, k)
            assert list(got["multiplicity"]) == list(gold[tag + "multiplicity"])
            assert list(got["n_SE"]) == list(gold[tag + "n_SE"]) and gold[tag + "n_SE"][-1] == 0
            assert ec.average_pulse(gold[tag + "coords"], gold[tag + "pulses"], gold["gains"], gold["seg_status"], 7,
                                    fix_last_event_n_SE=True)["n_SE"][-1] > 0


def test_host_tables_reproduce_the_recorded_tables(gold):
    h = ec.HostTables(3, 20)
    for b in range(2):
        tag = "tab%d_" % b
        s = ec.average_pulse(gold[tag + "coords"], gold[tag + "pulses"], gold["gains"], gold["seg_status"],
                             len(gold[tag + "labels"]))
        h.add(s, gold[tag + "predictions"], gold[tag + "labels"])
    assert np.array_equal(h.t["mult_n"], gold["tab_mult_acc_1"])
    assert np.array_equal(h.t["ene_psd_n"], gold["tab_ene_psd_acc_1"])
    assert np.array_equal(h.t["ene_psd_m"], gold["tab_ene_psd_acc_0"].astype(np.int64))
    assert np.array_equal(h.t["pos_n"], gold["tab_pos_acc_1"])
    assert np.array_equal(h.t["confusion_energy"], gold["tab_confusion_energy"])
    assert np.array_equal(h.t["confusion_SE"], gold["tab_confusion_SE"])
    assert np.array_equal(h.t["n_wfs"], gold["tab_n_wfs"]) and np.array_equal(h.t["n_labelled_wfs"], gold["tab_n_labelled_wfs"])


def test_constructor_defaults_keys_and_shapes(gold):
    from waveformml_amd.psd.evaluator import PSDEvaluator
    sig = inspect.signature(PSDEvaluator.__init__).parameters
    for k in ["n_bins", "n_mult", "emin", "emax", "psd_min", "psd_max", "nx", "ny", "n_samples", "n_confusion", "n_SE_max"]:
        assert float(sig[k].default) == float(gold["default_" + k]), k
    assert sig["gains"].default is None and sig["seg_status"].default is None
    assert sig["fix_last_event_n_SE"].default is False
    assert [n if not n.startswith("$") else "dt_dev" for n in gold["metric_names"]] == ec.METRIC_NAMES
    with pytest.raises(RuntimeError, match="no CPU path"):
        PSDEvaluator(["a", "b"], "cpu")
    from waveformml_amd.psd.evaluator import result_shapes
    shapes = result_shapes([str(n) for n in gold["class_names"]])
    assert sorted(shapes) == [str(k) for k in gold["result_keys"]]
    for k, ref in zip(gold["result_keys"], gold["result_shapes"]):
        assert list(shapes[str(k)]) == [int(v) for v in ref if v > 0], k


def test_header_and_binding_agree_on_the_new_symbols():
    from waveformml_amd import _lib
    text = open(os.path.join(ROOT, "include", "wfsparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)
    assert lib.wfs_eval_table_ints(100, 10, 10, 4, 14, 11, 3) == 2 * 12 + 2 * 102 * 102 + 2 * 16 * 13 + 11 * 9 + 6 * 9 + 4 + 3
