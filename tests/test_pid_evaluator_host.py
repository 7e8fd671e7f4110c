"""CPU checks of the PID evaluator / pairwise metric tables against tests/golden/pid_evaluator_cases.npz (recorded from the
reference's own functions by tests/golden/make_pid_evaluator_goldens.py).  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import pid_evaluator_cases as pc


@pytest.fixture(scope="module")
def gold():
    return pc.load_golden()


def _metrics(gold, name):
    i = 0
    while "%s_m%d_n" % (name, i) in gold:
        yield i, gold["%s_m%d_mean" % (name, i)], gold["%s_m%d_n" % (name, i)], gold["%s_m%d_dev" % (name, i)]
        i += 1


def test_closed_form_triple_equals_the_recorded_sequential_welford(gold):
    """mean, M2 -> sqrt(M2 / (n - 1)) of metric_accumulate_1d + finalize2d from (sum of matches, n), to 1e-12, on every
    golden; the sum of matches is the recorded mean times the recorded count, an integer to rounding."""
    from waveformml_amd.psd.metric_pairs import triple_1d
    seen = 0
    for name in pc.case_names(gold) + ["psd_tab"]:
        for _i, mean, n, dev in _metrics(gold, name):
            m = np.round(mean * n).astype(np.int64)
            assert np.abs(m - mean * n).max() < 1e-9
            got = triple_1d(m, n)
            assert np.array_equal(got[1], n) and got[1].dtype == np.int64
            assert np.abs(got[0] - mean).max() <= 1e-12 and np.abs(got[2] - dev).max() <= 1e-12
            seen += int(n.sum() > 0)
            assert (dev[n <= 2] == 0).all()
    assert seen >= 40 and any(d.max() > 0 for n_ in ["two_adds_f32"] for _i, _m, _n, d in _metrics(gold, n_))


def test_constructor_range_arithmetic_equals_the_recorded_ranges(gold):
    from waveformml_amd.psd import pid_evaluator as pe
    from waveformml_amd.psd.metric_pairs import bin_edge_range
    from waveformml_amd.psd.segments import segment_status
    s = pe.metric_setup()
    assert s["E_scale"] == float(gold["E_scale"]) and s["z_scale"] == float(gold["z_scale"])
    assert s["metric_names"] == [str(n) for n in gold["metric_names"]]
    assert np.array_equal(np.array(s["metric_params"], np.float64), gold["pid_metric_params"])
    assert np.array_equal(np.array(s["normalized_ranges"]), gold["pid_ranges"])
    assert np.array_equal(np.array([bin_edge_range(*p[:2], int(p[2])) for p in s["metric_params"]]), gold["pid_edges"])
    alt = pe.metric_setup(e_scale=8.0, bin_overrides={"4": [-500.0, 500.0, 40]})
    assert np.array_equal(np.array(alt["normalized_ranges"]), gold["alt_ranges"])
    assert [int(p[2]) for p in alt["metric_params"]] == list(gold["alt_nbins"])
    assert [pe.E_INDEX, pe.PSD_INDEX, pe.Z_INDEX] == list(gold["phys_indices"])
    assert np.array_equal(segment_status(), gold["seg_status"])
    assert [pe.PID_MAPPED_NAMES[i] for i in range(5)] == ["Ionization", "Recoil", "Neutron Capture", "Ingress", "Muon"]
    with pytest.raises(IOError):
        pe.metric_setup(bin_overrides={"z": [0, 1, 2]})
    assert np.array_equal(np.array([bin_edge_range(*p[:2], int(p[2])) for p in gold["psd_metric_params"]]), gold["psd_ranges"])


def test_new_symbols_are_exported_and_declared():
    from waveformml_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("wfs_metric_pairs_table_ints", "wfs_metric_pairs_accumulate", "wfs_match_categories", "wfs_pid_table_ints",
              "wfs_pid_row_stats"):
        assert hasattr(lib, n), "libwfsparse.so does not export %s" % n
        assert n in _lib.SIGNATURES


def test_table_size_functions_match_the_python_layout(gold):
    from waveformml_amd import _lib
    from waveformml_amd.psd.metric_pairs import table_layout
    lib = _lib.load()
    for nb, C in ((list(gold["pid_nbins"]), 5), (list(gold["psd_nbins"]), 2), (list(gold["psd_nbins"]), 3), ([7], 1),
                  ([2040, 4], 5), ([3] * 16, 2)):
        nb = [int(n) for n in nb]
        want = pc.table_ints(nb, C)
        assert int(lib.wfs_metric_pairs_table_ints(len(nb), _lib.i32_array(nb), C)) == want
        assert sum(2 * int(np.prod(s)) for _k, s in table_layout(nb, C)) == want
    assert [k for k, _s in table_layout([1, 2, 3, 4], 1)][4:] == ["0_1", "0_2", "0_3", "1_2", "1_3", "2_3"]
    assert int(lib.wfs_metric_pairs_table_ints(17, _lib.i32_array([3] * 17), 2)) == 0          # above the maximum
    assert int(lib.wfs_pid_table_ints(10, 6)) == 25 * (1 + 8 + 11)


def test_host_restatement_matches_every_golden(gold):
    seg = gold["seg_status"]
    for name in pc.case_names(gold):
        bs = pc.batches_of(gold, name)
        if str(gold[name + "_kind"]) == "pid":
            host = pc.HostPIDTables(seg, gold["pid_nbins"], gold["pid_ranges"], float(gold["E_scale"]))
            for k, b in enumerate(bs):
                host.add(b["coords"], b["pred"], b["targ"], b["phys"], int(b["n_valid"]))
                rows = pc.pid_rows(b["coords"], b["pred"], b["targ"], b["phys"], seg, int(b["n_valid"]))
                rec = gold["%s_b%d_rows" % (name, k)]
                for j, key in enumerate(("accuracy", "mult", "se", "n_se")):
                    assert np.array_equal(rows[key], rec[j]), (name, key)
            for key in ("SE_confusion", "confusion_SE", "confusion_energy"):
                assert np.array_equal(getattr(host, key), gold["%s_%s" % (name, key)]), (name, key)
            pairs = host.pairs
        else:
            pairs = pc.HostPairTables(gold[name + "_nbins"], gold[name + "_ranges"], int(gold[name + "_C"]))
            for b in bs:
                nv = len(b["result"]) if b["n_valid"] < 0 else int(b["n_valid"])
                pairs.add(b["params"][:, :nv], b["result"][:nv], b["category"][:nv])
        for i, _mean, n, _dev in _metrics(gold, name):
            assert np.array_equal(pairs.n1[i], n), (name, i)
        for (i, j), n in pairs.n2.items():
            assert np.array_equal(n, gold["%s_p%d_%d_n" % (name, i, j)]), (name, i, j)
            assert np.array_equal(pairs.m2[(i, j)], gold["%s_p%d_%d_val" % (name, i, j)]), (name, i, j)


def test_case_list_covers_what_it_says(gold):
    names = pc.case_names(gold)
    assert len(names) == 18 and not gold["pid_fall_through_found"].any() and not gold["psd_fall_through_found"].any()
    b = pc.batches_of(gold, "padded")[0]
    assert 0 < int(b["n_valid"]) < len(b["coords"]) and b["coords"][-1, 2] == 999
    assert gold["seven_se_b0_rows"][3].max() == 7 > int(gold["n_SE_max"])
    assert gold["edges_f32_m0_n"][:, 0].sum() > 0 and gold["edges_f32_m0_n"][:, 101].sum() > 0
    assert np.isnan(pc.batches_of(gold, "edges_f32")[0]["phys"][:, 0]).any()
    assert gold["empty_class_m0_n"][3].sum() == 0 and gold["all_wrong_m0_mean"].max() == 0
    assert np.array_equal(gold["dispatch_C2_p0_1_n"], gold["dispatch_C3_p0_1_n"][:2]) and gold["dispatch_C3_p0_1_n"][2].sum() == 0
    assert 2 * (2042 + 6) == 4096 and gold["dispatch_C2_p0_1_n"].sum() > 30          # MP_LDS_CELLS, csrc/metricpairs.hip
