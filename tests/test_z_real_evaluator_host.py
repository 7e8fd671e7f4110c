"""CPU checks of psd/real_z_evaluator.py and of LitZ's phys-target route: the constructor arithmetic, table shapes and
ranges against the constants recorded from the reference (tests/golden/z_real_evaluator_cases.npz), the category encoding
of the sample tables and the host-side all-z sum, the factor of three on the last class metric, and which evaluator and
which ``test_step`` a config selects.  No kernel is launched here."""
import copy

import numpy as np
import pytest
import torch

import z_real_evaluator_cases as zc
from test_host_mirror import _z_config
from waveformml_amd.psd import real_z_evaluator  # noqa: F401  (the module under test: no test here runs without it)


@pytest.fixture(scope="module")
def gold():
    return zc.load_golden()


def test_constructor_arithmetic_matches_the_recorded_constants(gold):
    from waveformml_amd.psd import real_z_evaluator as rz
    from waveformml_amd.psd.metric_pairs import bin_edge_range
    from waveformml_amd.psd.segments import blind_left, segment_status
    s = rz.z_real_setup()
    assert s["E_scale"] == float(gold["E_scale"]) and s["z_scale"] == float(gold["z_scale"])
    assert [rz.E_INDEX, rz.PSD_INDEX, rz.Z_INDEX] == gold["phys_indices"].tolist()
    assert (s["n_mult"], s["n_z"], s["n_E"]) == (int(gold["n_mult"]), int(gold["n_z"]), int(gold["n_E"])) == (6, 100, 100)
    assert s["E_bounds"] == gold["E_bounds"].tolist() and s["mult_bounds"] == gold["mult_bounds"].tolist()
    assert s["z_bounds"] == gold["z_bounds"].tolist() == [0.0, 1176.0]
    assert np.array_equal(np.array(s["default_bins"], np.float64), gold["default_bins"])
    assert [s["E_low"], s["E_high"]] == gold["E_range"].tolist()
    assert s["metric_names"] == [str(n) for n in gold["metric_names"]]
    assert [int(p[2]) for p in s["metric_params"]] == gold["class_nbins"].tolist()
    assert np.array_equal(np.array(s["normalized_ranges"]), gold["class_ranges"])          # bit for bit
    assert (rz.PULSE_ANALYSIS_SAMPLES, rz.NUM_Z_BINS) == (int(gold["n_samples"]), int(gold["n_zbins"]))
    assert np.array_equal(np.array(s["sample_params"], np.float64), gold["sample_params"])
    ranges = [bin_edge_range(float(p[0]), float(p[1]), int(p[2])) for p in s["sample_params"]]
    assert np.array_equal(np.array(ranges), gold["sample_ranges"])                          # get_bins' real last edge
    shapes = dict(rz.table_shapes())
    assert list(shapes) == [str(n) for n in gold["table_names"]]
    for k, v in shapes.items():
        assert v == tuple(gold["shape_" + k])
    assert rz.PID_MAP == {int(k): int(v) for k, v in gold["pid_map"]}
    assert np.array_equal(segment_status(), gold["seg_status"]) and np.array_equal(blind_left(), gold["blind_detl"])
    se = gold["seg_status"] == 0.5
    assert (gold["blind_detl"][se] == 1).any() and (gold["blind_detl"][se] == 0).any()      # both orientations exist
    # an e_scale and a bin override move the energy axis as AD1Evaluator does
    alt = rz.z_real_setup(e_scale=8.0, bin_overrides={"0": [0.0, 6.0, 40]})
    assert alt["E_scale"] == 8.0 and alt["n_E"] == 40 and (alt["E_low"], alt["E_high"]) == (0.0, 0.75)
    assert dict(rz.table_shapes(n_E=40))["z_E_dual"] == (102, 42)


def test_pid_is_mapped_once_and_the_callers_array_is_left_alone():
    from waveformml_amd.psd.real_z_evaluator import map_pid
    pid = np.array([1, 4, 6, 256, 258, 512, 2, 7, 0, 3], np.int64)
    keep = pid.copy()
    once = map_pid(pid)
    assert np.array_equal(pid, keep)
    assert once.tolist() == [0, 1, 2, 3, 2, 4, 2, 7, 0, 3]          # 2 and 7 are not in the map and stay
    # the reference's second mapping (a batch without class 3) would turn Recoil into Ionization and Muon into Recoil
    assert map_pid(once).tolist()[:6] == [0, 0, 2, 3, 2, 1]


def test_z_slices_and_category_encoding(gold):
    from waveformml_amd.psd.real_z_evaluator import N_SLICES, sample_category, z_slice
    z = np.array([-700., -600., np.nextafter(-600., 0.), -480., np.nextafter(-480., 0.), 0., 480., np.nextafter(480., 600.),
                  np.nextafter(600., 0.), 600., 900., np.nan])
    assert z_slice(z).tolist() == [0, 0, 1, 1, 2, 5, 9, 10, 10, 11, 11, -1]
    cat = sample_category(z, np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 7, 0]), 5)
    assert cat.tolist() == [0, 1, 7, 8, 14, 25, 46, 52, 53, 59, N_SLICES * 5, N_SLICES * 5]
    assert sample_category(z[:3], np.zeros(3), 1).tolist() == [0, 0, 1]
    # against the recorded tables: every valid row enters its category once per PMT side
    from waveformml_amd.psd.real_z_evaluator import map_pid
    zi = int(gold["phys_indices"][2])
    for name in ("special", "no_class3", "no_pid", "padded"):
        m = zc.meta_of(gold, name)
        C = 5 if m["has_pid"] else 1
        want = np.zeros(N_SLICES * C + 1, np.int64)
        rows = 0
        for bt in zc.batches_of(gold, name):
            nv = len(bt["coords"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            co = bt["coords"][:nv]
            t = bt["targ"][co[:, 2], zi, co[:, 0], co[:, 1]]
            cls = map_pid(bt["pid"][:nv]) if m["has_pid"] else np.zeros(nv, np.int64)
            want += np.bincount(sample_category((t - 0.5) * 1200., cls, C), minlength=len(want))
            rows += nv
        got = gold[name + "_smp_m0_n"].sum(axis=1)
        assert np.array_equal(got, 2 * want[:-1]), name
        # the reference's all-z aggregator holds every row: the sliced ones plus the leftover category
        assert int(gold[name + "_allz_m0_n"].sum()) == 2 * rows == int(got.sum()) + 2 * int(want[-1])
    assert int(gold["no_class3_allz_m0_n"].sum()) > int(gold["no_class3_smp_m0_n"].sum())     # PID 7 matches no class


def _random_raw(rng, layout):
    raw = {}
    for key, shape, tabs in layout:
        n = rng.integers(0, 4, shape).astype(np.int64)
        v = [rng.integers(1, 1 << 30, shape).astype(np.int64) * (n > 0) for _ in range(tabs - 1)]
        raw[key] = [n] + v
    return raw


def test_all_z_tables_are_the_integer_sum_over_categories_and_the_factor_of_three():
    from waveformml_amd.psd import real_z_evaluator as rz
    from waveformml_amd.psd.metric_pairs import real_table_layout, real_triple_1d
    rng = np.random.default_rng(3)
    C, names = 2, ["sample 0", "sample 1"]
    layout = real_table_layout([4, 3], rz.N_SLICES * C + 1)
    raw = _random_raw(rng, layout)
    flat = np.concatenate([a.reshape(-1) for key, _s, _t in layout for a in raw[key]])
    back = rz.raw_real_tables(flat, layout)
    assert all(np.array_equal(a, b) for k in raw for a, b in zip(raw[k], back[k]))
    aggs, left = rz.split_sample_tables(raw, names, C)
    assert len(aggs) == 13
    for i in range(rz.N_SLICES):
        assert np.array_equal(aggs[i]["metrics"]["sample 0"][1], raw[0][0][i * C:(i + 1) * C])
        assert np.array_equal(aggs[i]["pairs"]["0_1"][1], raw["0_1"][0][i * C:(i + 1) * C])
    assert np.array_equal(left["metrics"]["sample 1"][1], raw[1][0][-1:])
    allz = aggs[-1]
    assert allz["metrics"]["sample 0"][1].shape == (1, 6) and allz["pairs"]["0_1"][1].shape == (1, 6, 5)
    assert np.array_equal(allz["pairs"]["0_1"][1][0], raw["0_1"][0].sum(axis=0))
    assert np.array_equal(allz["pairs"]["0_1"][0][0], raw["0_1"][1].sum(axis=0) / 2.0 ** 32)
    want = real_triple_1d(*[a.sum(axis=0, keepdims=True) for a in raw[0]])       # formed from the summed integers
    for a, b in zip(allz["metrics"]["sample 0"], want):
        assert np.array_equal(a, b)
    # the last metric entered three times: a factor on n, S and Q, the other metrics and the pairs untouched
    names4 = ["energy", "psd", "multiplicity", "z"]
    layout = real_table_layout([3, 3, 2, 3], 5)
    raw = _random_raw(rng, layout)
    once, thrice = rz.finish_real_tables(raw, names4), rz.finish_real_tables(raw, names4, 3)
    assert np.array_equal(thrice["metrics"]["z"][1], 3 * once["metrics"]["z"][1])
    assert np.allclose(thrice["metrics"]["z"][0], once["metrics"]["z"][0], rtol=1e-15, atol=0)   # the mean stays
    for a, b in zip(thrice["metrics"]["z"], real_triple_1d(*[3 * t for t in raw[3]])):
        assert np.array_equal(a, b)
    for k in ("energy", "psd", "multiplicity"):
        assert all(np.array_equal(a, b) for a, b in zip(once["metrics"][k], thrice["metrics"][k]))
    assert all(np.array_equal(once["pairs"][k][0], thrice["pairs"][k][0]) for k in once["pairs"])


def test_the_reference_counts_the_last_class_metric_three_times(gold):
    for name in ("two_adds_f32", "special", "no_class3"):
        n = [int(gold["%s_class_m%d_n" % (name, i)].sum()) for i in range(4)]
        assert n[0] == n[1] == n[2] > 0 and n[3] == 3 * n[0], name
        assert int(gold[name + "_class_p0_3_n"].sum()) == n[0]


def test_recorded_baseline_cases_hold_what_they_are_meant_to(gold):
    """The ``special`` batch: event 0 = (a, b, d) with a, b single-ended, d double-ended, d diagonal to a and a to b: a is
    averaged from d, b could only take a's value but a is row 0 of the batch, so b stays at 0.5; event 2 repeats the
    chain away from row 0, where b takes the averaged a; event 1 has no double-ended row; one double-ended truth is 0.5."""
    bt = zc.batches_of(gold, "special")[0]
    co, base, seg = bt["coords"], bt["baseline"], gold["seg_status"]
    zi = int(gold["phys_indices"][2])
    t = bt["targ"][co[:, 2], zi, co[:, 0], co[:, 1]].astype(np.float32)
    st = seg[co[:, 0], co[:, 1]]
    assert st[0] == 0.5 and st[1] == 0.5 and st[2] == 0.0
    assert base[0] == t[2] and base[1] == np.float32(0.5)
    e1 = co[:, 2] == 1
    assert (st[e1] == 0.5).all() and (base[e1] == np.float32(0.5)).all()
    e2 = np.flatnonzero(co[:, 2] == 2)
    assert base[e2[0]] == t[e2[2]] and base[e2[1]] != np.float32(0.5) and st[e2[1]] == 0.5
    assert t[e2[3]] == np.float32(0.5) and st[e2[3]] == 0.0
    assert base.dtype == np.float32
    keep = st != 0.5
    assert np.array_equal(base[keep & (t != 0.5)], t[keep & (t != 0.5)])


def _phys_config(imports, **test_params):
    cfg = copy.deepcopy(_z_config(imports))
    cfg["dataset_config"]["test_dataset_params"] = dict(test_params)
    return cfg


def test_litz_detects_phys_targets_and_chooses_the_evaluator():
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitZ, real_evaluator_params, test_has_phys
    plain = load_config(copy.deepcopy(_z_config(["oracle.spconv"])))
    phys = load_config(_phys_config(["oracle.spconv"], label_name="phys", additional_fields=["PID"]))
    indexed = load_config(_phys_config(["oracle.spconv"], label_name="phys", label_index=4))
    other = load_config(_phys_config(["oracle.spconv"], label_name="z"))
    assert [test_has_phys(c) for c in (plain, phys, indexed, other)] == [False, True, False, False]
    cfg = _phys_config(["oracle.spconv"], label_name="phys", additional_fields=["PID"])
    cfg["evaluation_config"] = {"wf_analysis": True, "additional_field_names": ["x"]}
    merged = real_evaluator_params(load_config(cfg), {"wf_analysis": True, "additional_field_names": ["x"]})
    assert merged == {"wf_analysis": True, "additional_field_names": ["PID"]}       # the dataset's fields win
    torch.manual_seed(0)
    m = LitZ(load_config(cfg))
    assert m.test_has_phys is True
    # the evaluators have no CPU path: the refusal names the class that was chosen
    with pytest.raises(RuntimeError, match="ZEvaluatorRealWFNorm runs on the GPU"):
        m.evaluator
    p = LitZ(plain)
    assert p.test_has_phys is False
    with pytest.raises(RuntimeError, match="ZEvaluator runs on the GPU"):
        p.evaluator


def test_a_config_without_phys_targets_takes_the_path_it_took():
    """``test_has_phys`` is computed once in ``LitZ.__init__`` and read in exactly two places, ``_make_evaluator`` and
    ``test_step``, each of which runs the earlier statements unchanged in its ``else`` branch; training and validation
    never read it.  So a config without phys targets sees the same calls with the same arguments: its ``test_step``
    scores the whole target and leaves the four-entry tuple.  The phys route scores column ``z_index`` of the seven
    planes and leaves five entries."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitZ
    rng = np.random.default_rng(2)
    rows = sorted({(int(rng.integers(0, 14)), int(rng.integers(0, 11)), e) for e in range(4) for _ in range(3)},
                  key=lambda r: r[2])
    c = torch.tensor(rows, dtype=torch.int32)
    f = torch.from_numpy(rng.random((len(rows), 40)).astype(np.float32))
    z = torch.from_numpy(rng.random(len(rows)).astype(np.float32))
    phys_t = torch.from_numpy(rng.random((len(rows), 7)).astype(np.float32))
    phys_t[:, 4] = z
    pid = torch.from_numpy(rng.integers(0, 5, len(rows)))
    torch.manual_seed(0)
    plain = LitZ(load_config(copy.deepcopy(_z_config(["oracle.spconv"]))))
    torch.manual_seed(0)
    real = LitZ(load_config(_phys_config(["oracle.spconv"], label_name="phys", additional_fields=["PID"])))
    plain.eval(), real.eval()
    with torch.no_grad():
        a = plain.test_step(([c, f.clone()], z), 0)
        b = real.test_step(([c, [f.clone(), pid]], phys_t), 0)
    assert len(plain.last_test_outputs) == 4 and tuple(plain.last_test_outputs[1].shape) == (4, 1, 14, 11)
    pred, target, cc, ff, fields = real.last_test_outputs
    assert tuple(target.shape) == (4, 7, 14, 11) and tuple(pred.shape) == (4, 1, 14, 11) and fields[0] is pid
    assert torch.equal(ff, f) and cc is c
    # the same weights and the same z column: the same loss and the same prediction map
    assert torch.equal(a["test_loss"], b["test_loss"]) and torch.equal(pred, plain.last_test_outputs[0])
    assert torch.equal(target[:, 4:5], plain.last_test_outputs[1])
