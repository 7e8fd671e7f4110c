"""CPU checks around the GPU per-segment evaluators (psd/segment_evaluator.py, csrc/segstats.hip): the goldens recorded
from the reference's row walks load, the NumPy restatement in tests/segment_evaluator_cases.py reproduces them, constructor
defaults / result keys / shapes / dtypes match the recorded ones, the evaluators refuse a CPU device, and the header and
the ctypes table agree on the new symbols.  No kernel is launched here."""
import inspect
import os
import re

import numpy as np
import pytest

import segment_evaluator_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["wfs_seg_z_table_ints", "wfs_seg_energy_table_ints", "wfs_seg_z_accumulate", "wfs_seg_energy_accumulate"]


@pytest.fixture(scope="module")
def gold():
    return sc.load_golden()


def test_goldens_load_and_reach_the_edges(gold):
    for dt in sc.DTYPES:
        c0, c1 = gold[dt + "_b0_coords"], gold[dt + "_b1_coords"]
        assert c0.dtype == np.int32 and len(c0) == 52 and len(c1) == 44
        assert sorted(np.bincount(c0[:, 2], minlength=10).tolist()) == [0, 0, 1, 2, 3, 6, 7, 10, 11, 12]
        assert c0[0, 2] == 1 and 4 not in c0[:, 2] and c0[-1, 2] == 9            # empty events 0 and 4, a last event with rows
        assert gold[dt + "_b0_pred"].shape == (10, 2, 14, 11) and gold[dt + "_b1_targ"].shape == (8, 2, 14, 11)
        x, y, e = c0[:, 0], c0[:, 1], c0[:, 2]
        tz, te = gold[dt + "_b0_targ"][e, 1, x, y], gold[dt + "_b0_targ"][e, 0, x, y]
        assert (tz < 0).any() and (tz >= 1).any() and {0.0, 0.5, 0.75, 1.0} <= set(tz.tolist())
        assert (te > 0).all() and (te * np.float32(12) == 9).any()              # strictly positive; one exactly at E_high
        status = gold["seg_status"][x, y]
        assert {0.0, 0.5, 1.0} <= set(status.tolist())
        h = gold[dt + "_after2_z_seg_sample_error"]
        assert h.dtype == np.int32 and h[:, :, 0].sum() > 0 and h[:, :, -1].sum() > 0
        n = gold[dt + "_after2_z_seg_mult_mae_n"]
        assert n.sum() == 96 and n[:, :, 6].sum() == 7 + 10 + 11 + 12 + 7 + 12 + 11      # the z overflow column: mult > 6
        ne = gold[dt + "_after2_e_seg_mult_Emape_n"]
        assert ne[:, :, 10].sum() == 11 + 12 + 12 + 11                                   # the energy one: mult > 10


def test_restatement_reproduces_the_recorded_tables(gold):
    """Integer tables exactly, float tables to 1e-5 of each table's largest entry (the reference keeps float32 running
    sums, the restatement rounds once); both after one batch and after two."""
    seg, samples = gold["seg_status"], gold["sample_segs"]
    for dt in sc.DTYPES:
        z, zE = sc.HostZTables(seg, sample_segs=samples), sc.HostZTables(seg, use_energy=True, sample_segs=samples)
        en = sc.HostEnergyTables(seg)
        for b in range(2):
            c, p, t = (gold["%s_b%d_%s" % (dt, b, k)] for k in ("coords", "pred", "targ"))
            z.add(c, p[:, 1], t[:, 1], E=t[:, 0])
            zE.add(c, p[:, 1], t[:, 1], E=t[:, 0])
            en.add(c, p[:, 0], t[:, 0])
            acc = "%s_after%d_" % (dt, b + 1)
            sc.assert_tables_match(z.results(), gold, acc + "z_", sc.Z_PAIRS + ("seg_sample_error",))
            sc.assert_tables_match(zE.results(), gold, acc + "zE_", sc.Z_PAIRS + ("seg_sample_error",))
            sc.assert_tables_match(en.results(), gold, acc + "e_", sc.E_PAIRS)
        assert z.results()["E_mult_mae_single"][1].sum() == 0 and zE.results()["E_mult_mae_dual"][1].sum() > 0


def test_restatement_walks():
    assert sc.multiplicity([1, 1, 3, 3, 3, 7]).tolist() == [2, 2, 3, 3, 3, 1]
    assert sc.mult_column(np.array([1, 6, 7, 12]), 6).tolist() == [0, 5, 6, 6]
    # exactly on an edge the value belongs to the bin above; at `high` to the overflow bin
    assert sc.z_bin([-600.0, 0.0, 300.0, 600.0, -600.5, 599.9], 1200., 20).tolist() == [1, 11, 16, 21, 0, 20]
    assert sc.walk_bin([-1000.0, 600.0, -600.0, 1000.0, -1050.0, 1050.0], -1000., 1000., 40., 50).tolist() == \
        [1, 41, 11, 51, 0, 51]
    assert sc.walk_bin([9.0, 0.0, 8.99], 0., 9., 0.45, 20).tolist() == [21, 1, 20]


def test_defaults_keys_shapes_dtypes(gold):
    from waveformml_amd.psd import segment_evaluator as se
    from waveformml_amd.psd.segments import segment_status
    sig = inspect.signature(se.ZEvaluator.__init__).parameters
    for k in ("nmult", "n_bins", "n_err_bins", "error_low", "error_high", "z_scale", "E_low", "E_high", "true_E_high",
              "E_scale", "nx", "ny"):
        assert float(sig[k].default) == float(gold["z_default_" + k]) == float(sc.Z_DEFAULTS[k]), k
    assert np.array_equal(np.asarray(sig["sample_segs"].default), gold["sample_segs"])
    assert sig["seg_status"].default is None and sig["use_energy"].default is False
    assert np.array_equal(segment_status(), gold["seg_status"]) and gold["seg_status"].dtype == np.float32
    sig = inspect.signature(se.EnergyEvaluator.__init__).parameters
    for k in ("n_mult", "n_E", "n_z", "E_scale"):
        assert float(sig[k].default) == float(gold["e_default_" + k]), k
    assert list(sig["E_bounds"].default) == list(gold["e_default_E_bounds"]) == [0.0, 9.0]
    for tag, shapes in (("z", se.z_result_shapes()), ("e", se.energy_result_shapes())):
        assert sorted(shapes) == [str(k) for k in gold[tag + "_result_keys"]]
        for k, ref, pair, dtype in zip(gold[tag + "_result_keys"], gold[tag + "_result_shapes"],
                                       gold[tag + "_result_is_pair"], gold[tag + "_result_dtypes"]):
            assert list(shapes[str(k)]) == [int(v) for v in ref if v > 0], k
            assert str(dtype) == ("float32" if pair else "int32") and bool(pair) == (str(k).find("seg_sample_error") < 0)
    assert se.energy_result_shapes()["E_mult_single"] == (22, 11) and se.energy_result_shapes()["seg_mult_Emape_cal"] == (14, 11, 11)
    assert inspect.signature(se.ZEvaluator.add).parameters.keys() >= {"predictions", "target", "c", "f", "E",
                                                                      "target_is_cal", "additional_fields"}


def test_cpu_device_is_refused():
    from waveformml_amd.psd import segment_evaluator as se
    for make in (se.ZEvaluator, se.EnergyEvaluator, se.EZEvaluator):
        with pytest.raises(RuntimeError, match="no CPU path"):
            make("cpu")
    with pytest.raises(ValueError, match="planes"):
        se.EZEvaluator("cpu", planes="zE")


def test_lit_modules_keep_their_test_step_and_name_an_evaluator():
    """test_step's return value is what it was; what the evaluator needs is left in last_test_outputs."""
    import copy
    import torch
    from test_host_mirror import _z_config
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitSegmentBase, LitZ
    torch.manual_seed(0)
    m = LitZ(load_config(copy.deepcopy(_z_config(["oracle.spconv"]))))
    assert isinstance(LitSegmentBase.evaluator, property) and m.last_test_outputs is None
    c = torch.tensor([[1, 2, 0], [3, 4, 0], [5, 6, 1]], dtype=torch.int32)
    f = torch.rand(3, 40)
    z = torch.rand(3)
    m.eval()
    with torch.no_grad():
        res = m.test_step(([c, f], z), 0)
    assert sorted(res) == ["test_loss"]
    pred, targ, cc, ff = m.last_test_outputs
    assert pred.shape == targ.shape == (2, 1, 14, 11) and cc is c and float(targ[1, 0, 5, 6]) == float(z[2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.evaluator


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
    assert lib.wfs_seg_z_table_ints(14, 11, 6, 20, 50, 3) == 2 * 14 * 11 * 7 + 8 * 22 * 7 + 3 * 7 * 52
    assert lib.wfs_seg_energy_table_ints(14, 11, 10, 20) == 2 * 14 * 11 * 11 + 4 * 22 * 11
    assert "WFS_SEG_FIXED_ONE 4294967296.0" in text
