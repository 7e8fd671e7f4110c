"""Host checks for ClassificationMetrics (no GPU): the float64 restatement of tests/class_metrics_cases.py against naive
loops, against the torch-CPU composition and against the curves RECORDED from the reference's ROCCurve
(tests/golden/class_metrics_cases.npz); the margin of every generated row; header, binding and argument limits of the
two exports.  Nothing here reads the reference tree."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import class_metrics_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


@pytest.mark.parametrize("C,T,dtype", [(2, 100, "f32"), (3, 7, "bf16"), (5, 100, "f16"), (9, 1, "f32")])
def test_restatement_against_naive_loops(C, T, dtype):
    x, labels, _n, _r = cc.make_case(40, C, T, dtype, seed=C)
    labels[3], labels[17] = -100, -100
    mask = (np.arange(len(labels)) % 3 != 0).astype(np.uint8)
    thr = cc.thresholds(T)
    for kw in (dict(), dict(mask=mask), dict(n_valid=29), dict(mask=mask, n_valid=0)):
        a, b = cc.host_tables(x, labels, C, thr, **kw), cc.naive_tables(x, labels, C, thr, **kw)
        assert a["head"] == b["head"] and np.array_equal(a["confusion"], b["confusion"]), kw
        assert np.array_equal(a["roc"], b["roc"]), kw
        assert (np.isnan(a["loss"]) and np.isnan(b["loss"])) or abs(a["loss"] - b["loss"]) <= 1e-12 * max(1, abs(b["loss"]))
        n, _c, _l, ignored = a["head"]
        assert a["confusion"].sum() == n and all(a["roc"][k].sum() == n for k in range(C))
        assert n + ignored == (len(labels) if "n_valid" not in kw else kw["n_valid"])


@pytest.mark.parametrize("name", sorted(cc.RECORDED))
def test_restatement_against_torch_cpu_and_the_recorded_curves(gold, name):
    x, labels, C, T, _dtype = cc.recorded_case(name)
    assert np.array_equal(x, gold[name + "_logits"]) and np.array_equal(labels, gold[name + "_labels"])   # the builder repeats
    thr = cc.thresholds(T)
    host = cc.host_tables(x, labels, C, thr)
    logits, target = torch.from_numpy(x), torch.from_numpy(labels)
    prob = torch.softmax(logits, dim=1)
    pred = torch.argmax(prob, dim=1)
    assert np.array_equal(torch.bincount(target * C + pred, minlength=C * C).reshape(C, C).numpy(), host["confusion"])
    assert int((pred == target).sum()) == host["head"][1]
    assert abs(float(torch.nn.functional.cross_entropy(logits.double(), target)) - host["loss"]) <= 1e-12 * host["loss"]
    for k in range(C):
        tn, fp, fn, tp = cc.rates(host["roc"][k])
        for i, t in enumerate(thr):
            positive = (prob[:, k] >= float(t)).numpy()                   # a python float, as ROCCurve's thresholds
            is_k = labels == k
            assert (tp[i], fp[i], fn[i], tn[i]) == ((positive & is_k).sum(), (positive & ~is_k).sum(),
                                                    (~positive & is_k).sum(), (~positive & ~is_k).sum()), (k, i)
    assert np.array_equal(cc.reference_curve(host["roc"][0]), gold[name + "_roc0"], equal_nan=True)
    assert np.array_equal(cc.reference_curve(host["roc"][C - 1]), gold[name + "_rocl"], equal_nan=True)


def test_results_from_tables_names_the_rates_correctly(gold):
    from waveformml_amd.psd.class_metrics import rates_from_bins, results_from_tables, thresholds
    x, labels, C, T, _dtype = cc.recorded_case("c5_f32")
    thr = cc.thresholds(T)
    assert np.array_equal(thresholds(T), thr) and thr.dtype == np.float32
    host = cc.host_tables(x, labels, C, thr)
    n, correct, loss_rows, ignored = host["head"]
    head = np.array([n, correct, loss_rows, int(round(host["loss"] * loss_rows * 2.0 ** 32)), ignored], np.int64)
    res = results_from_tables(head, host["confusion"], host["roc"], thr, [str(k) for k in range(C)])
    assert res["n"] == n and res["acc"] == correct / n and abs(res["loss"] - host["loss"]) <= 2.0 ** -32
    for k in range(C):
        got = rates_from_bins(host["roc"][k])
        for a, b in zip(got, cc.rates(host["roc"][k])):
            assert a.dtype == np.int64 and np.array_equal(a, b)
        c = res["classes"][str(k)]
        tn, fp, fn, tp = got
        assert np.array_equal(c["tpr"], tp / (tp + fn)) and np.array_equal(c["fpr"], fp / (fp + tn))
        assert 0.0 <= c["auc"] <= 1.0
    # the reference's row 0 is the true NEGATIVE rate of the [true, predicted] matrix
    curve = res["roc_curve"](0)
    assert curve.dtype == np.float32 and np.array_equal(curve, gold["c5_f32_roc0"], equal_nan=True)
    c0 = res["classes"]["0"]
    assert np.allclose(curve[0], 1.0 - c0["fpr"], atol=1e-6) and np.allclose(curve[1], 1.0 - c0["tpr"], atol=1e-6)
    assert np.array_equal(res["roc_curve"](C - 1), gold["c5_f32_rocl"], equal_nan=True)
    empty = results_from_tables(np.zeros(5, np.int64), np.zeros((2, 2), np.int64), np.zeros((2, 2, 4), np.int64),
                                cc.thresholds(3), ["a", "b"])
    assert np.isnan(empty["acc"]) and np.isnan(empty["loss"]) and np.isnan(empty["roc_curve"](1)).all()


@pytest.mark.parametrize("C,T,dtype", [(2, 100, "f32"), (5, 100, "bf16"), (5, 1024, "f16"), (32, 100, "f32")])
def test_every_generated_row_satisfies_the_margin(C, T, dtype):
    x, labels, n, _redrawn = cc.make_case(500, C, T, dtype, seed=5)
    assert n == 500 and len(labels) == len(x) > n
    assert cc.margin_ok(x[:n], cc.thresholds(T)).all()
    assert np.array_equal(cc.round_to(x, dtype), x)


def test_header_binding_and_limits():
    from waveformml_amd import _lib
    from waveformml_amd.psd import class_metrics as cm
    text = open(os.path.join(ROOT, "include", "wfsparse.h")).read()
    for name, value in (("MAX_CLASSES", _lib.WFS_CLASS_METRICS_MAX_CLASSES), ("MAX_THRESH", _lib.WFS_CLASS_METRICS_MAX_THRESH),
                        ("LDS_BYTES", _lib.WFS_CLASS_METRICS_LDS_BYTES)):
        assert int(re.search(r"#define WFS_CLASS_METRICS_%s (\d+)" % name, text).group(1)) == value
    assert len(_lib.SIGNATURES["wfs_class_metrics_accumulate"][1]) == 15
    lib = _lib.load()
    assert _lib.WFS_ABI_VERSION == 6
    for C, T in ((2, 1), (5, 100), (32, 100), (7, 1024), (2, 1024)):
        assert lib.wfs_class_metrics_table_ints(C, T) == cm.table_ints(C, T) == 5 + C * C + 2 * C * (T + 1)
        assert 4 * (6 + C * C + 2 * C * (T + 1) + T) <= _lib.WFS_CLASS_METRICS_LDS_BYTES
    for C, T in ((1, 100), (33, 100), (5, 0), (5, 1025), (8, 1024), (32, 300)):
        assert lib.wfs_class_metrics_table_ints(C, T) == 0
        with pytest.raises(ValueError, match="2 .. 32.*1 .. 1024.*65536"):
            cm.table_ints(C, T)
        with pytest.raises(ValueError, match="LDS"):
            cm.ClassificationMetrics("cpu", C, T)
        # the entry point refuses the same shapes before it touches the device
        one = ctypes.c_int64(0)
        p = ctypes.addressof(one)
        assert lib.wfs_class_metrics_accumulate(p, 0, C, p, -100, None, 1, None, C, p, T, p, p, 0, None) == _lib.WFS_EINVAL
        assert "classes" in _lib.last_error()
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)
    bad = [dict(dtype=7), dict(stride=4), dict(N=-1), dict(max_blocks=-1), dict(thr=None)]
    for kw in bad:
        a = dict(dtype=0, stride=5, N=1, max_blocks=0, thr=p)
        a.update(kw)
        assert lib.wfs_class_metrics_accumulate(p, a["dtype"], a["stride"], p, -100, None, a["N"], None, 5, a["thr"], 100, p,
                                                p, a["max_blocks"], None) == _lib.WFS_EINVAL, kw
    with pytest.raises(RuntimeError, match="no CPU path"):
        cm.ClassificationMetrics("cpu", 5)


def test_tables_score_only_under_a_plain_mean_cross_entropy():
    """evaluate.test_loop takes loss and accuracy from the tables only where they are what ``_score`` computes."""
    from types import SimpleNamespace
    from waveformml_amd.psd.evaluate import _tables_score
    metrics = SimpleNamespace(ignore_index=-100)
    ce = torch.nn.CrossEntropyLoss
    assert _tables_score(SimpleNamespace(criterion=ce()), metrics)
    assert not _tables_score(SimpleNamespace(criterion=ce()), None)
    for criterion in (ce(weight=torch.ones(3)), ce(reduction="sum"), ce(label_smoothing=0.1), ce(ignore_index=2),
                      torch.nn.NLLLoss(), torch.nn.MultiMarginLoss()):
        assert not _tables_score(SimpleNamespace(criterion=criterion), metrics), criterion
