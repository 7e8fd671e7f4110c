"""``module.metrics`` (psd/class_metrics.ClassificationMetrics) through the inference loops: LitPSD on the GEP fixture
config through evaluate.test_loop, eager and captured, and LitSegClassifier on the ioni fixtures through
evaluate.segment_test_loop, with and without ``SELoss``.

The oracle is the float64 restatement of tests/class_metrics_cases.py run on the VERY logits the loop handed to
``metrics.add`` (a recording wrapper copies them to the host at each call), so it never depends on eager and captured
logits agreeing bit for bit.  The restatement IS the kernel's rule (fp64 from the stored logits, one rounding to fp32), so
the integer tables are compared whole and exactly whatever the net's rows are; the margin of class_metrics_cases -- which
guards the comparison with torch's fp32 softmax, not this one -- is only counted and printed.  ``acc`` and ``loss`` agree with the
``metrics=None`` run of the same loop to 1e-5 relative, the project's fp32 bar."""
import copy
import inspect
import json
import os

import numpy as np
import pytest
import torch

import class_metrics_cases as cc
from test_segment_callers import IONI

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))


class Recording:
    """``metrics`` with every ``add``'s arguments copied to the host; everything else is the wrapped object's."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def add(self, logits, target, n_valid=None, loss_mask=None, **kw):
        assert n_valid is None
        self.calls.append((logits.detach().float().cpu().numpy().copy(), target.cpu().numpy().copy(),
                           None if loss_mask is None else loss_mask.cpu().numpy().astype(np.uint8)))
        self.inner.add(logits, target, n_valid=n_valid, loss_mask=loss_mask, **kw)

    def __getattr__(self, name):
        return getattr(self.inner, name)


def restated(rec, C):
    x = np.concatenate([c[0] for c in rec.calls])
    labels = np.concatenate([c[1] for c in rec.calls])
    mask = None if rec.calls[0][2] is None else np.concatenate([c[2] for c in rec.calls])
    thr = rec.inner.thresholds
    inside = int((~cc.margin_ok(x, thr)).sum())
    print("rows", len(labels), "inside the margin", inside)
    return cc.host_tables(x, labels, C, thr, ignore=rec.inner.ignore_index, mask=mask)


def check(res, host):
    print("head", (res["n"], res["correct"], res["loss_rows"], res["ignored"]), host["head"], "loss", res["loss"], host["loss"])
    assert (res["n"], res["correct"], res["loss_rows"], res["ignored"]) == host["head"]
    assert np.array_equal(res["confusion"], host["confusion"]) and np.array_equal(res["roc_bins"], host["roc"])
    assert res["confusion"].sum() == res["n"]
    assert abs(res["loss"] - host["loss"]) <= 2.0 ** -32


def close(a, b):
    return abs(a - b) <= 1e-5 * abs(b)


@pytest.mark.parametrize("capture", [False, True])
def test_lit_psd_test_loop_fills_the_metrics(capture):
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.class_metrics import ClassificationMetrics
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import test_loop
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.trainer import Trainer
    with open(os.path.join(HERE, "golden", "gep_config.json")) as fh:
        cfg = json.load(fh)
    names = list(cfg["system_config"]["type_names"])
    torch.manual_seed(0)
    mod = LitPSD(load_config(copy.deepcopy(cfg))).to(DEV)
    mod.eval()
    batches = []
    for s in range(3):
        c, f, y = synthetic.generate(8, 150, len(names), seed=70 + s, layout="2d")
        batches.append(([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV)], torch.from_numpy(y).to(DEV)))
    plain = test_loop(mod, batches, DEV, capture=capture)
    assert sorted(plain) == ["events", "test_acc", "test_loss"]
    metrics = mod.metrics
    assert isinstance(metrics, ClassificationMetrics) and metrics is mod.metrics
    assert metrics.class_names == names and metrics.n_classes == len(names) and metrics.ignore_index == -100
    rec = Recording(metrics)
    out = test_loop(mod, batches, DEV, capture=capture, metrics=rec)
    assert sorted(out) == sorted(list(plain) + ["metrics"]) and out["events"] == plain["events"] == 24
    assert len(rec.calls) == 3
    res = out["metrics"]
    check(res, restated(rec, len(names)))
    assert res["n"] == 24 and res["loss_rows"] == 24
    print("loop", out["test_loss"], out["test_acc"], "plain", plain["test_loss"], plain["test_acc"])
    assert close(out["test_loss"], plain["test_loss"]) and close(out["test_acc"], plain["test_acc"])
    assert close(res["loss"], plain["test_loss"]) and close(res["acc"], plain["test_acc"])
    # the tables keep summing over loops until reset(); the loop's own scores are of its own batches
    again = test_loop(mod, batches, DEV, capture=capture, metrics=metrics)
    assert again["metrics"]["n"] == 48 and np.array_equal(again["metrics"]["confusion"], 2 * res["confusion"])
    assert close(again["test_loss"], plain["test_loss"]) and close(again["test_acc"], plain["test_acc"])
    assert "metrics" in inspect.signature(Trainer.test).parameters


def _ioni_module_and_loader(se_loss):
    from torch.utils.data import DataLoader
    from waveformml_amd.psd import data as psd_data, h5data
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litseg import LitSegClassifier
    root = os.path.join(HERE, "golden", "h5", "r3", "ioni")
    label_map = {"1": 0, "4": 1, "6": 2, "256": 3, "258": 2, "512": 4}
    ds = h5data.HDF5Dataset([root], "*WaveformPairSim.h5", "WaveformPairs", "coord", "waveform", 12, label_name="PID",
                            label_map=label_map, normalize=True, additional_fields=["phys"])
    (_c0, f0), _y0 = ds[0]
    cfg = copy.deepcopy(IONI)
    cfg["net_config"]["imports"] = ["waveformml_amd.spconv" if m == "oracle.spconv" else m for m in cfg["net_config"]["imports"]]
    cfg["net_config"]["SELoss"] = se_loss
    cfg["system_config"]["n_samples"] = int(f0[0].shape[1]) // 2
    cfg["dataset_config"]["test_dataset_params"] = {"additional_fields": ["phys"]}
    torch.manual_seed(3)
    mod = LitSegClassifier(load_config(cfg)).to(DEV)
    # The freshly initialised net (twelve convolutions, eval-mode BatchNorm at its initial statistics) gives logits of
    # 1e-10, which the fp32 softmax of the module's own test_step cannot tell apart: it ties every class and predicts class
    # 0, while the tables predict by the stored logits (measured on an MI355X: test_acc 0.21875 against 0.125).  The net is
    # positively homogeneous, so scaling each convolution by 7 scales the logits by 7^12 = 1.4e10, to order one.
    with torch.no_grad():
        for p in mod.model.parameters():
            if p.dim() == 4:
                p.mul_(7.0)
    loader = list(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=psd_data.collate_fn))
    return mod, loader


@pytest.mark.parametrize("se_loss", [False, True])
def test_lit_seg_classifier_segment_test_loop_fills_the_metrics(se_loss):
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.pid_evaluator import PID_MAPPED_NAMES
    mod, loader = _ioni_module_and_loader(se_loss)
    plain = segment_test_loop(mod, copy.deepcopy(loader), DEV)
    assert sorted(plain) == ["rows", "test_acc", "test_loss"]
    metrics = mod.metrics
    assert metrics is mod.metrics and metrics.n_classes == 5
    assert metrics.class_names == [PID_MAPPED_NAMES[i] for i in range(5)]          # the config names no types
    rec = Recording(metrics)
    out = segment_test_loop(mod, copy.deepcopy(loader), DEV, metrics=rec, evaluator=mod.evaluator)
    assert sorted(out) == sorted(list(plain) + ["evaluation", "metrics"])
    assert out["test_loss"] == plain["test_loss"] and out["test_acc"] == plain["test_acc"] and out["rows"] == plain["rows"]
    assert len(rec.calls) == len(loader) and (rec.calls[0][2] is not None) == se_loss
    assert mod.last_test_logits is not None and mod.last_test_logits.shape[1] == 5
    res = out["metrics"]
    host = restated(rec, 5)
    check(res, host)
    assert res["n"] == out["rows"] and res["ignored"] == 0
    print("metrics", res["loss"], res["acc"], "plain", plain["test_loss"], plain["test_acc"])
    assert close(res["acc"], plain["test_acc"])
    if se_loss:
        assert 0 < res["loss_rows"] <= res["n"]                    # accuracy counts every row, the loss the single-ended
        # the loop's loss is the mean of the batches' single-ended means weighted by ALL their rows
        rows = np.array([len(c[1]) for c in rec.calls], np.float64)
        means = [cc.host_tables(c[0], c[1], 5, metrics.thresholds, mask=c[2])["loss"] for c in rec.calls]
        assert close(float((rows * means).sum() / rows.sum()), plain["test_loss"])
    else:
        assert res["loss_rows"] == res["n"] and close(res["loss"], plain["test_loss"])
    assert np.array_equal(res["roc_curve"](0), cc.reference_curve(host["roc"][0]), equal_nan=True)
    assert sorted(res["classes"]) == sorted(metrics.class_names)
