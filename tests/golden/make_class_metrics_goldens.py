"""Generates tests/golden/class_metrics_cases.npz from the REFERENCE's own ``ROCCurve`` (src/evaluation/ROCCurve.py, the
reference tree, this container only).  No reference text is written anywhere; the npz holds arrays only.  The layout of
the file is described in tests/class_metrics_cases.py.

How the reference is run
  * ``ROCCurve`` is imported from the reference's FILE (importlib, by path) and used unmodified: ``update`` on torch's
    fp32 CPU ``softmax`` of the case's logits and its labels, then ``compute``, for class indices 0 and C - 1.
  * It imports ``ConfusionMatrix`` and ``Metric`` from torchmetrics, which is not installed here.  A stub module of this
    project's own stands in ``sys.modules``: a ``Metric`` base with nothing in it, and a ``ConfusionMatrix`` RESTATED from
    torchmetrics 0.2 (the version the reference's requirements.txt pins): a float32 [num_classes, num_classes] state, an
    update that thresholds float predictions with ``(preds >= threshold).int()`` and adds the ``bincount`` of
    ``target * num_classes + preds`` reshaped to the matrix, and a ``compute`` that returns the state as float32.  PARITY
    UNPINNED: the restatement cannot be held against the library here.  The quirks of ``compute()`` -- which
    cells it divides -- are the reference's own.
  * ``update`` writes the binary target through a shallow copy of its argument, so it is handed a clone per call.
  * Before anything is written, the torch-CPU composition (``softmax``, ``argmax``, ``bincount``, ``prob[:, k] >= thr`` for
    every threshold) is held against the restatement of tests/class_metrics_cases.py on every recorded case, crafted rows
    included, and the recorded curves against ``reference_curve`` of the restatement's bins.

Run:  python tests/golden/make_class_metrics_goldens.py [reference root]
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import class_metrics_cases as cc  # noqa: E402


class Metric:
    def __init__(self, *args, **kwargs):
        pass


class ConfusionMatrix(Metric):
    """torchmetrics 0.2's, restated: see the module docstring."""

    def __init__(self, num_classes, normalize=None, threshold=0.5):
        super().__init__()
        assert normalize is None
        self.num_classes, self.threshold = num_classes, threshold
        self.confmat = torch.zeros(num_classes, num_classes)

    def update(self, preds, target):
        if preds.is_floating_point():
            preds = (preds >= self.threshold).int()
        unique = (target.view(-1) * self.num_classes + preds.view(-1)).to(torch.long)
        bins = torch.bincount(unique, minlength=self.num_classes ** 2)
        self.confmat += bins.reshape(self.num_classes, self.num_classes)

    def compute(self):
        return self.confmat.float()


def reference_roc_class():
    stub = types.ModuleType("torchmetrics")
    stub.Metric, stub.ConfusionMatrix = Metric, ConfusionMatrix
    sys.modules["torchmetrics"] = stub
    spec = importlib.util.spec_from_file_location("reference_ROCCurve", os.path.join(REF, "src", "evaluation", "ROCCurve.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ROCCurve


def torch_tables(x, labels, C, thr):
    """The torch-CPU composition that the reference's test_step amounts to."""
    logits, target = torch.from_numpy(x), torch.from_numpy(labels)
    prob = torch.softmax(logits, dim=1)
    pred = torch.argmax(prob, dim=1)
    confusion = torch.bincount(target * C + pred, minlength=C * C).reshape(C, C).numpy()
    T = len(thr)
    # roc bins from per-threshold comparisons: the bin of a row is the number of thresholds it meets
    met = torch.stack([prob >= float(t) for t in thr]).sum(dim=0).numpy()              # python floats, as ROCCurve's
    met32 = torch.stack([prob >= t for t in torch.from_numpy(thr)]).sum(dim=0).numpy()
    assert np.array_equal(met, met32)         # a python-float threshold compares as its float32 image
    roc = np.zeros((C, 2, T + 1), np.int64)
    for k in range(C):
        np.add.at(roc[k], ((labels == k).astype(np.int64), met[:, k]), 1)
    loss = float(torch.nn.functional.cross_entropy(logits.double(), target))
    return confusion, roc, int((pred == target).sum()), loss


def main():
    ROCCurve = reference_roc_class()
    out = {}
    for name in cc.RECORDED:
        x, labels, C, T, _dtype = cc.recorded_case(name)
        thr = cc.thresholds(T)
        host = cc.host_tables(x, labels, C, thr)
        confusion, roc, correct, loss = torch_tables(x, labels, C, thr)
        assert np.array_equal(confusion, host["confusion"]) and np.array_equal(roc, host["roc"]), name
        assert correct == host["head"][1] and abs(loss - host["loss"]) <= 1e-12 * max(1.0, abs(loss)), name
        prob = torch.softmax(torch.from_numpy(x), dim=1)
        out[name + "_logits"], out[name + "_labels"] = x, labels
        for tag, k in (("roc0", 0), ("rocl", C - 1)):
            curve = ROCCurve(class_index=k, n_thresh=T)
            # two updates, as two batches
            half = len(labels) // 2
            curve.update(prob[:half].clone(), torch.from_numpy(labels[:half]).clone())
            curve.update(prob[half:].clone(), torch.from_numpy(labels[half:]).clone())
            got = curve.compute().numpy()
            assert got.dtype == np.float32 and got.shape == (2, T)
            assert np.array_equal(got, cc.reference_curve(host["roc"][k]), equal_nan=True), (name, tag)
            out[name + "_" + tag] = got
    np.savez_compressed(cc.GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (cc.GOLDEN, len(out), os.path.getsize(cc.GOLDEN)))


if __name__ == "__main__":
    main()
