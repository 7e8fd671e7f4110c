"""``ClassificationMetrics``: what the reference's two classification modules keep per validation / test step -- a
``torchmetrics.Accuracy``, a ``ConfusionMatrix(num_classes=n_type)`` summed over the batches
(src/engineering/LitPSD.py, LitSegClassifier.py) and ``ROCCurve`` (src/evaluation/ROCCurve.py: ``n_thresh`` binary
confusion matrices of ``softmax(logits)[:, class_index]`` against the thresholds ``(i + 1) / n_thresh``) -- on the GPU,
with the mean cross-entropy beside them.

``add`` is ONE HIP launch on the current stream (csrc/classmetrics.hip) that reads every logit row once and adds exact
integers into persistent tables; nothing is read back until ``results()``.  The ROC tables are kept for EVERY class, not
for one ``class_index``: per class and binary target a histogram of the bin ``#{i : p >= thr[i]}`` of the row's
probability, from which the host forms every threshold's TN / FP / FN / TP by cumulative sums.

Arithmetic of a row: the prediction is the first index of the largest logit; the probabilities are formed in fp64 from
the stored logits and rounded once to fp32, then compared ``>=`` with the fp32 thresholds, which is what torchmetrics
0.2's ``(preds >= threshold)`` does on an fp32 tensor.  A probability within an fp32 rounding of a threshold may fall on
the other side of it than torch's fp32 softmax puts it.

``roc_curve`` keeps the reference's ``compute()`` formula AS IT STANDS: row 0 is ``res[0, 0] / (res[0, 0] + res[0, 1])``,
which on torchmetrics' [true, predicted] matrix is TN / (TN + FP) -- the true NEGATIVE rate, although the reference's
docstring calls it the true positive rate -- and row 1 is FN / (FN + TP).  ``tpr`` / ``fpr`` are what their names say.
torchmetrics is not available to hold this to: its ConfusionMatrix is restated from version 0.2 (parity unpinned,
DESIGN.md 7).
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .eval_common import FIXED_ONE, check_n_valid, raise_flags, read_back, require_device_tensors, require_gpu

FLAG_TEXT = {1: "a logit of a counted row was not finite",
             2: "a label lay outside [0, n_classes) and was not ignore_index",
             4: "a cross-entropy term reached 2^15, or the loss sum left int64"}
HEAD = ("n", "correct", "loss_rows", "loss_sum", "ignored")


def table_ints(n_classes, n_thresh):
    """``wfs_class_metrics_table_ints``, or a ``ValueError`` that names the limits."""
    n = int(_lib.load().wfs_class_metrics_table_ints(int(n_classes), int(n_thresh)))
    if n == 0:
        raise ValueError(
            "ClassificationMetrics: n_classes = %d must lie in 2 .. %d, n_thresh = %d in 1 .. %d, and the workgroup's LDS "
            "image 4 * (6 + C * C + 2 * C * (T + 1) + T) = %d bytes must fit %d"
            % (n_classes, _lib.WFS_CLASS_METRICS_MAX_CLASSES, n_thresh, _lib.WFS_CLASS_METRICS_MAX_THRESH,
               4 * (6 + n_classes * n_classes + 2 * n_classes * (n_thresh + 1) + n_thresh),
               _lib.WFS_CLASS_METRICS_LDS_BYTES))
    return n


def thresholds(n_thresh):
    """ROCCurve's ``(i + 1.0) / n_thresh`` as the fp32 values an fp32 tensor is compared with."""
    return np.array([np.float32((i + 1.0) / n_thresh) for i in range(n_thresh)], np.float32)


def rates_from_bins(bins):
    """``bins`` int64 [2, T + 1] (binary target, bin) of one class -> tn, fp, fn, tp as int64 [T]: the row is predicted
    positive at threshold i when its bin is above i."""
    above = bins[:, ::-1].cumsum(axis=1)[:, ::-1][:, 1:]            # [2, T]: rows with bin > i
    total = bins.sum(axis=1, keepdims=True)
    return total[0] - above[0], above[0], total[1] - above[1], above[1]


def _ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return a.astype(np.float64) / b.astype(np.float64)             # an empty denominator: NaN, as torch's division


class ClassificationMetrics:
    def __init__(self, device, n_classes, n_thresh=100, class_names=None, ignore_index=-100):
        self.n_classes, self.n_thresh, self.ignore_index = int(n_classes), int(n_thresh), int(ignore_index)
        n = table_ints(self.n_classes, self.n_thresh)
        self.device = require_gpu(device, "ClassificationMetrics")
        self.class_names = list(class_names) if class_names is not None else [str(k) for k in range(self.n_classes)]
        if len(self.class_names) != self.n_classes:
            raise ValueError("ClassificationMetrics: %d class names for %d classes" % (len(self.class_names), self.n_classes))
        self.thresholds = thresholds(self.n_thresh)
        self._thr = torch.from_numpy(self.thresholds).to(self.device)
        C, T = self.n_classes, self.n_thresh
        self._layout = [("head", (len(HEAD),)), ("confusion", (C, C)), ("roc", (C, 2, T + 1))]
        assert n == sum(int(np.prod(s)) for _k, s in self._layout)
        self.tables = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, logits, target, n_valid=None, loss_mask=None, max_blocks=0):
        """``logits`` [N, n_classes] fp32 / bf16 / fp16 whose last dimension is contiguous (a row stride above
        ``n_classes`` and any element offset are taken as they are), ``target`` int64 [N], ``n_valid`` the device-side
        row count of a capacity-padded batch, ``loss_mask`` bool / uint8 [N]: the rows whose cross-entropy term enters
        ``loss`` (every counted row without one).  One launch on the current stream; nothing is read back, the caller's
        tensors are only read."""
        require_device_tensors(logits, target, loss_mask)
        if logits.dim() != 2 or logits.shape[1] != self.n_classes or (logits.shape[0] > 0 and logits.stride(1) != 1):
            raise RuntimeError("ClassificationMetrics.add: logits must be [N, %d] with a contiguous last dimension, got "
                               "%s with strides %s" % (self.n_classes, tuple(logits.shape), tuple(logits.stride())))
        rows = int(logits.shape[0])
        if target.dtype != torch.int64 or tuple(target.shape) != (rows,):
            raise RuntimeError("ClassificationMetrics.add: target must be int64 [N] class indices")
        check_n_valid(n_valid, "ClassificationMetrics.add")
        if loss_mask is not None:
            if loss_mask.dtype == torch.bool:
                loss_mask = loss_mask.view(torch.uint8)
            if loss_mask.dtype != torch.uint8 or tuple(loss_mask.shape) != (rows,):
                raise RuntimeError("ClassificationMetrics.add: loss_mask must be bool or uint8 [N]")
        if rows == 0:
            return
        stride = int(logits.stride(0)) if rows > 1 else self.n_classes
        if stride < self.n_classes:
            raise RuntimeError("ClassificationMetrics.add: a row stride of %d elements is below n_classes" % stride)
        p = _lib.ptr
        _lib.check(_lib.load().wfs_class_metrics_accumulate(
            ctypes.c_void_p(logits.data_ptr()), _lib.dtype_code(logits), stride, p(target), self.ignore_index,
            p(loss_mask), rows, p(n_valid), self.n_classes, p(self._thr), self.n_thresh, p(self.tables), p(self.flags),
            int(max_blocks), _lib.stream_ptr()))

    def reset(self):
        self.tables.zero_()
        self.flags.zero_()

    def state_tensors(self):
        """The persistent accumulators: integer sums over batches, so N ranks combine them with one SUM all-reduce."""
        return [self.tables]

    def results(self):
        """One read-back.  ``n`` rows counted, ``correct``, ``acc`` = correct / n, ``loss`` = the mean cross-entropy over
        ``loss_rows``, ``ignored``; ``confusion`` int64 [C, C] (rows true, columns predicted); ``thresholds``; ``roc_bins``
        int64 [C, 2, T + 1]; per class name in ``classes`` the int64 [T] ``tn`` / ``fp`` / ``fn`` / ``tp``, ``tpr``,
        ``fpr`` and a trapezoid ``auc``; ``roc_curve(class_index=0)``: the float32 [2, T] of the reference's
        ``ROCCurve.compute()``."""
        cur = read_back(self.flags, self.tables)
        raise_flags("ClassificationMetrics", int(cur.take(1)[0]), FLAG_TEXT)
        tabs = {name: cur.take(shape).copy() for name, shape in self._layout}
        return results_from_tables(tabs["head"], tabs["confusion"], tabs["roc"], self.thresholds, self.class_names)


def results_from_tables(head, confusion, roc, thr, class_names):
    """``results()`` from the three integer tables (host arrays): everything derived is formed here, from exact integers."""
    h = {k: int(v) for k, v in zip(HEAD, head)}
    res = dict(n=h["n"], correct=h["correct"], loss_rows=h["loss_rows"], ignored=h["ignored"],
               acc=h["correct"] / h["n"] if h["n"] else float("nan"),
               loss=h["loss_sum"] / FIXED_ONE / h["loss_rows"] if h["loss_rows"] else float("nan"),
               confusion=confusion, thresholds=thr, roc_bins=roc, classes={})
    for k, name in enumerate(class_names):
        tn, fp, fn, tp = rates_from_bins(roc[k])
        tpr, fpr = _ratio(tp, tp + fn), _ratio(fp, fp + tn)
        # the trapezoid rule over the curve from (1, 1) -- threshold 0, every row positive -- through the T points down to
        # (0, 0), a threshold above 1
        x, y = np.concatenate([[1.0], fpr, [0.0]]), np.concatenate([[1.0], tpr, [0.0]])
        auc = float(np.sum((x[:-1] - x[1:]) * (y[:-1] + y[1:]) * 0.5))
        res["classes"][name] = dict(tn=tn, fp=fp, fn=fn, tp=tp, tpr=tpr, fpr=fpr, auc=auc)

    def roc_curve(class_index=0):
        c = res["classes"][class_names[class_index]]
        with np.errstate(divide="ignore", invalid="ignore"):
            # res[0, 0] / (res[0, 0] + res[0, 1]) and res[1, 0] / (res[1, 0] + res[1, 1]) of [true, predicted] matrices,
            # which torchmetrics 0.2 keeps and returns in fp32
            tn, fp, fn, tp = (c[k].astype(np.float32) for k in ("tn", "fp", "fn", "tp"))
            return np.stack([tn / (tn + fp), fn / (fn + tp)])
    res["roc_curve"] = roc_curve
    return res
