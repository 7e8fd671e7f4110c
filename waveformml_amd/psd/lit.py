"""``LitPSD``: host-side mirror of the reference's LightningModule for PSD classification
(src/engineering/LitPSD.py:20-151) on psd/litbase.LitBase: one label per event, a mean-reduced criterion.
"""
import torch
from torch import nn

from .litbase import LitBase, evaluation_params


class LitPSD(LitBase):
    def __init__(self, config, trial=None):
        n_type = config.system_config.n_type
        super().__init__(config, trial)
        self.n_type = n_type
        self.softmax = nn.LogSoftmax(dim=1)
        self.last_test_logits = None          # test_step's logits, for evaluate.test_loop(..., evaluator=..., metrics=...)
        self._metrics = None

    def _make_evaluator(self, device):
        """The reference's ``self.evaluator = PSDEvaluator(system_config.type_names, ...)`` (src/engineering/LitPSD.py:
        35-46); ``None`` when the config names no types.  As there, the dataset class picks it: ``PulseDatasetDet`` (the
        last dotted component of ``dataset_class``) gets ``PhysEvaluator`` with ``evaluation_config`` as keywords, every
        other class ``PSDEvaluator``.  The reference's third branch, ``PulseDatasetWaveformNorm`` -> ``TensorEvaluator``,
        is not wired: its ``test_step`` calls ``add(batch, predictions, pred)``, which ``TensorEvaluator.add`` cannot
        take."""
        names = getattr(self.config.system_config, "type_names", None)
        if not names:
            return None
        dataset_class = str(getattr(self.config.dataset_config, "dataset_class", ""))
        if dataset_class.split(".")[-1] == "PulseDatasetDet":
            from .phys_evaluator import PhysEvaluator
            return PhysEvaluator(list(names), device, **evaluation_params(self.config))
        from .evaluator import PSDEvaluator
        return PSDEvaluator(list(names), device, n_samples=getattr(self.config.system_config, "n_samples", 150))

    def _class_names(self):
        names = getattr(self.config.system_config, "type_names", None)
        return list(names) if names else None

    @property
    def metrics(self):
        """The reference's ``torchmetrics.Accuracy`` / ``ConfusionMatrix(num_classes=n_type)`` (and LitSegClassifier's
        ``ROCCurve``) as one psd/class_metrics.ClassificationMetrics, built on first use on the device the model lives on,
        as ``evaluator`` is.  Nothing calls it implicitly: hand it to ``evaluate.test_loop`` /
        ``evaluate.segment_test_loop(..., metrics=module.metrics)``."""
        if self._metrics is None:
            from .class_metrics import ClassificationMetrics
            self._metrics = ClassificationMetrics(next(self.model.parameters()).device, self.n_type,
                                                  class_names=self._class_names(),
                                                  ignore_index=getattr(self.criterion, "ignore_index", -100))
        return self._metrics

    def _predict(self, c, f, target, n_valid=None):
        # the reference reads the batch size back from the last coordinate row (SPConvNet.py:63, a device->host
        # sync); one label per event means it equals len(target), which is known on the host
        if hasattr(self.model, "batch_size_hint"):
            self.model.batch_size_hint = int(target.shape[0])
        return self.model([c, f, n_valid] if n_valid is not None else [c, f])

    # reference LitPSD.training_step, :94-104
    def training_step(self, batch, batch_idx):
        c, f, n_valid, target = self._unpack(batch)
        predictions = self._predict(c, f, target, n_valid)
        loss = self._loss(predictions, target)
        self.log("train_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    # reference LitPSD.validation_step, :106-128
    def validation_step(self, batch, batch_idx):
        c, f, n_valid, target = self._unpack(batch)
        predictions = self._predict(c, f, target, n_valid)
        loss = self.criterion.forward(predictions, target)
        pred = torch.argmax(self.softmax(predictions), dim=1)
        acc = (pred == target).float().mean()
        results = {"val_loss": loss, "val_acc": acc}
        self.log_dict(results, on_epoch=True, prog_bar=True, logger=True)
        return results

    # reference LitPSD.test_step, :130-151 (evaluator plumbing is out of scope)
    def test_step(self, batch, batch_idx):
        c, f, n_valid, target = self._unpack(batch)
        if self.occlude_index:                       # falsy for index 0, exactly as the reference (:134)
            f[:, self.occlude_index] = 0
        predictions = self._predict(c, f, target, n_valid)
        self.last_test_logits = predictions.detach()
        loss = self.criterion.forward(predictions, target)
        pred = torch.argmax(self.softmax(predictions), dim=1)
        acc = (pred == target).float().mean()
        results = {"test_loss": loss, "test_acc": acc}
        self.log_dict(results, on_epoch=True, logger=True)
        return results
