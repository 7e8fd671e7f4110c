"""``LitSegClassifier``: host-side mirror of the reference's per-SEGMENT classifier (src/engineering/LitSegClassifier.py:15-100
on src/engineering/LitBase.py:13-55): the net -- ``SPConvNet.SPConvPreserveNet`` in config/examples/IoniClassifierCNN.json --
returns one logit row per ACTIVE segment [N, n_type], the target holds one label per row, the criterion is mean-reduced
(``net_config.SELoss``: over the rows of single-ended segments only).  ``evaluator`` is the reference's ``PIDEvaluator`` on
the GPU (psd/pid_evaluator.py); ``test_step`` keeps what its ``add`` takes in ``last_test_outputs``, so
``evaluate.segment_test_loop(module, loader, device, evaluator=module.evaluator)`` fills the PID tables without a read-back
per batch.  ``metrics`` is the reference's ``torchmetrics.Accuracy``, ``ConfusionMatrix`` and ``ROCCurve`` as one
psd/class_metrics.ClassificationMetrics (ROC tables for every class): ``test_step`` keeps the logits in ``last_test_logits``
and, under ``SELoss``, the single-ended rows in ``last_test_loss_mask``, so ``segment_test_loop(..., metrics=module.metrics)``
fills them with one launch per batch.  The torch_geometric ``Data`` batch form is out of scope.
"""
import torch

from .lit import LitPSD


class LitSegClassifier(LitPSD):
    per_row_targets = True            # one label per active segment (row): psd/graph.GraphedTrainStep pads them per row

    def __init__(self, config, trial=None):
        super().__init__(config, trial)
        self.softmax = torch.nn.Softmax(dim=1)          # LitPSD's is a LogSoftmax
        self.last_test_loss_mask = None                 # SELoss: the rows test_step's loss is the mean over

    def _make_evaluator(self, device):
        """The ``PIDEvaluator`` the reference builds in ``__init__`` (LitSegClassifier.py:26-33)."""
        from .pid_evaluator import PIDEvaluator
        return PIDEvaluator(device, **self._segment_evaluator_params())

    def _class_names(self):
        """``system_config.type_names``, else the PID evaluator's class names where they are as many as ``n_type``."""
        names = super()._class_names()
        if names is None:
            from .pid_evaluator import PID_MAPPED_NAMES
            if self.n_type == len(PID_MAPPED_NAMES):
                names = [PID_MAPPED_NAMES[i] for i in range(self.n_type)]
        return names

    # reference LitSegClassifier._process_batch, :36-63
    def _process_batch(self, batch):
        c, f, additional_fields, n_valid, target = self._inputs(batch)
        predictions = self.model([c, f, n_valid] if n_valid is not None else [c, f])
        logits = predictions if predictions.dtype == torch.float32 else predictions.float()
        self._loss_mask = None
        if self.SE_only:
            # the reference indexes predictions[se_inds] / target[se_inds]; the same mean over the same rows with a
            # static shape: every other row's target becomes the criterion's ignore_index
            se_inds = self._loss_mask = self.SE_mask[0, 0, c[:, 0].long(), c[:, 1].long()] == 1.0
            ignore = torch.full_like(target, getattr(self.criterion, "ignore_index", -100))
            loss = self._loss(logits, torch.where(se_inds, target, ignore))
        else:
            loss = self._loss(logits, target)
        return loss, predictions, target, c, f, additional_fields

    def training_step(self, batch, batch_idx):
        loss = self._process_batch(batch)[0]
        self.log("train_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def validation_step(self, batch, batch_idx):
        loss, predictions, target = self._process_batch(batch)[:3]
        pred = torch.argmax(self.softmax(predictions), dim=1)
        results = {"val_loss": loss, "val_acc": (pred == target).float().mean()}
        self.log_dict(results, on_epoch=True, prog_bar=True, logger=True)
        return results

    def test_step(self, batch, batch_idx):
        loss, predictions, target, c, _f, additional_fields = self._process_batch(batch)
        pred = torch.argmax(self.softmax(predictions), dim=1)
        self.last_test_outputs = (pred, target, c, additional_fields)
        self.last_test_logits, self.last_test_loss_mask = predictions.detach(), self._loss_mask
        results = {"test_loss": loss, "test_acc": (pred == target).float().mean()}
        self.log_dict(results, on_epoch=True, logger=True)
        return results
