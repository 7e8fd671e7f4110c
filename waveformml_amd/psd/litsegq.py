"""``LitSegQuantifier``: host-side mirror of the reference's per-SEGMENT regression module
(src/engineering/LitSegQuantifier.py on src/engineering/LitBase.py): the net returns one number per ACTIVE segment
([N, 1], squeezed), the target holds the physics row of every segment ([N, n_phys], scored on column
``dataset_params.label_index``) or the one quantity itself ([N]), the criterion is mean-reduced -- with
``net_config.SELoss`` over the rows of single-ended segments only -- and the mean squared error over the same rows is
logged beside it (``val_mse`` / ``test_mse``; the reference's torchmetrics ``MeanSquaredError`` per step).

The loss.  A mean-reduced ``L1Loss`` / ``MSELoss`` on the GPU is one HIP launch forward and one backward
(spconv.functional.MaskedRegressionLossFunction, csrc/segloss.hip): the single-ended mask, the target column and the
valid-row count of a captured step (psd/graph.GraphedTrainStep, ``per_row_targets``: rows and targets padded to a
capacity, the padding targets hold the captured step's fill value) are applied inside the kernel, which selects the
rows that do not count OUT, so whatever they hold the loss stays finite and their gradient is exactly 0.  Any other
criterion, and the CPU, take ``masked_regression_composition``: the same masks as a torch composition with a static
shape (a ``reduction='none'`` copy of the criterion summed under ``where``), written once here.

``evaluator`` is the reference's ``SegEvaluator`` on the GPU (psd/quantifier_evaluator.py); ``test_step`` keeps what its
``add`` takes in ``last_test_outputs``, so ``evaluate.segment_test_loop(module, loader, device,
evaluator=module.evaluator)`` fills the tables without a read-back per batch.  The reference REPLACES its evaluator
parameters with ``evaluation_config`` when the config has one and so loses ``additional_field_names`` (and with them the
PID classes); here ``evaluation_config`` is merged over them.

The reference config's net, ``GraphNet.GraphNet``, is psd/graphnet.py (config/segment_quantifier_graph.json).  Out of
scope: the torch_geometric ``Data`` batch form, ``write_script``.
"""
import copy

import torch

from .litbase import LitBase


def masked_regression_composition(criterion_none, predictions, scored, counted):
    """``(loss, mse)`` over the rows where ``counted`` is true, as a torch composition with a static shape:
    ``criterion_none`` is the criterion with ``reduction='none'``.  Rows that are not counted are replaced before the
    criterion sees them, not multiplied by zero afterwards."""
    zero = torch.zeros_like(predictions)
    p, t = torch.where(counted, predictions, zero), torch.where(counted, scored.to(predictions.dtype), zero)
    count = counted.sum().to(predictions.dtype)
    per = criterion_none(p, t)
    loss = torch.where(counted, per, torch.zeros_like(per)).sum() / count
    mse = torch.where(counted, (p - t) ** 2, zero).sum() / count
    return loss, mse.detach()


class LitSegQuantifier(LitBase):
    per_row_targets = True            # one target row per active segment: psd/graph.GraphedTrainStep pads them per row
    # Trainer.validate: the captured eval runner (psd/evaluate) scores logits as a classifier; this module validates
    # through its own validation_step
    captured_validation = False

    def __init__(self, config, trial=None):
        if not hasattr(config.system_config, "n_type"):
            config.system_config.n_type = 1           # one number per segment: the nets read it (net.py, graphnet.py)
        super().__init__(config, trial)
        self.target_index = config.dataset_config.dataset_params.label_index
        self.criterion_none = copy.deepcopy(self.criterion)
        self.criterion_none.reduction = "none"

    def _make_evaluator(self, device):
        """The ``SegEvaluator`` the reference builds in ``__init__`` (LitSegQuantifier.py:16-28): the per-row evaluators'
        keywords, then ``target_index``."""
        from .quantifier_evaluator import SegEvaluator
        params = self._segment_evaluator_params()
        params["target_index"] = self.target_index
        return SegEvaluator(device, **params)

    def _loss(self, predictions, target, c, n_valid=None):
        """(loss, mse) over the counted rows: below ``n_valid`` and, with ``SELoss``, on a single-ended segment."""
        mask = self.SE_mask if self.SE_only else None
        if predictions.is_cuda:
            from ..spconv import functional as Fsp
            if Fsp.can_fuse_regression_loss(self.criterion, predictions, target):
                return Fsp.masked_regression_loss(predictions, target, Fsp.regression_loss_kind(self.criterion),
                                                  col=self.target_index, coords=c, se_mask=mask, n_valid=n_valid)
        scored = target[:, self.target_index] if target.dim() > 1 else target
        counted = torch.ones(predictions.shape[0], dtype=torch.bool, device=predictions.device)
        if n_valid is not None:
            counted = torch.arange(predictions.shape[0], device=predictions.device) < n_valid.reshape(())
        if mask is not None:
            x = c[:, 0].long().clamp(0, mask.shape[2] - 1)          # padding rows: any segment, they are not counted
            y = c[:, 1].long().clamp(0, mask.shape[3] - 1)
            counted = counted & (mask[0, 0, x, y] == 1.0)
        if predictions.dtype != torch.float32:
            predictions = predictions.float()            # 16-bit rows: the criterion in fp32 (LitPSD does the same)
        return masked_regression_composition(self.criterion_none, predictions, scored, counted)

    # reference LitSegQuantifier._process_batch
    def _process_batch(self, batch):
        c, f, additional_fields, n_valid, target = self._inputs(batch)
        predictions = self.model([c, f, n_valid] if n_valid is not None else [c, f]).squeeze(1)
        loss, mse = self._loss(predictions, target, c, n_valid)
        return loss, predictions, target, c, f, additional_fields, mse

    def training_step(self, batch, batch_idx):
        loss = self._process_batch(batch)[0]
        self.log("train_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def validation_step(self, batch, batch_idx):
        out = self._process_batch(batch)
        results = {"val_loss": out[0], "val_mse": out[6]}
        self.log_dict(results, on_epoch=True, prog_bar=True, logger=True)
        return results

    def test_step(self, batch, batch_idx):
        loss, predictions, target, c, _f, additional_fields, mse = self._process_batch(batch)
        # what the reference hands its evaluator (LitSegQuantifier.py:84)
        self.last_test_outputs = (predictions.detach(), target, c, additional_fields)
        results = {"test_loss": loss, "test_mse": mse}
        self.log_dict(results, on_epoch=True, logger=True)
        return results
