"""``LitWaveform``: host-side mirror of the reference's per-pulse module (src/engineering/LitWaveform.py on
src/engineering/LitBase.py:13-55): one waveform row per PMT pulse, one target per ROW, a mean-reduced criterion
(``L1Loss``, ``MSELoss`` or ``CrossEntropyLoss``), on psd/litbase.LitBase: ``configure_optimizers`` is the shared one, so
FlatSGD / FlatAdam / FlatAdamW take over a flat GPU parameter.

``use_detector_number`` appends the pulse's detector position to its row (n_samples += 3, fill_coords), for the
308-PMT detector only.  (The reference's error message for another count reads a misspelt attribute and raises
AttributeError instead of the IOError it builds; here it is the IOError.)

Captured training (psd/graph.GraphedTrainStep, ``per_row_targets``): the batch is padded to a row capacity and the
step gets the valid row count in device memory.  The loss is then the mean over the valid rows only -- the
reduction='none' criterion summed under a row mask, divided by the count -- so padding rows add nothing to the loss
and receive a zero gradient whatever the criterion (``ignore_index`` covers CrossEntropy alone).

``net_class`` ``WaveformModels.RecurrentWaveformNet`` gets its rows as [N, n_samples, 1] (``squeeze_index`` 2), every
other net as [N, 1, n_samples].  A net that declares ``takes_n_valid`` (ConvWaveformNet: BatchNorm statistics) is handed
the batch's valid-row count -- a device tensor in a captured step, else None -- in its ``n_valid`` attribute for the call.

``evaluator`` is the reference's ``TensorEvaluator`` on the GPU (psd/tensor_evaluator.py); ``test_step`` keeps what its
``add`` takes in ``last_test_outputs``, so ``evaluate.segment_test_loop(module, loader, device,
evaluator=module.evaluator)`` fills the per-PMT and the binned loss tables without a read-back per batch.

Out of scope: ``write_script`` / TorchScript export.
"""
import torch
from torch import nn

from .litbase import LitBase, evaluation_params, test_has_phys


class LitWaveform(LitBase):
    per_row_targets = True            # one target per pulse (row): the captured step pads them per row
    # Trainer.validate: the captured eval runner (psd/evaluate) scores logits as a classifier; this module validates
    # through its own validation_step (L1 / MSE have no accuracy: val_acc is NaN)
    captured_validation = False

    def __init__(self, config, trial=None):
        nc = config.net_config
        use_detector_number = getattr(nc, "use_detector_number", False)
        if use_detector_number:
            # before the net is built: it reads n_samples
            if not hasattr(nc, "num_detectors"):
                raise IOError("net config must contain 'num_detectors' property if 'use_detector_number' set to true")
            config.system_config.n_samples = config.system_config.n_samples + 3
            if nc.num_detectors != 308:
                raise IOError("num detectors " + str(nc.num_detectors) + " not supported")
        super().__init__(config, trial)
        self.use_detector_number = use_detector_number
        if use_detector_number:
            self.detector_num_factor_x = 1. / (self.nx - 1)
            self.detector_num_factor_y = 1. / (self.ny - 1)
        self.write_script = False
        self.squeeze_index = 2 if nc.net_class.endswith("RecurrentWaveformNet") else 1
        dc = config.dataset_config
        self.test_has_phys = test_has_phys(config)
        self.target_index = dc.dataset_params.label_index if hasattr(dc.dataset_params, "label_index") else None
        self.use_accuracy = False
        if nc.criterion_class == "L1Loss":
            self.metric_name = "mean absolute error"
        elif nc.criterion_class == "MSELoss":
            self.metric_name = "mean squared error"
        elif nc.criterion_class.startswith("BCE") or nc.criterion_class.startswith("CrossEntropy"):
            self.use_accuracy = True
            self.metric_name = "Accuracy"
        else:
            self.metric_name = "?"
        self.loss_no_reduce = self.criterion_class(*nc.criterion_params, reduction="none")
        if self.use_accuracy:
            self.softmax = nn.Softmax(dim=1)

    def _make_evaluator(self, device):
        """The ``TensorEvaluator`` the reference builds in ``__init__`` (LitWaveform.py:39-63; it raises on the CPU):
        ``calgroup`` from ``dataset_config``, ``target_has_phys``, ``target_index`` and ``metric_name`` as the
        constructor derives them, then ``config.evaluation_config`` as keyword arguments (one that repeats a name of
        the four raises TypeError)."""
        from .tensor_evaluator import TensorEvaluator
        return TensorEvaluator(device, calgroup=getattr(self.config.dataset_config, "calgroup", None),
                               target_has_phys=self.test_has_phys, target_index=self.target_index,
                               metric_name=self.metric_name, **evaluation_params(self.config))

    def fill_coords(self, coords, det):
        """Detector number -> (x, y, end) of the pulse (reference LitWaveform.fill_coords): segment det // 2 on the
        14 x 11 grid, scaled to [0, 1]; the PMT end det % 2."""
        seg = torch.floor_divide(det, 2)
        coords[:, 0] = (seg % 14) * self.detector_num_factor_x
        coords[:, 1] = torch.floor_divide(seg, 14) * self.detector_num_factor_y
        coords[:, 2] = det % 2

    def _rows(self, c, f):
        if self.use_detector_number:
            det = c.reshape(-1) if c.dim() == 2 and c.shape[1] == 1 else c
            coords = torch.zeros((f.shape[0], 3), dtype=f.dtype, device=f.device)
            self.fill_coords(coords, det)
            f = torch.cat((f, coords), dim=1)
        return f

    def _predict(self, f, target, phys=False, n_valid=None):
        if getattr(self.model, "takes_n_valid", False):
            # a net with batch statistics: the padding rows of a captured batch must stay out of them
            self.model.n_valid = n_valid
            try:
                predictions = self.model(f.unsqueeze(self.squeeze_index)).squeeze(1)
            finally:
                self.model.n_valid = None
        else:
            predictions = self.model(f.unsqueeze(self.squeeze_index)).squeeze(1)
        if predictions.dim() == 2 and (target.dim() == 1 or (target.dim() == 2 and phys)):
            predictions = predictions.squeeze(1)
        if predictions.dtype != torch.float32:
            predictions = predictions.float()            # 16-bit rows: the criterion in fp32 (LitPSD does the same)
        return predictions

    def _loss(self, predictions, target, n_valid=None):
        # the fused cross-entropy takes a padded batch too: its padding rows hold ignore_index (psd/graph.py)
        if n_valid is None or self._fuses_cross_entropy(predictions, target):
            return super()._loss(predictions, target)
        # a capacity-padded batch: the mean over the first n_valid rows, with no host read-back of the count
        per = self.loss_no_reduce(predictions, target)
        valid = torch.arange(per.shape[0], device=per.device) < n_valid.reshape(())
        if per.dim() > 1:
            valid = valid.reshape((-1,) + (1,) * (per.dim() - 1))
        count = n_valid.reshape(()).to(per.dtype) * (per[0].numel() if per.dim() > 1 else 1)
        return torch.where(valid, per, torch.zeros_like(per)).sum() / count

    def training_step(self, batch, batch_idx):
        c, f, n_valid, target = self._unpack(batch)
        predictions = self._predict(self._rows(c, f), target, n_valid=n_valid)
        loss = self._loss(predictions, target, n_valid)
        self.log("train_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def validation_step(self, batch, batch_idx):
        c, f, n_valid, target = self._unpack(batch)
        predictions = self._predict(self._rows(c, f), target, n_valid=n_valid)
        loss = self._loss(predictions, target, n_valid)
        results = {"val_loss": loss}
        if self.use_accuracy:
            pred = torch.argmax(self.softmax(predictions), dim=1)
            results["val_accuracy"] = (pred == target).float().mean()
        self.log_dict(results, on_epoch=True, prog_bar=True, logger=True)
        return results

    def test_step(self, batch, batch_idx):
        c, f, _n_valid, target = self._unpack(batch)
        f = self._rows(c, f)
        if self.occlude_index:                       # falsy for index 0, exactly as the reference
            f[:, self.occlude_index] = 0
        predictions = self._predict(f, target, phys=self.test_has_phys)
        scored = target[:, self.target_index] if self.test_has_phys else target
        loss = self.criterion.forward(predictions, scored)
        # what the reference hands its evaluator (LitWaveform.py:139-146)
        self.last_test_outputs = (c, f, target, self.loss_no_reduce(predictions, scored).detach())
        results = {"test_loss": loss}
        if self.use_accuracy:
            pred = torch.argmax(self.softmax(predictions), dim=1)
            results["val_accuracy"] = (pred == target).float().mean()     # the reference's key in test_step
        self.log_dict(results, on_epoch=True, logger=True)
        return results
