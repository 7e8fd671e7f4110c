"""``LitZ`` and ``LitEZ``: host-side mirrors of the reference's per-segment regression modules
(src/engineering/LitZ.py:31-139, src/engineering/LitEZ.py:8-91, on src/engineering/LitBase.py:13-55,110-174): the net
predicts a dense [B, out, 14, 11] map, the loss compares it with the targets of the ACTIVE segments only -- both the mask
and the dense target come from ``SparseConvTensor(...).dense()`` (wfs_to_dense) -- with a sum-reduced criterion divided by
the number of rows (``net_config.SELoss``: of the single-ended segments only, psd/segments.py).

``net_config.fused_segment_loss`` (this project's own key) trains them on the fused HIP segment loss instead
(spconv.functional.SegmentMapLossFunction, csrc/segloss.hip: one launch forward, one backward, no read-back), which
also takes a capacity-padded batch: with the key the modules train through ``Trainer(capture=True)`` on
``FlatSGD`` / ``FlatAdam``.  Without it every bit of the mirrored behaviour stays.

Both sit on psd/litbase.LitBase through ``LitSegmentBase``.  The evaluators the reference's ``test_step`` feeds (ZEvaluatorWF, EZEvaluatorWF without a calibration group) are
psd/segment_evaluator.py, and for ``LitZ`` with phys test targets (``test_has_phys``) psd/real_z_evaluator.py; ``test_step`` leaves what it would hand them in ``last_test_outputs`` and
psd/evaluate.segment_test_loop does the hand-over.  Their plots and the calibration-database variants are out of scope.
"""
import torch

from .litbase import LitBase, additional_field_names, evaluation_params, test_has_phys
from .pid_evaluator import Z_INDEX
from .znet import SingleEndedEZConv, SingleEndedZConv


def real_evaluator_params(config, params):
    """``evaluation_config`` as keyword arguments with ``test_dataset_params.additional_fields`` written over it as
    ``additional_field_names`` (LitZ.py:43-48); no ``excludes`` rename here."""
    params = dict(params)
    names = additional_field_names(config)
    if names is not None:
        params["additional_field_names"] = names
    return params


def calibration_from_config(config):
    """``dataset_config.calibration_file``, an ``.npz`` of calibration curves (calibration.py), is this project's
    counterpart of the reference's ``dataset_config.calgroup`` (LitZ.py:57-58, LitEZ.py:31-32): the curves a Calibrator
    would read from the calibration database, loaded for the evaluator.  Returns the keyword arguments the evaluator gets:
    none without a file, else the curves and the waveform length of ``system_config.n_samples`` (the reference hard-codes
    150 there)."""
    path = getattr(config.dataset_config, "calibration_file", None)
    if path is None:
        return {}
    from .calibration import CalibrationCurves
    return {"calibration": CalibrationCurves.load(path), "n_samples": int(config.system_config.n_samples)}


class LitSegmentBase(LitBase):
    """What LitZ and LitEZ share: LitBase with ``event_predictions=False`` (a sum-reduced criterion) and the segment loss.
    Their evaluators (LitZ.py:43-60, LitEZ.py:24-35, the case without a calibration group) get
    ``config.evaluation_config`` as keyword arguments."""
    # without net_config.fused_segment_loss the optimizer steps model.parameters() even after Trainer.fit has set
    # optimizer_parameters: a gap kept on purpose ("A preserved gap")
    flat_optimizer = False
    FUSED_KEY = "fused_segment_loss"

    def __init__(self, config, trial=None):
        super().__init__(config, trial, event_predictions=False)
        if hasattr(config.net_config, "UseFFT"):
            raise NotImplementedError("UseFFT feeds complex features; not on the mirrored path")
        self.fused_segment_loss = bool(getattr(config.net_config, self.FUSED_KEY, False))
        self.segment_loss_kind = None
        if self.fused_segment_loss:
            from ..spconv import functional as Fsp
            self.segment_loss_kind = Fsp.segment_loss_kind(self.criterion)
            if self.segment_loss_kind is None:
                # no silent fall-back inside a captured step: the composition cannot take its padded batch
                raise ValueError("net_config.%s covers a sum-reduced plain L1Loss or MSELoss, not %s: remove the key to "
                                 "train on the torch composition" % (self.FUSED_KEY, type(self.criterion).__name__))
            # what Trainer.fit and psd/graph.GraphedTrainStep read: one target per row, padded per row; the flat
            # parameter goes to the optimizer; validation stays on validation_step (dense maps for the evaluators)
            self.per_row_targets, self.flat_optimizer, self.captured_validation = True, True, False

    def _unpack(self, batch):
        c, f, n_valid, target = LitBase._unpack(batch)
        if n_valid is not None and not (self.fused_segment_loss and c.is_cuda):
            raise ValueError("LitZ / LitEZ do not take a capacity-padded batch (a valid-row count as third element of "
                             "the inner list): the segment loss reads the batch size back from the host")
        return c, f, n_valid, target

    def _fuses_segment_loss(self, batch):
        """The training step takes the fused loss: the key is set and the batch lives on the GPU (CPU tensors, the
        oracle route, keep the composition).  Padded and exact-size batches alike, so that a replay, an eager step
        beside it and the eager trainer run the same arithmetic."""
        return self.fused_segment_loss and batch[0][0].is_cuda

    def _dense_maps_need_exact_size(self, n_valid):
        if n_valid is not None:
            raise ValueError("LitZ / LitEZ score a capacity-padded batch in training_step only (net_config.%s): the "
                             "dense maps of validation_step / test_step read the batch size back from the host"
                             % self.FUSED_KEY)

    def _dense_map(self, c, f):
        """The net's map for the dense-map route (validation_step, test_step, the composition): over the batch's OWN
        events, read off its last coordinate row as ``_calc_segment_loss`` reads them -- whatever ``batch_size_hint`` a
        captured training step has left on the net (its row capacity, psd/graph.GraphedTrainStep)."""
        return self.model([c, f], batch_size=int(c[-1, -1]) + 1)

    def _fused_segment_loss(self, c, predictions, target, cols, n_valid):
        """``(total, per_plane)``: plane ``p`` of ``predictions`` against column ``cols[p]`` of ``target``."""
        from ..spconv import functional as Fsp
        return Fsp.segment_map_loss(predictions, c, target, cols, self.segment_loss_kind,
                                    se_mask=self.SE_mask if self.SE_only else None, n_valid=n_valid)

    # reference LitBase._calc_segment_loss, :124-174
    def _calc_segment_loss(self, coo, predictions, target, use_float=True, target_index=None, sparse_mask=None):
        sp = self.model.spconv
        batch_size = int(coo[-1, -1]) + 1
        num_predictions = coo.shape[0]
        if target.shape[0] != num_predictions:
            raise ValueError("if using segment loss, target must have same number of elements in first dimension as "
                             "coordinate tensor")
        idx = coo[:, self.model.permute_tensor].contiguous()
        if sparse_mask is None:
            ones = torch.ones((num_predictions, predictions.shape[1]), dtype=torch.float32, device=predictions.device)
            sparse_mask = sp.SparseConvTensor(ones, idx, self.model.spatial_size, batch_size).dense()
        t = target.unsqueeze(1) if target.dim() == 1 else target
        target_tensor = sp.SparseConvTensor(t, idx, self.model.spatial_size, batch_size).dense()
        predictions = sparse_mask * predictions
        if target_index is None:
            want = target_tensor if use_float else target_tensor.squeeze(1)
        else:
            want = target_tensor[:, target_index, :, :]
            want = want.unsqueeze(1) if use_float else want
        if self.SE_only:
            loss = self.criterion.forward(self.SE_mask * predictions, self.SE_mask * want)
            num_predictions = torch.sum(self.SE_mask * sparse_mask)
        else:
            loss = self.criterion.forward(predictions, want)
        return loss / num_predictions, target_tensor, predictions, sparse_mask


class LitZ(LitSegmentBase):
    model_class = SingleEndedZConv

    def __init__(self, config, trial=None):
        super().__init__(config, trial)
        # reference LitZ.__init__, :34-37: real detector data carries the seven phys planes as test targets
        self.test_has_phys = test_has_phys(config)

    # reference LitZ._process_batch, :89-108
    def _process_batch(self, batch, target_index=None):
        c, f, additional_fields, n_valid, target = self._inputs(batch)
        self._dense_maps_need_exact_size(n_valid)
        predictions = self._dense_map(c, f)
        loss, target_tensor, predictions, _ = self._calc_segment_loss(c, predictions, target, target_index=target_index)
        return loss, predictions, target_tensor, c, f, additional_fields

    def _fused_train_loss(self, batch):
        """The training loss on the fused kernel: one plane against the per-row target."""
        c, f, _additional, n_valid, target = self._inputs(batch)
        predictions = self.model([c, f, n_valid] if n_valid is not None else [c, f])
        return self._fused_segment_loss(c, predictions, target, (0,), n_valid)[0]

    def training_step(self, batch, batch_idx):
        if self._fuses_segment_loss(batch):
            loss = self._fused_train_loss(batch)
        else:
            loss = self._process_batch(batch)[0]
        self.log("train_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def validation_step(self, batch, batch_idx):
        loss = self._process_batch(batch)[0]
        self.log("val_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def _make_evaluator(self, device):
        params = evaluation_params(self.config)
        if self.test_has_phys:
            from .real_z_evaluator import ZEvaluatorRealWFNorm
            return ZEvaluatorRealWFNorm(device, **real_evaluator_params(self.config, params))
        from .segment_evaluator import ZEvaluator
        for k, v in calibration_from_config(self.config).items():
            params.setdefault(k, v)
        return ZEvaluator(device, **params)

    def test_step(self, batch, batch_idx):
        if self.test_has_phys:
            # reference LitZ.test_step, :134-139: column z_index of the phys target is scored
            loss, predictions, target_tensor, c, f, additional_fields = self._process_batch(batch, target_index=Z_INDEX)
            self.last_test_outputs = (predictions.detach(), target_tensor.detach(), c, f, additional_fields)
        else:
            loss, predictions, target_tensor, c, f, _ = self._process_batch(batch)
            self.last_test_outputs = (predictions.detach(), target_tensor.detach(), c, f)
        results = {"test_loss": loss}
        self.log_dict(results, on_epoch=True, logger=True)
        return results


class LitEZ(LitSegmentBase):
    """Energy + z regression: a 2-plane prediction map, the loss the sum of the two per-plane segment losses
    (reference LitEZ._process_batch, :57-73; the second call reuses the first call's active-segment mask)."""
    model_class = SingleEndedEZConv

    def __init__(self, config, trial=None):
        super().__init__(config, trial)
        nc = config.net_config
        self.zscale = getattr(nc, "zscale", 1200.)
        self.escale = getattr(nc, "escale", 12.)
        self.e_adjust = getattr(nc, "e_adjust", 12.)
        self.e_factor = self.escale / self.e_adjust
        self.phys_coord = nc.algorithm == "features"

    def _scaled_features(self, f, in_place):
        """The head of the reference's ``_process_batch``: columns 0, 2 and 3 of physics-coordinate features times
        ``e_factor``, in place as the reference does it on the dense-map route.  The fused training route scales a COPY
        (the same products): a captured step's static feature buffer is read again by the warm-up replays with no
        hand-over in between, and its calibration step runs on the caller's own first batch, which the trainer then
        trains on -- an in-place factor would compound in both."""
        if self.phys_coord and self.e_factor != 1.:
            if not in_place:
                f = f.clone()
            f[:, 0] *= self.e_factor
            f[:, 2] *= self.e_factor
            f[:, 3] *= self.e_factor
        if self.occlude_index:
            f[:, self.occlude_index] = 0
        return f

    def _process_batch(self, batch):
        c, f, n_valid, target = self._unpack(batch)
        self._dense_maps_need_exact_size(n_valid)
        f = self._scaled_features(f, in_place=True)
        predictions = self._dense_map(c, f)
        ZLoss, target_z, predictions_z, sparse_mask = self._calc_segment_loss(c, predictions[:, 0].unsqueeze(1),
                                                                              target[:, 0])
        ELoss, target_E, predictions_E, _ = self._calc_segment_loss(c, predictions[:, 1].unsqueeze(1), target[:, 1],
                                                                    sparse_mask=sparse_mask)
        predictions = torch.cat((predictions_z, predictions_E), dim=1)
        target_tensor = torch.cat((target_z, target_E), dim=1)
        return c, f, predictions, target_tensor, ZLoss + ELoss, ELoss, ZLoss

    def training_step(self, batch, batch_idx):
        if self._fuses_segment_loss(batch):
            # both planes in ONE launch: per_plane = (ZLoss, ELoss), the loss their sum
            c, f, n_valid, target = self._unpack(batch)
            f = self._scaled_features(f, in_place=False)
            predictions = self.model([c, f, n_valid] if n_valid is not None else [c, f])
            loss = self._fused_segment_loss(c, predictions, target, (0, 1), n_valid)[0]
        else:
            loss = self._process_batch(batch)[4]
        self.log("train_loss", loss, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def validation_step(self, batch, batch_idx):
        _, _, _, _, loss, ELoss, ZLoss = self._process_batch(batch)
        results = {"val_loss": loss, "val_MAE_E": ELoss, "val_MAE_z": ZLoss}
        self.log_dict(results, on_epoch=True, prog_bar=True, logger=True)
        return results

    def _make_evaluator(self, device):
        from .segment_evaluator import EZEvaluator
        params = evaluation_params(self.config)
        params.setdefault("E_scale", self.e_adjust)            # the reference passes e_scale=self.e_adjust
        for k, v in calibration_from_config(self.config).items():
            params.setdefault(k, v)
        return EZEvaluator(device, **params)

    def test_step(self, batch, batch_idx):
        c, f, predictions, target_tensor, loss, ELoss, ZLoss = self._process_batch(batch)
        self.last_test_outputs = (predictions.detach(), target_tensor.detach(), c, f)
        results = {"test_loss": loss, "test_MAE_E": ELoss, "test_MAE_z": ZLoss}
        self.log_dict(results, on_epoch=True, logger=True)
        return results
