"""``LitBase``: host-side mirror of the base of the reference's Lightning modules (src/engineering/LitBase.py:13-76):
the constructor wiring, ``configure_optimizers``, the logging surface, the batch prologue, the classifier loss and the
lazily built evaluator that LitPSD, LitSegClassifier, LitSegQuantifier, LitZ / LitEZ (through litz.LitSegmentBase) and
LitWaveform share.

pytorch_lightning 1.2 (which the reference subclasses) is not installable here, so this is a plain ``nn.Module`` with the
same constructor, attributes (``model``, ``criterion``, ``lr``, ``modules``) and step semantics;
``waveformml_amd.psd.trainer.Trainer`` plays the part of ``pl.Trainer`` for it.  Where Lightning IS present,
INTEGRATION.md shows the two-line change that makes the reference's own modules use the MI355X operators instead (only
the ``imports`` list changes).
"""
import logging

import torch
from torch import nn

from .config import DictionaryUtility, ModuleUtility
from .segments import SE_DEAD_PMTS, segment_status, single_ended_mask


def test_has_phys(config):
    """The reference's ``test_has_phys`` (LitZ.py:34-37, LitWaveform.py): the test dataset's label is the whole
    ``"phys"`` row, without a ``label_index`` that picks one column of it."""
    params = getattr(config.dataset_config, "test_dataset_params", None)
    return params is not None and getattr(params, "label_name", None) == "phys" and not hasattr(params, "label_index")


def evaluation_params(config):
    """``config.evaluation_config`` as keyword arguments for an evaluator; ``{}`` without one."""
    params = getattr(config, "evaluation_config", None)
    return DictionaryUtility.to_dict(params) if params is not None else {}


def additional_field_names(config):
    """``dataset_config.test_dataset_params.additional_fields`` as a list; ``None`` without them."""
    params = getattr(getattr(config, "dataset_config", None), "test_dataset_params", None)
    return list(params.additional_fields) if hasattr(params, "additional_fields") else None


class LitBase(nn.Module):
    model_class = None                # a subclass that fixes its net (litz.LitSegmentBase); else net_config.net_class
    flat_optimizer = True             # configure_optimizers takes Trainer.fit's flat parameter (optimizer_parameters)
    per_row_targets = False           # one target per event; True: per row, psd/graph.GraphedTrainStep pads them per row
    captured_validation = True        # Trainer.validate may score the logits through the captured eval runner

    def __init__(self, config, trial=None, event_predictions=True):
        super().__init__()
        self.trial = trial
        self.pylog = logging.getLogger(__name__)
        self.config = config
        self.nx, self.ny = 14, 11
        self.lr = config.optimize_config.lr
        self.modules_util = ModuleUtility(config.net_config.imports + config.dataset_config.imports +
                                          config.optimize_config.imports)
        self.model = (type(self).model_class or self.modules_util.retrieve_class(config.net_config.net_class))(config)
        self.criterion_class = self.modules_util.retrieve_class(config.net_config.criterion_class)
        self.criterion = self.criterion_class(*config.net_config.criterion_params,
                                              reduction="mean" if event_predictions else "sum")
        self.occlude_index = getattr(config.dataset_config, "occlude_index", None)
        self.SE_only = bool(getattr(config.net_config, "SELoss", False))
        if self.SE_only:
            # the reference takes the table from its SingleEndedEvaluator; `net_config.SE_dead_pmts` replaces the default
            dead = getattr(config.net_config, "SE_dead_pmts", SE_DEAD_PMTS)
            self.register_buffer("SE_mask", single_ended_mask(segment_status(dead, self.nx, self.ny)))
        self.logged = {}
        self.optimizer_parameters = None      # set to [flat parameter] by ddp.FlatGradAllReducer(flatten=True)
        self._evaluator = None
        self.last_test_outputs = None         # what test_step leaves for evaluate.segment_test_loop to hand the evaluator

    def _make_evaluator(self, device):
        raise NotImplementedError

    @property
    def evaluator(self):
        """The evaluator the reference builds in ``__init__``, built on first use by the class's ``_make_evaluator`` on
        the device the model lives on and kept once there is one (``None`` is asked for again).  Nothing calls it
        implicitly: hand it to ``evaluate.test_loop`` / ``evaluate.segment_test_loop(..., evaluator=module.evaluator)``."""
        if self._evaluator is None:
            self._evaluator = self._make_evaluator(next(self.model.parameters()).device)
        return self._evaluator

    def _segment_evaluator_params(self):
        """Keyword arguments of the per-row evaluators (LitSegClassifier.py:26-33): ``additional_field_names`` from the
        test dataset, ``evaluation_config`` written over it, then ``excludes``, the reference's name for the dead PMTs."""
        params = {}
        names = additional_field_names(self.config)
        if names is not None:
            params["additional_field_names"] = names
        params.update(evaluation_params(self.config))
        if "excludes" in params:
            params["dead_pmts"] = params.pop("excludes")
        return params

    def forward(self, x):
        return self.model(x)

    def log(self, name, value, **kwargs):
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def log_dict(self, d, **kwargs):
        for k, v in d.items():
            self.log(k, v)

    # reference LitBase.configure_optimizers, :60-76
    def configure_optimizers(self):
        oc = self.config.optimize_config
        flat = self.optimizer_parameters if self.flat_optimizer else None
        params = flat if flat is not None else self.model.parameters()
        kwargs = DictionaryUtility.to_dict(oc.optimizer_params)
        opt_class = self.modules_util.retrieve_class(oc.optimizer_class)
        if flat is not None and len(flat) == 1:
            # one flat tensor: torch's multi-tensor ("foreach") kernels would run it on a handful of blocks (and so
            # does its "fused" SGD: measured 74 us against 19 us for the four single-tensor launches)
            import inspect
            on_gpu = all(p.is_cuda for p in flat)
            if opt_class is torch.optim.SGD and on_gpu:
                from .optim import FlatSGD
                opt_class = FlatSGD               # the whole update in one HIP launch, lr in device memory
            else:
                if opt_class in (torch.optim.Adam, torch.optim.AdamW) and on_gpu:
                    from .optim import FlatAdam, FlatAdamW
                    # one HIP launch, hyperparameters in device memory: steps inside a captured graph
                    opt_class = FlatAdamW if opt_class is torch.optim.AdamW else FlatAdam
                if "foreach" in inspect.signature(opt_class.__init__).parameters and "foreach" not in kwargs:
                    kwargs["foreach"] = False
        optimizer = opt_class(params, lr=self.lr, **kwargs)
        if getattr(oc, "scheduler_class", None):
            if not hasattr(oc, "scheduler_params"):
                raise IOError("Optimizer config has a learning scheduler class specified. You must also set "
                              "lr_schedule_parameters (dictionary of key value pairs).")
            scheduler = self.modules_util.retrieve_class(oc.scheduler_class)(
                optimizer, **DictionaryUtility.to_dict(oc.scheduler_params))
            return [optimizer], [scheduler]
        return optimizer

    @staticmethod
    def _unpack(batch):
        """((coords, feats), target) as the reference's collate_fn builds it -> (coords, feats, n_valid, target); a
        third element of the inner list is the device-side count of valid rows of a capacity-padded batch
        (psd/graph.py), else ``n_valid`` is None."""
        inputs, target = batch
        return inputs[0], inputs[1], (inputs[2] if len(inputs) > 2 else None), target

    def _inputs(self, batch):
        """``_unpack`` and the head of the reference's ``_process_batch`` / ``test_step``: a feature LIST is the
        features followed by the test dataset's additional fields, and column ``occlude_index`` of the features is
        zeroed.  Returns (coords, feats, additional_fields, n_valid, target)."""
        c, f, n_valid, target = self._unpack(batch)
        additional_fields = None
        if isinstance(f, list):
            additional_fields, f = f[1:], f[0]
        if self.occlude_index:                       # falsy for index 0, exactly as the reference (LitPSD.py:134)
            f[:, self.occlude_index] = 0
        return c, f, additional_fields, n_valid, target

    def _fuses_cross_entropy(self, predictions, target):
        if not predictions.is_cuda:
            return False
        from ..spconv import functional as Fsp
        return Fsp.can_fuse_cross_entropy(self.criterion, predictions, target)

    def _loss(self, predictions, target):
        """``self.criterion.forward`` -- through the one-launch HIP kernel when the criterion is a plain
        CrossEntropyLoss(mean) on GPU logits (same value; torch needs six launches for loss + gradient)."""
        if self._fuses_cross_entropy(predictions, target):
            from ..spconv import functional as Fsp
            return Fsp.cross_entropy_mean(predictions, target, self.criterion.ignore_index)
        return self.criterion.forward(predictions, target)
