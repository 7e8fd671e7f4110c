"""``ExtractedFeatureConvNet``: host-side mirror of the reference's network for extracted-feature rows
(src/models/ExtractedFeatureConvNet.py): an ``ExtractedFeatureConv`` stack (psd/blocks.py) from ``n_features`` channels on
the 14 x 11 grid, ``ToDense``, flatten, a ``LinearBlock`` head.  The rows are what ``PulseDatasetDet`` reads: seven
physics quantities per segment.

The wrapper is ``SPConvNet``'s: the same ``[coords, feats]`` / ``[coords, feats, n_valid]`` forward, the same hand-over of
batch-first indices and event offsets from a captured step (psd/graph.py), the same head routes -- so ``Trainer(capture=
True)`` and ``evaluate.test_loop(capture=True)`` run it as they run ``SPConvNet``.  Parameter names follow the reference
(``model.network.<i>``, ``linear.<i>``).  The operator package is the module the config's ``imports`` binds to ``spconv``
(default: waveformml_amd.spconv; the reference imports spconv itself).
"""
import logging

import torch
from torch import nn

from .blocks import ExtractedFeatureConv, LinearBlock
from .config import DictionaryUtility, ModuleUtility
from .net import SPConvNet


class ExtractedFeatureConvNet(SPConvNet):
    def __init__(self, config):
        nn.Module.__init__(self)
        self.log = logging.getLogger(__name__)
        if config.net_config.net_type != "2DConvolution":
            raise IOError("config.net_config.net_type must be 2DConvolution")
        self.system_config = config.system_config
        self.net_config = config.net_config
        self.nfeatures = self.system_config.n_features
        self.ntype = self.system_config.n_type
        self.modules_util = ModuleUtility(self.net_config.imports)
        if "spconv" in self.modules_util.modules:
            self.spconv = self.modules_util.modules["spconv"]
        else:
            import waveformml_amd.spconv as sp
            self.spconv = sp
        self.ndim = 2
        self.spatial_size = [14, 11]
        size = [14, 11, self.nfeatures]
        hparams = self.net_config.hparams
        self.model = ExtractedFeatureConv(self.spconv, self.nfeatures, hparams.out_planes, hparams.n_conv, size,
                                          **DictionaryUtility.to_dict(hparams.conv))
        self.schedule = self.model.schedule
        flat_size = 1
        for s in self.model.out_size:
            flat_size *= s
        self.n_linear = flat_size
        self.log.debug("Flattened size of the SCN network output is {}".format(flat_size))
        self.linear = LinearBlock(flat_size, self.ntype, hparams.n_lin).func
        self.register_buffer("permute_tensor", torch.LongTensor([2, 0, 1]), persistent=False)   # batch index first
        self.batch_size_hint = None
        self.batch_events = None

    @property
    def sparseModel(self):
        """What ``SPConvNet``'s forward runs: the stack of ``self.model`` (registered once, under the reference's name)."""
        return self.model.network
