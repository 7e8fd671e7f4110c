"""``TemporalWaveformNet``: mirror of the reference's per-pulse TCN regressor / classifier
(src/models/WaveformModels.py:8-45).  One waveform row per PMT pulse, [N, 1, n_samples] -> TemporalConvNet(1, planes,
**conv_params) -> Flatten -> LinearBlock(n_samples * planes[-1], out_size, n_lin).

The TCN is psd/tcn.TemporalConvNet with ``fused=True``: its multi-channel plans run on the wfs_tcnc_* kernels
(csrc/tcnc.hip); the linear head runs through spconv.functional.head_forward (skinny / wide HIP linears).  Same
modules, parameters and state_dict as the reference's net.

``RecurrentWaveformNet`` (WaveformModels.py:93-110): [N, n_samples, 1] -> psd/recurrent.RecurrentNet(n_samples, 1, n_hidden,
n_layers, n_lin, out_size, **rnn_params) with ``fused=True``: the Elman RNN runs on the wfs_rnn_* scan kernels
(csrc/rnn.hip), the linear head as above.
"""
import logging

from torch import nn

from .blocks import LinearBlock
from .config import DictionaryUtility
from .recurrent import RecurrentNet
from .tcn import TemporalConvNet


def temporal_planes(hparams):
    """The reference's channel plan, quirks included (WaveformModels.py:21-27): ``n_expand`` levels rising to
    ``expansion_factor`` channels, then ``n_contract`` levels counting DOWN TO 0, whose last entry is replaced by
    ``out_planes``.  A config without these hparams raises AttributeError, as the reference does."""
    expand_factor = float(hparams.expansion_factor / hparams.n_expand)
    planes = [int(round(expand_factor * (i + 1))) for i in range(hparams.n_expand)]
    contract_factor = float((hparams.expansion_factor - hparams.out_planes) / hparams.n_contract)
    planes += [int(round(contract_factor * (hparams.n_contract - i - 1))) for i in range(hparams.n_contract)]
    planes[-1] = hparams.out_planes
    return planes


class TemporalWaveformNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.log = logging.getLogger(__name__)
        self.system_config = config.system_config
        self.net_config = config.net_config
        self.nsamples = self.system_config.n_samples
        self.flattened_size = self.nsamples
        hp = config.net_config.hparams
        self.output_size = hp.out_size if hasattr(hp, "out_size") else 1
        self.planes = temporal_planes(hp)
        if config.net_config.net_type == "TemporalConvolution":
            self.model = TemporalConvNet(1, self.planes, fused=True, **DictionaryUtility.to_dict(hp.conv_params))
        if hp.n_lin > 0:
            self.linear = LinearBlock(self.flattened_size * self.planes[-1], self.output_size, hp.n_lin).func
            self.flatten = nn.Flatten()

    def forward(self, x):
        from ..spconv.functional import head_forward
        x = self.model(x)
        if hasattr(self, "linear"):
            x = self.flatten(x)
            x = head_forward(x, self.linear)
        return x


class RecurrentWaveformNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.log = logging.getLogger(__name__)
        self.system_config = config.system_config
        self.net_config = config.net_config
        self.nsamples = self.system_config.n_samples
        hp = self.net_config.hparams
        if config.net_config.net_type == "RNN":
            self.model = RecurrentNet(self.nsamples, 1, hp.n_hidden, hp.n_layers, hp.n_lin, hp.out_size, fused=True,
                                      **DictionaryUtility.to_dict(hp.rnn_params))
        else:
            raise IOError("{} not supported net type".format(config.net_config.net_type))

    def forward(self, x):
        return self.model(x)
