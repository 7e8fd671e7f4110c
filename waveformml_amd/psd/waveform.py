"""``TemporalWaveformNet``: mirror of the reference's per-pulse TCN regressor / classifier
(src/models/WaveformModels.py:8-45).  One waveform row per PMT pulse, [N, 1, n_samples] -> TemporalConvNet(1, planes,
**conv_params) -> Flatten -> LinearBlock(n_samples * planes[-1], out_size, n_lin).

The TCN is psd/tcn.TemporalConvNet with ``fused=True``: its multi-channel plans run on the wfs_tcnc_* kernels
(csrc/tcnc.hip); the linear head runs through spconv.functional.head_forward (skinny / wide HIP linears).  Same
modules, parameters and state_dict as the reference's net.

``RecurrentWaveformNet`` (WaveformModels.py:93-110): [N, n_samples, 1] -> psd/recurrent.RecurrentNet(n_samples, 1, n_hidden,
n_layers, n_lin, out_size, **rnn_params) with ``fused=True``: the Elman RNN runs on the wfs_rnn_* scan kernels
(csrc/rnn.hip), the linear head as above.

``ConvWaveformNet`` (WaveformModels.py:108-146): [N, 1, n_samples] -> psd/convnet.Conv1DNet(n_samples, **cnn_params) with
``fused=True`` -- the Conv1d + BatchNorm1d + ReLU stack on the wfs_conv1d_* kernels (csrc/conv1d.hip) -> Flatten ->
LinearPlanes (floor-interpolated widths, a ReLU after every Linear).  With ``use_detector_number`` the row's last three
entries bypass the conv stack and are concatenated in front of the linears.  Its BatchNorm statistics must not see the
padding rows of a captured batch: ``takes_n_valid`` makes LitWaveform hand it the valid-row count per call.

``LinearWaveformNet`` (WaveformModels.py:42-85): a LinearPlanes (or a LinearBlock) over the raw row, the reference's
plan logic with its quirks.
"""
import logging
from math import floor

import torch
from torch import nn

from .blocks import LinearBlock, LinearPlanes
from .config import DictionaryUtility
from .convnet import Conv1DNet
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


class ConvWaveformNet(nn.Module):
    takes_n_valid = True              # LitWaveform sets ``n_valid`` (device count of valid rows, or None) around a call

    def __init__(self, config):
        super().__init__()
        self.log = logging.getLogger(__name__)
        self.system_config = config.system_config
        self.net_config = config.net_config
        self.nsamples = self.system_config.n_samples
        self.num_inputs = self.nsamples
        self.n_valid = None
        if hasattr(config.net_config, "use_detector_number"):
            self.use_detector_number = config.net_config.use_detector_number
            self.num_inputs -= 3          # (whatever the flag's value, as the reference)
        else:
            self.use_detector_number = False
        hp = self.net_config.hparams
        if config.net_config.net_type == "CNN":
            self.model = Conv1DNet(self.num_inputs, fused=True, **DictionaryUtility.to_dict(hp.cnn_params))
        else:
            raise IOError("{} not supported net type".format(config.net_config.net_type))
        if hasattr(hp, "n_lin"):
            out = self.model.out_size[0] * self.model.out_size[1]
            if self.use_detector_number:
                out += 3
            planes = [int(floor(out - i * ((out - hp.out_size) / hp.n_lin))) for i in range(hp.n_lin + 1)]
            self.linear = LinearPlanes(planes, activation=nn.ReLU())
            self.flatten = nn.Flatten()

    def forward(self, x):
        from ..spconv.functional import head_forward
        det = None
        if self.use_detector_number:
            det = x[:, 0, self.nsamples - 3:]
            x = x[:, :, 0:self.nsamples - 3]
        x = self.model(x, n_valid=self.n_valid)
        if hasattr(self, "linear"):
            x = self.flatten(x)
            if self.use_detector_number:
                x = torch.cat((x, det), dim=1)
            x = head_forward(x, self.linear.net)
        return x


def linear_planes(hparams, n_samples, out_size):
    """LinearWaveformNet's widths, quirks included (WaveformModels.py:54-74): [n_samples] alone without ``n_expand``;
    else ``n_expand`` widths rising to n_samples * expansion_factor, then widths falling by a step computed from
    ``n_contract`` -- or, without it, from ``n_lin - n_expand`` -- but always ``hparams.n_contract`` of them (so the branch
    that derived the count from ``n_lin`` raises AttributeError, as the reference does); the last one is ``out_size``."""
    planes = [n_samples]
    if hasattr(hparams, "n_expand"):
        if hparams.n_expand > 0:
            if not hasattr(hparams, "expansion_factor"):
                raise IOError("config.net_config.hparams.expansion_factor must be set if n_expand > 0")
            step = float((planes[0] * hparams.expansion_factor - planes[0]) / hparams.n_expand)
            planes += [int(round(planes[0] + step * (i + 1))) for i in range(hparams.n_expand)]
        if not hasattr(hparams, "n_contract"):
            if not hasattr(hparams, "n_lin"):
                raise IOError("if n_expand is set, must either set n_contract or n_lin")
            n_contract = hparams.n_lin - hparams.n_expand
        else:
            n_contract = hparams.n_contract
        step = float((planes[-1] - out_size) / n_contract)
        top = planes[-1]
        planes += [int(round(top - step * (i + 1))) for i in range(hparams.n_contract)]
        planes[-1] = out_size
    return planes


class LinearWaveformNet(nn.Module):
    """``linear`` is a LinearPlanes (parameters ``linear.net.{2i}``), or -- without ``n_expand`` -- the Sequential of a
    LinearBlock (``linear.{i}``; the reference keeps the LinearBlock object itself there, which registers no parameter
    and cannot be called)."""

    def __init__(self, config):
        super().__init__()
        self.log = logging.getLogger(__name__)
        self.system_config = config.system_config
        self.net_config = config.net_config
        self.nsamples = self.system_config.n_samples
        self.flattened_size = self.nsamples
        hp = self.net_config.hparams
        out_size = hp.out_size if hasattr(hp, "out_size") else 1
        self.planes = linear_planes(hp, self.nsamples, out_size)
        if len(self.planes) == 1:
            if not hasattr(hp, "n_lin"):
                raise IOError("config.net_config.hparams.n_lin must be >= 1 if n_expand and n_contract not set")
            self.linear = LinearBlock(self.nsamples, out_size, hp.n_lin).func
        else:
            self.linear = LinearPlanes(self.planes, activation=nn.ReLU())

    def forward(self, x):
        from ..spconv.functional import head_forward
        layers = self.linear.net if isinstance(self.linear, LinearPlanes) else self.linear
        rows = head_forward(x.reshape(-1, x.shape[-1]), layers)          # 2-D rows: what the HIP linears take
        return rows.reshape(tuple(x.shape[:-1]) + (rows.shape[-1],))
