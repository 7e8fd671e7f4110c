"""Alias module: ``"net_class": "WaveformModels.TemporalWaveformNet"`` with ``"waveformml_amd.psd.WaveformModels"`` in
``net_config.imports`` (cf. reference config/examples/SingleWaveformTCN.json); ``WaveformModels.RecurrentWaveformNet`` likewise
(config/examples/SingleWaveformRNN.json), ``WaveformModels.ConvWaveformNet`` and ``WaveformModels.LinearWaveformNet``."""
from .waveform import ConvWaveformNet, LinearWaveformNet, RecurrentWaveformNet, TemporalWaveformNet  # noqa: F401
