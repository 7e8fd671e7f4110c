"""Alias module: ``"net_class": "WaveformModels.TemporalWaveformNet"`` with ``"waveformml_amd.psd.WaveformModels"`` in
``net_config.imports`` (cf. reference config/examples/SingleWaveformTCN.json); ``WaveformModels.RecurrentWaveformNet`` likewise
(config/examples/SingleWaveformRNN.json)."""
from .waveform import RecurrentWaveformNet, TemporalWaveformNet  # noqa: F401
