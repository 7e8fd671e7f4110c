"""Alias module: ``"net_class": "WaveformModels.TemporalWaveformNet"`` with ``"waveformml_amd.psd.WaveformModels"`` in
``net_config.imports`` (cf. reference config/examples/SingleWaveformTCN.json)."""
from .waveform import TemporalWaveformNet  # noqa: F401
