"""Alias module: ``"imports": ["waveformml_amd.psd.LitWaveform"], "run_class": "LitWaveform"`` (cf. reference
config/examples/SingleWaveformTCN.json:2-8)."""
from .litwaveform import LitWaveform  # noqa: F401
