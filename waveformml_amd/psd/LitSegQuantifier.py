"""Alias module: ``"imports": ["waveformml_amd.psd.LitSegQuantifier"], "run_class": "LitSegQuantifier"`` (cf. reference
config/examples/SegQuantifier.json:2-8)."""
from .litsegq import LitSegQuantifier  # noqa: F401
