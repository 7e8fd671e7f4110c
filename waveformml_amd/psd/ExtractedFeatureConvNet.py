"""Alias module so that reference-style config strings (``"net_class": "ExtractedFeatureConvNet.ExtractedFeatureConvNet"``
with ``"waveformml_amd.psd.ExtractedFeatureConvNet"`` in ``imports``) resolve here."""
from .featurenet import ExtractedFeatureConvNet  # noqa: F401
