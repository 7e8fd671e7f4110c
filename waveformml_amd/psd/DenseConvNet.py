"""Alias module so that reference-style config strings (``"net_class": "DenseConvNet.DenseConvNet"`` with
``"waveformml_amd.psd.DenseConvNet"`` in ``imports``) resolve here."""
from .densenet import DenseConvNet  # noqa: F401
