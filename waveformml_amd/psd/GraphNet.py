"""Alias module so that reference-style config strings (``"net_class": "GraphNet.GraphNet"`` with
``"waveformml_amd.psd.GraphNet"`` in ``imports``; cf. reference config/examples/IoniClassifierGraph.json) resolve here."""
from .graphnet import BatchNorm, FiLMConv, GraphLayer, GraphNet  # noqa: F401
