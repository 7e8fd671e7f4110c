"""One config per Lightning-module mirror, and the layout record tests/golden/lit_module_layout.json holds for each:
the ordered ``state_dict()`` keys with shapes and dtypes, the ordered top-level ``named_children()`` names and the
buffer names.  Shared by tests/golden/make_lit_module_layout.py (which writes the file) and tests/test_litbase_host.py
(which compares against it).  Layout only, no float values: the file does not depend on the torch build.

The configs are the ones the host tests already build; the per-segment ones carry ``SELoss`` so that the ``SE_mask``
buffer is part of the record."""
import copy
import importlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_IMPORTS = ["torch.nn", "waveformml_amd.psd.SPConvNet", "oracle.spconv"]


def _json(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return json.load(f)


def _psd():
    cfg = _json("tests", "golden", "gep_config.json")
    cfg["net_config"]["imports"] = ["oracle.spconv" if m == "waveformml_amd.spconv" else m
                                    for m in cfg["net_config"]["imports"]]
    return cfg


def _seg_classifier():
    from test_segment_callers import IONI
    cfg = copy.deepcopy(IONI)
    cfg["net_config"]["SELoss"] = True
    return cfg


def _seg_quantifier():
    cfg = _json("config", "segment_quantifier_z.json")
    cfg["net_config"]["imports"] = list(CPU_IMPORTS)
    return cfg


def _z():
    from test_host_mirror import _z_config
    cfg = copy.deepcopy(_z_config(["oracle.spconv"]))
    cfg["net_config"]["SELoss"] = True
    return cfg


def _ez():
    from test_segment_callers import ez_config
    return ez_config(["oracle.spconv"])


def _waveform(criterion="L1Loss"):
    cfg = _json("config", "waveform_tcn_z.json")
    cfg["net_config"]["criterion_class"] = criterion
    return cfg


# name -> (module, class, config dictionary)
CASES = {
    "LitPSD": ("waveformml_amd.psd.LitPSD", "LitPSD", _psd),
    "LitSegClassifier": ("waveformml_amd.psd.LitSegClassifier", "LitSegClassifier", _seg_classifier),
    "LitSegQuantifier": ("waveformml_amd.psd.LitSegQuantifier", "LitSegQuantifier", _seg_quantifier),
    "LitZ": ("waveformml_amd.psd.litz", "LitZ", _z),
    "LitEZ": ("waveformml_amd.psd.LitEZ", "LitEZ", _ez),
    "LitWaveform": ("waveformml_amd.psd.LitWaveform", "LitWaveform", _waveform),
    "LitWaveform_cross_entropy": ("waveformml_amd.psd.LitWaveform", "LitWaveform", lambda: _waveform("CrossEntropyLoss")),
}


def lit_class(name):
    module, cls, _ = CASES[name]
    return getattr(importlib.import_module(module), cls)


def build(name, edit=None):
    """The module of case ``name``; ``edit(cfg)`` changes the config dictionary first."""
    from waveformml_amd.psd.config import load_config
    cfg = CASES[name][2]()
    if edit is not None:
        edit(cfg)
    return lit_class(name)(load_config(cfg))


def layout(module):
    return {
        "state_dict": [[k, list(v.shape), str(v.dtype)] for k, v in module.state_dict().items()],
        "children": [n for n, _ in module.named_children()],
        "buffers": [n for n, _ in module.named_buffers()],
    }
