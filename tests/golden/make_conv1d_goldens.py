"""Generates tests/golden/conv1d_plans.json by importing the REFERENCE's own Python (/root/reference, this container
only), on the CPU:

  * src/models/ConvBlocks.py      Conv1DNet           -> channel plan, per-layer (kernel, stride, padding), out_size,
                                                         state_dict keys and shapes
  * src/models/WaveformModels.py  ConvWaveformNet     -> the same through a config, plus the widths of its linears
  * src/models/WaveformModels.py  LinearWaveformNet   -> the widths of its linears, or the exception it raises

Third-party modules that are not installed here are replaced by the inert stand-ins of make_reference_goldens.py for
the IMPORT only.  The committed JSON is data (inputs and recorded results); no reference source is copied.

Run:  python tests/golden/make_conv1d_goldens.py
"""
import json
import os
import sys

from torch import nn

from make_reference_goldens import REF, _stub_modules

HERE = os.path.dirname(os.path.abspath(__file__))

CONV1D = [  # Conv1DNet keyword arguments
    dict(length=59, num_channels=1, out_size=8, num_expand=2, num_contract=2, expand_factor=16, size_factor=5,
         pad_factor=1, stride_factor=2, min_kernel=2),                      # config/waveform_cnn_z.json
    dict(length=12, num_channels=1, out_size=8, num_expand=2, num_contract=2, expand_factor=16, size_factor=5,
         pad_factor=1, stride_factor=2, min_kernel=2),                      # ... on the pulse fixture's rows
    dict(length=59, num_channels=1, out_size=4, num_expand=0, num_contract=1, expand_factor=1),             # n == 1
    dict(length=59, num_channels=1, out_size=4, num_expand=1, num_contract=0 + 1, expand_factor=3, stride_factor=0),
    dict(length=64, num_channels=1, out_size=6, num_expand=0, num_contract=1, expand_factor=1, size_factor=4,
         pad_factor=1, stride_factor=3),                                    # n == 1 with a stride
    dict(length=62, num_channels=2, out_size=5, num_expand=1, num_contract=2, expand_factor=4, size_factor=6,
         pad_factor=1, stride_factor=3),                                    # stride 3; 6.5 -> 6 channels, 0.5 -> 0 padding
    dict(length=150, num_channels=1, out_size=3, num_expand=3, num_contract=2, expand_factor=7, size_factor=9,
         pad_factor=1, stride_factor=3, min_kernel=3),                      # strides 1 1 2 2 3 (1.5 and 2.5 round to even)
    dict(length=59, num_channels=1, out_size=3, num_expand=1, num_contract=1, expand_factor=6, size_factor=1,
         pad_factor=0, stride_factor=0, min_kernel=2),                      # every kernel clamped to min_kernel
    dict(length=100, num_channels=3, out_size=2, num_expand=2, num_contract=3, expand_factor=2.5, size_factor=7,
         pad_factor=0.5, stride_factor=2, min_kernel=4),                    # fractional factors, kernels clamped to 4
    dict(length=1024, num_channels=1, out_size=4, num_expand=1, num_contract=1, expand_factor=12, size_factor=7,
         pad_factor=1, stride_factor=2),
    dict(length=59, num_channels=4, out_size=16, num_expand=1, num_contract=1, expand_factor=16, size_factor=16,
         pad_factor=1, stride_factor=0),
]

CNN_Z = dict(num_channels=1, out_size=8, num_expand=2, num_contract=2, expand_factor=16, size_factor=5, pad_factor=1,
             stride_factor=2, min_kernel=2)
CONV_NETS = [  # (n_samples as the net sees it, net_config entries, hparams)
    (59, {"net_type": "CNN"}, {"n_lin": 2, "out_size": 1, "cnn_params": CNN_Z}),
    (62, {"net_type": "CNN", "use_detector_number": True}, {"n_lin": 2, "out_size": 1, "cnn_params": CNN_Z}),
    (62, {"net_type": "CNN", "use_detector_number": True}, {"n_lin": 2, "out_size": 2, "cnn_params": CNN_Z}),
    (59, {"net_type": "CNN"}, {"n_lin": 2, "out_size": 2, "cnn_params": CNN_Z}),
    (62, {"net_type": "CNN", "use_detector_number": False}, {"n_lin": 3, "out_size": 1, "cnn_params": CNN_Z}),
    (15, {"net_type": "CNN", "use_detector_number": True}, {"n_lin": 1, "out_size": 1, "cnn_params": CNN_Z}),
    (59, {"net_type": "CNN"}, {"out_size": 1, "cnn_params": CNN_Z}),                       # no linears
    (59, {"net_type": "TemporalConvolution"}, {"n_lin": 2, "out_size": 1, "cnn_params": CNN_Z}),
]

LINEAR_NETS = [  # (n_samples, hparams)
    (59, {"n_expand": 1, "expansion_factor": 2, "n_contract": 2, "n_lin": 3, "out_size": 1}),
    (59, {"n_expand": 2, "expansion_factor": 1.5, "n_contract": 3}),
    (62, {"n_expand": 0, "n_contract": 2, "out_size": 2}),
    (59, {"n_lin": 3, "out_size": 1}),
    (59, {"n_lin": 2}),
    (59, {"n_expand": 1, "n_contract": 2}),                        # no expansion_factor
    (59, {"n_expand": 1, "expansion_factor": 2}),                  # neither n_contract nor n_lin
    (59, {"n_expand": 1, "expansion_factor": 2, "n_lin": 3}),      # n_contract derived from n_lin, then read anyway
    (59, {"out_size": 1}),                                         # nothing to build from
]


def _state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _linears(seq):
    return [[m.in_features, m.out_features] for m in seq if isinstance(m, nn.Linear)]


def _conv_record(net):
    convs = [m for m in net.network if isinstance(m, nn.Conv1d)]
    return dict(planes=[convs[0].in_channels] + [c.out_channels for c in convs],
                layers=[[c.kernel_size[0], c.stride[0], c.padding[0]] for c in convs],
                bias=[c.bias is not None for c in convs], out_size=list(net.out_size),
                modules=[type(m).__name__ for m in net.network], state=_state(net))


def _attempt(build):
    try:
        return build(), None
    except Exception as e:             # noqa: BLE001  -- the exception's type is the recorded result
        return None, type(e).__name__


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    from src.models.ConvBlocks import Conv1DNet
    from src.models.WaveformModels import ConvWaveformNet, LinearWaveformNet
    from src.utils.util import DictionaryUtility

    def config(n_samples, net_config, hparams):
        return DictionaryUtility.to_object({"system_config": {"n_samples": n_samples},
                                            "net_config": dict(net_config, hparams=hparams)})
    out = {"conv1d": [], "conv_nets": [], "linear_nets": []}
    for kw in CONV1D:
        out["conv1d"].append(dict(args=kw, **_conv_record(Conv1DNet(**kw))))
    for n_samples, nc, hp in CONV_NETS:
        net, err = _attempt(lambda: ConvWaveformNet(config(n_samples, nc, hp)))
        rec = dict(n_samples=n_samples, net_config=nc, hparams=hp, raises=err)
        if net is not None:
            rec.update(conv=_conv_record(net.model), num_inputs=net.num_inputs,
                       linears=_linears(net.linear.net) if hasattr(net, "linear") else None,
                       linear_modules=[type(m).__name__ for m in net.linear.net] if hasattr(net, "linear") else None,
                       state=_state(net))
        out["conv_nets"].append(rec)
    for n_samples, hp in LINEAR_NETS:
        net, err = _attempt(lambda: LinearWaveformNet(config(n_samples, {"net_type": "Linear"}, hp)))
        rec = dict(n_samples=n_samples, hparams=hp, raises=err)
        if net is not None:
            planes = isinstance(net.linear, nn.Module)              # LinearPlanes; else the LinearBlock object
            rec.update(kind="LinearPlanes" if planes else "LinearBlock",
                       linears=_linears(net.linear.net if planes else net.linear.func),
                       linear_modules=[type(m).__name__ for m in (net.linear.net if planes else net.linear.func)],
                       state=_state(net))
        out["linear_nets"].append(rec)
    path = os.path.join(HERE, "conv1d_plans.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
