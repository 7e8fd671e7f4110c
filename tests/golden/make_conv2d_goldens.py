"""Generates tests/golden/conv2d_plans.json by importing the REFERENCE's own Python (/root/reference, this container
only), on the CPU:

  * src/models/ConvBlocks.py     Conv2DBlock    -> channel frames, per-layer (kernel, stride, padding, dilation, bias),
                                                   out_size, module type names, state_dict keys and shapes, or the
                                                   name of the exception it raises
  * src/models/DenseConvNet.py   DenseConvNet   -> the same through a config, plus n_linear and the linears' widths

Third-party modules that are not installed here are replaced by the inert stand-ins of make_reference_goldens.py for
the IMPORT only.  The committed JSON is data (inputs and recorded results); no reference source is copied.

Run:  python tests/golden/make_conv2d_goldens.py
"""
import json
import os
import sys

from torch import nn

from make_reference_goldens import REF, _stub_modules

HERE = os.path.dirname(os.path.abspath(__file__))

SIZE = [14, 11]
C1 = dict(size_factor=3, pad_factor=1, stride_factor=1, dil_factor=1)         # config/psd_c1_dense.json

BLOCKS = [  # (nin, nout, n, keyword arguments); size = [14, 11, nin]
    (300, 64, 3, C1),                                                          # the C1 config
    (20, 6, 3, dict(pad_factor=1.)),                                           # 3 x 3 then clamped 2 x 2 kernels
    (20, 5, 3, dict()),                                                        # pad_factor 0: the map shrinks
    (20, 6, 3, dict(size_factor=3, pad_factor=1., stride_factor=2.)),          # stride 2 at the last layer
    (16, 4, 4, dict(size_factor=3, pad_factor=1., stride_factor=3.)),          # strides 1 1 2 3
    (20, 6, 2, dict(size_factor=3, pad_factor=1., dil_factor=2.)),             # padding from dil_factor, not the dilation
    (20, 6, 3, dict(size_factor=3, pad_factor=1., pointwise_factor=0.5)),      # pointwise first layer, decay from i - 1
    (300, 158, 2, dict(size_factor=3, pad_factor=1., pointwise_factor=0.34)),  # 300 -> 252 -> 158
    (20, 6, 3, dict(size_factor=1)),                                           # every kernel clamped to 2
    (20, 6, 3, dict(size_factor=5, pad_factor=1.)),                            # 5 3 2
    (12, 6, 3, dict(size_factor=3, pad_factor=1., expansion_factor=1.5, n_expansion=1)),     # expansion then contraction
    (12, 6, 4, dict(size_factor=3, pad_factor=1., expansion_factor=2., n_expansion=2, pointwise_factor=0.25)),
    (21, 1, 2, dict(size_factor=3, pad_factor=1.)),                            # one channel out
    (20, 6, 2, dict(size_factor=3, pad_factor=1., dropout=0.3)),               # Dropout modules
    (20, 6, 2, dict(size_factor=3, pad_factor=1., trainable_weights=True)),    # conv bias
    (20, 6, 1, dict()),                                                        # n == 1: ZeroDivisionError
    (20, 6, 2, dict(n_expansion=2)),                                           # ValueError ("< n")
    (20, 6, 2, dict(n_expansion=1, pointwise_factor=0.5)),                     # ValueError ("< n - 1")
]

NETS = [  # (n_samples, n_type, hparams or None)
    (150, 2, {"n_conv": 3, "n_lin": 2, "out_planes": 64, "conv_params": C1}),
    (10, 2, {"n_conv": 3, "n_lin": 2, "out_planes": 64, "conv_params": C1}),                  # the tests' shrunk C1
    (10, 3, {"n_conv": 2, "n_lin": 1, "out_planes": 4}),                                      # no conv_params
    (10, 2, {"n_conv": 3, "n_lin": 3, "out_planes": 5,
             "conv_params": dict(size_factor=3, pad_factor=1., stride_factor=2., pointwise_factor=0.5, dropout=0.2)}),
    (10, 2, {"n_conv": 2, "n_lin": 2, "out_planes": 6,
             "conv_params": dict(size_factor=3, pad_factor=1., dil_factor=2., trainable_weights=True)}),
    (10, 2, {"n_conv": 1, "n_lin": 2, "out_planes": 6}),                                      # ZeroDivisionError
    (10, 2, {"n_conv": 2, "n_lin": 2, "out_planes": 6, "conv_params": dict(n_expansion=2)}),  # ValueError
    (10, 2, {"n_conv": 2, "out_planes": 6}),                                                  # n_lin missing
    (10, 2, {"n_lin": 2, "out_planes": 6}),                                                   # n_conv missing
    (10, 2, None),                                                                            # no hparams at all
]


def _state(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def _block_record(block):
    convs = [m for m in block.model if isinstance(m, nn.Conv2d)]
    return dict(nframes=[convs[0].in_channels] + [c.out_channels for c in convs],
                layers=[[c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]] for c in convs],
                square=all(c.kernel_size[0] == c.kernel_size[1] and c.stride[0] == c.stride[1]
                           and c.padding[0] == c.padding[1] and c.dilation[0] == c.dilation[1] for c in convs),
                bias=[c.bias is not None for c in convs], out_size=list(block.out_size),
                modules=[type(m).__name__ for m in block.model],
                dropout=[m.p for m in block.model if isinstance(m, nn.Dropout)], state=_state(block))


def _attempt(build):
    try:
        return build(), None
    except Exception as e:             # noqa: BLE001  -- the exception's type is the recorded result
        return None, type(e).__name__


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    from src.models.ConvBlocks import Conv2DBlock
    from src.models.DenseConvNet import DenseConvNet
    from src.utils.util import DictionaryUtility

    def config(n_samples, n_type, hparams):
        net = {"imports": ["torch.nn"]}
        if hparams is not None:
            net["hparams"] = hparams
        return DictionaryUtility.to_object({"system_config": {"n_samples": n_samples, "n_type": n_type},
                                            "net_config": net})
    out = {"blocks": [], "nets": []}
    for nin, nout, n, kw in BLOCKS:
        block, err = _attempt(lambda: Conv2DBlock(nin, nout, n, SIZE + [nin], **kw))
        rec = dict(nin=nin, nout=nout, n=n, size=SIZE + [nin], kwargs=kw, raises=err)
        if block is not None:
            rec.update(_block_record(block))
        out["blocks"].append(rec)
    for n_samples, n_type, hp in NETS:
        net, err = _attempt(lambda: DenseConvNet(config(n_samples, n_type, hp)))
        rec = dict(n_samples=n_samples, n_type=n_type, hparams=hp, raises=err)
        if net is not None:
            rec.update(block=_block_record(net.model), n_linear=int(net.n_linear),
                       linears=[[m.in_features, m.out_features] for m in net.linear],
                       state=_state(net))
        out["nets"].append(rec)
    path = os.path.join(HERE, "conv2d_plans.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, {k: len(v) for k, v in out.items()},
          [r["raises"] for r in out["blocks"]], [r["raises"] for r in out["nets"]])


if __name__ == "__main__":
    main()
