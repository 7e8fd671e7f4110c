"""Generates tests/golden/feature_net_schedules.json by importing the REFERENCE's ``ExtractedFeatureConv`` builder
(/root/reference/src/models/SPConvBlocks.py, this container only) with `spconv` replaced by the recorder of
make_reference_goldens.py (its constructors only remember their arguments).  The JSON is data: constructor arguments in,
the layer list (class, positional arguments, keyword arguments) and ``out_size`` out, or the name of the exception the
builder raises; no reference source is copied.

Cases: n = 2, 3 and 5; with and without dropout; stride_factor 1 and 2; pad_factor 0 and 1; ``trainable_weights`` (the
8th positional argument of the conv, which lands in ``bias``); and n = 1, which raises.

Run:  python tests/golden/make_feature_net_goldens.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_block_goldens as blocks     # noqa: E402
import make_reference_goldens as base   # noqa: E402


def main():
    base._stub_modules()
    sys.path.insert(0, base.REF)
    from src.models.SPConvBlocks import ExtractedFeatureConv
    out = []
    for n in (2, 3, 5, 1):
        for nin, nout in ((7, 16), (7, 3), (12, 40)):
            for kw in (dict(), dict(dropout=0.2), dict(stride_factor=2), dict(pad_factor=1.0),
                       dict(pad_factor=1.0, stride_factor=2, size_factor=5, expansion_factor=4.5, dropout=0.1),
                       dict(pad_factor=0.5, expansion_factor=6.0), dict(trainable_weights=True, dil_factor=2),
                       dict(size_factor=1, expansion_factor=2.0)):
                args = dict(nin=nin, nout=nout, n=n, size=[14, 11, nin], **kw)
                blk, err = blocks.attempt(lambda: ExtractedFeatureConv(**dict(args, size=list(args["size"]))))
                rec = dict(args=args, error=err)
                if blk is not None:
                    rec.update(layers=blocks.layers_of(blk.alg), out_size=[int(v) for v in blk.out_size])
                out.append(rec)
    assert all(r["error"] == "AssertionError" for r in out if r["args"]["n"] == 1)
    with open(os.path.join(HERE, "feature_net_schedules.json"), "w") as f:
        json.dump(out, f)
    print(len(out), "cases,", sum(1 for r in out if r["error"]), "raise")


if __name__ == "__main__":
    main()
