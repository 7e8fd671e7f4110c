"""Generates tests/golden/lit_module_layout.json: for one config per Lightning-module mirror (tests/lit_layout_cases.py)
the ordered ``state_dict()`` keys with shapes and dtypes, the ordered top-level ``named_children()`` names and the buffer
names.  It was written at the commit BEFORE the six modules were put on ``psd/litbase.LitBase``, so the file pins the
layout checkpoints were saved with; run it again only to add a case, and then at a commit whose layout is trusted.

Run (after ``make -C waveformml_amd/csrc``):  python tests/golden/make_lit_module_layout.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lit_layout_cases as lc  # noqa: E402


def main():
    out = {name: lc.layout(lc.build(name)) for name in lc.CASES}
    with open(os.path.join(HERE, "lit_module_layout.json"), "w") as f:
        json.dump(out, f, indent=0)
    print({k: len(v["state_dict"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
