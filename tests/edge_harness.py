"""Shared by the GPU edge modules of the dense stack kernels (tests/test_gpu_dense_edges.py,
tests/test_gpu_conv1d_edges.py): the poisoned buffer with guarded trailing elements, the bit-for-bit comparison and the
error table printed when a module ends.  (Not a test module: nothing here is collected.)
"""
import os
import time

import pytest
import torch

from waveform_cases import DEV

SENT = -768.0                      # exactly representable in bf16 and fp16
PAD = 5                            # trailing elements behind every buffer
NAN = float("nan")


class Buf:
    """`n` elements filled with `fill` and PAD trailing elements filled with `tail`; `.t` is the buffer itself."""

    def __init__(self, shape, dtype, fill, tail=None):
        n = 1
        for s in shape:
            n *= s
        assert n > 0
        self.tail = fill if tail is None else tail
        self.flat = torch.full((n + PAD,), fill, dtype=dtype, device=DEV)
        self.flat[n:] = self.tail
        self.t = self.flat[:n].view(shape)

    def check_tail(self, what):
        tail = self.flat[self.t.numel():].float()
        kept = torch.isnan(tail) if self.tail != self.tail else tail == self.tail
        assert bool(kept.all()), "%s: an element behind the buffer was written" % what


def bits_equal(a, b, names):
    for n in names:
        assert torch.equal(a[n].contiguous().view(torch.uint8), b[n].contiguous().view(torch.uint8)), n


def error_report(worst, groups, env, key_format="%-14s %-5s %-5s"):
    """A module-scoped autouse fixture: when the module ends, print the worst error / bar of every key of `worst`
    ({key tuple: {group: ratio}}) and write the table to the file the environment variable `env` names, if set."""

    @pytest.fixture(scope="module", autouse=True)
    def _error_report():
        t0 = time.time()
        yield
        lines = ["# worst |got - want| / (bar x scale) per tensor group (<= 1 passes): case, row type, mode, "
                 + ", ".join(groups)]
        for key, w in sorted(worst.items()):
            lines.append((key_format + " %s") % (tuple(key) + (" ".join("%.4f" % w[g] if g in w else "-" for g in groups),)))
        text = "\n".join(lines)
        print("\n" + text + "\n# module wall time %.1f s" % (time.time() - t0))
        path = os.environ.get(env)
        if path:
            with open(path, "w") as f:
                f.write(text + "\n")

    return _error_report
