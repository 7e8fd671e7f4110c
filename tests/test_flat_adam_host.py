"""Host side of the Adam / AdamW update (no device): the C ABI declaration and its binding, the captured step's
decision which optimizers step inside the graph (psd/graph.steps_in_graph), torch's step for tensors the HIP path
does not take."""
import os
import re

import numpy as np
import torch

from waveformml_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adam_step_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "wfsparse.h")) as f:
        header = f.read()
    m = re.search(r"\bint wfs_adam_step\(([^;]*)\);", header)
    assert m is not None
    restype, argtypes = _lib.SIGNATURES["wfs_adam_step"]
    assert len(m.group(1).split(",")) == len(argtypes) == 13
    assert _lib.WFS_ABI_VERSION == 6          # a new symbol is a compatible change


def test_which_optimizers_step_inside_the_graph():
    from waveformml_amd.psd.graph import steps_in_graph
    from waveformml_amd.psd.optim import FlatAdam, FlatAdamW, FlatSGD
    p = [torch.nn.Parameter(torch.zeros(8))]
    assert steps_in_graph(FlatSGD(p, lr=0.1, momentum=0.9, nesterov=True))
    assert steps_in_graph(FlatAdam(p, lr=1e-3))
    assert steps_in_graph(FlatAdamW(p, lr=1e-3))
    assert steps_in_graph(torch.optim.SGD(p, lr=0.1, momentum=0.9))
    assert not steps_in_graph(torch.optim.Adam(p, lr=1e-3))
    assert not steps_in_graph(torch.optim.AdamW(p, lr=1e-3))
    assert not steps_in_graph(torch.optim.RMSprop(p, lr=1e-3))


def test_flat_adam_on_cpu_tensors_is_torch_adam():
    """A CPU tensor is not the HIP path's: FlatAdam / FlatAdamW step exactly as torch does."""
    from waveformml_amd.psd.optim import FlatAdam, FlatAdamW
    rng = np.random.default_rng(3)
    w0 = rng.standard_normal(1001).astype(np.float32)
    for ref_cls, cls in ((torch.optim.Adam, FlatAdam), (torch.optim.AdamW, FlatAdamW)):
        pr, pf = (torch.nn.Parameter(torch.from_numpy(w0.copy())) for _ in range(2))
        ref, opt = ref_cls([pr], lr=1e-2, weight_decay=1e-2), cls([pf], lr=1e-2, weight_decay=1e-2)
        for _ in range(3):
            g = torch.from_numpy(rng.standard_normal(1001).astype(np.float32))
            pr.grad, pf.grad = g.clone(), g.clone()
            ref.step()
            opt.step()
        assert torch.equal(pr, pf)
        assert float(opt.state[pf]["step"]) == 3.0
