"""What the pointer-table autograd Functions of the waveform front ends share (psd/tcn.py, psd/recurrent.py): the kernels
read a net's parameters, and write their gradients, through a device array of address records -- one record per
convolution / per (layer, direction), ``width`` parameter addresses followed by ``width`` gradient addresses, 0 = absent."""
import inspect

import torch

from ..spconv.functional import as_grad, grad_like          # noqa: F401  (as_grad: used by the front ends through here)


def ptr_table(cache, key, rows, device):
    """Device array of pointer records (int64), cached by the addresses it holds: in a captured step parameters and
    gradient slots never move, so the table is built (one small H2D copy) during the eager warm-up only."""
    tab = cache.get(key)
    if tab is None:
        if len(cache) > 64:
            cache.clear()
        tab = torch.tensor(rows, dtype=torch.int64, device=device)
        cache[key] = tab
    return tab


def ptr_cache(module):
    """The module's cache of pointer tables, made at its first fused call."""
    if not hasattr(module, "_ptr_cache"):
        module._ptr_cache = {}
    return module._ptr_cache


def kernel_params(groups):
    """The groups' tensors in one flat list (None entries kept: an absent bias or weight_g) -- None unless every tensor is
    what the kernels read: contiguous fp32 on the GPU."""
    out = []
    for group in groups:
        for t in group:
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                return None
        out += list(group)
    return out


def draw_seed(device):
    """A fresh 64-bit dropout seed from torch's generator into device memory (reproducible under torch.manual_seed, and
    a captured graph draws a new one per replay); the kernels derive every mask from it."""
    return torch.randint(-2 ** 62, 2 ** 62, (1,), dtype=torch.int64, device=device)


def first_param(function):
    """Where ``*params`` starts among the inputs of ``function.forward(ctx, ..., *params)``: the offset of the
    parameters' entries in ctx.needs_input_grad and of their gradients in backward's return."""
    return list(inspect.signature(function.forward).parameters).index("params") - 1


def _addr(t):
    return t.data_ptr() if t is not None else 0


def fwd_rows(params, width):
    """The forward's records: the parameters' addresses, no gradient slots."""
    return [[_addr(t) for t in params[i: i + width]] + [0] * width for i in range(0, len(params), width)]


def bwd_rows(ctx, params, width, first):
    """The backward's records and the gradients they point to: a slot (spconv/functional.grad_like -- the flat gradient
    buffer's where there is one) for every present parameter whose entry of ctx.needs_input_grad, from ``first`` on, is
    set; None for the others."""
    need = ctx.needs_input_grad[first: first + len(params)]
    grads = [grad_like(p) if (p is not None and nd) else None for p, nd in zip(params, need)]
    rows = [[_addr(t) for t in list(params[i: i + width]) + grads[i: i + width]] for i in range(0, len(params), width)]
    return rows, grads

