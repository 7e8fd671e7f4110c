"""``Conv1DNet``: mirror of the reference's dense 1-D conv stack (src/models/ConvBlocks.py:176-217), the front end of
ConvWaveformNet: ``num_expand + num_contract`` layers of ``nn.Conv1d(stride, zero padding, bias)`` -> ``nn.BatchNorm1d``
-> ``nn.ReLU`` whose channel counts rise then fall and whose kernel, stride and padding follow decaying factors
(``conv1d_plan``, quirks included).  Same module tree as the reference (``network.{3i}`` the conv, ``network.{3i+1}`` the
BatchNorm), so parameters, buffers, initialisation and checkpoints are the reference's.

With ``fused=True`` a GPU call inside wfs_conv1d_ok's bounds runs the WHOLE stack as one FusedConv1dStackFunction on
the kernels of csrc/conv1d.hip (include/wfsparse.h, wfs_conv1d_fwd / wfs_conv1d_bwd): layers + 1 launches forward,
layers + 2 backward, the batch statistics, the running statistics and ``num_batches_tracked`` on the device.  The
modules' tensors are read through their names at every call, so ``module.to("cuda")`` and FlatGradAllReducer (which
re-points ``p.data`` into one flat buffer) leave them the tensors the kernels read, and the gradients land in the flat
gradient buffer's slots (spconv/functional.grad_like).  Everything else -- CPU tensors, plans out of bounds, parameters
that are not contiguous fp32, a BatchNorm with ``momentum=None`` or without affine parameters or running statistics,
the flag off -- is the torch composition ``self.network(x)``.

``n_valid`` (a device int64 count, from a captured step's capacity-padded batch): rows at or beyond it take no part in
the batch statistics or in any gradient and come out as zeros.  Only the kernels can honour it without a host
read-back: a call that carries one and cannot run on them raises.
"""
import ctypes
from math import ceil

import torch
from torch import nn
from torch.autograd import Function

from .. import _lib
from . import _fused
from .blocks import conv_output_size

CONV1D_CALLS = [0]      # forward calls that ran on the conv-stack kernels (tests and tools read it)


def conv1d_plan(length, num_channels, out_size, num_expand, num_contract, expand_factor, size_factor=3, pad_factor=1,
                stride_factor=0, min_kernel=2):
    """(planes, layers, out_size) of the reference's Conv1DNet: ``planes`` the channel counts [c0 .. cn] (the last one
    forced to ``out_size``), ``layers`` one (fs, st, pd, L_out) per layer, ``out_size`` = [L_out, C_out] of the stack.
    Kernel and padding shrink with a factor that decays linearly from 1 (first layer) to 0 (last), the stride grows
    linearly up to ``stride_factor``; a single layer takes the factors as they are; strides below 1 become 1, kernels
    below ``min_kernel`` become ``min_kernel``; ``round`` is Python's (half to even); lengths are ``int()`` of a true
    division (blocks.conv_output_size)."""
    planes = [num_channels]
    if num_expand > 0:
        step = float((planes[0] * expand_factor - planes[0]) / num_expand)
        planes += [int(round(planes[0] + step * (i + 1))) for i in range(num_expand)]
    step = float((planes[-1] - out_size) / num_contract)
    top = planes[-1]
    planes += [int(round(top - step * (i + 1))) for i in range(num_contract)]
    planes[-1] = out_size
    size = [length, num_channels]
    n = num_expand + num_contract
    layers = []
    for i in range(n):
        if n > 1:
            decay = 1. - i / (n - 1)
            st = int(round(stride_factor * i / (n - 1)))
        else:
            decay = 1.
            st = int(stride_factor)
        st = max(st, 1)
        fs = max(int(ceil(size_factor * decay)), min_kernel)
        pd = int(round(pad_factor * ((fs - 1) / 2.) * decay))
        size = conv_output_size(size, planes[i + 1], fs, st, pd, 1, 1)
        layers.append((fs, st, pd, size[0]))
    return planes, layers, size


class FusedConv1dStackFunction(Function):
    """[N, c0, L] through the whole stack on the kernels.  ``plan`` = (c0, channels, fs, st, pd) as tuples; ``bn`` =
    (momentum, eps) tuples per layer; ``n_valid`` a device int64 count or None; ``params``: per layer its (conv.weight,
    conv.bias, bn.weight, bn.bias, running_mean, running_var, num_batches_tracked).  The backward writes every parameter
    gradient into the gradient slots (spconv/functional.grad_like)."""

    @staticmethod
    def forward(ctx, x, plan, bn, training, n_valid, cache, *params):
        lib = _lib.load()
        x = x.contiguous()
        c0, channels, fs, st, pd = plan
        N, _c, L = x.shape
        n = len(channels)
        arrays = tuple(_lib.i32_array(v) for v in (channels, fs, st, pd))
        rows = _fused.fwd_rows(params, 7)
        tab = _fused.ptr_table(cache, ("cfwd",) + tuple(map(tuple, rows)), rows, x.device)
        saved = torch.empty((int(lib.wfs_conv1d_saved_floats(N, L, c0, *arrays, n)),), dtype=torch.float32, device=x.device)
        lout = L
        for f, s, p in zip(fs, st, pd):
            lout = (lout + 2 * p - f) // s + 1
        y = torch.empty((N, channels[-1], lout), dtype=x.dtype, device=x.device)
        momentum, eps = ((ctypes.c_float * n)(*[float(v) for v in vals]) for vals in bn)
        _lib.check(lib.wfs_conv1d_fwd(_lib.ptr(x), N, L, c0, *arrays, n, _lib.ptr(tab), momentum, eps, int(training),
                                      _lib.ptr(saved), _lib.ptr(y), _lib.dtype_code(x), _lib.ptr(n_valid),
                                      _lib.stream_ptr()))
        CONV1D_CALLS[0] += 1
        ctx.save_for_backward(x, saved)
        ctx.params, ctx.plan, ctx.training = params, plan, int(training)
        ctx.n_valid, ctx.cache = n_valid, cache
        return y

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        x, saved = ctx.saved_tensors
        c0, channels, fs, st, pd = ctx.plan
        first = FusedConv1dStackFunction.first_param
        N, _c, L = x.shape
        n = len(channels)
        arrays = tuple(_lib.i32_array(v) for v in (channels, fs, st, pd))
        dy = _fused.as_grad(grad_output, x.dtype)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        rows, grads = _fused.bwd_rows(ctx, ctx.params, 7, first)
        tab = _fused.ptr_table(ctx.cache, ("cbwd",) + tuple(map(tuple, rows)), rows, x.device)
        ws = torch.empty((int(lib.wfs_conv1d_bwd_workspace_floats(N, L, c0, *arrays, n)),), dtype=torch.float32,
                         device=x.device)
        _lib.check(lib.wfs_conv1d_bwd(_lib.ptr(x), _lib.ptr(dy), N, L, c0, *arrays, n, _lib.ptr(tab), ctx.training,
                                      _lib.ptr(saved), _lib.ptr(dx), _lib.ptr(ws), _lib.dtype_code(x),
                                      _lib.ptr(ctx.n_valid), _lib.stream_ptr()))
        return (dx,) + (None,) * (first - 1) + tuple(grads)


FusedConv1dStackFunction.first_param = _fused.first_param(FusedConv1dStackFunction)


class Conv1DNet(nn.Module):
    def __init__(self, length, num_channels, out_size, num_expand, num_contract, expand_factor, size_factor=3,
                 pad_factor=1, stride_factor=0, min_kernel=2, fused=False):
        super().__init__()
        self.planes, self.layers, self.out_size = conv1d_plan(length, num_channels, out_size, num_expand, num_contract,
                                                              expand_factor, size_factor, pad_factor, stride_factor,
                                                              min_kernel)
        mods = []
        for i, (fs, st, pd, _l) in enumerate(self.layers):
            mods += [nn.Conv1d(self.planes[i], self.planes[i + 1], fs, stride=st, padding=pd),
                     nn.BatchNorm1d(self.planes[i + 1]), nn.ReLU()]
        self.network = nn.Sequential(*mods)
        # fused=True: the stack runs on the conv-stack kernels (wfs_conv1d_*) where they take it
        self.fused = bool(fused)

    def _stack(self):
        """[(conv, bn)] of the stack as it stands (a loaded or edited ``network`` included)."""
        mods = list(self.network)
        return [(mods[i], mods[i + 1]) for i in range(0, len(mods) - 2, 3)]

    def _plan(self):
        """(c0, channels, fs, st, pd) read off the modules, or None when a module is not what the kernels compute."""
        mods = list(self.network)
        if not mods or len(mods) % 3:
            return None
        channels, fs, st, pd = [], [], [], []
        for i in range(0, len(mods), 3):
            conv, bn, act = mods[i: i + 3]
            if not (type(conv) is nn.Conv1d and type(bn) is nn.BatchNorm1d and type(act) is nn.ReLU):
                return None
            if (conv.dilation != (1,) or conv.groups != 1 or conv.padding_mode != "zeros"
                    or not isinstance(conv.padding, tuple) or (channels and conv.in_channels != channels[-1])):
                return None
            if (not bn.affine or not bn.track_running_stats or bn.momentum is None or bn.running_mean is None
                    or bn.num_features != conv.out_channels):
                return None
            channels.append(conv.out_channels)
            fs.append(conv.kernel_size[0])
            st.append(conv.stride[0])
            pd.append(conv.padding[0])
        return mods[0].in_channels, tuple(channels), tuple(fs), tuple(st), tuple(pd)

    def _kernel_params(self):
        """The layers' seven tensors in the kernels' order -- None unless they are what the kernels read: contiguous
        fp32 on the GPU (the batch counter int64)."""
        groups = []
        for conv, bn in self._stack():
            nbt = bn.num_batches_tracked
            if nbt is None or nbt.dtype != torch.int64 or not nbt.is_cuda:
                return None
            floats = _fused.kernel_params([(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)])
            if floats is None:
                return None
            groups += floats + [nbt]
        return groups

    def _can_fuse(self, x):
        if not (self.fused and x.is_cuda and x.dim() == 3 and x.shape[0] > 0
                and x.dtype in (torch.float32, torch.bfloat16, torch.float16)):
            return None
        plan = self._plan()
        if plan is None or x.shape[1] != plan[0]:
            return None
        arrays = [_lib.i32_array(v) for v in plan[1:]]
        if _lib.load().wfs_conv1d_ok(plan[0], *arrays, len(plan[1]), int(x.shape[2]), _lib.dtype_code(x)) != _lib.WFS_OK:
            return None
        params = self._kernel_params()
        if params is None:
            return None
        return plan, params

    def forward(self, x, n_valid=None):
        go = self._can_fuse(x)
        if go is None:
            if n_valid is not None:
                raise RuntimeError("Conv1DNet: a valid-row count needs the conv-stack kernels (BatchNorm statistics over "
                                   "the valid rows only), and they do not take this call")
            return self.network(x)
        plan, params = go
        bns = [bn for _conv, bn in self._stack()]
        bn_args = (tuple(bn.momentum for bn in bns), tuple(bn.eps for bn in bns))
        return FusedConv1dStackFunction.apply(x, plan, bn_args, self.training, n_valid, _fused.ptr_cache(self), *params)
