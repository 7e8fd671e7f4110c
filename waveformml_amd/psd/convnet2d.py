"""``Conv2DBlock``: mirror of the reference's dense 2-D conv stack (src/models/ConvBlocks.py:220-289), the body of
DenseConvNet: ``n`` layers of ``nn.Conv2d(stride, zero padding, dilation, bias = trainable_weights)`` -> ``nn.BatchNorm2d``
-> ``nn.ReLU`` (-> ``nn.Dropout`` when ``dropout`` is truthy) whose channel counts follow the expansion / contraction
frames of the sparse blocks and whose kernel, stride, padding and dilation follow ``conv2d_plan`` (quirks included).  Same
module tree as the reference (``model.{k}``), so parameters, buffers, initialisation and checkpoints are the reference's.

With ``fused=True`` a GPU call inside wfs_conv2d_ok's bounds runs the WHOLE stack as one FusedConv2dStackFunction on
the kernels of csrc/conv2d.hip (include/wfsparse.h, wfs_conv2d_fwd / wfs_conv2d_bwd): the three products of every layer
as implicit GEMMs on the matrix cores, the batch statistics, the running statistics and ``num_batches_tracked`` on the
device, the dropout masks from a seed in device memory.  The kernels read the map channels-last (what ``densify_rows``
writes; any other input is converted) and write the output channels-first, the order the reference flattens.  The
modules' tensors are read through their names at every call (psd/convnet.py).  Everything else -- CPU tensors, plans
out of bounds, parameters that are not contiguous fp32, a BatchNorm with ``momentum=None`` or without affine parameters
or running statistics, the flag off -- is the torch composition ``self.model(x)``.
"""
import ctypes
from math import ceil

import torch
from torch import nn
from torch.autograd import Function

from .. import _lib
from . import _fused
from .blocks import conv_output_size, expansion_contraction_frames

CONV2D_CALLS = [0]      # forward calls that ran on the conv-stack kernels (tests and tools read it)


def conv2d_plan(nin, nout, n, size, size_factor=3, pad_factor=0., stride_factor=1.0, dil_factor=1., expansion_factor=1.,
                n_expansion=0, pointwise_factor=0.):
    """(nframes, [(fs, st, pd, dil)], out_size) of the reference's Conv2DBlock; ``size`` = [spatial..., channels].  The
    kernel shrinks with a factor that decays linearly from 1 to 0 over the layers (from the SECOND layer on when the
    first is the pointwise one: the decay uses i - 1) and is clamped to >= 2; the stride grows linearly up to
    ``stride_factor`` (``n == 1`` divides by zero there, as the reference does); the dilation is dil_factor ** i; the
    padding scales with ``dil_factor`` itself, not with the layer's dilation; ``round`` is Python's (half to even)."""
    pw = pointwise_factor > 0
    nframes = expansion_contraction_frames(nin, nout, n, pointwise_factor, expansion_factor, n_expansion)
    ndim = len(size) - 1
    out_size = size
    layers = []
    for i in range(n):
        if n > 1:
            decay = 1. - (i - 1) / (n - 1) if pw else 1. - i / (n - 1)
        else:
            decay = 1.
        fs = max(int(ceil(size_factor * decay)), 2)
        st = max(int(round(stride_factor * i / (n - 1))), 1)
        dil = int(round(dil_factor ** i))
        pd = int(round(pad_factor * ((fs - 1) / 2.) * dil_factor * decay))
        if i == 0 and pw:
            pd, fs, dil, st = 0, 1, 1, 1
        layers.append((fs, st, pd, dil))
        out_size = conv_output_size(out_size, nframes[i + 1], fs, st, pd, dil, ndim)
    return nframes, layers, out_size


def densify_rows(feats, coords, batch_size, height, width, n_valid=None):
    """Rows [n, C] at coords [n, 3] = (x, y, event) -> the dense map as a [B, C, H, W] tensor in channels_last memory
    (the kernels' input layout) in ONE launch (wfs_densify_rows): zeros where no row lands, rows at or beyond
    ``n_valid`` (a device int64 count) and rows with coordinates outside the map skipped, equal coordinates summed in
    row order.  Equals ``sparse_coo_tensor(...).to_dense().permute(0, 3, 1, 2)``.  No gradient: the rows are inputs."""
    lib = _lib.load()
    feats = feats.detach().contiguous()
    if coords.dtype != torch.int32 or not coords.is_contiguous():
        coords = coords.to(torch.int32).contiguous()
    n, C = feats.shape
    out = torch.empty((batch_size, height, width, C), dtype=feats.dtype, device=feats.device)
    _lib.check(lib.wfs_densify_rows(_lib.ptr(feats), _lib.ptr(coords), n, C, batch_size, height, width,
                                    _lib.ptr(n_valid), _lib.ptr(out), _lib.dtype_code(feats), _lib.stream_ptr()))
    return out.permute(0, 3, 1, 2)


def _f32_array(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


class FusedConv2dStackFunction(Function):
    """[B, c0, H, W] through the whole stack on the kernels.  ``plan`` = (c0, channels, fs, st, pd, dil) as tuples;
    ``bn`` = (momentum, eps, dropout p) tuples per layer; ``seed`` a device int64 tensor (None: no dropout);
    ``params``: per layer its (conv.weight, conv.bias or None, bn.weight, bn.bias, running_mean, running_var,
    num_batches_tracked).  The backward writes every parameter gradient into the gradient slots
    (spconv/functional.grad_like)."""

    @staticmethod
    def forward(ctx, x, plan, bn, training, seed, cache, *params):
        lib = _lib.load()
        x = x.permute(0, 2, 3, 1).contiguous()            # [B, H, W, C]: no copy of a channels_last tensor
        c0, channels, fs, st, pd, dil = plan
        B, H, W, _c = x.shape
        n = len(channels)
        arrays = tuple(_lib.i32_array(v) for v in (channels, fs, st, pd, dil))
        code = _lib.dtype_code(x)
        rows = _fused.fwd_rows(params, 7)
        tab = _fused.ptr_table(cache, ("c2fwd",) + tuple(map(tuple, rows)), rows, x.device)
        saved = torch.empty((int(lib.wfs_conv2d_saved_floats(B, H, W, c0, *arrays, n, code)),), dtype=torch.float32,
                            device=x.device)
        ho, wo = H, W
        for f, s, p, d in zip(fs, st, pd, dil):
            ho = (ho + 2 * p - d * (f - 1) - 1) // s + 1
            wo = (wo + 2 * p - d * (f - 1) - 1) // s + 1
        y = torch.empty((B, channels[-1], ho, wo), dtype=x.dtype, device=x.device)
        momentum, eps, drop = (_f32_array(v) for v in bn)
        _lib.check(lib.wfs_conv2d_fwd(_lib.ptr(x), B, H, W, c0, *arrays, n, _lib.ptr(tab), momentum, eps, drop,
                                      _lib.ptr(seed), int(training), _lib.ptr(saved), _lib.ptr(y), code,
                                      _lib.stream_ptr()))
        CONV2D_CALLS[0] += 1
        ctx.save_for_backward(x, saved)
        ctx.params, ctx.plan, ctx.training = params, plan, int(training)
        ctx.seed, ctx.cache, ctx.drop = seed, cache, bn[2]
        return y

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        x, saved = ctx.saved_tensors
        c0, channels, fs, st, pd, dil = ctx.plan
        first = FusedConv2dStackFunction.first_param
        B, H, W, _c = x.shape
        n = len(channels)
        arrays = tuple(_lib.i32_array(v) for v in (channels, fs, st, pd, dil))
        code = _lib.dtype_code(x)
        dy = _fused.as_grad(grad_output, x.dtype)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        rows, grads = _fused.bwd_rows(ctx, ctx.params, 7, first)
        tab = _fused.ptr_table(ctx.cache, ("c2bwd",) + tuple(map(tuple, rows)), rows, x.device)
        ws = torch.empty((int(lib.wfs_conv2d_bwd_workspace_floats(B, H, W, c0, *arrays, n, code)),), dtype=torch.float32,
                         device=x.device)
        _lib.check(lib.wfs_conv2d_bwd(_lib.ptr(x), _lib.ptr(dy), B, H, W, c0, *arrays, n, _lib.ptr(tab),
                                      _f32_array(ctx.drop), _lib.ptr(ctx.seed), ctx.training, _lib.ptr(saved),
                                      _lib.ptr(dx), _lib.ptr(ws), code, _lib.stream_ptr()))
        if dx is not None:
            dx = dx.permute(0, 3, 1, 2)                   # channels_last memory, as the input's
        return (dx,) + (None,) * (first - 1) + tuple(grads)


FusedConv2dStackFunction.first_param = _fused.first_param(FusedConv2dStackFunction)


class Conv2DBlock(nn.Module):
    def __init__(self, nin, nout, n, size, size_factor=3, pad_factor=0., stride_factor=1.0, dil_factor=1.,
                 expansion_factor=1., n_expansion=0, pointwise_factor=0., dropout=None, trainable_weights=False,
                 fused=False):
        super().__init__()
        self.dropout = dropout
        self.ndim = len(size) - 1
        self.nframes, self.layers, self.out_size = conv2d_plan(nin, nout, n, size, size_factor, pad_factor,
                                                               stride_factor, dil_factor, expansion_factor, n_expansion,
                                                               pointwise_factor)
        self.alg = []
        for i, (fs, st, pd, dil) in enumerate(self.layers):
            # `trainable_weights` is the conv's bias flag, as in the reference
            self.alg.append(nn.Conv2d(self.nframes[i], self.nframes[i + 1], (fs, fs), (st, st), pd, (dil, dil), 1,
                                      trainable_weights))
            self.alg.append(nn.BatchNorm2d(self.nframes[i + 1]))
            self.alg.append(nn.ReLU())
            if self.dropout:
                self.alg.append(nn.Dropout(self.dropout))
        self.model = nn.Sequential(*self.alg)
        # fused=True: the stack runs on the conv-stack kernels (wfs_conv2d_*) where they take it
        self.fused = bool(fused)

    def _plan(self):
        """((c0, channels, fs, st, pd, dil), [(conv, bn, dropout p)]) read off the modules as they stand (a loaded or
        edited ``model`` included), or None when a module is not what the kernels compute."""
        mods = list(self.model)
        channels, fs, st, pd, dil, stack = [], [], [], [], [], []
        i = 0
        while i < len(mods):
            if i + 3 > len(mods):
                return None
            conv, bn, act = mods[i: i + 3]
            i += 3
            p = 0.
            if i < len(mods) and type(mods[i]) is nn.Dropout:
                p = float(mods[i].p)
                i += 1
            if not (type(conv) is nn.Conv2d and type(bn) is nn.BatchNorm2d and type(act) is nn.ReLU):
                return None
            square = all(v[0] == v[1] for v in (conv.kernel_size, conv.stride, conv.dilation)
                         ) and isinstance(conv.padding, tuple) and conv.padding[0] == conv.padding[1]
            if (not square or conv.groups != 1 or conv.padding_mode != "zeros"
                    or (channels and conv.in_channels != channels[-1])):
                return None
            if (not bn.affine or not bn.track_running_stats or bn.momentum is None or bn.running_mean is None
                    or bn.num_features != conv.out_channels or not 0. <= p < 1.):
                return None
            channels.append(conv.out_channels)
            fs.append(conv.kernel_size[0])
            st.append(conv.stride[0])
            pd.append(conv.padding[0])
            dil.append(conv.dilation[0])
            stack.append((conv, bn, p))
        if not stack:
            return None
        return (stack[0][0].in_channels, tuple(channels), tuple(fs), tuple(st), tuple(pd), tuple(dil)), stack

    @staticmethod
    def _kernel_params(stack):
        """The layers' seven tensors in the kernels' order -- None unless they are what the kernels read: contiguous
        fp32 on the GPU (the batch counter int64)."""
        groups = []
        for conv, bn, _p in stack:
            nbt = bn.num_batches_tracked
            if nbt is None or nbt.dtype != torch.int64 or not nbt.is_cuda:
                return None
            floats = _fused.kernel_params([(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)])
            if floats is None:
                return None
            groups += floats + [nbt]
        return groups

    def can_fuse(self, x):
        """(plan, stack, params) when this call runs on the kernels, else None."""
        if not (self.fused and x.is_cuda and x.dim() == 4 and x.shape[0] > 0
                and x.dtype in (torch.float32, torch.bfloat16, torch.float16)):
            return None
        got = self._plan()
        if got is None or x.shape[1] != got[0][0]:
            return None
        plan, stack = got
        arrays = [_lib.i32_array(v) for v in plan[1:]]
        if _lib.load().wfs_conv2d_ok(plan[0], *arrays, len(plan[1]), int(x.shape[0]), int(x.shape[2]), int(x.shape[3]),
                                     int(self.training), _lib.dtype_code(x)) != _lib.WFS_OK:
            return None
        params = self._kernel_params(stack)
        if params is None:
            return None
        return plan, stack, params

    def forward(self, x, seed=None):
        """``seed``: a device int64 tensor the dropout masks are derived from (default: drawn from torch's generator at
        every training call; only the kernels take one)."""
        go = self.can_fuse(x)
        if go is None:
            return self.model(x)
        plan, stack, params = go
        drop = tuple(p if self.training else 0. for _c, _b, p in stack)
        if seed is None and any(p > 0 for p in drop):
            seed = _fused.draw_seed(x.device)
        bn_args = (tuple(bn.momentum for _c, bn, _p in stack), tuple(bn.eps for _c, bn, _p in stack), drop)
        return FusedConv2dStackFunction.apply(x, plan, bn_args, self.training, seed, _fused.ptr_cache(self), *params)
