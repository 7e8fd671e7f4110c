"""Causal dilated 1-D conv front end (hybrid config C5): mirror of the reference's TemporalConvNet
(src/models/ConvBlocks.py:105-173, itself the locuslab TCN): per level two weight-normed Conv1d with
left padding (k-1)*d chomped on the right, ReLU, dropout, residual; dilation doubles per level.

The reference only ever builds it with ONE channel (``TemporalConvNet(1, [1] * n_dil, ...)``,
src/models/SPConvNet.py:83-92).  In that shape every level is two k-tap causal FIR filters per waveform row, and the
whole net runs as one HIP launch per direction with the row resident in LDS (include/wfsparse.h, wfs_tcn_fwd /
wfs_tcn_bwd; csrc/tcn.hip), dropout included (training mode: masks from a counter-based hash of a seed drawn from torch's
generator -- the same distribution as nn.Dropout, not the same bits).  Same modules, parameters and state_dict as the
torch composition below, which remains the path for everything else (more channels, CPU tensors, rows too long for the
LDS-resident backward).

Any other channel plan -- TemporalWaveformNet's ``TemporalConvNet(1, planes, ...)`` -- runs on the multi-channel kernels
(wfs_tcnc_*, csrc/tcnc.hip) when the module is built with ``fused=True`` (default off: the torch composition, as
before): weight norm in one launch, two launches per level forward, four per level and one for all weight gradients
backward.  Plans outside wfs_tcnc_ok's bounds take the torch composition.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.nn.utils import weight_norm

from .. import _lib
from . import _fused


class _Chomp(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.n = n

    def forward(self, x):
        return x[:, :, :-self.n].contiguous()


class TemporalBlock(nn.Module):
    def __init__(self, n_in, n_out, kernel_size, stride, dilation, padding, dropout=0.2):
        super().__init__()
        layers = []
        self.convs = []
        for cin in (n_in, n_out):
            conv = weight_norm(nn.Conv1d(cin, n_out, kernel_size, stride=stride, padding=padding, dilation=dilation))
            conv.weight.data.normal_(0, 0.01)
            self.convs.append(conv)
            layers += [conv, _Chomp(padding), nn.ReLU()]
            if dropout != 0:
                layers.append(nn.Dropout(dropout))
        self.net = nn.Sequential(*layers)
        self.downsample = nn.Conv1d(n_in, n_out, 1) if n_in != n_out else None
        if self.downsample is not None:
            self.downsample.weight.data.normal_(0, 0.01)
        self.relu = nn.ReLU()
        self.shape = (n_in, n_out, kernel_size, stride, dilation, padding, dropout)

    def forward(self, x):
        res = x if self.downsample is None else self.downsample(x)
        return self.relu(self.net(x) + res)


def _tcn_launch_fwd(x, taps, bias, dropout, seed):
    """wfs_tcn_fwd on contiguous rows [N, L] and effective taps [levels, 2, k] / biases [levels, 2] -> rows [N, L]."""
    N, L = x.shape
    levels, _, k = taps.shape
    y = torch.empty_like(x)
    _lib.check(_lib.load().wfs_tcn_fwd(_lib.ptr(x), N, L, _lib.ptr(taps), _lib.ptr(bias), levels, k, _lib.ptr(y),
                                       _lib.dtype_code(x), float(dropout), _lib.ptr(seed), _lib.stream_ptr()))
    return y


def _tcn_launch_bwd(x, grad_output, taps, bias, dropout, seed):
    """wfs_tcn_bwd -> (dx [N, L], the per-row partial sums [N, levels, 2, k + 1] of d taps and d bias)."""
    N, L = x.shape
    levels, _, k = taps.shape
    dy = _fused.as_grad(grad_output, x.dtype)
    dx = torch.empty_like(x)
    partial = torch.empty((N, levels, 2, k + 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().wfs_tcn_bwd(_lib.ptr(x), _lib.ptr(dy), N, L, _lib.ptr(taps), _lib.ptr(bias), levels, k,
                                       _lib.ptr(dx), _lib.ptr(partial), _lib.dtype_code(x), dropout, _lib.ptr(seed),
                                       _lib.stream_ptr()))
    return dx, partial


class FusedTCNFunction(Function):
    """The two fused kernels on EFFECTIVE taps (what the module's FusedNormedTCNFunction wraps with the weight norm):
    rows [N, L], effective taps [levels, 2, k] and biases [levels, 2] (fp32, on the GPU) -> rows [N, L].
    ``dropout`` > 0 with ``seed`` (int64 [1] on the GPU) applies the levels' dropout inside the kernels."""

    @staticmethod
    def forward(ctx, x, taps, bias, dropout=0.0, seed=None):
        x, taps, bias = x.contiguous(), taps.contiguous(), bias.contiguous()
        y = _tcn_launch_fwd(x, taps, bias, dropout, seed)
        ctx.save_for_backward(x, taps, bias)
        ctx.dropout, ctx.seed = float(dropout), seed
        return y

    @staticmethod
    def backward(ctx, grad_output):
        x, taps, bias = ctx.saved_tensors
        k = taps.shape[2]
        dx, partial = _tcn_launch_bwd(x, grad_output, taps, bias, ctx.dropout, ctx.seed)
        sums = partial.sum(0)
        return dx, sums[:, :, :k].contiguous(), sums[:, :, k].contiguous(), None, None


class FusedNormedTCNFunction(Function):
    """rows [N, L] through the whole front end.  ``params``: per convolution (2 per level) the weight-norm parameters
    weight_v [1, 1, k], weight_g [1, 1, 1] and the bias [1] (or None) -- the effective taps w = g v / |v| are formed by ONE
    launch (wfs_tcn_taps_fwd), the backward's per-row partial sums are turned into d weight_v, d weight_g, d bias by ONE
    launch (wfs_tcn_taps_bwd) that writes straight into the parameters' gradient slots (spconv/functional.grad_like).
    ``dropout`` > 0 with ``seed`` (int64 [1] on the GPU) applies the levels' dropout inside the kernels."""

    @staticmethod
    def forward(ctx, x, k, dropout, seed, cache, *params):
        x = x.contiguous()
        n_conv = len(params) // 3
        levels = n_conv // 2
        for v, g in zip(params[0::3], params[1::3]):
            assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == k and g.numel() == 1
        rows = _fused.fwd_rows(params, 3)
        tab = _fused.ptr_table(cache, ("fwd",) + tuple(map(tuple, rows)), rows, x.device)
        taps = torch.empty((levels, 2, k), dtype=torch.float32, device=x.device)
        bias = torch.empty((levels, 2), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().wfs_tcn_taps_fwd(_lib.ptr(tab), n_conv, k, _lib.ptr(taps), _lib.ptr(bias), _lib.stream_ptr()))
        y = _tcn_launch_fwd(x, taps, bias, dropout, seed)
        ctx.save_for_backward(x, taps, bias)
        ctx.params = params
        ctx.dropout, ctx.seed, ctx.k, ctx.cache = float(dropout), seed, k, cache
        return y

    @staticmethod
    def backward(ctx, grad_output):
        x, taps, bias = ctx.saved_tensors
        first = FusedNormedTCNFunction.first_param
        dx, partial = _tcn_launch_bwd(x, grad_output, taps, bias, ctx.dropout, ctx.seed)
        rows, grads = _fused.bwd_rows(ctx, ctx.params, 3, first)
        if any(t is not None for t in grads):
            tab = _fused.ptr_table(ctx.cache, ("bwd",) + tuple(map(tuple, rows)), rows, x.device)
            _lib.check(_lib.load().wfs_tcn_taps_bwd(_lib.ptr(tab), len(rows), ctx.k, _lib.ptr(partial), x.shape[0],
                                                    _lib.stream_ptr()))
        return (dx,) + (None,) * (first - 1) + tuple(grads)


FusedNormedTCNFunction.first_param = _fused.first_param(FusedNormedTCNFunction)

TCNC_CALLS = [0]      # forward calls that ran on the multi-channel kernels (tests and tools read it)


class FusedMultiTCNFunction(Function):
    """[N, c0, L] through TemporalConvNet(c0, channels, k) on the multi-channel kernels.  ``params``: per convolution in
    the order of wfs_tcnc_n_conv (per level conv1, conv2, then the downsample if any) its (weight_v, weight_g, bias) --
    the downsample's (weight, None, bias).  The backward writes every parameter gradient from ONE launch into the
    gradient slots (spconv/functional.grad_like)."""

    @staticmethod
    def forward(ctx, x, c0, channels, k, dropout, seed, cache, *params):
        lib = _lib.load()
        x = x.contiguous()
        N, _c, L = x.shape
        levels = len(channels)
        ch = _lib.i32_array(channels)
        rows = _fused.fwd_rows(params, 3)
        tab = _fused.ptr_table(cache, ("mfwd",) + tuple(map(tuple, rows)), rows, x.device)
        wts = torch.empty((int(lib.wfs_tcnc_weights_floats(c0, ch, levels, k)),), dtype=torch.float32, device=x.device)
        saved = torch.empty((int(lib.wfs_tcnc_saved_floats(N, L, c0, ch, levels)),), dtype=torch.float32, device=x.device)
        y = torch.empty((N, channels[-1], L), dtype=x.dtype, device=x.device)
        _lib.check(lib.wfs_tcnc_taps_fwd(_lib.ptr(tab), c0, ch, levels, k, _lib.ptr(wts), _lib.stream_ptr()))
        _lib.check(lib.wfs_tcnc_fwd(_lib.ptr(x), N, L, c0, ch, levels, k, _lib.ptr(wts), _lib.ptr(saved), _lib.ptr(y),
                                    _lib.dtype_code(x), float(dropout), _lib.ptr(seed), _lib.stream_ptr()))
        TCNC_CALLS[0] += 1
        ctx.save_for_backward(x, wts, saved)
        ctx.params, ctx.plan = params, (c0, tuple(channels), k)
        ctx.dropout, ctx.seed, ctx.cache = float(dropout), seed, cache
        return y

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        x, wts, saved = ctx.saved_tensors
        c0, channels, k = ctx.plan
        first = FusedMultiTCNFunction.first_param
        N, _c, L = x.shape
        levels = len(channels)
        ch = _lib.i32_array(channels)
        dy = _fused.as_grad(grad_output, x.dtype)
        dx = torch.empty_like(x)
        rows, grads = _fused.bwd_rows(ctx, ctx.params, 3, first)
        tab = _fused.ptr_table(ctx.cache, ("mbwd",) + tuple(map(tuple, rows)), rows, x.device)
        ws = torch.empty((int(lib.wfs_tcnc_bwd_workspace_floats(N, L, c0, ch, levels, k)),), dtype=torch.float32,
                         device=x.device)
        _lib.check(lib.wfs_tcnc_bwd(_lib.ptr(x), _lib.ptr(dy), N, L, c0, ch, levels, k, _lib.ptr(wts), _lib.ptr(saved),
                                    _lib.ptr(dx), _lib.ptr(ws), _lib.ptr(tab), _lib.dtype_code(x), ctx.dropout,
                                    _lib.ptr(ctx.seed), _lib.stream_ptr()))
        return (dx,) + (None,) * (first - 1) + tuple(grads)


FusedMultiTCNFunction.first_param = _fused.first_param(FusedMultiTCNFunction)


class TemporalConvNet(nn.Module):
    def __init__(self, num_inputs, num_channels, kernel_size=3, dropout=0.2, fused=False):
        super().__init__()
        blocks = []
        for i, n_out in enumerate(num_channels):
            d = 2 ** i
            n_in = num_inputs if i == 0 else num_channels[i - 1]
            blocks.append(TemporalBlock(n_in, n_out, kernel_size, 1, d, (kernel_size - 1) * d, dropout))
        self.network = nn.Sequential(*blocks)
        self.kernel_size, self.dropout = kernel_size, dropout
        self.single_channel = num_inputs == 1 and all(c == 1 for c in num_channels)
        # fused=True: any other channel plan runs on the multi-channel kernels (wfs_tcnc_*) where they take it
        self.fused = bool(fused)
        self.num_inputs, self.channels = int(num_inputs), [int(c) for c in num_channels]

    def _can_fuse_multi(self, x):
        """The multi-channel kernels take this call: opted in, GPU rows of a supported dtype, a plan inside
        wfs_tcnc_ok's bounds, and parameters the kernels read (contiguous fp32 on the GPU)."""
        if not (self.fused and x.is_cuda and x.dim() == 3 and x.shape[1] == self.num_inputs and x.shape[0] > 0
                and x.dtype in (torch.float32, torch.bfloat16, torch.float16)):
            return False
        if self.training and self.dropout != 0 and not 0.0 <= self.dropout < 1.0:
            return False
        lib = _lib.load()
        if lib.wfs_tcnc_ok(self.num_inputs, _lib.i32_array(self.channels), len(self.channels), self.kernel_size,
                           int(x.shape[2]), _lib.dtype_code(x)) != _lib.WFS_OK:
            return False
        return self._multi_params() is not None

    def _multi_params(self):
        """(v, g, b) per convolution in the kernels' order; the downsample as (weight, None, bias).  None unless every
        tensor is contiguous fp32 on the GPU."""
        trips = []
        for blk in self.network:
            trips += [(conv.weight_v, conv.weight_g, conv.bias) for conv in blk.convs]
            if blk.downsample is not None:
                trips.append((blk.downsample.weight, None, blk.downsample.bias))
        return _fused.kernel_params(trips)

    def _dropout_args(self, x):
        """(p, seed) of this call: dropout runs in training mode only, on ONE draw from torch's generator."""
        if self.training and self.dropout > 0:
            return self.dropout, _fused.draw_seed(x.device)
        return 0.0, None

    def _forward_multi(self, x):
        p, seed = self._dropout_args(x)
        return FusedMultiTCNFunction.apply(x, self.num_inputs, tuple(self.channels), self.kernel_size, p, seed,
                                           _fused.ptr_cache(self), *self._multi_params())

    def _can_fuse(self, x):
        levels, k = len(self.network), self.kernel_size
        if not (self.single_channel and x.is_cuda and x.dim() == 3 and x.shape[1] == 1
                and x.dtype in (torch.float32, torch.bfloat16, torch.float16) and 1 <= levels <= 8 and 1 <= k <= 8
                and 1 <= x.shape[2] <= 4096 and x.shape[0] > 0):
            return False
        if self.training and not 0.0 <= self.dropout < 1.0:
            return False                                  # p = 1 (everything dropped) is torch's business
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if _lib.load().wfs_tcn_lds_bytes(int(x.shape[2]), levels, 1) > 150 * 1024:
                return False                              # the backward keeps (3 levels + 4) rows in LDS
        return True

    def effective_taps(self):
        """[levels, 2, k] taps after weight norm (w = g v / |v|, differentiable) and [levels, 2] biases."""
        taps, bias = [], []
        for blk in self.network:
            for conv in blk.convs:
                taps.append(torch._weight_norm(conv.weight_v, conv.weight_g, 0).reshape(-1))
                bias.append(conv.bias.reshape(()) if conv.bias is not None else conv.weight_v.new_zeros(()))
        levels = len(self.network)
        return torch.stack(taps).reshape(levels, 2, -1).float(), torch.stack(bias).reshape(levels, 2).float()

    def _norm_params(self):
        """(weight_v, weight_g, bias) of every convolution, level by level -- None unless they are what the fused
        weight-norm kernels read: contiguous fp32 tensors on the GPU."""
        return _fused.kernel_params((conv.weight_v, conv.weight_g, conv.bias) for blk in self.network for conv in blk.convs)

    def forward(self, x):
        if self._can_fuse(x):
            params = self._norm_params()
            if params is not None:
                rows = x.reshape(x.shape[0], x.shape[2])
                p, seed = self._dropout_args(x)
                return FusedNormedTCNFunction.apply(rows, self.kernel_size, p, seed, _fused.ptr_cache(self), *params).reshape(x.shape)
        if self.fused and not self.single_channel and self._can_fuse_multi(x):
            return self._forward_multi(x)
        return self.network(x)
