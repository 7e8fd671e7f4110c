"""``RecurrentBlock`` / ``RecurrentNet``: mirror of the reference's Elman-RNN pulse net (src/models/RecurrentBlocks.py):
``nn.RNN(input_size, hidden_size, n_layers, nonlinearity, bias, dropout, bidirectional, batch_first=True)`` over
[N, seq_len, input_size] rows, Flatten, LinearBlock(hidden_size * seq_len, out_size, n_lin).

``RecurrentBlock.rnn`` stays a ``torch.nn.RNN``: it holds the parameters, so initialisation (and the RNG draws it
consumes), parameter names (``rnn_block.rnn.weight_ih_l0`` ...) and checkpoints are the reference's.  With ``fused=True``
a GPU call inside wfs_rnn_ok's bounds never runs ``nn.RNN.forward`` (a library RNN): it runs the scan kernels of
csrc/rnn.hip (include/wfsparse.h, wfs_rnn_fwd / wfs_rnn_bwd) on the holder's parameters, read through their names at
every call -- so ``module.to("cuda")`` and FlatGradAllReducer (which re-points ``p.data`` into one flat buffer) leave
them the tensors the kernels read, and the gradients land in the flat gradient buffer's slots
(spconv/functional.grad_like).  Everything else -- CPU tensors, shapes out of bounds, the flag off -- is ``self.rnn(x)``.

Dropout between layers (training mode) has nn.RNN's placement and distribution with this project's generator: the
kernels derive every mask from one int64 seed drawn from torch's generator per call (not the same bits as nn.RNN).
``hidden`` of the fused path is for inspection: no gradient flows through it (RecurrentNet drops it, as the reference).
"""
import torch
from torch import nn
from torch.autograd import Function

from .. import _lib
from . import _fused
from .blocks import LinearBlock

RNN_CALLS = [0]      # forward calls that ran on the scan kernels (tests and tools read it)

_NONLIN = {"relu": _lib.WFS_RNN_RELU, "tanh": _lib.WFS_RNN_TANH}


class FusedRNNFunction(Function):
    """[N, T, I] -> (out [N, T, dirs H], hidden [layers dirs, N, H]).  ``params``: per (layer, direction) in nn.RNN's
    order its (weight_ih, weight_hh, bias_ih, bias_hh), the biases None without bias.  The backward writes every
    parameter gradient from one call into the gradient slots (spconv/functional.grad_like)."""

    @staticmethod
    def forward(ctx, x, shape, dropout, seed, cache, *params):
        lib = _lib.load()
        x = x.contiguous()
        I, H, layers, dirs, nonlin = shape
        N, T, _i = x.shape
        rows = _fused.fwd_rows(params, 4)
        tab = _fused.ptr_table(cache, ("rfwd",) + tuple(map(tuple, rows)), rows, x.device)
        saved = torch.empty((int(lib.wfs_rnn_saved_floats(N, T, I, H, layers, dirs)),), dtype=torch.float32,
                            device=x.device)
        y = torch.empty((N, T, dirs * H), dtype=x.dtype, device=x.device)
        hidden = torch.empty((layers * dirs, N, H), dtype=x.dtype, device=x.device)
        _lib.check(lib.wfs_rnn_fwd(_lib.ptr(x), N, T, I, H, layers, dirs, nonlin, _lib.ptr(tab), _lib.ptr(saved),
                                   _lib.ptr(y), _lib.ptr(hidden), _lib.dtype_code(x), float(dropout), _lib.ptr(seed),
                                   _lib.stream_ptr()))
        RNN_CALLS[0] += 1
        ctx.save_for_backward(saved)
        ctx.params, ctx.shape, ctx.xinfo = params, shape, (N, T, x.dtype, x.device)
        ctx.dropout, ctx.seed, ctx.cache = float(dropout), seed, cache
        ctx.mark_non_differentiable(hidden)
        return y, hidden

    @staticmethod
    def backward(ctx, grad_output, _grad_hidden):
        lib = _lib.load()
        saved, = ctx.saved_tensors
        I, H, layers, dirs, nonlin = ctx.shape
        N, T, dtype, device = ctx.xinfo
        first = FusedRNNFunction.first_param
        dy = _fused.as_grad(grad_output, dtype)
        dx = torch.empty((N, T, I), dtype=dtype, device=device) if ctx.needs_input_grad[0] else None
        rows, grads = _fused.bwd_rows(ctx, ctx.params, 4, first)
        tab = _fused.ptr_table(ctx.cache, ("rbwd",) + tuple(map(tuple, rows)), rows, device)
        ws = torch.empty((int(lib.wfs_rnn_bwd_workspace_floats(N, T, I, H, layers, dirs)),), dtype=torch.float32,
                         device=device)
        _lib.check(lib.wfs_rnn_bwd(_lib.ptr(dy), N, T, I, H, layers, dirs, nonlin, _lib.ptr(tab), _lib.ptr(saved),
                                   _lib.ptr(dx), _lib.ptr(ws), _lib.dtype_code(dy), ctx.dropout, _lib.ptr(ctx.seed),
                                   _lib.stream_ptr()))
        return (dx,) + (None,) * (first - 1) + tuple(grads)


FusedRNNFunction.first_param = _fused.first_param(FusedRNNFunction)


class RecurrentBlock(nn.Module):
    def __init__(self, input_size, hidden_size, n_layers, nonlinearity='relu', bias=True, dropout=0., bidirectional=False,
                 fused=False):
        super().__init__()
        self.hidden_size = hidden_size
        self.n_layers = n_layers
        self.rnn = nn.RNN(input_size, hidden_size, n_layers, nonlinearity=nonlinearity, bias=bias, dropout=dropout,
                          bidirectional=bidirectional, batch_first=True)
        self.fused = bool(fused)

    def _fused_params(self):
        """(weight_ih, weight_hh, bias_ih, bias_hh) per (layer, direction), read from the holder by name; None unless
        every tensor is contiguous fp32 on the GPU."""
        rnn = self.rnn
        names = ("weight_ih", "weight_hh") + (("bias_ih", "bias_hh") if rnn.bias else ())
        return _fused.kernel_params(
            [getattr(rnn, "%s_l%d%s" % (n, layer, sfx)) for n in names] + ([] if rnn.bias else [None, None])
            for layer in range(rnn.num_layers) for sfx in (("", "_reverse") if rnn.bidirectional else ("",)))

    def _can_fuse(self, x):
        rnn = self.rnn
        if not (self.fused and x.is_cuda and x.dim() == 3 and x.shape[2] == rnn.input_size and x.shape[0] > 0
                and x.dtype in (torch.float32, torch.bfloat16, torch.float16) and rnn.nonlinearity in _NONLIN
                and getattr(rnn, "proj_size", 0) == 0):
            return False
        if self.training and rnn.dropout != 0 and not 0.0 <= rnn.dropout < 1.0:
            return False                                      # p = 1 (everything dropped) is torch's business
        if _lib.load().wfs_rnn_ok(rnn.input_size, rnn.hidden_size, rnn.num_layers, 2 if rnn.bidirectional else 1,
                                  _NONLIN[rnn.nonlinearity], int(x.shape[1]), _lib.dtype_code(x)) != _lib.WFS_OK:
            return False
        return self._fused_params() is not None

    def forward(self, x):
        if self.fused and self._can_fuse(x):
            rnn = self.rnn
            seed, p = None, 0.0
            if self.training and rnn.dropout > 0 and rnn.num_layers > 1:
                seed, p = _fused.draw_seed(x.device), rnn.dropout
            shape = (rnn.input_size, rnn.hidden_size, rnn.num_layers, 2 if rnn.bidirectional else 1,
                     _NONLIN[rnn.nonlinearity])
            return FusedRNNFunction.apply(x, shape, p, seed, _fused.ptr_cache(self), *self._fused_params())
        return self.rnn(x)

    def init_hidden(self, batch_size):
        return torch.zeros(self.n_layers, batch_size, self.hidden_size)


class RecurrentNet(nn.Module):
    def __init__(self, seq_len, input_size, hidden_size, n_layers, n_lin, out_size, nonlinearity='relu', bias=True,
                 dropout=0., bidirectional=False, fused=False):
        super().__init__()
        self.rnn_block = RecurrentBlock(input_size, hidden_size, n_layers, nonlinearity=nonlinearity, bias=bias,
                                        dropout=dropout, bidirectional=bidirectional, fused=fused)
        if n_lin > 0:
            self.linear = LinearBlock(hidden_size * seq_len, out_size, n_lin).func
        else:
            self.linear = None
        self.out_size = out_size
        self.flatten = nn.Flatten()

    def forward(self, x):
        from ..spconv.functional import head_forward
        out, _hidden = self.rnn_block(x)
        out = self.flatten(out)
        if self.linear:
            return head_forward(out, self.linear)
        if self.out_size == 1:
            return out[:, -1]
        raise IOError("must have n_lin > 0 if out_size is > 1")
