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
from .blocks import LinearBlock
from .tcn import _ptr_table

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
        rows = []
        for r in range(len(params) // 4):
            rows.append([t.data_ptr() if t is not None else 0 for t in params[4 * r: 4 * r + 4]] + [0, 0, 0, 0])
        tab = _ptr_table(cache, ("rfwd",) + tuple(a for r in rows for a in r[:4]), rows, x.device)
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
        from ..spconv.functional import grad_like
        lib = _lib.load()
        saved, = ctx.saved_tensors
        I, H, layers, dirs, nonlin = ctx.shape
        N, T, dtype, device = ctx.xinfo
        params = ctx.params
        dy = grad_output.contiguous()
        if dy.dtype != dtype:
            dy = dy.to(dtype)
        dx = torch.empty((N, T, I), dtype=dtype, device=device) if ctx.needs_input_grad[0] else None
        grads, rows = [], []
        for r in range(len(params) // 4):
            ps = params[4 * r: 4 * r + 4]
            need = ctx.needs_input_grad[5 + 4 * r: 5 + 4 * r + 4]
            gs = [grad_like(p) if (p is not None and nd) else None for p, nd in zip(ps, need)]
            grads += gs
            rows.append([t.data_ptr() if t is not None else 0 for t in list(ps) + gs])
        tab = _ptr_table(ctx.cache, ("rbwd",) + tuple(a for r in rows for a in r), rows, device)
        ws = torch.empty((int(lib.wfs_rnn_bwd_workspace_floats(N, T, I, H, layers, dirs)),), dtype=torch.float32,
                         device=device)
        _lib.check(lib.wfs_rnn_bwd(_lib.ptr(dy), N, T, I, H, layers, dirs, nonlin, _lib.ptr(tab), _lib.ptr(saved),
                                   _lib.ptr(dx), _lib.ptr(ws), _lib.dtype_code(dy), ctx.dropout, _lib.ptr(ctx.seed),
                                   _lib.stream_ptr()))
        return (dx, None, None, None, None) + tuple(grads)


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
        out = []
        for layer in range(rnn.num_layers):
            for sfx in ("", "_reverse") if rnn.bidirectional else ("",):
                names = ["weight_ih_l%d%s", "weight_hh_l%d%s"] + (["bias_ih_l%d%s", "bias_hh_l%d%s"] if rnn.bias else [])
                four = [getattr(rnn, n % (layer, sfx)) for n in names] + ([] if rnn.bias else [None, None])
                for t in four:
                    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                        return None
                out += four
        return out

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
                # a fresh 64-bit seed per call from torch's generator (reproducible under torch.manual_seed, and a captured
                # graph draws a new one per replay); the kernels derive every mask from it
                seed = torch.randint(-2 ** 62, 2 ** 62, (1,), dtype=torch.int64, device=x.device)
                p = rnn.dropout
            if not hasattr(self, "_ptr_cache"):
                self._ptr_cache = {}
            shape = (rnn.input_size, rnn.hidden_size, rnn.num_layers, 2 if rnn.bidirectional else 1,
                     _NONLIN[rnn.nonlinearity])
            return FusedRNNFunction.apply(x, shape, p, seed, self._ptr_cache, *self._fused_params())
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
