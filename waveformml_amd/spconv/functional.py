"""Autograd functions over libwfsparse: counterpart of ``spconv.functional`` (spconv 1.2.1,
SURVEY.md A.4: ``indice_conv`` / ``indice_subm_conv`` / ``indice_inverse_conv`` and their backward).

All three are the same output-stationary gather kernel with a different table (include/wfsparse.h):

    mode      forward table (rows R)        dX table (rows)          dW stationary / gathered
    conv      nbr_in  [K,M]  gathers X[N]   nbr_out [K,N] dY[M]      S = X [N],  G = dY, nbr_out
    subm      nbr_out mirrored (or nbr_in)  nbr_out [K,N] dY[N]      S = X [N],  G = dY, nbr_out
    inverse   nbr_out [K,N]  gathers X[M]   nbr_in  [K,M] dY[N]      S = dY [N], G = X,  nbr_out (swap)

With duplicate input coordinates the inverse of nbr_out is not a function; the two products that
need it (conv/subm forward, inverse dX) then use the atomic scatter form.
"""
import ctypes

import torch
from torch.autograd import Function

from .. import _lib

CONV, SUBM, INVERSE = 0, 1, 2

# bench.py's accounting pass (never active inside a timed region): when this is a list, every launch
# appends its ALGORITHMIC work as SURVEY.md 8d defines it -- each tensor counted once, the rulebook
# at 8 bytes per pair (spconv's encoding), filters fp32.
ACCOUNT = None


def _account(kind, table, R, rows_in, c_in, rows_out, c_out, K, cw_in, cw_out, esize):
    if ACCOUNT is None:
        return
    pairs = int((table >= 0).sum().item()) if table is not None else int(R)
    ACCOUNT.append(dict(kind=kind, pairs=pairs,
                        bytes=rows_in * c_in * esize + rows_out * c_out * esize + pairs * 8 + K * cw_in * cw_out * 4,
                        flops=2 * pairs * cw_in * cw_out))


def _features_ok(t):
    if not t.is_cuda:
        raise RuntimeError("waveformml_amd.spconv: features must be on the GPU (there is no CPU path)")
    return t.contiguous()


def as_grad(dy, dtype):
    """The incoming gradient as the kernels read it: contiguous, in the rows' dtype."""
    dy = dy.contiguous()
    return dy if dy.dtype == dtype else dy.to(dtype)


def _rows(shape, like, r_dev):
    """Row-dimensioned output.  In device-count mode rows beyond the valid count are never written NOR read
    by the kernels, so they can stay uninitialised (the conv bias gradient's column sum honours the count too)."""
    return torch.empty(shape, dtype=like.dtype, device=like.device)


def _masked_column_sum(t, r_dev):
    """sum over the valid rows of t [R, C] (fp32): the conv bias gradient (include/wfsparse.h wfs_column_sum)."""
    lib = _lib.load()
    t = t.contiguous()
    R, C = int(t.shape[0]), int(t.shape[1])
    out = torch.empty((C,), dtype=torch.float32, device=t.device)
    ws = torch.empty((int(lib.wfs_column_sum_workspace_bytes(C)),), dtype=torch.uint8, device=t.device)
    _lib.check(lib.wfs_column_sum(_lib.ptr(t), R, C, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.dtype_code(t),
                                  _lib.ptr(r_dev), _lib.stream_ptr()))
    return out


# Every layer runs in libwfsparse: the 32- and 2-channel MFMA kernels of conv_mfma.hip, the shape-generic 32 x 32-tile MFMA
# kernels of gather_conv.hip (k_gconv_mfma / k_gdw_mfma: 16 / 24 / 64-channel layers) and, from 128 channels on a side,
# the dense 128 x 128-tile matrix-core products of wide.hip (the reference's GEP.json 300 -> 252 -> 158 -> 64 stack,
# SparseConv2DPreserve's 130 ... 154 channels, the hybrid net's 2048 -> 1697 -> 1021 -> 345 stack of BASELINE
# configs[4]) -- 16-bit MFMA for 16-bit rows, exact-fp32 MFMA for fp32 rows.  No torch.mm / library GEMM on this path.


def _fast_shape(Cx, Cy):
    """Channel pairs with shape-specialised kernels (conv_mfma.hip)."""
    return (Cx == 32 and Cy == 32) or (Cx == 2 and Cy == 32) or (Cx == 32 and Cy == 2)


def filters16(W, like):
    """[K, Cin, Cout] fp32 filters in the row type of ``like``, padded as the wide products read them (one conversion
    per layer and step: the forward pass keeps it for dX).  None for fp32 rows whose filters are read in place."""
    lib = _lib.load()
    K, Cw_in, Cw_out = int(W.shape[0]), int(W.shape[1]), int(W.shape[2])
    if like.dtype == torch.float32 and Cw_out % 4 == 0:
        return None
    code = _lib.dtype_code(like)
    out = torch.empty((int(lib.wfs_wide_filters_bytes(K, Cw_in, Cw_out, code)),), dtype=torch.uint8, device=W.device)
    _lib.check(lib.wfs_wide_filters(_lib.ptr(W), K, Cw_in, Cw_out, code, _lib.ptr(out), _lib.stream_ptr()))
    return out


def takes_wide_path(K, R, X, Cy):
    return bool(X.is_cuda and X.dtype in (torch.float32, torch.bfloat16, torch.float16)
                and _lib.load().wfs_wide_conv_ok(K, R, X.shape[0], int(X.shape[1]), int(Cy), _lib.dtype_code(X)))


def _wide_gather_conv(lib, table, kmap, K, identity_k, R, X, W, transpose_w, bias, r_dev, w16=None):
    """>= 128 channels on a side: one dense matrix-core product over the shorter side of the layer
    (csrc/wide.hip; include/wfsparse.h wfs_wide_gather_conv)."""
    Cw_in, Cw_out = int(W.shape[-2]), int(W.shape[-1])
    Cx, Cy = int(X.shape[1]), (Cw_in if transpose_w else Cw_out)
    assert W.dtype == torch.float32 and W.is_contiguous() and X.is_contiguous()
    assert Cx == (Cw_out if transpose_w else Cw_in), (X.shape, W.shape, transpose_w)
    assert table is None or (table.dtype == torch.int32 and table.shape == (K, R)), (None if table is None else table.shape, K, R)
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == Cy)
    Y = _rows((R, Cy), X, r_dev)
    nbytes = lib.wfs_wide_conv_workspace_bytes(K, R, X.shape[0], Cx, Cy, 0 if table is None else 1, _lib.dtype_code(X))
    ws = torch.empty((int(nbytes),), dtype=torch.uint8, device=X.device)
    _lib.check(lib.wfs_wide_gather_conv(_lib.ptr(table), kmap, K, identity_k, R, _lib.ptr(X), X.shape[0], Cx, _lib.ptr(W),
                                        _lib.ptr(w16), Cw_in, Cw_out, 1 if transpose_w else 0, _lib.ptr(bias), _lib.ptr(Y),
                                        _lib.dtype_code(X), _lib.ptr(r_dev), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    _account("gather_conv", table, R, X.shape[0], Cx, R, Cy, K, Cw_in, Cw_out, X.element_size())
    return Y


def gather_conv(table, kmap, K, identity_k, R, X, W, transpose_w, bias, r_dev=None, w16=None, packed_kl=0, image=None):
    """Y[r] = bias + sum_k X[table[kmap[k], r]] . W[k]   (W fp32 [K, Cin, Cout]; ^T if transpose_w).
    ``packed_kl`` > 0: ``table`` is the packed by-input table [K / packed_kl, R] (Rulebook.table_by_in).
    ``image``: W's filter image of this orientation in X's row type (include/wfsparse.h "filter images"), or None."""
    lib = _lib.load()
    Cw_in, Cw_out = int(W.shape[-2]), int(W.shape[-1])
    if packed_kl:
        assert transpose_w and kmap is None and table.shape == (K // packed_kl, R), (table.shape, K, packed_kl, R)
        Y = _rows((R, Cw_in), X, r_dev)
        _lib.check(lib.wfs_gather_conv_image(_lib.ptr(table), None, K, identity_k, R, _lib.ptr(X), X.shape[0], X.shape[1],
                                             _lib.ptr(W), Cw_in, Cw_out, 1, None, _lib.ptr(Y), _lib.dtype_code(X),
                                             _lib.ptr(r_dev), packed_kl, _lib.ptr(image), _lib.stream_ptr()))
        if ACCOUNT is not None:
            _account("gather_conv", (table >> 3).clamp_(min=-1), R, X.shape[0], X.shape[1], R, Cw_in, K, Cw_in, Cw_out,
                     X.element_size())
        return Y
    if X.is_cuda and lib.wfs_wide_conv_ok(K, R, X.shape[0], int(X.shape[1]), Cw_in if transpose_w else Cw_out, _lib.dtype_code(X)):
        return _wide_gather_conv(lib, table, kmap, K, identity_k, R, X, W, transpose_w, bias, r_dev, w16)
    if transpose_w and not _fast_shape(Cw_out, Cw_in):
        # the shape-generic MFMA kernel reads the filter with the OUTPUT channel on the lanes: for dX that is a strided
        # walk over W[k] (a new 128-B line per lane and step; 47 vs 26 us measured at 64 channels) -- hand it W[k]^T
        # instead (one small transpose launch: the filters are at most a few MB)
        W, transpose_w = W.transpose(1, 2).contiguous(), False
        Cw_in, Cw_out = Cw_out, Cw_in
    Cy = Cw_in if transpose_w else Cw_out
    Y = _rows((R, Cy), X, r_dev)
    assert W.dtype == torch.float32 and W.is_contiguous()
    assert X.dim() == 2 and X.shape[1] == (Cw_out if transpose_w else Cw_in), (X.shape, W.shape, transpose_w)
    assert table is None or (table.dtype == torch.int32 and table.shape == (K, R)), (None if table is None else table.shape, K, R)
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == Cy)
    _lib.check(lib.wfs_gather_conv_image(_lib.ptr(table), kmap, K, identity_k, R, _lib.ptr(X), X.shape[0], X.shape[1],
                                         _lib.ptr(W), Cw_in, Cw_out, 1 if transpose_w else 0, _lib.ptr(bias),
                                         _lib.ptr(Y), _lib.dtype_code(X), _lib.ptr(r_dev), 0, _lib.ptr(image),
                                         _lib.stream_ptr()))
    _account("gather_conv", table, R, X.shape[0], X.shape[1], R, Cy, K, Cw_in, Cw_out, X.element_size())
    return Y


def scatter_conv(table, K, identity_k, R, X, W, transpose_w, n_out, bias):
    """fp32-atomic form for duplicate coordinates: Y[table[k, r]] += X[r] . W[k]."""
    lib = _lib.load()
    Cw_in, Cw_out = int(W.shape[-2]), int(W.shape[-1])
    Cy = Cw_in if transpose_w else Cw_out
    Y = torch.zeros((n_out, Cy), dtype=torch.float32, device=X.device)
    if bias is not None:
        Y += bias
    assert table.dtype == torch.int32 and table.shape == (K, R)
    _lib.check(lib.wfs_scatter_conv(_lib.ptr(table), K, identity_k, R, _lib.ptr(X), X.shape[1], _lib.ptr(W), Cw_in,
                                    Cw_out, 1 if transpose_w else 0, _lib.ptr(Y), _lib.dtype_code(X),
                                    _lib.stream_ptr()))
    return Y.to(X.dtype)


# ---- parameter gradients written where the optimizer reads them ---------------------------------------------------
# A runner that keeps all parameters / gradients in ONE flat buffer each (psd/ddp.FlatGradAllReducer) registers the
# pair here.  Backward passes then allocate a parameter's gradient as a VIEW of its slot in the flat gradient buffer
# (grad_like), so the kernels write it in place and the runner's pack step has nothing left to copy.
_GRAD_SLOTS = []          # [(weakref(flat_param), weakref(flat_grad))]


def register_grad_slots(flat_param, flat_grad):
    import weakref
    _GRAD_SLOTS[:] = [(p, g) for (p, g) in _GRAD_SLOTS if p() is not None and g() is not None]
    _GRAD_SLOTS.append((weakref.ref(flat_param), weakref.ref(flat_grad)))


_SLOTS_WRITTEN = set()    # slot addresses handed out during the current backward pass


def reset_grad_slots():
    """Forget which slots the current / last backward pass wrote (runs at the end of every backward pass that handed
    one out, and from FlatGradAllReducer.reset())."""
    _SLOTS_WRITTEN.clear()


def grad_like(param, shape=None):
    """An fp32 tensor of ``shape`` (default: param's) for d loss / d param: the parameter's slot in a registered flat
    gradient buffer when ``param`` is a contiguous fp32 view into the matching flat parameter buffer, else fresh memory.

    A slot is handed out ONCE per backward pass and only while the parameter has no gradient yet: a module called twice
    in one graph (two gradients for one parameter, summed by autograd) or a second backward() without reset (gradient
    accumulation, ``p.grad += new``) gets fresh memory for the further gradients -- two operands of autograd's add
    must never alias the same slot."""
    shape = tuple(param.shape) if shape is None else tuple(shape)
    if (param is not None and param.is_cuda and param.dtype == torch.float32 and param.is_contiguous()
            and param.grad is None):
        for pref, gref in _GRAD_SLOTS:
            fp, fg = pref(), gref()
            if fp is None or fg is None or fp.device != param.device or fg.dtype != torch.float32:
                continue
            off = param.data_ptr() - fp.data_ptr()
            if 0 <= off and off + 4 * param.numel() <= 4 * fp.numel() and off % 4 == 0:
                slot = fg.data_ptr() + off
                if slot in _SLOTS_WRITTEN:
                    # a second gradient for this parameter in one pass: autograd is about to ADD it to the first one,
                    # so a pending (deferred) second stage of the first must land in the slot now, and the slot no
                    # longer counts as "filled by a deferred reduction" (the sum is wherever autograd puts it)
                    flush_deferred_dw()
                    _SHARED_SLOTS.add(slot)
                    break
                if not _SLOTS_WRITTEN:
                    try:
                        torch.autograd.Variable._execution_engine.queue_callback(reset_grad_slots)
                    except RuntimeError:          # not inside a backward pass (direct call): the caller resets
                        pass
                _SLOTS_WRITTEN.add(slot)
                return fg[off // 4: off // 4 + param.numel()].view(shape)
    return torch.empty(shape, dtype=torch.float32, device=param.device)


# Deferred second stages of gather_dw (include/wfsparse.h, wfs_dw_job): while a runner has deferral switched on, the
# slab reductions of a whole backward pass are collected and run as ONE launch by flush_deferred_dw() -- only for
# gradients that live in a registered slot (the runner reads the slot, never the tensor autograd holds).
_DEFERRED_DW = None       # None: off; else a list of (DwJob, workspace tensor)
_DEFERRED_SLOTS = set()   # slot addresses written by the last flush
_SHARED_SLOTS = set()     # slots that received more than one gradient in the pass (grad_like)


def defer_dw(on):
    global _DEFERRED_DW
    _DEFERRED_DW = [] if on else None
    _DEFERRED_SLOTS.clear()
    _SHARED_SLOTS.clear()


def was_deferred(slot_ptr):
    return slot_ptr in _DEFERRED_SLOTS and slot_ptr not in _SHARED_SLOTS


def flush_deferred_dw():
    """One launch for every pending slab reduction (no-op when nothing is pending)."""
    if not _DEFERRED_DW:
        return
    lib = _lib.load()
    jobs = (_lib.DwJob * len(_DEFERRED_DW))(*[j for (j, _ws) in _DEFERRED_DW])
    for at in range(0, len(_DEFERRED_DW), 16):
        n = min(16, len(_DEFERRED_DW) - at)
        _lib.check(lib.wfs_dw_reduce_jobs(ctypes.cast(ctypes.byref(jobs, at * ctypes.sizeof(_lib.DwJob)),
                                                      ctypes.POINTER(_lib.DwJob)), n, _lib.stream_ptr()))
    for j, _ws in _DEFERRED_DW:
        _DEFERRED_SLOTS.add(int(j.dW))
    del _DEFERRED_DW[:]


def _dw_job(grad):
    """A DwJob for the kernel to fill when the slab reduction of ``grad`` can join the pass's deferred ones: deferral is
    on and ``grad`` sits in a slot of a registered flat gradient buffer.  Else None (the kernel reduces at once)."""
    if _DEFERRED_DW is not None and grad is not None and grad._base is not None:
        return _lib.DwJob()
    return None


def _queue_dw_job(job, ws):
    """After the call that was handed ``job`` (ctypes passes a DwJob by reference, None as NULL): if it left a second stage
    pending, flush_deferred_dw() runs it; ``ws`` holds its slabs until then."""
    if job is not None and job.nslabs > 0:
        _DEFERRED_DW.append((job, ws))


def gather_dw(table, K, identity_k, R, S, G, swap, kmap=None, r_dev=None, like=None, packed_kl=0):
    """dW[k,a,b] = sum_r S[r,a] G[table[kmap[k],r], b]  (swap: dW[k,b,a]).
    ``like``: the parameter this is the gradient of (grad_like: written straight into its slot of a registered flat
    gradient buffer)."""
    lib = _lib.load()
    Cs, Cg = int(S.shape[1]), int(G.shape[1])
    shape = (K, Cg, Cs) if swap else (K, Cs, Cg)
    if like is not None and like.numel() == K * Cs * Cg:
        dW = grad_like(like, shape)
    else:
        dW = torch.empty(shape, dtype=torch.float32, device=S.device)
    assert S.dtype == G.dtype and S.shape[0] == R
    assert table is None or (table.dtype == torch.int32 and table.shape == ((K // packed_kl if packed_kl else K), R))
    nbytes = lib.wfs_gather_dw_workspace_bytes(K, R, Cs, Cg)
    ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=S.device)
    job = _dw_job(dW)
    _lib.check(lib.wfs_gather_dw(_lib.ptr(table), kmap, K, identity_k, R, _lib.ptr(S), Cs, _lib.ptr(G), G.shape[0],
                                 Cg, 1 if swap else 0, _lib.ptr(dW), _lib.dtype_code(S), _lib.ptr(ws), ws.numel(),
                                 _lib.ptr(r_dev), job, packed_kl, _lib.stream_ptr()))
    _queue_dw_job(job, ws)
    if ACCOUNT is not None:
        _account("gather_dw", (table >> 3).clamp_(min=-1) if packed_kl else table, R, R, Cs, G.shape[0], Cg, K, Cs, Cg,
                 S.element_size())
    return dW


def conv_backward(table, K, identity_k, R, X, dY, W, r_dev=None, like=None, packed_kl=0, image_t=None):
    """(dX, dW) of a conv / SubM layer in one call (include/wfsparse.h wfs_conv_backward): 32 -> 32 layers with 16-bit
    rows run both products in ONE launch.  ``like``: the filter parameter (its gradient goes straight into its slot of a
    registered flat gradient buffer, the slab reduction joins the step's deferred ones)."""
    lib = _lib.load()
    Cin, Cout = int(X.shape[1]), int(dY.shape[1])
    if like is not None and like.numel() == K * Cin * Cout:
        dW = grad_like(like, (K, Cin, Cout))
    else:
        dW = torch.empty((K, Cin, Cout), dtype=torch.float32, device=X.device)
    dX = _rows((R, Cin), dY, r_dev)
    ws = torch.empty((max(int(lib.wfs_gather_dw_workspace_bytes(K, R, Cin, Cout)), 1),), dtype=torch.uint8, device=X.device)
    job = _dw_job(dW)
    _lib.check(lib.wfs_conv_backward_image(_lib.ptr(table), K, identity_k, R, _lib.ptr(X), _lib.ptr(dY), dY.shape[0], Cin,
                                           Cout, _lib.ptr(W), _lib.ptr(dX), _lib.ptr(dW), _lib.dtype_code(X), _lib.ptr(ws),
                                           ws.numel(), _lib.ptr(r_dev), job, packed_kl, _lib.ptr(image_t),
                                           _lib.stream_ptr()))
    _queue_dw_job(job, ws)
    if ACCOUNT is not None:
        # SURVEY.md 8d "backward": X, dY and dX once each, the rulebook twice (8 B per pair), the filters twice
        dense = (table >> 3).clamp_(min=-1) if packed_kl else table
        pairs = int((dense >= 0).sum().item())
        es = X.element_size()
        fused = Cin == 32 and Cout == 32 and _one_launch_rows(X.dtype) and K <= 27      # one launch
        if fused:
            ACCOUNT.append(dict(kind="conv_backward", pairs=pairs,
                                bytes=2 * R * Cin * es + dY.shape[0] * Cout * es + 2 * pairs * 8 + 2 * K * Cin * Cout * 4,
                                flops=4 * pairs * Cin * Cout))
        else:
            _account("gather_dw", dense, R, R, Cin, dY.shape[0], Cout, K, Cin, Cout, es)
            _account("gather_conv", dense, R, dY.shape[0], Cout, R, Cin, K, Cin, Cout, es)
    return dX, dW


# Mirrors csrc/conv_mfma.hip's wfs_split_bf16(): fp32 rows run on the three-piece (split-bf16) kernels unless the library's
# WFS_SPLIT_BF16 is "0".  Only those kernels have the one-launch backward for fp32 rows.
SPLIT_BF16 = __import__("os").environ.get("WFS_SPLIT_BF16", "1") != "0"


def _one_launch_rows(dtype):
    """Row types whose 32 -> 32 dW and dX run in one launch (wfs_conv_backward; else it issues two)."""
    return dtype in (torch.bfloat16, torch.float16) or (dtype == torch.float32 and SPLIT_BF16)


class SparseConvFunction(Function):
    """features [n_in, Cin], filters [*k, Cin, Cout] fp32, bias [Cout] or None -> [n_out, Cout]."""

    @staticmethod
    def forward(ctx, features, filters, bias, rulebook, mode, images=None):
        rb = rulebook
        features = _features_ok(features)
        K = rb.K
        W = filters.detach().reshape(K, filters.shape[-2], filters.shape[-1]).float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        ident = rb.centre_k if rb.subm else -1
        w16 = None
        # the layer's filter images (psd/graph.py): only for the rows and the filter they were made for
        img_fwd = img_t = None
        if (images is not None and mode != INVERSE and images[0] == features.dtype and tuple(W.shape) == (K, 32, 32)
                and W.data_ptr() == filters.data_ptr() and K <= 27):
            img_fwd, img_t = images[1], images[2]
        ctx.img_t = img_t
        if mode == INVERSE:
            assert features.shape[0] == rb.M, "inverse conv input must be the coupled conv's output set"
            w16 = filters16(W, features) if takes_wide_path(K, rb.N, features, W.shape[2]) else None
            out = gather_conv(rb.nbr_out, None, K, ident, rb.N, features, W, False, b, rb.n_dev, w16)
        elif rb.has_dup:
            out = scatter_conv(rb.nbr_out, K, ident, rb.N, features, W, False, rb.M, b)
        else:
            assert features.shape[0] == rb.N
            table, kmap = rb.table_by_out()
            w16 = filters16(W, features) if takes_wide_path(K, rb.M, features, W.shape[2]) else None
            out = gather_conv(table, kmap, K, ident, rb.M, features, W, False, b, rb.m_dev, w16, image=img_fwd)
        ctx.save_for_backward(features, filters, bias)
        ctx.rb, ctx.mode = rb, mode
        ctx.w16 = w16 if ctx.needs_input_grad[0] else None       # the 16-bit filters of a wide layer: dX reads them again
        return out

    @staticmethod
    def backward(ctx, grad_output):
        features, filters, bias = ctx.saved_tensors
        rb, mode = ctx.rb, ctx.mode
        K = rb.K
        dY = as_grad(grad_output, features.dtype)
        W = filters.detach().reshape(K, filters.shape[-2], filters.shape[-1]).float().contiguous()
        ident = rb.centre_k if rb.subm else -1
        dX = dW = db = None
        if mode == INVERSE:
            if ctx.needs_input_grad[0]:
                if rb.has_dup:
                    dX = scatter_conv(rb.nbr_out, K, ident, rb.N, dY, W, True, rb.M, None)
                else:
                    dX = gather_conv(rb.nbr_in, None, K, ident, rb.M, dY, W, True, None, rb.m_dev, ctx.w16)
            if ctx.needs_input_grad[1]:
                dW = gather_dw(rb.nbr_out, K, ident, rb.N, dY, features, True, None, rb.n_dev, filters)
        elif (ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and not rb.has_dup and features.shape[1] == 32
              and dY.shape[1] == 32 and features.is_cuda and _one_launch_rows(features.dtype)):
            table, pk = rb.table_by_in(32, 32, features, 3)
            if pk and rb.table_by_in(32, 32, dY, 1)[1] != pk:
                table, pk = rb.nbr_out, 0
            dX, dW = conv_backward(table, K, ident, rb.N, features, dY, W, rb.n_dev, filters, pk, ctx.img_t)
        else:
            if ctx.needs_input_grad[1]:
                if features.shape[1] == 2 and dY.shape[1] == 32 and K <= 27 and not rb.has_dup:
                    # narrow input, wide output (first layer): keep the wide dY rows stationary
                    table, kmap = rb.table_by_out()
                    dW = gather_dw(table, K, ident, rb.M, dY, features, True, kmap, rb.m_dev, filters)
                else:
                    table, pk = rb.table_by_in(features.shape[1], dY.shape[1], features, 3)
                    dW = gather_dw(table, K, ident, rb.N, features, dY, False, None, rb.n_dev, filters, pk)
            if ctx.needs_input_grad[0]:
                table, pk = rb.table_by_in(dY.shape[1], W.shape[1], dY, 1)
                dX = gather_conv(table, None, K, ident, rb.N, dY, W, True, None, rb.n_dev, ctx.w16, pk,
                                 image=ctx.img_t if dY.dtype == features.dtype else None)
        if dW is not None:
            dW = dW.reshape(filters.shape).to(filters.dtype)
        if bias is not None and ctx.needs_input_grad[2]:
            # dY has one row per OUTPUT of this product: rb.N rows for an inverse conv, rb.M otherwise
            db = _masked_column_sum(dY, rb.n_dev if mode == INVERSE else rb.m_dev).to(bias.dtype)
        return dX, dW, db, None, None, None


def maxpool_fwd(table, kmap, K, R, X, r_dev=None):
    """Y[r] = max(0, max_k X[table[k, r]]) through the by-output table (include/wfsparse.h wfs_maxpool_fwd)."""
    lib = _lib.load()
    C = int(X.shape[1])
    assert X.dim() == 2 and table.dtype == torch.int32 and table.shape == (K, R), (X.shape, table.shape, K, R)
    Y = _rows((R, C), X, r_dev)
    _lib.check(lib.wfs_maxpool_fwd(_lib.ptr(table), kmap, K, R, _lib.ptr(X), X.shape[0], C, _lib.ptr(Y),
                                   _lib.dtype_code(X), _lib.ptr(r_dev), _lib.stream_ptr()))
    _account("maxpool_fwd", table, R, X.shape[0], C, R, C, K, 0, 0, X.element_size())
    return Y


def maxpool_bwd(table, K, packed_kl, N, X, Y, dY, n_dev=None):
    """dX[j] = sum_k (X[j] == Y[o]) ? dY[o] : 0 with o = table[k, j] through the by-input table, dense or packed
    (include/wfsparse.h wfs_maxpool_bwd)."""
    lib = _lib.load()
    C = int(X.shape[1])
    assert X.shape[0] == N and Y.shape == dY.shape and Y.shape[1] == C and X.dtype == Y.dtype == dY.dtype
    assert table.dtype == torch.int32 and table.shape == ((K // packed_kl if packed_kl else K), N), (table.shape, K, N)
    dX = _rows((N, C), X, n_dev)
    _lib.check(lib.wfs_maxpool_bwd(_lib.ptr(table), K, packed_kl, N, _lib.ptr(X), _lib.ptr(Y), _lib.ptr(dY), Y.shape[0], C,
                                   _lib.ptr(dX), _lib.dtype_code(X), _lib.ptr(n_dev), _lib.stream_ptr()))
    if ACCOUNT is not None:
        # X read and dX written once each; Y and dY once each; the rulebook at 8 bytes per pair
        pairs = int(((table >> 3).clamp_(min=-1) if packed_kl else table).ge(0).sum().item())
        ACCOUNT.append(dict(kind="maxpool_bwd", pairs=pairs, flops=0,
                            bytes=(2 * N + 2 * Y.shape[0]) * C * X.element_size() + pairs * 8))
    return dX


class SparseMaxPoolFunction(Function):
    """features [n_in, C] -> [n_out, C]: spconv's indice_maxpool over a rulebook (csrc/pool.hip).  No parameters."""

    @staticmethod
    def forward(ctx, features, rulebook):
        rb = rulebook
        features = _features_ok(features)
        if rb.has_dup:
            raise RuntimeError("waveformml_amd.spconv: SparseMaxPool needs distinct input coordinates")
        assert features.shape[0] == rb.N
        table, kmap = rb.table_by_out()
        out = maxpool_fwd(table, kmap, rb.K, rb.M, features, rb.m_dev)
        ctx.save_for_backward(features, out)
        ctx.rb = rb
        return out

    @staticmethod
    def backward(ctx, grad_output):
        features, out = ctx.saved_tensors
        rb = ctx.rb
        if not ctx.needs_input_grad[0]:
            return None, None
        dY = as_grad(grad_output, features.dtype)
        table, pk = rb.nbr_out_packed, rb.packed_kl
        if table is None or not _lib.load().wfs_maxpool_packed_ok(pk, rb.K, int(features.shape[1]), _lib.dtype_code(features)):
            table, pk = rb.nbr_out, 0
        return maxpool_bwd(table, rb.K, pk, rb.N, features, out, dY, rb.n_dev), None


def indice_maxpool(features, rulebook):
    return SparseMaxPoolFunction.apply(features, rulebook)


class PointwiseConvFunction(Function):
    """1 x 1 convolution with >= 128 channels on a side: Y = X . W (+ bias) on the matrix cores of
    csrc/wide.hip instead of spconv's ``torch.mm(features, weight.view(in, out))`` (spconv 1.2.1 conv.py; the hybrid
    net's 2048 -> 1697 layer, reference src/models/SPConvBlocks.py:498)."""

    @staticmethod
    def forward(ctx, features, filters, bias, n_dev):
        features = _features_ok(features)
        R = int(features.shape[0])
        W = filters.detach().reshape(1, filters.shape[-2], filters.shape[-1]).float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        w16 = filters16(W, features) if takes_wide_path(1, R, features, W.shape[2]) else None
        out = gather_conv(None, None, 1, 0, R, features, W, False, b, n_dev, w16)
        ctx.save_for_backward(features, filters, bias)
        ctx.n_dev = n_dev
        ctx.w16 = w16 if ctx.needs_input_grad[0] else None
        return out

    @staticmethod
    def backward(ctx, grad_output):
        features, filters, bias = ctx.saved_tensors
        n_dev = ctx.n_dev
        R = int(features.shape[0])
        dY = as_grad(grad_output, features.dtype)
        W = filters.detach().reshape(1, filters.shape[-2], filters.shape[-1]).float().contiguous()
        dX = dW = db = None
        if ctx.needs_input_grad[1]:
            dW = gather_dw(None, 1, 0, R, features, dY, False, None, n_dev, filters)
            dW = dW.reshape(filters.shape).to(filters.dtype)
        if ctx.needs_input_grad[0]:
            dX = gather_conv(None, None, 1, 0, R, dY, W, True, None, n_dev, ctx.w16)
        if bias is not None and ctx.needs_input_grad[2]:
            db = _masked_column_sum(dY, n_dev).to(bias.dtype)
        return dX, dW, db, None


def pointwise_conv(features, filters, bias, n_dev=None):
    return PointwiseConvFunction.apply(features, filters, bias, n_dev)


def _dense_map_ok(cell_map, spatial, batch_size, C, features):
    """Shapes wfs_to_dense_mapped covers, and the map must be of THIS dense shape."""
    v = 1
    for s_ in spatial:
        v *= int(s_)
    pack = 1 if features.dtype == torch.float32 else 2
    return (cell_map[3] == v and v % pack == 0 and C % 4 == 0 and 4 <= C <= 128 and 1 <= batch_size <= 65535
            and features.shape[0] > 0)


class ToDenseFunction(Function):
    """SparseConvTensor.dense(): [M, C] -> [B, C, *spatial] (A.1)."""

    @staticmethod
    def forward(ctx, features, indices, spatial_shape, batch_size, unique, m_dev=None, cell_map=None):
        lib = _lib.load()
        features = _features_ok(features)
        indices = indices.contiguous()
        M, C = features.shape
        ndim = indices.shape[1] - 1
        spatial = [int(s) for s in spatial_shape]
        ctx.cell_map = None
        if cell_map is not None and unique and _dense_map_ok(cell_map, spatial, int(batch_size), C, features):
            # the producing conv's cell -> row map: every cell written once, no zero fill, whole runs per channel
            ticket, slot, _keep, V = cell_map
            out = torch.empty([int(batch_size), C] + spatial, dtype=features.dtype, device=features.device)
            _lib.check(lib.wfs_to_dense_mapped(_lib.ptr(features), ticket, slot, M, _lib.ptr(m_dev), int(batch_size), V,
                                               C, _lib.ptr(out), _lib.dtype_code(features), _lib.stream_ptr()))
            ctx.cell_map = cell_map
            ctx.meta = (spatial, int(batch_size), M, C)
            ctx.m_dev = m_dev
            ctx.like = (features.dtype, features.device)
            return out
        out = torch.zeros([int(batch_size), C] + spatial, dtype=features.dtype, device=features.device)
        winner = None
        if not unique:
            cells = int(batch_size)
            for s in spatial:
                cells *= s
            winner = torch.empty((cells,), dtype=torch.int32, device=features.device)
        _lib.check(lib.wfs_to_dense(_lib.ptr(features), _lib.ptr(indices), M, ndim, _lib.i32_array(spatial),
                                    int(batch_size), C, _lib.ptr(out), _lib.ptr(winner), _lib.dtype_code(features),
                                    _lib.ptr(m_dev), _lib.stream_ptr()))
        ctx.save_for_backward(indices)
        ctx.meta = (spatial, int(batch_size), M, C)
        ctx.m_dev = m_dev
        return out

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        spatial, batch_size, M, C = ctx.meta
        if ctx.cell_map is not None:
            ticket, slot, _keep, V = ctx.cell_map
            dtype, device = ctx.like
            dY = as_grad(grad_output, dtype)
            dX = torch.empty((M, C), dtype=dtype, device=device)     # every valid row has exactly one cell
            _lib.check(lib.wfs_to_dense_bwd_mapped(_lib.ptr(dY), ticket, slot, M, _lib.ptr(ctx.m_dev), batch_size, V, C,
                                                   _lib.ptr(dX), _lib.dtype_code(dX), _lib.stream_ptr()))
            return dX, None, None, None, None, None, None
        (indices,) = ctx.saved_tensors
        dY = grad_output.contiguous()
        dX = _rows((M, C), dY, ctx.m_dev)
        _lib.check(lib.wfs_to_dense_bwd(_lib.ptr(dY), _lib.ptr(indices), M, len(spatial), _lib.i32_array(spatial),
                                        batch_size, C, _lib.ptr(dX), _lib.dtype_code(dY), _lib.ptr(ctx.m_dev),
                                        _lib.stream_ptr()))
        return dX, None, None, None, None, None, None


def _bn_relu_forward(x, weight, bias, running_mean, running_var, momentum, eps, training, relu, n_dev, batches_tracked):
    """(y, save_mean, save_invstd) of y = [relu](BatchNorm1d(x)) over the active rows: the two forward launches."""
    lib = _lib.load()
    N, C = x.shape
    y = _rows(tuple(x.shape), x, n_dev)
    for t in (weight, bias, running_mean, running_var):
        assert t is None or (t.dtype == torch.float32 and t.numel() == C and t.is_contiguous())
    save_mean = torch.empty((C,), dtype=torch.float32, device=x.device)
    save_invstd = torch.empty((C,), dtype=torch.float32, device=x.device)
    ws = torch.empty((max(int(lib.wfs_bn_workspace_bytes(N, C)), 1),), dtype=torch.uint8, device=x.device)
    _lib.check(lib.wfs_bn_relu_fwd(_lib.ptr(x), N, C, _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(running_mean),
                                   _lib.ptr(running_var), _lib.ptr(batches_tracked) if training else None,
                                   float(momentum), float(eps), 1 if training else 0,
                                   1 if relu else 0, _lib.ptr(y), _lib.ptr(save_mean), _lib.ptr(save_invstd),
                                   _lib.ptr(ws), ws.numel(), _lib.dtype_code(x), _lib.ptr(n_dev),
                                   _lib.stream_ptr()))
    return y, save_mean, save_invstd


class BatchNormReLUFunction(Function):
    """nn.BatchNorm1d (+ nn.ReLU) over the active rows [N, C] in two launches per direction
    (reference: the plain modules inside spconv.SparseSequential, src/models/SPConvBlocks.py:505-508)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, training, relu, n_dev=None,
                batches_tracked=None):
        x = _features_ok(x)
        y, save_mean, save_invstd = _bn_relu_forward(x, weight, bias, running_mean, running_var, momentum, eps, training,
                                                     relu, n_dev, batches_tracked)
        ctx.save_for_backward(x, weight, bias, save_mean, save_invstd)
        ctx.flags = (bool(training), bool(relu))
        ctx.n_dev = n_dev
        return y

    @staticmethod
    def backward(ctx, grad_output):
        x, weight, bias, save_mean, save_invstd = ctx.saved_tensors
        training, relu = ctx.flags
        dx, dgamma, dbeta = bn_relu_backward(x, grad_output, weight, bias, save_mean, save_invstd, training, relu, ctx.n_dev)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


def bn_relu_backward(x, grad_output, weight, bias, save_mean, save_invstd, training, relu, n_dev):
    """(dx, dgamma, dbeta) of y = [relu](BatchNorm1d(x)) over the active rows, given dL/dy (two launches: the sums
    sum(g), sum(g * xhat) with the ReLU mask recomputed from x, then the elementwise pass)."""
    lib = _lib.load()
    N, C = x.shape
    dy = as_grad(grad_output, x.dtype)
    dx = _rows(tuple(x.shape), x, n_dev)
    dgamma = grad_like(weight) if weight is not None else None
    dbeta = grad_like(bias) if bias is not None else None
    ws = torch.empty((max(int(lib.wfs_bn_workspace_bytes(N, C)), 1),), dtype=torch.uint8, device=x.device)
    _lib.check(lib.wfs_bn_relu_bwd(_lib.ptr(x), _lib.ptr(dy), N, C, _lib.ptr(weight), _lib.ptr(bias),
                                   _lib.ptr(save_mean), _lib.ptr(save_invstd), 1 if training else 0,
                                   1 if relu else 0, _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws),
                                   ws.numel(), _lib.dtype_code(x), _lib.ptr(n_dev), _lib.stream_ptr()))
    return dx, dgamma, dbeta


def batch_norm_relu(features, bn, relu, n_dev=None):
    """Apply an nn.BatchNorm1d module (and optionally the nn.ReLU that follows it) to [N, C] features
    (``n_dev``: device-side count of valid rows, see include/wfsparse.h "device-side row counts")."""
    training = bn.training or (bn.running_mean is None and bn.running_var is None)
    tracked = bn.num_batches_tracked if (bn.training and bn.track_running_stats) else None   # bumped by the kernel
    return BatchNormReLUFunction.apply(
        features, bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
        bn.running_var if bn.track_running_stats else None, bn.momentum, bn.eps, training, relu, n_dev, tracked)


def can_fuse_batch_norm(bn, features):
    """The fused kernels cover what the reference's nets use: float32 parameters, a fixed momentum,
    fp32 / bf16 / fp16 features on the GPU, any channel count (beyond what one block covers -- 1024 channels, or 256
    when C is not a multiple of 4; the hybrid net starts at 2 T = 2048 -- the library runs channel slices)."""
    c = bn.num_features
    return (type(bn) is torch.nn.BatchNorm1d and bn.momentum is not None and features.is_cuda and features.dim() == 2
            and features.dtype in (torch.float32, torch.bfloat16, torch.float16) and features.shape[0] > 0
            and 1 <= c <= 65536
            and (bn.weight is None or bn.weight.dtype == torch.float32)
            and (bn.training or bn.running_mean is not None))


def first_conv_bn_backward(table, kmap, K, identity_k, R, z, dY, features, gamma, beta, save_mean, save_invstd, relu,
                           r_dev, filters):
    """(dW [K, 2, 32], dgamma, dbeta) of y = [relu](BatchNorm1d(z)), z = the first conv (2 -> 32, no bias) of the network
    input ``features``, from dL/dy in two launches and without a dz tensor (include/wfsparse.h
    wfs_first_conv_bn_backward): the bits of bn_relu_backward + gather_dw.  The gradients go straight into their slots
    of a registered flat gradient buffer; dW's slab reduction joins the pass's deferred ones as gather_dw's does."""
    lib = _lib.load()
    dW = grad_like(filters, (K, 2, 32)) if filters.numel() == K * 64 else torch.empty((K, 2, 32), dtype=torch.float32,
                                                                                      device=z.device)
    dgamma = grad_like(gamma) if gamma is not None else None
    dbeta = grad_like(beta) if beta is not None else None
    assert z.dtype == dY.dtype == features.dtype and z.shape == dY.shape == (R, 32) and features.shape[1] == 2
    assert table.dtype == torch.int32 and table.shape == (K, R)
    ws = torch.empty((int(lib.wfs_first_conv_bn_backward_workspace_bytes(K, R)),), dtype=torch.uint8, device=z.device)
    job = _dw_job(dW)
    _lib.check(lib.wfs_first_conv_bn_backward(_lib.ptr(table), kmap, K, identity_k, R, _lib.ptr(z), _lib.ptr(dY),
                                              _lib.ptr(features), features.shape[0], _lib.ptr(gamma), _lib.ptr(beta),
                                              _lib.ptr(save_mean), _lib.ptr(save_invstd), 1 if relu else 0, _lib.ptr(dW),
                                              _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.dtype_code(z), _lib.ptr(ws),
                                              ws.numel(), _lib.ptr(r_dev), job, _lib.stream_ptr()))
    _queue_dw_job(job, ws)
    if ACCOUNT is not None:
        _account("gather_dw", table, R, R, 32, features.shape[0], 2, K, 32, 2, z.element_size())
    return dW, dgamma, dbeta


def first_conv_bn_ok(features, filters, conv_bias, rulebook, bn):
    """Does FirstConvBNFunction cover this conv + BatchNorm pair?  2 -> 32 channels, K <= 27, distinct outputs, no conv
    bias, 16-bit rows that need no gradient (the network input), BatchNorm normalising with batch statistics."""
    rb = rulebook
    return bool(features.is_cuda and features.dim() == 2 and features.shape[1] == 2 and filters.shape[-2] == 2
                and filters.shape[-1] == 32 and filters.dtype == torch.float32 and rb.K <= 27 and not rb.has_dup
                and conv_bias is None and features.dtype in (torch.bfloat16, torch.float16)
                and not features.requires_grad and bn.num_features == 32 and features.shape[0] > 0 and rb.M > 0
                and (bn.training or (bn.running_mean is None and bn.running_var is None))
                and type(bn) is torch.nn.BatchNorm1d and bn.momentum is not None
                and (bn.weight is None or bn.weight.dtype == torch.float32))


class FirstConvBNFunction(Function):
    """First conv (2 -> 32, no bias) + nn.BatchNorm1d (+ nn.ReLU) of a sparse stack as one autograd node.  The forward
    launches are those of SparseConvFunction and BatchNormReLUFunction, in their order (``between`` runs after the conv:
    SparseSequential forks its rulebook prefetch there); the backward (first_conv_bn_backward) has the BatchNorm
    backward's elementwise pass inside the dW kernel: one launch and the dz tensor fewer, the same gradients bit for
    bit."""

    @staticmethod
    def forward(ctx, features, filters, weight, bias, running_mean, running_var, momentum, eps, relu, rulebook,
                batches_tracked, between):
        rb = rulebook
        features = _features_ok(features)
        K = rb.K
        W = filters.detach().reshape(K, 2, 32).float().contiguous()
        ident = rb.centre_k if rb.subm else -1
        assert features.shape[0] == rb.N
        table, kmap = rb.table_by_out()
        z = gather_conv(table, kmap, K, ident, rb.M, features, W, False, None, rb.m_dev, None)
        if between is not None:
            between()
        y, save_mean, save_invstd = _bn_relu_forward(z, weight, bias, running_mean, running_var, momentum, eps, True,
                                                     relu, rb.m_dev, batches_tracked)
        ctx.save_for_backward(features, filters, weight, bias, z, save_mean, save_invstd)
        ctx.rb, ctx.relu = rb, bool(relu)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        features, filters, weight, bias, z, save_mean, save_invstd = ctx.saved_tensors
        rb = ctx.rb
        dY = as_grad(grad_output, z.dtype)
        table, kmap = rb.table_by_out()
        dW, dgamma, dbeta = first_conv_bn_backward(table, kmap, rb.K, rb.centre_k if rb.subm else -1, rb.M, z, dY,
                                                   features, weight, bias, save_mean, save_invstd, ctx.relu, rb.m_dev,
                                                   filters)
        dW = dW.reshape(filters.shape).to(filters.dtype)
        return (None, dW if ctx.needs_input_grad[1] else None, dgamma if ctx.needs_input_grad[2] else None,
                dbeta if ctx.needs_input_grad[3] else None, None, None, None, None, None, None, None, None)


def first_conv_bn_relu(features, filters, rulebook, bn, relu, between=None):
    """conv (filters, no bias) -> ``bn`` [-> ReLU] over a rulebook first_conv_bn_ok() accepted."""
    tracked = bn.num_batches_tracked if (bn.training and bn.track_running_stats) else None
    return FirstConvBNFunction.apply(
        features, filters, bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
        bn.running_var if bn.track_running_stats else None, bn.momentum, bn.eps, relu, rulebook, tracked, between)


class SkinnyLinearFunction(Function):
    """nn.Linear with a handful of outputs over a long input row (the PSD head: [B, 35840] -> [B, 3]):
    Y = X W^T + b with X fp32/bf16, W/b/Y fp32 (reference src/models/SPConvNet.py:67-68)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        x = _features_ok(x)
        B, I = x.shape
        O = weight.shape[0]
        w = weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        y = torch.empty((B, O), dtype=torch.float32, device=x.device)
        _lib.check(lib.wfs_head_fwd(_lib.ptr(x), B, I, _lib.ptr(w), _lib.ptr(b), O, _lib.ptr(y), _lib.dtype_code(x),
                                    _lib.stream_ptr()))
        ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        x, weight, bias = ctx.saved_tensors
        B, I = x.shape
        O = weight.shape[0]
        g = grad_output.float().contiguous()
        w = weight.detach().float().contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = grad_like(weight, (O, I)) if ctx.needs_input_grad[1] else None
        ws = torch.empty((max(int(lib.wfs_head_workspace_bytes(B, I, O)), 1),), dtype=torch.uint8, device=x.device)
        want_db = bias is not None and ctx.needs_input_grad[2]
        db = grad_like(bias, (O,)) if (want_db and dw is not None) else None
        job = _dw_job(dw) if dx is not None else None           # deferred only when dx is wanted too
        _lib.check(lib.wfs_head_bwd(_lib.ptr(x), _lib.ptr(g), B, I, _lib.ptr(w), O, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                    _lib.dtype_code(x), _lib.ptr(ws), ws.numel(), job, _lib.stream_ptr()))
        _queue_dw_job(job, ws)          # the sum over the dW partials joins the pass's deferred reductions
        if want_db and db is None:
            db = g.sum(0)
        return dx, (dw.to(weight.dtype) if dw is not None else None), (db.to(bias.dtype) if db is not None else None)


class SparseHeadFunction(Function):
    """ToDense -> view(-1, n_linear) -> nn.Linear(n_linear, n_type) straight off the sparse rows (csrc/shead.hip;
    include/wfsparse.h wfs_sparse_head_fwd): features [M, C] of the last conv, its cell -> row map, fp32 weight
    [O, C * V] / bias [O] of the Linear -> logits [batch, O] fp32.  The dense [batch, C, *spatial] tensor never exists
    (reference src/models/SPConvNet.py:65-68)."""

    @staticmethod
    def forward(ctx, features, weight, bias, cell_map, batch_size, m_dev):
        lib = _lib.load()
        features = _features_ok(features)
        M, C = features.shape
        ticket, slot, _keep, V = cell_map
        O = int(weight.shape[0])
        w = weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        y = torch.empty((int(batch_size), O), dtype=torch.float32, device=features.device)
        ws = torch.empty((int(lib.wfs_sparse_head_workspace_bytes(int(batch_size), V, C, O)),), dtype=torch.uint8,
                         device=features.device)
        _lib.check(lib.wfs_sparse_head_fwd(_lib.ptr(features), ticket, slot, M, _lib.ptr(m_dev), int(batch_size), V, C,
                                           _lib.ptr(w), _lib.ptr(b), O, _lib.ptr(y), _lib.dtype_code(features),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        ctx.save_for_backward(features, weight, bias)
        ctx.cell_map, ctx.batch_size, ctx.m_dev = cell_map, int(batch_size), m_dev
        return y

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        features, weight, bias = ctx.saved_tensors
        M, C = features.shape
        ticket, slot, _keep, V = ctx.cell_map
        O = int(weight.shape[0])
        g = grad_output.float().contiguous()
        w = weight.detach().float().contiguous()
        dx = _rows((M, C), features, ctx.m_dev) if ctx.needs_input_grad[0] else None
        dw = grad_like(weight, (O, C * V)) if ctx.needs_input_grad[1] else None
        want_db = bias is not None and ctx.needs_input_grad[2]
        db = grad_like(bias, (O,)) if (want_db and dw is not None) else None
        ws = torch.empty((int(lib.wfs_sparse_head_workspace_bytes(ctx.batch_size, V, C, O)),), dtype=torch.uint8,
                         device=features.device)
        job = _dw_job(dw)
        _lib.check(lib.wfs_sparse_head_bwd(_lib.ptr(features), _lib.ptr(g), ticket, slot, M, _lib.ptr(ctx.m_dev),
                                           ctx.batch_size, V, C, _lib.ptr(w), O, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                           _lib.dtype_code(features), _lib.ptr(ws), ws.numel(), job, _lib.stream_ptr()))
        _queue_dw_job(job, ws)          # the sum over the per-slice dW partials joins the deferred reductions
        if want_db and db is None:
            db = g.sum(0)
        return (dx, (dw.to(weight.dtype) if dw is not None else None), (db.to(bias.dtype) if db is not None else None),
                None, None, None)


# WFS_SPARSE_HEAD=0: the dense route (dense() + the streaming head kernels)
SPARSE_HEAD = __import__("os").environ.get("WFS_SPARSE_HEAD", "1") != "0"


def can_use_sparse_head(x, layers):
    """x: the SparseConvTensor in front of a trailing ToDense; layers: the Linear stack behind the flatten."""
    if not SPARSE_HEAD or len(layers) != 1 or type(layers[0]) is not torch.nn.Linear:
        return False
    lin, f = layers[0], x.features
    cm = getattr(x, "cell_map", None)
    if cm is None or not f.is_cuda or f.dim() != 2 or f.shape[0] == 0 or lin.weight.dtype != torch.float32:
        return False
    if not (x.unique is True or x.n_valid is not None):
        return False
    V = 1
    for s_ in x.spatial_shape:
        V *= int(s_)
    C = int(f.shape[1])
    return bool(cm[3] == V and lin.in_features == C * V and f.dtype in (torch.float32, torch.bfloat16, torch.float16)
                and _lib.load().wfs_sparse_head_ok(int(x.batch_size), V, C, int(lin.out_features), _lib.dtype_code(f)))


def sparse_head(x, linear):
    return SparseHeadFunction.apply(x.features, linear.weight, linear.bias, x.cell_map, x.batch_size, x.n_valid)


def can_use_skinny_linear(linear, x):
    # long rows (I % 8 == 0, >= 1024: streamed) or short ones of any length (<= 4096: scalar kernels)
    return (type(linear) is torch.nn.Linear and x.is_cuda and x.dim() == 2 and linear.out_features <= 8
            and ((x.shape[1] % 8 == 0 and x.shape[1] >= 1024) or x.shape[1] <= 4096)
            and x.dtype in (torch.float32, torch.bfloat16, torch.float16) and linear.weight.dtype == torch.float32)


def skinny_linear(x, linear):
    return SkinnyLinearFunction.apply(x, linear.weight, linear.bias)


class WideLinearFunction(Function):
    """nn.Linear with many outputs on activations [B, I]: y = x W^T + b on the matrix cores (csrc/wide.hip;
    include/wfsparse.h wfs_wide_linear_fwd): 16-bit activations with the fp32 weights rounded to their type as
    operands, or fp32 activations on the exact-fp32 MFMA; fp32 accumulate, fp32 result -- the hybrid net's
    Linear(24150, 269) (reference src/models/SPConvNet.py:40-52)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        x = _features_ok(x)
        B, I = x.shape
        O = weight.shape[0]
        w = weight.detach().float().contiguous()
        b = None if bias is None else bias.detach().float().contiguous()
        y = torch.empty((B, O), dtype=torch.float32, device=x.device)
        ws = torch.empty((int(lib.wfs_wide_linear_workspace_bytes(B, I, O, _lib.dtype_code(x))),), dtype=torch.uint8, device=x.device)
        _lib.check(lib.wfs_wide_linear_fwd(_lib.ptr(x), B, I, _lib.ptr(w), _lib.ptr(b), O, _lib.ptr(y), _lib.dtype_code(x),
                                        _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        lib = _lib.load()
        x, weight, bias = ctx.saved_tensors
        B, I = x.shape
        O = weight.shape[0]
        g = grad_output.float().contiguous()
        w = weight.detach().float().contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = grad_like(weight, (O, I)) if ctx.needs_input_grad[1] else None
        db = _masked_column_sum(g, None) if (bias is not None and ctx.needs_input_grad[2]) else None
        ws = torch.empty((int(lib.wfs_wide_linear_workspace_bytes(B, I, O, _lib.dtype_code(x))),), dtype=torch.uint8, device=x.device)
        _lib.check(lib.wfs_wide_linear_bwd(_lib.ptr(x), _lib.ptr(g), B, I, _lib.ptr(w), O, _lib.ptr(dx), _lib.ptr(dw),
                                        None, _lib.dtype_code(x), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        return dx, (dw.to(weight.dtype) if dw is not None else None), (db.to(bias.dtype) if db is not None else None)


def can_use_wide_linear(linear, x):
    return bool(type(linear) is torch.nn.Linear and x.is_cuda and x.dim() == 2 and x.shape[0] > 0
                and x.dtype in (torch.float32, torch.bfloat16, torch.float16) and linear.weight.dtype == torch.float32
                and _lib.load().wfs_wide_linear_ok(x.shape[0], x.shape[1], linear.out_features, _lib.dtype_code(x)))


def wide_linear(x, linear):
    return WideLinearFunction.apply(x, linear.weight, linear.bias)


def head_forward(x, layers):
    """The dense head (reference src/models/SPConvNet.py:40-52: a Sequential of nn.Linear built by LinearBlock) on
    the flattened ToDense output: few-output layers on streamed 16-bit / fp32 rows (skinny_linear), wide layers of
    16-bit rows on the matrix cores (wide_linear), anything else as the torch module in the head's own dtype."""
    for layer in layers:
        if can_use_skinny_linear(layer, x):
            x = skinny_linear(x, layer)
        elif can_use_wide_linear(layer, x):
            x = wide_linear(x, layer)
        else:
            p = next(layer.parameters(), None)
            if p is not None and x.dtype != p.dtype:          # 16-bit activations, fp32 master weights
                x = x.to(p.dtype)
            x = layer(x)
    return x


class CrossEntropyMeanFunction(Function):
    """nn.CrossEntropyLoss(reduction='mean') on [B, C] fp32 logits: loss and d loss / d logits from one launch
    (reference criterion: src/engineering/LitBase.py:38-43, applied at LitPSD.py:102)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        lib = _lib.load()
        logits = _features_ok(logits)
        target = target.contiguous()
        B, C = logits.shape
        loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        _lib.check(lib.wfs_xent_mean_fwd_bwd(_lib.ptr(logits), _lib.ptr(target), B, C, int(ignore_index),
                                             _lib.ptr(loss), _lib.ptr(dlogits), _lib.stream_ptr()))
        ctx.dlogits = dlogits
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        unit = _UNIT_LOSS_GRAD.get(grad_output.device)
        if unit is not None and grad_output.data_ptr() == unit.data_ptr():
            return ctx.dlogits, None, None            # d loss / d loss = 1, handed in by unit_loss_grad(): no multiply
        return ctx.dlogits * grad_output, None, None


# zero-initialised workspaces of the two fused regression losses (the fold of csrc/wfs_lossfold.h), one per device and size:
# the kernel's ticket word must be 0 before the first launch and every launch leaves it 0, so a buffer is zeroed once and
# reused (a captured step bakes its address into the graph; the entry is never freed).  One stream at a time per device, as
# everything in this module.
_LOSS_WORKSPACE = {}


def reset_regression_loss_workspaces():
    """Zero every cached workspace of the masked regression loss and of the segment map loss (after a failed or
    abandoned launch)."""
    for work in _LOSS_WORKSPACE.values():
        work.zero_()


def _coords_ok(coords, n_cap):
    return coords is not None and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 3 and \
        coords.shape[0] == n_cap


def _loss_checks(name, tensors, shapes, target, n_cap, se_mask, mask_shape, n_valid):
    """The argument checks of the two fused losses, in the order both had them: ``tensors`` on the GPU, the loss's own
    ``shapes`` -- (ok, text) pairs, the first with ``target`` [N] or [N, n_cols] -- the mask as a contiguous float32
    [nx, ny] (of ``mask_shape`` when that is given) and ``n_valid`` a device int64.  Returns ``(n_cols, se_mask)``."""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("waveformml_amd: tensor must live on the GPU (there is no CPU path); got %s" % t.device)
    target_ok = target.dim() in (1, 2) and target.shape[0] == n_cap
    for k, (ok, text) in enumerate(shapes):
        if not (ok and (k > 0 or target_ok)):
            raise RuntimeError("%s: %s" % (name, text))
    if se_mask is not None:
        se_mask = se_mask.reshape(se_mask.shape[-2:]).contiguous()
        if se_mask.dtype != torch.float32 or (mask_shape is not None and tuple(se_mask.shape) != mask_shape):
            raise RuntimeError("%s: the mask must be float32%s" % (name, " [%d, %d]" % mask_shape if mask_shape else ""))
    if n_valid is not None and (n_valid.dtype != torch.int64 or not n_valid.is_cuda):
        raise RuntimeError("%s: n_valid must be a device int64" % name)
    return (int(target.shape[1]) if target.dim() == 2 else 1), se_mask


def _loss_buffers(device, nbytes, n_out):
    """The cached zeroed workspace of ``nbytes`` with its size, and fresh ``out`` fp32 [n_out] and ``count`` int64 [1]."""
    key = (device, nbytes)
    if key not in _LOSS_WORKSPACE:
        _LOSS_WORKSPACE[key] = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)
    return (_LOSS_WORKSPACE[key], nbytes, torch.empty((n_out,), dtype=torch.float32, device=device),
            torch.empty((1,), dtype=torch.int64, device=device))


def _loss_grad(grad):
    return (grad if grad.dtype == torch.float32 else grad.float()).contiguous()


def _loss_kind(criterion, reduction):
    if getattr(criterion, "reduction", None) != reduction:
        return None
    if type(criterion) is torch.nn.L1Loss:
        return _lib.WFS_LOSS_L1
    if type(criterion) is torch.nn.MSELoss:
        return _lib.WFS_LOSS_MSE
    return None


class MaskedRegressionLossFunction(Function):
    """Mean-reduced nn.L1Loss / nn.MSELoss of ``pred`` [N] against ``target`` [N] or column ``col`` of ``target``
    [N, n_cols] over the rows below ``n_valid`` that lie on a single-ended segment (``se_mask`` [nx, ny] == 1.0 at the
    row's (x, y)): the reference's ``criterion(predictions[se_inds], target[se_inds, target_index])``
    (src/engineering/LitSegQuantifier.py) with a static shape.  One HIP launch forward, one backward (csrc/segloss.hip);
    returns ``(loss, mse)``, fp32 scalars, ``mse`` = the mean of d^2 over the same rows whatever the kind (no gradient).
    Rows that are not counted are selected out: whatever they hold, the loss stays finite and their gradient is 0.

    Precondition: ONE stream at a time per device.  The forward's workgroups hand over through a ticket word in a
    workspace that is cached per (device, size), zeroed once and left zero by every completed launch; ``loss``, ``mse``
    and the count are written by the workgroup that draws the last ticket.  Two forwards of the same size running at
    once on different streams, or a launch that was cut short, leave the ticket off zero, and the outputs of later
    calls of that size are then never written (they are ``torch.empty``: a fill would be a second launch).  A process
    that met a failed launch calls ``reset_regression_loss_workspaces()`` before it goes on."""

    @staticmethod
    def forward(ctx, pred, target, col, coords, se_mask, n_valid, kind, max_blocks=0):
        lib = _lib.load()
        n_cap = int(pred.shape[0])
        n_cols, mask = _loss_checks(
            "masked_regression_loss", (pred, target),
            ((pred.dim() == 1, "pred must be [N] and target [N] or [N, n_cols], got %s and %s"
              % (tuple(pred.shape), tuple(target.shape))),
             (se_mask is None or _coords_ok(coords, n_cap), "a mask needs coords int32 [N, 3] = (x, y, event)")),
            target, n_cap, se_mask, None, n_valid)
        pred, target = pred.contiguous(), target.contiguous()
        col = int(col) if target.dim() == 2 else 0
        nx = ny = 0
        if mask is not None:
            nx, ny = int(mask.shape[0]), int(mask.shape[1])
        coords = coords.contiguous() if mask is not None else None
        work, nbytes, out, count = _loss_buffers(pred.device, int(lib.wfs_masked_regression_loss_workspace_bytes(n_cap)), 2)
        p = _lib.ptr
        _lib.check(lib.wfs_masked_regression_loss(
            p(pred), _lib.dtype_code(pred), p(target), _lib.dtype_code(target), n_cols, col, p(coords), p(mask), nx, ny,
            n_cap, p(n_valid), int(kind), int(max_blocks), p(work), nbytes, p(out), p(count), _lib.stream_ptr()))
        ctx.save_for_backward(pred, target, coords, mask, n_valid, count)
        ctx.args = (n_cols, col, nx, ny, n_cap, int(kind))
        loss, mse = out[0], out[1]
        ctx.mark_non_differentiable(mse)
        return loss, mse

    @staticmethod
    def backward(ctx, grad_loss, _grad_mse):
        pred, target, coords, se_mask, n_valid, count = ctx.saved_tensors
        n_cols, col, nx, ny, n_cap, kind = ctx.args
        dpred = torch.empty_like(pred)
        p = _lib.ptr
        _lib.check(_lib.load().wfs_masked_regression_loss_backward(
            p(pred), _lib.dtype_code(pred), p(target), _lib.dtype_code(target), n_cols, col, p(coords), p(se_mask), nx, ny,
            n_cap, p(n_valid), kind, p(count), p(_loss_grad(grad_loss)), p(dpred), _lib.stream_ptr()))
        return dpred, None, None, None, None, None, None, None


def regression_loss_kind(criterion):
    """WFS_LOSS_L1 / WFS_LOSS_MSE for a mean-reduced nn.L1Loss / nn.MSELoss, else None."""
    return _loss_kind(criterion, "mean")


def can_fuse_regression_loss(criterion, pred, target):
    return (regression_loss_kind(criterion) is not None and pred.is_cuda and target.is_cuda and pred.dim() == 1
            and target.dim() in (1, 2) and target.shape[0] == pred.shape[0]
            and pred.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and target.dtype in (torch.float32, torch.bfloat16, torch.float16))


def masked_regression_loss(pred, target, kind, col=0, coords=None, se_mask=None, n_valid=None, max_blocks=0):
    """``(loss, mse)`` of ``MaskedRegressionLossFunction``; ``kind`` from ``regression_loss_kind``."""
    return MaskedRegressionLossFunction.apply(pred, target, col, coords, se_mask, n_valid, kind, max_blocks)


class SegmentMapLossFunction(Function):
    """The segment loss of LitZ / LitEZ (reference LitBase._calc_segment_loss, LitBase.py:124-174) without its dense
    target and mask maps: ``map`` [B, planes, nx, ny] is scored at the ACTIVE segments only, plane ``p`` against column
    ``cols[p]`` of ``target`` [N] or [N, n_cols], over the rows below ``n_valid`` whose (x, y, event) lies inside the map
    and (with ``se_mask``) on a single-ended segment: the sum of |d| / d^2 over those rows divided by their number.  One
    HIP launch forward, one backward that writes the whole gradient map (csrc/segloss.hip).  Returns
    ``(total, per_plane)``: ``total`` a 0-dim fp32 scalar, the sum of the per-plane losses and the only differentiable
    output; ``per_plane`` [planes] (LitEZ's ZLoss, ELoss).  Rows that are not counted, and map cells without a counted
    row, are selected out: whatever they hold the loss stays finite and their gradient is exactly 0.

    The workspace scheme and the ONE-stream precondition are MaskedRegressionLossFunction's."""

    @staticmethod
    def forward(ctx, map, coords, target, cols, kind, se_mask=None, n_valid=None, max_blocks=0):
        lib = _lib.load()
        n_cap = int(coords.shape[0])
        n_cols, se_mask = _loss_checks(
            "segment_map_loss", (map, coords, target),
            ((map.dim() == 4 and _coords_ok(coords, n_cap),
              "map must be [B, planes, nx, ny], coords int32 [N, 3] = (x, y, event) and target [N] or [N, n_cols], got "
              "%s, %s %s and %s" % (tuple(map.shape), coords.dtype, tuple(coords.shape), tuple(target.shape))),),
            target, n_cap, se_mask, tuple(map.shape[-2:]), n_valid)
        map, target, coords = map.contiguous(), target.contiguous(), coords.contiguous()
        B, planes, nx, ny = (int(v) for v in map.shape)
        cols = tuple(int(c) for c in cols)
        if len(cols) != planes:
            raise RuntimeError("segment_map_loss: %d planes need %d target columns, got %r" % (planes, planes, cols))
        work, nbytes, out, count = _loss_buffers(map.device, int(lib.wfs_segment_map_loss_workspace_bytes(n_cap, planes)),
                                                 planes + 1)
        p = _lib.ptr
        _lib.check(lib.wfs_segment_map_loss(
            p(map), _lib.dtype_code(map), B, planes, nx, ny, p(coords), p(target), _lib.dtype_code(target), n_cols,
            _lib.i32_array(cols), p(se_mask), n_cap, p(n_valid), int(kind), int(max_blocks), p(work), nbytes, p(out),
            p(count), _lib.stream_ptr()))
        ctx.save_for_backward(map, coords, target, se_mask, n_valid, count)
        ctx.args = (n_cols, cols, n_cap, int(kind))
        total, per_plane = out[planes], out[:planes]
        ctx.mark_non_differentiable(per_plane)
        ctx.set_materialize_grads(False)            # no zeros-fill for per_plane's gradient on the way back
        return total, per_plane

    @staticmethod
    def backward(ctx, grad_total, _grad_planes):
        if grad_total is None:
            return (None,) * 8
        map, coords, target, se_mask, n_valid, count = ctx.saved_tensors
        n_cols, cols, n_cap, kind = ctx.args
        B, planes, nx, ny = (int(v) for v in map.shape)
        dmap = torch.empty_like(map)
        p = _lib.ptr
        _lib.check(_lib.load().wfs_segment_map_loss_backward(
            p(map), _lib.dtype_code(map), B, planes, nx, ny, p(coords), p(target), _lib.dtype_code(target), n_cols,
            _lib.i32_array(cols), p(se_mask), n_cap, p(n_valid), kind, p(count), p(_loss_grad(grad_total)), p(dmap),
            _lib.stream_ptr()))
        return dmap, None, None, None, None, None, None, None


def segment_loss_kind(criterion):
    """WFS_LOSS_L1 / WFS_LOSS_MSE for a SUM-reduced plain nn.L1Loss / nn.MSELoss (what the segment modules build), else
    None."""
    return _loss_kind(criterion, "sum")


def segment_map_loss(map, coords, target, cols, kind, se_mask=None, n_valid=None, max_blocks=0):
    """``(total, per_plane)`` of ``SegmentMapLossFunction``; ``kind`` from ``segment_loss_kind``."""
    return SegmentMapLossFunction.apply(map, coords, target, cols, kind, se_mask, n_valid, max_blocks)


# ``loss.backward()`` makes autograd fill a fresh ones tensor for d loss / d loss (a launch) and the loss node multiply
# by it (another).  A runner that owns the backward call passes this persistent tensor instead:
#     torch.autograd.backward(loss, grad_tensors=unit_loss_grad(loss.device))
# and the fused cross-entropy recognises it (by address) and returns its gradient unscaled.
_UNIT_LOSS_GRAD = {}


def unit_loss_grad(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _UNIT_LOSS_GRAD:
        _UNIT_LOSS_GRAD[device] = torch.ones((), dtype=torch.float32, device=device)
    return _UNIT_LOSS_GRAD[device]


def can_fuse_cross_entropy(criterion, logits, target):
    return (type(criterion) is torch.nn.CrossEntropyLoss and criterion.reduction == "mean" and criterion.weight is None
            and getattr(criterion, "label_smoothing", 0.0) == 0.0 and logits.is_cuda and logits.dim() == 2
            and logits.dtype == torch.float32 and target.dtype == torch.int64 and target.dim() == 1
            and logits.shape[0] >= 1 and logits.shape[1] <= 4096)


def cross_entropy_mean(logits, target, ignore_index=-100):
    return CrossEntropyMeanFunction.apply(logits, target, ignore_index)


# 16-bit storage: bf16, and fp16 for the reference's ``half_precision`` / ``use_half`` (float16 features,
# src/datasets/HDF5Dataset.py:227-228).  Both have native kernels (fp32 accumulate, fp32 master filters).
def indice_conv(features, filters, bias, rulebook, images=None):
    return SparseConvFunction.apply(features, filters, bias, rulebook, CONV, images)


def indice_subm_conv(features, filters, bias, rulebook, images=None):
    return SparseConvFunction.apply(features, filters, bias, rulebook, SUBM, images)


def indice_inverse_conv(features, filters, bias, rulebook):
    return SparseConvFunction.apply(features, filters, bias, rulebook, INVERSE)


def to_dense(features, indices, spatial_shape, batch_size, unique, m_dev=None, cell_map=None):
    return ToDenseFunction.apply(features, indices, spatial_shape, batch_size, unique, m_dev, cell_map)
