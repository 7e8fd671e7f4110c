"""What the GPU evaluators share (evaluator, pid_evaluator, segment_evaluator, quantifier_evaluator, real_z_evaluator,
tensor_evaluator, metric_pairs): the argument checks of ``add``, the segment-status upload, the zero-filled per-row
buffers, and the one read-back of ``results()`` with the cursor that cuts it into named tables.
"""
import numpy as np
import torch

from .segments import segment_status

FIX_BITS = 32                   # the fixed-point image of a value: v = round(value * 2^32)
FIXED_ONE = float(1 << FIX_BITS)        # WFS_SEG_FIXED_ONE, include/wfsparse.h


def require_gpu(device, what):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("waveformml_amd: %s runs on the GPU (there is no CPU path); got %s" % (what, device))
    return device


_HOST_TENSOR = "waveformml_amd: tensor must live on the GPU (there is no CPU path); got %s"
_N_VALID = "%s: n_valid must be a device int64"


def require_device_tensors(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(_HOST_TENSOR % t.device)


def check_n_valid(n_valid, what):
    if n_valid is not None and (n_valid.dtype != torch.int64 or not n_valid.is_cuda):
        raise RuntimeError(_N_VALID % what)


def check_coords(c, n_valid, what):
    """``c`` a device int32 [N, 3] and ``n_valid`` None or a device int64: the two checks above without a call of
    their own, since every ``add`` passes here between its launches."""
    if not c.is_cuda:
        raise RuntimeError(_HOST_TENSOR % c.device)
    if c.dtype != torch.int32 or c.dim() != 2 or c.shape[1] != 3:
        raise RuntimeError("%s: coords must be int32 [N, 3] = (x, y, event)" % what)
    if n_valid is not None and (n_valid.dtype != torch.int64 or not n_valid.is_cuda):
        raise RuntimeError(_N_VALID % what)


def seg_status_tensor(device, seg_status, dead_pmts, nx, ny, text="seg_status must be [%d, %d]"):
    """The [nx, ny] float32 segment status on the device: the caller's, or the one ``dead_pmts`` gives.  ``text``: the
    message for a wrong shape, where an evaluator checks a second array under the same one."""
    s = segment_status(dead_pmts, nx, ny) if seg_status is None else np.asarray(seg_status, np.float32)
    if s.shape != (nx, ny):
        raise ValueError(text % (nx, ny))
    return torch.from_numpy(np.ascontiguousarray(s)).to(device)


def pid_field(additional_fields, index, what):
    """The PID column out of ``additional_fields``; its type is the caller's check, under the caller's text."""
    if additional_fields is None:
        raise RuntimeError("%s: additional_field_names holds \"PID\" but no additional fields came" % what)
    return additional_fields[index]


def raise_flags(name, flags, text):
    """Raise with the text of every bit of ``flags`` that ``text`` names; nothing with none set."""
    if flags:
        raise RuntimeError("%s: %s" % (name, "; ".join(t for b, t in text.items() if flags & b)))


def reserve_offsets(owner, events):
    """``owner._offsets`` (None at first), the event offsets of ``events + 1`` int32: allocated again only when the count
    changes."""
    off = owner._offsets
    if off is None or off.shape[0] != events + 1:
        off = owner._offsets = torch.zeros(events + 1, dtype=torch.int32, device=owner.device)
    return off


def reserve_rows(owner, rows, buffers, events=None):
    """Zero-filled per-batch buffers on ``owner.device``: allocated on the first call (``owner._rows_cap`` is -1 then) and
    again only when the row count changes.  ``buffers``: ``(attribute, dtype, shape)`` with -1 where the row count goes.
    ``events``: ``reserve_offsets`` for that count too."""
    if rows != owner._rows_cap:
        for name, dtype, shape in buffers:
            setattr(owner, name, torch.zeros([rows if k == -1 else k for k in shape], dtype=dtype, device=owner.device))
        owner._rows_cap = rows
    if events is not None:
        reserve_offsets(owner, events)


class TableCursor:
    """Walks a flat host array of int64 in the order the tables were packed."""

    def __init__(self, host):
        self.host, self.at = host, 0

    def take(self, shape):
        """The next ``prod(shape)`` values as a view of that shape."""
        size = int(np.prod(shape))
        if self.at + size > self.host.shape[0]:
            raise ValueError("TableCursor: %d values asked at %d of %d" % (size, self.at, self.host.shape[0]))
        out = self.host[self.at:self.at + size].reshape(shape)
        self.at += size
        return out

    def take_pair(self, shape):
        """(count table, fixed-point sum table): how every (count, sum) pair is laid out."""
        n = self.take(shape)
        return n, self.take(shape)

    def rest(self):
        out = self.host[self.at:]
        self.at = self.host.shape[0]
        return out


def read_back(*tensors):
    """The given device tensors as one int64 array on the host, in ONE copy, behind a ``TableCursor``.  Flags (int32)
    are widened; a float64 tensor goes in as its bits (``t.view(torch.int64)``) by the caller."""
    flat = [t.reshape(-1).to(torch.int64) for t in tensors]
    return TableCursor((flat[0] if len(flat) == 1 else torch.cat(flat)).cpu().numpy())
