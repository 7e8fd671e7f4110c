"""Waveform rows -> voxels on the GPU: the hand-over of the hybrid 3-D net (BASELINE configs[4]: feat [n, 1, 2T] -> TCN
-> voxelise -> SubM3d head).  The reference only ever voxelised offline (its 3-D datasets, src/datasets/PulseDataset.py:
543-625); here the voxel set is cut out of the batch inside the step (include/wfsparse.h, wfs_voxelize_*; csrc/
voxelize.hip): sample t of row r is a voxel iff either PMT's RAW sample exceeds the threshold, its features are the two
PMTs' values of the front end's output at t, and voxels come row-major, t ascending -- the host 3-D layout's order
(psd/synthetic.py).  There is no CPU path.

Eager: exact size, one read-back of the voxel count.  Device-count mode (the rows carry ``n_valid``, as in a captured
step): the output has ``out_capacity`` rows (calibrated by psd/graph.py; before that, the bound rows x samples), the count
stays on the device (``st.n_valid``), and a batch with more voxels than the capacity sets a sticky flag that
GraphedTrainStep.check() reports -- nothing is cut silently."""
import torch
from torch import nn
from torch.autograd import Function

from .. import _lib
from ..spconv import ops


class VoxelizeFunction(Function):
    """(values [n_cap, 2T], rows [n_cap, 2T], coords int32 [n_cap, 3] = (x, y, evt)) -> (feats [V, 2], indices int32
    [V, 4] = (evt, x, y, t), v_dev int64 [1], events int32 (wfs_event_offsets table of the voxels), offsets int32
    [n_cap * S + 1]: exclusive voxel offset of every 64-sample slice, S = ceil(T / 64) per row).  Differentiable in
    ``values`` only.  ``n_dev`` None: eager, V exact; else V = ``v_cap`` (capacity) and ``overflow`` (int32 [1], sticky)
    is set when the batch has more voxels."""

    @staticmethod
    def forward(ctx, values, rows, coords, threshold, batch_size, n_dev, v_cap, overflow):
        lib = _lib.load()
        n_cap, L = rows.shape
        T = L // 2
        dev = rows.device
        offsets = torch.empty((int(lib.wfs_voxelize_offsets_ints(n_cap, T)),), dtype=torch.int32, device=dev)
        v_dev = torch.empty((1,), dtype=torch.int64, device=dev)
        events = torch.empty((int(lib.wfs_event_offsets_ints(int(batch_size))),), dtype=torch.int32, device=dev)
        dtype = _lib.dtype_code(rows)
        stream = _lib.stream_ptr()
        bound = n_cap * T
        cap = bound if (n_dev is None or v_cap is None) else int(v_cap)
        if overflow is None:
            overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.wfs_voxelize_plan(_lib.ptr(rows), _lib.ptr(coords), n_cap, T, _lib.ptr(n_dev), float(threshold),
                                         int(batch_size), cap, _lib.ptr(offsets), _lib.ptr(v_dev), _lib.ptr(events),
                                         _lib.ptr(overflow), dtype, stream))
        if n_dev is None:
            cap = int(v_dev.item())               # the one read-back of the eager form
        indices = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        feats = torch.empty((cap, 2), dtype=rows.dtype, device=dev)
        _lib.check(lib.wfs_voxelize_emit(_lib.ptr(rows), _lib.ptr(values), _lib.ptr(coords), n_cap, T, float(threshold),
                                         _lib.ptr(offsets), cap, _lib.ptr(indices), _lib.ptr(feats), dtype, stream))
        ctx.save_for_backward(indices, offsets)
        ctx.shape = (n_cap, T, cap)
        ctx.mark_non_differentiable(indices, v_dev, events, offsets)
        return feats, indices, v_dev, events, offsets

    @staticmethod
    def backward(ctx, dfeat, *_):
        lib = _lib.load()
        indices, offsets = ctx.saved_tensors
        n_cap, T, cap = ctx.shape
        dY = None
        if ctx.needs_input_grad[0]:
            dfeat = dfeat.contiguous()
            dY = torch.empty((n_cap, 2 * T), dtype=dfeat.dtype, device=dfeat.device)
            _lib.check(lib.wfs_voxelize_bwd(_lib.ptr(dfeat), _lib.ptr(indices), _lib.ptr(offsets), n_cap, T, cap,
                                            _lib.ptr(dY), _lib.dtype_code(dfeat), _lib.stream_ptr()))
        return dY, None, None, None, None, None, None, None


def voxelize(rows, values=None, coords=None, threshold=0.0, batch_size=None, n_valid=None, out_capacity=None,
             overflow=None):
    """Functional form; see VoxelizeFunction.  ``values`` defaults to ``rows``; ``batch_size`` to the last row's event
    + 1 (a read-back).  Returns (feats, indices, v_dev, events, slice offsets)."""
    for t in (rows, values, coords):
        if t is not None and not t.is_cuda:
            raise RuntimeError("waveformml_amd.psd.voxel: tensors must live on the GPU (there is no CPU path); got %s"
                               % t.device)
    values = rows if values is None else values
    if rows.dim() != 2 or rows.shape[1] % 2 or values.shape != rows.shape or values.dtype != rows.dtype:
        raise RuntimeError("waveformml_amd.psd.voxel: rows and values must be [n, 2T] of one dtype")
    if coords is None or coords.dtype != torch.int32 or tuple(coords.shape) != (rows.shape[0], 3):
        raise RuntimeError("waveformml_amd.psd.voxel: coords must be int32 [n, 3] = (x, y, evt)")
    if batch_size is None:
        batch_size = int(coords[-1, -1]) + 1 if coords.shape[0] else 1
    return VoxelizeFunction.apply(values.contiguous(), rows.contiguous(), coords.contiguous(), float(threshold),
                                  max(1, int(batch_size)), n_valid, out_capacity, overflow)


class Voxelizer(nn.Module, ops.StickyFlags):
    """The hybrid net's voxeliser: ``threshold`` on the raw rows, and -- once a captured step has calibrated it --
    ``out_capacity`` voxels in device-count mode.  Its overflow flag follows the sticky-flag protocol of the conv layers
    (spconv.ops.StickyFlags): ``calibration_count()`` is the voxel count of the last eager call."""

    def __init__(self, threshold=0.0):
        super().__init__()
        self.threshold = float(threshold)
        self.out_capacity = None
        self.last_count = None

    def calibration_count(self):
        return self.last_count

    def forward(self, rows, values, coords, batch_size, spatial_shape, spconv, n_valid=None):
        if n_valid is None:
            feats, indices, v_dev, events, _ = voxelize(rows, values, coords, self.threshold, batch_size)
            self.last_count = int(indices.shape[0])
        else:
            flag = ops._sticky_flags(1, rows.device, self._sticky_flags(), "overflow")
            feats, indices, v_dev, events, _ = voxelize(rows, values, coords, self.threshold, batch_size, n_valid,
                                                        self.out_capacity, flag)
        st = spconv.SparseConvTensor(feats, indices, spatial_shape, batch_size)
        if n_valid is not None:
            st.n_valid = v_dev
            st.events = events            # first voxel of every event: what the event-local SubM build starts from
        return st
