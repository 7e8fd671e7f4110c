"""Prediction writers: a data file in, the trained model on the GPU, a copy of the file out whose ``EZ`` / ``phys``
columns hold the predictions (reference WritePredictions.py -> src/datasets/PredictionWriter.py).

The reference's ``swap_values`` walks every 2048-row chunk row by row on the host (``normalize_waveforms``,
``swap_sparse_from_dense`` / ``swap_sparse_from_event``), builds two tensors from numpy arrays, runs the model and copies
the result back.  Here a chunk's RAW compound records make one trip:

    file --(libwfh5w, one raw read)--> page-locked buffer --(one copy)--> device
         wfs_predict_prepare   records -> coords (events renumbered), feature rows (gain-normalised), n_valid
         the forward           eager, or a psd/graph.GraphedEvalStep replay (``capture=True``)
         wfs_predict_scatter   the output -> the float32 prediction columns of the records, in place
    device --(one copy)--> page-locked buffer --(libwfh5w, one append)--> file

Chunks are the reference's ``H5Input.next_chunk(nrows, preserve_event=True)`` (src/datasets/HDF5IO.py:55-79): ``nrows``
rows extended to the end of their last event, the remainder whole once ``current + nrows >= length`` -- cut on the host
from the event column with vectorised numpy (``chunk_bounds``), so output rows line up with the reference's chunk for chunk.

Constructors and names follow the reference: ``PredictionWriter(path, input_path, config, checkpoint, **kwargs)`` with
``n_buffer_rows``, ``n_rows_per_read``, ``map_location``, ``datatype``; ``ZPredictionWriter`` (LitZ, ``EZ[:, 1]``),
``IRNPredictionWriter`` (LitPSD, ``phys[:, 4:]``), ``IRNIMPredictionWriter`` (LitSegClassifier, ``phys[:, 2:]``).
There is no calibration database: ``gains=`` is an array [14, 11, 2] and ``calgroup=`` raises.  Left out and departures:
DESIGN.md 7."""
import os
import time

import numpy as np
import torch

from .. import _lib
from . import h5records
from .config import load_config
from .pid_evaluator import Z_NORMALIZATION_FACTOR

MAX_RANGE = 2 ** 14 - 1                      # reference src/datasets/HDF5Dataset.py:14-16
STAGES = ("read", "h2d", "prepare", "forward", "scatter", "d2h", "append")


def extension_type_name(path):
    """Table (= compound type) name by file name, reference H5CompoundTypes.extension_type_map."""
    if str(path).endswith("WFNorm.h5"):
        return "WaveformPairNorm"
    if str(path).endswith("Phys.h5"):
        raise NotImplementedError("PhysPulse files are not swap-writer inputs (DESIGN.md 7)")
    return "WaveformPairCal"


def chunk_bounds(events, nrows):
    """[(row0, row1)] of ``H5Input.next_chunk(nrows, preserve_event=True)`` called until it returns None, from the event
    column alone: one numpy pass for the run ends, then one step per CHUNK."""
    events = np.asarray(events)
    n, nrows = int(events.shape[0]), int(nrows)
    if nrows < 1:
        raise ValueError("n_rows_per_read must be positive")
    if n == 0:
        return []
    last = np.flatnonzero(events[1:] != events[:-1])                  # last row of every run but the final one
    run_end = np.concatenate([last + 1, [n]])                         # exclusive end of every run
    out, cur = [], 0
    while True:
        if cur + nrows >= n:
            out.append((cur, n))
            return out
        end = int(run_end[np.searchsorted(run_end, cur + nrows - 1, side="right")])   # end of the run of the last row
        out.append((cur, end))
        if end >= n:
            return out
        cur = end


def chunk_events(events, bounds):
    """Events per chunk by the reference's rule (a new event wherever the number changes; row 0 of a chunk starts one)."""
    events = np.asarray(events)
    if events.shape[0] == 0:
        return []
    change = np.concatenate([[0], np.cumsum(events[1:] != events[:-1])])
    return [int(change[r1 - 1] - change[r0]) + 1 for r0, r1 in bounds]


def gain_factors(gains, scale_factor=None, nx=14, ny=11):
    """``scale_factor * 690 / MAX_RANGE / gains`` in the reference's dtype (ZPredictionWriter.__init__): float32 when a
    scale factor is given, float64 otherwise."""
    if scale_factor is not None:
        g = np.asarray(gains, dtype=np.float32)
        full = np.full((nx, ny, 2), scale_factor * 690.0 / MAX_RANGE, dtype=np.float32)
    else:
        g = np.asarray(gains, dtype=np.float64)
        full = np.full((nx, ny, 2), 690.0 / MAX_RANGE)
    if g.shape != (nx, ny, 2):
        raise ValueError("gains must have shape (%d, %d, 2), got %s" % (nx, ny, g.shape))
    return np.divide(full, g)


def predict_prepare(records, n, item_size, coord_offset, feat_offset, feat_kind, width, gains, nx, ny, coords, feats,
                    n_valid, workspace):
    """wfs_predict_prepare on torch's current stream: ``coords`` / ``feats`` hold the capacity."""
    lib = _lib.load()
    _lib.check(lib.wfs_predict_prepare(_lib.ptr(records), n, item_size, coord_offset, feat_offset, feat_kind, width,
                                       _lib.ptr(gains), nx, ny, coords.shape[0], _lib.ptr(coords), _lib.ptr(feats),
                                       _lib.dtype_code(feats), _lib.ptr(n_valid), _lib.ptr(workspace),
                                       workspace.numel() if workspace is not None else 0, _lib.stream_ptr()))


def predict_scatter(records, n, item_size, member_offset, member_cols, col0, L, coords, src, mode, B, nx, ny,
                    affine=None):
    """wfs_predict_scatter on torch's current stream; ``affine`` = (sub, mul) or None."""
    lib = _lib.load()
    sub, mul = affine if affine is not None else (0.0, 1.0)
    _lib.check(lib.wfs_predict_scatter(_lib.ptr(records), n, item_size, member_offset, member_cols, col0, L,
                                       _lib.ptr(coords), _lib.ptr(src), _lib.dtype_code(src), mode, B, nx, ny,
                                       1 if affine is not None else 0, sub, mul, _lib.stream_ptr()))


class PredictionWriter(object):
    """Base class: subclasses name the module class and where its output goes (``_scatter``)."""

    def _module_class(self):
        """The Lightning-style module the checkpoint belongs to; the base class takes it from ``config.run_config``."""
        from .config import ModuleUtility
        run = self.config.run_config
        return ModuleUtility(run.imports).retrieve_class(run.run_class)

    def __init__(self, path, input_path, config, checkpoint, **kwargs):
        self.path, self.input_path = str(path), str(input_path)
        self.checkpoint_path, self.config_path = checkpoint, config
        self.config = load_config(config) if isinstance(config, (str, dict, os.PathLike)) else config
        self.model = None
        self.n_buffer_rows = 1024 * 16
        self.n_rows_per_read = 2048
        self.map_location = None
        self.capture = False
        self.device = "cuda:0"
        self.feature_dtype = torch.float32
        self.profile = False
        self.nx, self.ny = 14, 11
        self.gains = None
        if "calgroup" in kwargs:
            raise NotImplementedError("calgroup=%r needs the calibration database (PROSPECT_CALDB), which this project "
                                      "does not have: pass gains=<array [14, 11, 2]> (the evaluators take the curves "
                                      "as calibration=, psd/calibration.py)" % (kwargs["calgroup"],))
        datatype = kwargs.pop("datatype", None)
        if datatype == "PhysPulse":
            raise NotImplementedError("the PhysPulse conversion (convert_values) is left out: DESIGN.md 7")
        if datatype not in (None, "WaveformPairCal"):
            raise IOError("unrecognized datatype: {}, did you mean 'WaveformPairCal' or 'PhysPulse'?".format(datatype))
        gains, scale_factor = kwargs.pop("gains", None), kwargs.pop("scale_factor", None)
        for key, val in kwargs.items():
            setattr(self, key, val)
        if gains is not None:
            self.gains = gain_factors(gains, scale_factor, self.nx, self.ny)
        self.timings = dict.fromkeys(STAGES, 0.0)
        self.chunks_written, self.recaptures, self.capacity = 0, 0, (0, 0)
        self._step = None
        self.retrieve_model()

    # reference PredictionWriter.retrieve_model
    def retrieve_model(self):
        from .trainer import load_from_checkpoint
        self.model = load_from_checkpoint(self.checkpoint_path, self.config, self._module_class(),
                                          map_location=self.map_location or "cpu")
        self.model.eval()
        for p in self.model.parameters():
            p.requires_grad_(False)
        self.model.to(self.device)

    # ---- what a subclass states --------------------------------------------------------------------------------------
    def _scatter(self, records, n, item_size, table, coords, output, n_events):
        raise NotImplementedError()

    def _member(self, table, name):
        _n, offset, kind, count = table.member(name)
        if kind != h5records.F32:
            raise IOError("member %s of %s is not float32" % (name, table.table))
        return offset, count

    # ---- the loop ----------------------------------------------------------------------------------------------------
    def _mark(self, stage, t0):
        if self.profile:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.timings[stage] += now - t0
            return now
        return t0

    def _forward_eager(self, coords, feats, n_events):
        net = getattr(self.model, "model", None)
        if hasattr(net, "batch_size_hint"):
            net.batch_size_hint = int(n_events)
        return self.model([coords, feats])

    def _capture(self, coords, feats, n_events, min_rows):
        from .graph import GraphedEvalStep
        if self._step is not None:
            self._step.check()
            self._step.close()
            self._step = None
            self.recaptures += 1
        labels = torch.zeros((int(n_events),), dtype=torch.int64, device=coords.device)
        self._step = GraphedEvalStep(self.model, ((coords, feats), labels), min_rows=min_rows)
        self.capacity = (int(self._step.n_cap), int(self._step.n_events))

    @torch.no_grad()
    def write_predictions(self):
        dev = torch.device(self.device)
        torch.cuda.set_device(dev)
        table_name = extension_type_name(self.input_path)
        table = h5records.RecordInput(self.input_path, table_name)
        out = h5records.RecordOutput(self.path)
        try:
            out.copy_dataset(table, "Chanmap")                       # reference copy_chanmap, attributes included
            out.create_table_like(table)
            out.copy_table_attrs(table)
            _n, coord_off, ckind, ccount = table.member("coord")
            if ckind != h5records.I32 or ccount != 3:
                raise IOError("%s.coord must be int32 [3] (x, y, event)" % table_name)
            if table.has_member("waveform"):
                if self.gains is None:
                    raise IOError("Must pass calgroup argument in order to normalize WaveformPairCal data before passing "
                                  "to model")
                _n, feat_off, fkind, width = table.member("waveform")
                feat_kind, want = _lib.WFS_PREDICT_WAVEFORM, h5records.I16
            else:
                _n, feat_off, fkind, width = table.member("pulse")
                feat_kind, want = _lib.WFS_PREDICT_PULSE, h5records.F32
            if fkind != want:
                raise IOError("%s: waveform must be int16, pulse float32" % table_name)
            item = table.item_size
            # the event column, for cutting the chunks: the one thing the host looks at
            from .h5data import H5Table
            events = np.zeros((0,), np.int32)
            if table.n_rows > 0:
                with H5Table(self.input_path, table_name, "coord", "waveform" if feat_kind == _lib.WFS_PREDICT_WAVEFORM
                             else "pulse") as t:
                    events = t.read_member("coord", 0, table.n_rows).numpy().reshape(-1, 3)[:, 2]
            bounds = chunk_bounds(events, self.n_rows_per_read)
            counts = chunk_events(events, bounds)
            rows_max = max([r1 - r0 for r0, r1 in bounds], default=1)
            events_max = max(counts, default=1)
            host = torch.empty((rows_max, item), dtype=torch.uint8, pin_memory=True)
            records = torch.empty((rows_max, item), dtype=torch.uint8, device=dev)
            gains = torch.from_numpy(np.ascontiguousarray(self.gains, dtype=np.float64)).to(dev) \
                if self.gains is not None else None
            work = torch.empty((int(_lib.load().wfs_predict_workspace_ints(rows_max)),), dtype=torch.int32, device=dev)
            coords = torch.empty((rows_max, 3), dtype=torch.int32, device=dev)
            feats = torch.empty((rows_max, width), dtype=self.feature_dtype, device=dev)
            n_valid = torch.zeros((1,), dtype=torch.int64, device=dev)

            def prepare(n, c, f, nv):
                predict_prepare(records, n, item, coord_off, feat_off, feat_kind, width, gains, self.nx, self.ny, c, f,
                                nv, work)

            if self.capture and bounds:
                # captured on the LARGEST chunk (its strided layers are sized off it), with room for the most events
                big = max(range(len(bounds)), key=lambda i: bounds[i][1] - bounds[i][0])
                r0, r1 = bounds[big]
                table.read_records(r0, r1, host)
                records[:r1 - r0].copy_(host[:r1 - r0], non_blocking=True)
                prepare(r1 - r0, coords[:r1 - r0], feats[:r1 - r0], n_valid)
                self._capture(coords[:r1 - r0], feats[:r1 - r0], events_max, rows_max)
            written = 0
            for (r0, r1), n_events in zip(bounds, counts):
                n = r1 - r0
                t0 = time.perf_counter()
                table.read_records(r0, r1, host)
                t0 = self._mark("read", t0)
                records[:n].copy_(host[:n], non_blocking=True)
                t0 = self._mark("h2d", t0)
                if self.capture:
                    if n > self._step.n_cap or n_events > self._step.n_events:
                        # never cut silently: a chunk beyond the captured capacity captures again, sized on it
                        prepare(n, coords[:n], feats[:n], n_valid)
                        self._capture(coords[:n], feats[:n], max(n_events, self._step.n_events), max(n, self._step.n_cap))
                    step = self._step
                    torch.cuda.set_stream(step.stream)
                    prepare(n, step.coords, step.feats, step.n_valid)
                    if step.indices is not None:
                        step.indices.copy_(step.coords[:, step._perm])
                    step._event_offsets()
                    t0 = self._mark("prepare", t0)
                    step.graph.replay()
                    output, c, b_cap = step.logits, step.coords, step.n_events
                else:
                    c, f = coords[:n], feats[:n]
                    prepare(n, c, f, n_valid)
                    t0 = self._mark("prepare", t0)
                    output, b_cap = self._forward_eager(c, f, n_events), n_events
                t0 = self._mark("forward", t0)
                self._scatter(records, n, item, table, c, output.contiguous(), b_cap)
                t0 = self._mark("scatter", t0)
                host[:n].copy_(records[:n], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                t0 = self._mark("d2h", t0)
                out.append(host, n)
                written += n
                if written >= self.n_buffer_rows:
                    written = 0
                    out.flush()
                self._mark("append", t0)
                self.chunks_written += 1
            if self._step is not None:
                self._step.check()
            out.flush()
        finally:
            if self._step is not None:
                self._step.close()
                self._step = None
            table.close()
            out.close()


class ZPredictionWriter(PredictionWriter):
    """LitZ: dense [B, 1, 14, 11] -> ``(v - 0.5) * z_scale`` -> ``EZ[:, 1]`` (reference ZPredictionWriter.swap_values)."""

    def __init__(self, path, input_path, config, checkpoint, **kwargs):
        self.z_scale = Z_NORMALIZATION_FACTOR
        super().__init__(path, input_path, config, checkpoint, **kwargs)

    def _module_class(self):
        from .litz import LitZ
        return LitZ

    def _scatter(self, records, n, item_size, table, coords, output, n_events):
        offset, cols = self._member(table, "EZ")
        if output.dim() != 4 or output.shape[1] != 1:
            raise RuntimeError("ZPredictionWriter expects a dense [B, 1, nx, ny] output, got %s" % (tuple(output.shape),))
        predict_scatter(records, n, item_size, offset, cols, 1, 1, coords, output, _lib.WFS_PREDICT_DENSE, n_events,
                        self.nx, self.ny, affine=(0.5, float(np.float32(self.z_scale))))


class IRNPredictionWriter(PredictionWriter):
    """LitPSD: [B, n] per event -> ``phys[:, 4:]`` (reference IRNPredictionWriter.swap_values)."""

    def __init__(self, path, input_path, config, checkpoint, **kwargs):
        self.phys_index_replaced = 4
        super().__init__(path, input_path, config, checkpoint, **kwargs)

    def _module_class(self):
        from .lit import LitPSD
        return LitPSD

    def _scatter(self, records, n, item_size, table, coords, output, n_events):
        offset, cols = self._member(table, "phys")
        L = cols - self.phys_index_replaced
        if output.dim() != 2 or output.shape[1] != L:
            raise RuntimeError("IRNPredictionWriter expects [B, %d] per event, got %s" % (L, tuple(output.shape)))
        predict_scatter(records, n, item_size, offset, cols, self.phys_index_replaced, L, coords, output,
                        _lib.WFS_PREDICT_EVENT, n_events, self.nx, self.ny)


class IRNIMPredictionWriter(PredictionWriter):
    """LitSegClassifier: [N, n] per row -- or dense [B, n, 14, 11] with ``output_is_sparse=False`` -- -> ``phys[:, 2:]``
    (reference IRNIMPredictionWriter.swap_values)."""

    def __init__(self, path, input_path, config, checkpoint, **kwargs):
        self.phys_index_replaced = 2
        self.output_is_sparse = True
        super().__init__(path, input_path, config, checkpoint, **kwargs)

    def _module_class(self):
        from .litseg import LitSegClassifier
        return LitSegClassifier

    def _scatter(self, records, n, item_size, table, coords, output, n_events):
        offset, cols = self._member(table, "phys")
        L = cols - self.phys_index_replaced
        if self.output_is_sparse:
            if output.dim() != 2 or output.shape[1] != L or output.shape[0] < n:
                raise RuntimeError("IRNIMPredictionWriter expects [N, %d] per row, got %s" % (L, tuple(output.shape)))
            predict_scatter(records, n, item_size, offset, cols, self.phys_index_replaced, L, None, output,
                            _lib.WFS_PREDICT_ROWS, 0, self.nx, self.ny)
        else:
            if output.dim() != 4 or output.shape[1] != L:
                raise RuntimeError("IRNIMPredictionWriter expects a dense [B, %d, nx, ny] output, got %s"
                                   % (L, tuple(output.shape)))
            predict_scatter(records, n, item_size, offset, cols, self.phys_index_replaced, L, coords, output,
                            _lib.WFS_PREDICT_DENSE, n_events, self.nx, self.ny)
