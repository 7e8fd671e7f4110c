"""HDF5 -> sparse-COO items for the PSD path, read natively through libwfh5.so (include/wfh5.h).

Host-side mirror of the reference's dataset interface for this row:

  * ``HDF5Dataset``      reference src/datasets/HDF5Dataset.py:36-217 -- file discovery by pattern, natural sort on the
                         first ``_<n>`` of the name (:19-24), round-robin ordering across class directories with a
                         per-directory event budget (:152-183), ONE item = one file's event range ``[0, n-1]``,
                         ``[[coords, feats], labels]``, labels = directory index unless a ``labels`` dataset / member is
                         named, features scaled by 1/(2^14 - 1) when ``normalize`` (:14-17, :345-346)
  * ``PulseDataset2D`` / ``PulseDataset3D`` / ``PulseDatasetDet``   the table / pattern / batch-column bindings of
                         reference src/datasets/PulseDataset.py:543-625, :679-719
  * ``PulseDatasetRows`` and ``PulseDatasetPMT`` / ``PulseDatasetRealWFPair`` / ``PulseDatasetWFPairNorm``   the per-segment
                         bindings of :628-676 and :722-1232 (any table with (x, y, evt) rows, ``label_index``, the PMT
                         factors, the real-data label scaling, ``waveform_subset``)

What differs from the reference, on purpose:
  * rows are read with hyperslab selections of just the item's range and of just the ``coord`` / ``waveform`` members
    of a compound record (the reference loads every member of the whole table into numpy, :430-476, then slices);
  * the event column of the range search is ``batch_index`` (3 for the 3-D table); the reference searches column 2 for
    every 2-D coord array (:231-248), which for (x, y, t, evt) rows is the time sample.  Identical results whenever an
    item is a whole file, which is every file but the last one of a directory's budget;
  * no data cache: items are decoded straight into (optionally pinned) tensors;
  * ``normalize`` scales the features only (with ``additional_fields`` the reference multiplies the Python LIST of
    tensors by a float, :345-346, which raises).

Served since round 3 (reference :186-217, :250-347, :404-427): per-row label columns by member name
(``label_name: "PID"`` with ``label_map``, ``"phys"``, ``"EZ"``), ``additional_fields`` (returned as the reference's
``[feats, *fields]`` list), ``label_file_pattern`` files (first member of the ``label_name`` table, one entry per event),
length-based ranges (``event_based=False``) and any coordinate / feature member names.
"""
import ctypes
import os
import re
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libwfh5.so")

WFH5_OK, WFH5_EIO, WFH5_EFORMAT, WFH5_EINVAL = 0, 1, 2, 3
WFH5_GROUP, WFH5_COMPOUND = 0, 1
N_CHANNELS = 14
MAX_RANGE_INV = 1.0 / (2 ** N_CHANNELS - 1)

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
c_i64p = ctypes.POINTER(ctypes.c_int64)


class Info(ctypes.Structure):
    """struct wfh5_info"""
    _fields_ = [("n_rows", _i64), ("n_events", _i64), ("n_labels", _i64), ("coord_cols", _i32),
                ("feat_cols", _i32), ("feat_is_float", _i32), ("layout", _i32)]


# name -> (restype, argtypes); mirrors include/wfh5.h one to one (tests/test_abi.py checks the export list)
SIGNATURES = {
    "wfh5_last_error": (ctypes.c_char_p, []),
    "wfh5_open": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_vp)]),
    "wfh5_open_named": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                       ctypes.POINTER(_vp)]),
    "wfh5_member_info": (ctypes.c_int, [_vp, ctypes.c_char_p, c_i64p, ctypes.POINTER(_i32), ctypes.POINTER(_i32),
                                        ctypes.POINTER(_i32)]),
    "wfh5_read_member": (ctypes.c_int, [_vp, ctypes.c_char_p, _i64, _i64, _i32, _vp]),
    "wfh5_close": (None, [_vp]),
    "wfh5_get_info": (ctypes.c_int, [_vp, ctypes.POINTER(Info)]),
    "wfh5_read_rows": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp, ctypes.c_float]),
    "wfh5_read_labels": (ctypes.c_int, [_vp, _i64, _i64, _vp]),
    "wfh5_event_rows": (ctypes.c_int, [_vp, _i32, _i64, _i64, c_i64p, c_i64p]),
    "wfh5_set_threads": (ctypes.c_int, [ctypes.c_int]),
}


def set_threads(n):
    """Worker threads libwfh5 uses to inflate the chunks of a bulk read (default $WFH5_THREADS or 4)."""
    load().wfh5_set_threads(int(n))

_LIB = None


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libwfh5.so is missing at %s -- build it with `make -C waveformml_amd/csrc`" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


class H5Error(RuntimeError):
    pass


def _check(rc):
    if rc != WFH5_OK:
        raise H5Error("wfh5 error %d: %s" % (rc, load().wfh5_last_error().decode()))


class H5Table:
    """One open table of one file (a handle is not shared between DataLoader workers: open per use)."""

    def __init__(self, path, table, coord_name="coord", feat_name="waveform"):
        self._lib = load()
        self._h = _vp()
        _check(self._lib.wfh5_open_named(str(path).encode(), table.encode(), (coord_name or "").encode(),
                                         (feat_name or "").encode(), ctypes.byref(self._h)))
        info = Info()
        _check(self._lib.wfh5_get_info(self._h, ctypes.byref(info)))
        self.n_rows, self.n_events, self.n_labels = info.n_rows, info.n_events, info.n_labels
        self.coord_cols, self.feat_cols = info.coord_cols, info.feat_cols
        self.feat_is_float, self.layout = bool(info.feat_is_float), info.layout

    def close(self):
        if self._h and self._lib is not None:
            close = getattr(self._lib, "wfh5_close", None)
            if close is not None:          # None during interpreter shutdown
                close(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def event_rows(self, e0, e1, event_col):
        """Row range of events [e0, e1] inclusive (reference HDF5Dataset.py:238-248)."""
        r0, r1 = _i64(), _i64()
        _check(self._lib.wfh5_event_rows(self._h, event_col, e0, e1, ctypes.byref(r0), ctypes.byref(r1)))
        return r0.value, r1.value

    def read_rows(self, row0, row1, scale=1.0, pin_memory=False):
        n = row1 - row0
        coords = torch.empty((n, self.coord_cols), dtype=torch.int32, pin_memory=pin_memory)
        feats = torch.empty((n, self.feat_cols), dtype=torch.float32, pin_memory=pin_memory)
        _check(self._lib.wfh5_read_rows(self._h, row0, row1, coords.data_ptr(), feats.data_ptr(), scale))
        return coords, feats

    def member_info(self, name=None):
        """(rows, array length per row, is_float, stored element bytes) of a member / dataset; None: the first member."""
        rows, cols, fl, es = _i64(), _i32(), _i32(), _i32()
        _check(self._lib.wfh5_member_info(self._h, name.encode() if name else None, ctypes.byref(rows), ctypes.byref(cols),
                                          ctypes.byref(fl), ctypes.byref(es)))
        return rows.value, cols.value, bool(fl.value), es.value

    def read_member(self, name, row0, row1):
        """Rows [row0, row1) of any member: float members as float32, integer members as int64 (int32 when stored in at
        most 4 bytes, as numpy would hand them to torch); [n] for scalars, [n, len] for array members."""
        _rows, cols, fl, es = self.member_info(name)
        n = row1 - row0
        out = torch.empty((n, cols), dtype=torch.float32 if fl else torch.int64)
        _check(self._lib.wfh5_read_member(self._h, name.encode() if name else None, row0, row1, 1 if fl else 0,
                                          out.data_ptr()))
        if not fl and es <= 4:
            out = out.to(torch.int32)
        return out[:, 0].contiguous() if cols == 1 else out

    def read_labels(self, e0, e1):
        y = torch.empty((e1 - e0,), dtype=torch.int64)
        _check(self._lib.wfh5_read_labels(self._h, e0, e1, y.data_ptr()))
        return y


_SORT_RE = re.compile(r'_(\d+)')


def _sort_key(name):
    """Natural order on the first ``_<digits>`` of the path; names without one sort after, alphabetically
    (the reference's key returns int or the path itself, which Python 3 cannot compare when mixed;
    src/datasets/HDF5Dataset.py:19-24)."""
    nums = _SORT_RE.findall(str(name))
    return (0, int(nums[0]), str(name)) if nums else (1, 0, str(name))


def _needs_more_data(tally, n, all_files):
    return any(val < n and len(all_files[i]) > 0 for i, val in enumerate(tally))


class HDF5Dataset(Dataset):
    """See the module docstring.  Constructor arguments follow reference src/datasets/HDF5Dataset.py:86-104
    (``device`` is kept for signature parity; items are host tensors, moved by the step's own H2D copy)."""

    def __init__(self, file_paths, file_pattern, data_name, coordinate_name, feature_name, events_per_dir,
                 device=None, recursive=False, load_data=False, file_excludes=None, label_name=None,
                 label_file_pattern=None, data_cache_size=1, normalize=False, use_half=False, event_based=True,
                 additional_fields=None, label_map=None, batch_index=2, pin_memory=False):
        super().__init__()
        self.num_dirs = len(file_paths)
        self.normalize = normalize
        self.half_precision = use_half
        self.device = device
        self.batch_index = batch_index
        self.pin_memory = pin_memory
        self.n_events = [0] * self.num_dirs
        self.file_paths = [os.path.normpath(os.path.abspath(f)) for f in file_paths]
        self.info = {"file_paths": self.file_paths, "data_info": [], "data_cache_size": data_cache_size,
                     "data_name": data_name, "coord_name": coordinate_name, "feat_name": feature_name,
                     "label_name": label_name, "label_file_pattern": label_file_pattern,
                     "file_pattern": file_pattern, "events_per_dir": events_per_dir, "event_based": event_based,
                     "additional_fields": additional_fields, "label_map": label_map}
        self.ordered_file_set = []
        all_files = []
        for file_path in self.file_paths:
            p = Path(file_path)
            if not p.is_dir():
                raise RuntimeError("{0} is not a valid directory.".format(str(p.resolve())))
            files = sorted(p.glob(('**/' if recursive else '') + file_pattern), key=_sort_key)
            if file_excludes:
                files = [f for f in files if str(f.resolve()) not in file_excludes]
            if len(files) < 1 and file_excludes:
                raise RuntimeError('No remaining datasets available, lower the number of training and / or '
                                   'validation data')
            elif len(files) < 1:
                raise RuntimeError('No hdf5 datasets found')
            all_files.append(files)
        if len(all_files) == 1:
            ordered = [(f, 0) for f in all_files[0]]
        else:
            # round-robin across directories, always topping up the directory that is behind (reference :163-174)
            tally = [0] * len(all_files)
            ordered = []
            while sum(len(fs) for fs in all_files) > 0 and _needs_more_data(tally, events_per_dir, all_files):
                for i, file_set in enumerate(all_files):
                    while len(file_set) > 0 and tally[i] < events_per_dir:
                        f = file_set.pop(0)
                        ordered.append((f, i))
                        tally[i] += self._get_event_num(f)
                        if not tally[i] < max(tally):
                            break
        for f, dir_index in ordered:
            if self.n_events[dir_index] >= events_per_dir:
                continue
            self.ordered_file_set.append(str(f.resolve()))
            self._add_data_infos(str(f.resolve()), dir_index)

    def _table(self, file_path):
        return H5Table(file_path, self.info["data_name"], self.info["coord_name"], self.info["feat_name"])

    def _get_event_num(self, file_path):
        with self._table(file_path) as t:
            if not self.info["event_based"]:
                return t.n_rows                    # ranges count ROWS (reference :381-384)
            if t.n_events < 0:
                raise H5Error("%s:%s has no nevents attribute" % (file_path, self.info["data_name"]))
            return t.n_events

    def _label_file(self, file_path):
        """The label file that goes with a data file (reference :404-411, src/utils/util.py:527-537)."""
        fdir, fname = os.path.split(file_path)
        p1, p2 = self.info["file_pattern"].split("*"), self.info["label_file_pattern"].split("*")
        if len(p1) != len(p2):
            raise ValueError("incompatible patterns: {0} and {1}".format(p1, p2))
        for a, b in zip(p1, p2):
            if a == b == "":
                continue
            fname = fname.replace(a, b, 1)
        path = os.path.join(fdir, fname)
        if not os.path.exists(path):
            raise RuntimeError("No corresponding label file found for file {0}, tried {1}".format(file_path, path))
        return path

    def _convert_label(self, y, per_row, stored_int32=None):
        """The reference's label handling, per path (src/datasets/HDF5Dataset.py:582-585, :319-341):
        * ``label_map`` is applied IN PLACE, key by key in the map's order, to labels of any stored type -- so a value
          produced by an earlier key is remapped again by a later key equal to it (chained), exactly as the reference's
          ``for key, val in label_map.items(): y[y == key] = val``;
        * one label per ROW (the compound-table layout, :331-341): int64 class indices only when the member is stored as
          int32, float32 for EVERY other stored type (int8 / int16 / int64 columns included);
        * one label per EVENT (group layout, label files; :319-327): always int64."""
        if self.info["label_map"]:
            for k, v in self.info["label_map"].items():
                key = int(k) if not y.is_floating_point() else float(k)
                y[y == key] = v
        if per_row:
            # read_member hands every integer member of <= 4 bytes over as int32: the STORED width decides
            is_i32 = (y.dtype == torch.int32) if stored_int32 is None else bool(stored_int32)
            return y.to(torch.int64) if is_i32 else y.to(torch.float32)
        return y.to(torch.int64)

    def _add_data_infos(self, file_path, dir_index):
        n_file_events = self._get_event_num(file_path)
        n = min(n_file_events, self.info["events_per_dir"] - self.n_events[dir_index])
        self.n_events[dir_index] += n
        self.info["data_info"].append({"file_path": file_path, "name": self.info["data_name"],
                                       "modified": os.path.getmtime(file_path), "n_events": int(n_file_events),
                                       "event_range": [0, int(n) - 1], "dir_index": dir_index})

    def __len__(self):
        return len(self.info["data_info"])

    def __getitem__(self, index):
        di = self.info["data_info"][index]
        e0, e1 = di["event_range"]
        scale = MAX_RANGE_INV if self.normalize else 1.0
        label_name, label_file = self.info["label_name"], self.info["label_file_pattern"]
        with self._table(di["file_path"]) as t:
            if not self.info["event_based"]:
                r0, r1 = e0, e1 + 1                                    # the range IS the row range (reference :232-246)
            elif e0 == 0 and e1 + 1 >= di["n_events"]:
                r0, r1 = 0, t.n_rows
            else:
                r0, r1 = t.event_rows(e0, e1, min(self.batch_index, t.coord_cols - 1))
            coords, feats = t.read_rows(r0, r1, scale, self.pin_memory)
            extra = [t.read_member(f, r0, r1) for f in (self.info["additional_fields"] or [])]
            if label_name is None:
                y = torch.full((e1 + 1 - e0,), di["dir_index"], dtype=torch.int64)
            elif label_file is not None:
                y = None                                               # from the label file, below
            elif t.layout == WFH5_GROUP:
                y = self._convert_label(t.read_labels(e0, e1 + 1) if label_name == "labels"
                                        else t.read_member(label_name, e0, e1 + 1), False)   # one label per EVENT (:319-327)
            else:
                _r, _c, is_float, esize = t.member_info(label_name)
                y = self._convert_label(t.read_member(label_name, r0, r1), True,
                                        stored_int32=(not is_float and esize == 4))       # one label per ROW (:331-341)
        if y is None:
            # a separate label file: the FIRST member of its `label_name` table, one entry per event (:483, :319-327)
            with H5Table(self._label_file(di["file_path"]), label_name, "", "") as lt:
                y = self._convert_label(lt.read_member(None, e0, e1 + 1), False)
        if self.half_precision:
            feats = feats.half()
        if self.info["additional_fields"] is not None:
            return [coords, [feats] + extra], y                        # the reference's [feats, *fields] list (:250-262)
        return [coords, feats], y


class PulseDataset2D(HDF5Dataset):
    """``WaveformPairs`` tables of ``*WaveformPairSim.h5`` files: coord (x, y, evt), waveform [2 * nsamples]
    (reference src/datasets/PulseDataset.py:543-579)."""
    layout = "2d"

    def __init__(self, file_paths, n_per_dir, device=None, **kw):
        super().__init__(file_paths, "*WaveformPairSim.h5", "WaveformPairs", "coord", "waveform", n_per_dir,
                         device, batch_index=2, **kw)


class PulseDatasetWaveformNorm(HDF5Dataset):
    """``WaveformNorm`` tables of ``*PulseNorm.h5`` files: one row per PMT pulse, coord ``det`` [1], features
    ``data_name`` (default ``pulse``) [nsamples], stored normalised (``normalize=False``), no ``nevents``: an item's range
    counts ROWS (``event_based=False``); ``label_index`` picks label columns (reference src/datasets/PulseDataset.py:
    1128-1178)."""
    layout = "pulse"

    def __init__(self, file_paths, n_per_dir, device=None, data_name="pulse", label_index=None, **kw):
        super().__init__(file_paths, "*PulseNorm.h5", "WaveformNorm", "det", data_name, n_per_dir, device,
                         normalize=False, event_based=False, **kw)
        self.label_index = label_index

    def __getitem__(self, idx):
        val, label = super().__getitem__(idx)
        if self.label_index is not None:
            return val, label[:, self.label_index]
        return val, label


class PulseDatasetDet(HDF5Dataset):
    """``DetPulseCoord`` tables of ``*DetCoordSim.h5`` files: coord (x, y, evt), pulse float32 [7] = the extracted
    quantities E / 12, dt / 30 + 0.5, PE0 / 5000, PE1 / 5000, z / 1200 + 0.5, PSD, t offset / 30 of one segment, stored
    normalised (``normalize=False``) (reference src/datasets/PulseDataset.py:679-719)."""
    layout = "2d"

    def __init__(self, file_paths, n_per_dir, device=None, normalize=False, **kw):
        super().__init__(file_paths, "*DetCoordSim.h5", "DetPulseCoord", "coord", "pulse", n_per_dir, device,
                         normalize=normalize, batch_index=2, **kw)


class PulseDataset3D(HDF5Dataset):
    """``Waveform3DPairs`` tables of ``*Waveform3DPairSim.h5`` files: coord (x, y, t, evt), waveform [2]
    (reference src/datasets/PulseDataset.py:582-621)."""
    layout = "3d"

    def __init__(self, file_paths, n_per_dir, device=None, **kw):
        super().__init__(file_paths, "*Waveform3DPairSim.h5", "Waveform3DPairs", "coord", "waveform", n_per_dir,
                         device, batch_index=3, **kw)


class PulseDatasetRows(HDF5Dataset):
    """Any compound table with one coordinate row (x, y, evt) per feature row: the binding (file mask, table, coordinate
    and feature member) is the constructor's, ``label_index`` slices the label columns AFTER ``_convert_label``, as the
    reference's ``__getitem__`` of every class of src/datasets/PulseDataset.py:722-1232 does."""
    layout = "2d"

    def __init__(self, file_paths, n_per_dir, device, file_pattern, data_name, coordinate_name, feature_name,
                 label_index=None, **kw):
        super().__init__(file_paths, file_pattern, data_name, coordinate_name, feature_name, n_per_dir, device,
                         batch_index=2, **kw)
        self.label_index = label_index

    def __getitem__(self, idx):
        val, label = super().__getitem__(idx)
        if self.label_index is not None:
            return val, label[:, self.label_index]
        return val, label


class PulseDatasetPMT(PulseDatasetRows):
    """``DetPulseCoord`` tables of ``*PMTCoordSim.h5`` files: pulse [8] = two PMTs x four quantities, each column scaled
    by its own factor (reference src/datasets/PulseDataset.py:628-676)."""

    def __init__(self, file_paths, n_per_dir, device=None, **kw):
        m = float(2 ** N_CHANNELS - 1)
        self.normalization_factors = torch.tensor([1. / m, 1. / (m * 10), 0.001, 1.0, 1. / m, 1. / (m * 10), 0.001, 1.0],
                                                  dtype=torch.float32)
        kw["normalize"] = False
        super().__init__(file_paths, n_per_dir, device, "*PMTCoordSim.h5", "DetPulseCoord", "coord", "pulse", **kw)

    def __getitem__(self, idx):
        (c, f), y = super().__getitem__(idx)
        return [c, f * self.normalization_factors], y


Z_NORMALIZATION_FACTOR, E_NORMALIZATION_FACTOR = 1200., 12.


class PulseDatasetRealWFPair(PulseDatasetRows):
    """``WaveformPairCal`` tables of real-data files (``file_pattern``, default ``*WFCalFilteredSE.h5``): the label ``z``
    [mm] becomes ``z / 1200 + 0.5``, the label ``E`` [MeV] ``E / 12``; any other label is returned untouched (reference
    src/datasets/PulseDataset.py:1006-1062)."""

    def __init__(self, file_paths, n_per_dir, device=None, file_pattern="*WFCalFilteredSE.h5", label_name="z", **kw):
        super().__init__(file_paths, n_per_dir, device, file_pattern, "WaveformPairCal", "coord", "waveform",
                         label_name=label_name, normalize=True, **kw)
        self.norm_factor = {"z": 1. / Z_NORMALIZATION_FACTOR, "E": 1. / E_NORMALIZATION_FACTOR}.get(label_name)

    def __getitem__(self, idx):
        val, label = super().__getitem__(idx)
        if self.info["label_name"] == "z":
            return val, label * self.norm_factor + 0.5
        if self.info["label_name"] == "E":
            return val, label * self.norm_factor
        return val, label


class PulseDatasetWFPairNorm(PulseDatasetRows):
    """``WaveformPairNorm`` tables of ``*WFNorm.h5`` files, stored normalised.  ``waveform_subset = [lo, hi]`` keeps
    samples lo .. hi INCLUSIVE of both halves (left and right PMT) of every row (reference
    src/datasets/PulseDataset.py:1064-1125; with ``additional_fields`` the reference indexes the [feats, *fields] list
    itself, which raises: here the subset is taken of the features)."""

    def __init__(self, file_paths, n_per_dir, device=None, data_name="pulse", waveform_subset=None, **kw):
        super().__init__(file_paths, n_per_dir, device, "*WFNorm.h5", "WaveformPairNorm", "coord", data_name,
                         normalize=False, **kw)
        self.waveform_subset = waveform_subset
        self.waveform_inds = None

    def __getitem__(self, idx):
        val, label = super().__getitem__(idx)
        if self.waveform_subset is not None:
            feats = val[1][0] if isinstance(val[1], list) else val[1]
            if self.waveform_inds is None:
                n = feats.shape[1] // 2
                lo, hi = self.waveform_subset
                keep = torch.tensor([lo <= i <= hi for i in range(n)], dtype=torch.bool)
                self.waveform_inds = torch.cat([keep, keep])
            feats = feats[:, self.waveform_inds]
            if isinstance(val[1], list):
                val[1][0] = feats
            else:
                val[1] = feats
        return val, label
