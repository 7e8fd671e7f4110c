"""ctypes binding of libwfh5w.so (include/wfh5w.h): compound tables as RAW records between a file and a caller's host
buffer -- the file side of the prediction writers (psd/PredictionWriter.py).  Nothing is converted: a record buffer is a
``uint8 [rows, item_size]`` tensor (page-locked when it feeds an asynchronous copy), ``numpy_dtype()`` describes it for
host-side inspection."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libwfh5w.so")

WFH5W_OK, WFH5W_EIO, WFH5W_EFORMAT, WFH5W_EINVAL = 0, 1, 2, 3
I16, I32, I64, F32, F64, OTHER = 0, 1, 2, 3, 4, -1
KIND_DTYPES = {I16: "<i2", I32: "<i4", I64: "<i8", F32: "<f4", F64: "<f8"}
NAME_MAX = 64
# the attributes reference P2XTableWriter.copy_p2x_attrs copies, FIELD_<n>_NAME aside
P2X_ATTRS = ("CLASS", "TITLE", "VERSION", "abstime", "runtime", "calgrp", "nevents", "rname", "scalingfactor")

_vp, _i32, _i64, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
_cp = ctypes.c_char_p


class Member(ctypes.Structure):
    """struct wfh5w_member"""
    _fields_ = [("name", ctypes.c_char * NAME_MAX), ("offset", _i64), ("kind", _i32), ("count", _i32)]


# name -> (restype, argtypes); mirrors include/wfh5w.h one to one (tests/test_prediction_io.py checks the export list)
SIGNATURES = {
    "wfh5w_last_error": (_cp, []),
    "wfh5w_open_input": (ctypes.c_int, [_cp, _cp, ctypes.POINTER(_vp)]),
    "wfh5w_close_input": (None, [_vp]),
    "wfh5w_input_info": (ctypes.c_int, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    "wfh5w_input_member": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(Member)]),
    "wfh5w_read_records": (ctypes.c_int, [_vp, _i64, _i64, _vp, _sz]),
    "wfh5w_read_attr": (ctypes.c_int, [_vp, _cp, _vp, _sz, ctypes.POINTER(_i32), ctypes.POINTER(_i64)]),
    "wfh5w_create": (ctypes.c_int, [_cp, ctypes.POINTER(_vp)]),
    "wfh5w_close": (ctypes.c_int, [_vp]),
    "wfh5w_copy_dataset": (ctypes.c_int, [_vp, _vp, _cp]),
    "wfh5w_create_table_like": (ctypes.c_int, [_vp, _vp]),
    "wfh5w_create_table": (ctypes.c_int, [_vp, _cp, ctypes.POINTER(Member), _i32, _i64]),
    "wfh5w_append": (ctypes.c_int, [_vp, _vp, _i64]),
    "wfh5w_flush": (ctypes.c_int, [_vp]),
    "wfh5w_copy_table_attrs": (ctypes.c_int, [_vp, _vp]),
    "wfh5w_set_attr_string": (ctypes.c_int, [_vp, _cp, _cp]),
    "wfh5w_set_attr_f64": (ctypes.c_int, [_vp, _cp, ctypes.c_double]),
}

_LIB = None


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libwfh5w.so is missing at %s -- build it with `make -C waveformml_amd/csrc`" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


class H5RecordError(RuntimeError):
    pass


def _check(rc):
    if rc != WFH5W_OK:
        raise H5RecordError("wfh5w error %d: %s" % (rc, load().wfh5w_last_error().decode("utf-8", "replace")))


def _buffer_ptr(buf):
    """(address, bytes) of a contiguous host torch tensor or numpy array."""
    if hasattr(buf, "data_ptr"):
        if buf.is_cuda or not buf.is_contiguous():
            raise H5RecordError("record buffers are contiguous HOST tensors")
        return buf.data_ptr(), buf.numel() * buf.element_size()
    arr = np.asarray(buf)
    if not arr.flags["C_CONTIGUOUS"]:
        raise H5RecordError("record buffers must be contiguous")
    return arr.ctypes.data, arr.nbytes


def members_dtype(members, item_size):
    """numpy structured dtype of (name, offset, kind, count) members: the reference's H5CompoundTypes dtypes."""
    return np.dtype({"names": [m[0] for m in members],
                     "formats": [(KIND_DTYPES[m[2]], (m[3],)) if m[3] > 1 else KIND_DTYPES[m[2]] for m in members],
                     "offsets": [m[1] for m in members], "itemsize": int(item_size)})


class RecordInput:
    """One open compound table: ``n_rows``, ``item_size``, ``members`` = [(name, offset, kind, count)]."""

    def __init__(self, path, table):
        self._lib = load()
        self._h = _vp()
        self.path, self.table = str(path), table
        _check(self._lib.wfh5w_open_input(self.path.encode(), table.encode(), ctypes.byref(self._h)))
        n, size, nm = _i64(), _i64(), _i32()
        _check(self._lib.wfh5w_input_info(self._h, ctypes.byref(n), ctypes.byref(size), ctypes.byref(nm)))
        self.n_rows, self.item_size = n.value, size.value
        self.members = []
        for i in range(nm.value):
            m = Member()
            _check(self._lib.wfh5w_input_member(self._h, i, ctypes.byref(m)))
            self.members.append((m.name.decode(), m.offset, m.kind, m.count))

    def member(self, name):
        for m in self.members:
            if m[0] == name:
                return m
        raise KeyError("%s:%s has no member %s (members: %s)" % (self.path, self.table, name, [m[0] for m in self.members]))

    def has_member(self, name):
        return any(m[0] == name for m in self.members)

    def numpy_dtype(self):
        return members_dtype(self.members, self.item_size)

    def read_records(self, row0, row1, out):
        """Rows [row0, row1) into ``out`` (uint8 host tensor / array of at least that many records)."""
        addr, nbytes = _buffer_ptr(out)
        _check(self._lib.wfh5w_read_records(self._h, row0, row1, addr, nbytes))

    def read_attr(self, name):
        """str, float64 array, or None when the table has no such attribute."""
        buf = ctypes.create_string_buffer(1 << 16)
        is_str, n = _i32(), _i64()
        rc = self._lib.wfh5w_read_attr(self._h, name.encode(), buf, len(buf), ctypes.byref(is_str), ctypes.byref(n))
        if rc == WFH5W_EIO and b"no attribute" in self._lib.wfh5w_last_error():
            return None
        _check(rc)
        if is_str.value:
            return buf.raw[:n.value].decode("utf-8", "replace")
        return np.frombuffer(buf.raw[:8 * n.value], dtype=np.float64).copy()

    def close(self):
        if self._h and self._lib is not None:
            close = getattr(self._lib, "wfh5w_close_input", None)
            if close is not None:
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


class RecordOutput:
    """An output file with (at a time) one extendible gzip-9 table in chunks of 1024 rows."""

    def __init__(self, path):
        self._lib = load()
        self._h = _vp()
        self.path = str(path)
        _check(self._lib.wfh5w_create(self.path.encode(), ctypes.byref(self._h)))

    def copy_dataset(self, source, name):
        _check(self._lib.wfh5w_copy_dataset(self._h, source._h, name.encode()))

    def create_table_like(self, source):
        _check(self._lib.wfh5w_create_table_like(self._h, source._h))
        self.item_size = source.item_size

    def create_table(self, name, members, item_size):
        arr = (Member * len(members))()
        for a, (mname, offset, kind, count) in zip(arr, members):
            a.name, a.offset, a.kind, a.count = mname.encode(), int(offset), int(kind), int(count)
        _check(self._lib.wfh5w_create_table(self._h, name.encode(), arr, len(members), int(item_size)))
        self.item_size = int(item_size)

    def append(self, records, n_rows):
        addr, nbytes = _buffer_ptr(records)
        if int(n_rows) * getattr(self, "item_size", 0) > nbytes:
            raise H5RecordError("%d records of %d bytes from a buffer of %d" % (n_rows, getattr(self, "item_size", 0), nbytes))
        _check(self._lib.wfh5w_append(self._h, addr, int(n_rows)))

    def flush(self):
        _check(self._lib.wfh5w_flush(self._h))

    def copy_table_attrs(self, source):
        _check(self._lib.wfh5w_copy_table_attrs(self._h, source._h))

    def set_attr(self, name, value):
        if isinstance(value, str):
            _check(self._lib.wfh5w_set_attr_string(self._h, name.encode(), value.encode()))
        else:
            _check(self._lib.wfh5w_set_attr_f64(self._h, name.encode(), float(value)))

    def close(self):
        if self._h and self._lib is not None:
            h, self._h = self._h, _vp()
            _check(self._lib.wfh5w_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
