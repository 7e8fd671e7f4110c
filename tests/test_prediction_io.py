"""CPU checks of the prediction writers' host side: libwfh5w.so (include/wfh5w.h) writes what the existing reader
(libwfh5, psd/h5data.H5Table) reads back member for member; its member table knows the reference's layouts; the chunk
cutter equals the reference's ``H5Input.next_chunk`` (recorded in tests/golden/prediction_writer_cases.npz by
tests/golden/make_prediction_goldens.py); bad arguments fail with a message; the library survives damaged files under
AddressSanitizer + UBSan in a standalone driver; header, library and ctypes table mirror each other.  The vectorised
restatements of the reference's row walks that the GPU tests compose with a forward are held to the goldens here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prediction_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PRED = os.path.join(GOLD, "h5", "pred")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "prediction_writer_cases.npz"))


def _fixture(kind):
    return os.path.join(PRED, pc.FIXTURE_FILES[kind])


def _records(table):
    buf = np.zeros((table.n_rows, table.item_size), np.uint8)
    table.read_records(0, table.n_rows, buf)
    return buf.view(table.numpy_dtype()).reshape(-1)


def _assert_members_equal(path, table_name, feat, rec):
    """Every member through the EXISTING reader (float members as float32, integer members as integers)."""
    from waveformml_amd.psd.h5data import H5Table
    with H5Table(path, table_name, "coord", feat) as t:
        assert t.n_rows == len(rec)
        for name in rec.dtype.names:
            got = t.read_member(name, 0, t.n_rows).numpy()
            want = np.asarray(rec[name])
            want = want.astype(np.float32) if want.dtype.kind == "f" else want
            np.testing.assert_array_equal(got.reshape(want.shape), want.astype(got.dtype), err_msg=name)


@pytest.mark.parametrize("kind", ["cal", "norm"])
def test_fixture_files_read_back_through_the_existing_reader(kind, tmp_path):
    from waveformml_amd.psd import h5records
    rec, n_events = pc.fixture_records(kind)
    feat = "waveform" if kind == "cal" else "pulse"
    _assert_members_equal(_fixture(kind), pc.FIXTURE_TABLES[kind], feat, rec)
    members, item = pc.layout(kind)
    with h5records.RecordInput(_fixture(kind), pc.FIXTURE_TABLES[kind]) as t:
        # the member table equals the reference's layout: 324 / 584 bytes
        assert t.item_size == item == {"cal": 324, "norm": 584}[kind] and t.members == members
        assert t.numpy_dtype() == pc.dtype_of(members, item)
        got = _records(t)
        for name in rec.dtype.names:
            np.testing.assert_array_equal(got[name], rec[name], err_msg=name)
        assert t.read_attr("CLASS") == "TABLE" and t.read_attr("VERSION") == "3.0"
        assert [t.read_attr("FIELD_%d_NAME" % i) for i in range(len(members))] == [m[0] for m in members]
        assert t.read_attr("nevents").tolist() == [float(n_events)] and t.read_attr("abstime").tolist() == [1520304327.0]
        assert t.read_attr("calgrp") == "fixture_cal"
        assert (t.read_attr("rname") is None) == (kind == "norm") and t.read_attr("no_such") is None
    with h5records.RecordInput(_fixture(kind), "Chanmap") as c:
        assert c.n_rows == 28 and c.members == pc.CHANMAP and c.read_attr("TITLE") == "channel map"
        assert _records(c).tobytes() == pc.chanmap_rows().tobytes()

    # what a writer does around the model: Chanmap, a table of the input's type, its attributes, the rows in pieces
    out_path = str(tmp_path / "copy.h5")
    with h5records.RecordInput(_fixture(kind), pc.FIXTURE_TABLES[kind]) as t:
        buf = np.zeros((t.n_rows, t.item_size), np.uint8)
        t.read_records(0, t.n_rows, buf)
        with h5records.RecordOutput(out_path) as out:
            out.copy_dataset(t, "Chanmap")
            out.create_table_like(t)
            out.copy_table_attrs(t)
            for r0, r1 in ((0, 17), (17, 17), (17, 100), (100, t.n_rows)):
                out.append(np.ascontiguousarray(buf[r0:r1]), r1 - r0)
            out.flush()
        names = ["CLASS", "TITLE", "VERSION", "abstime", "runtime", "calgrp", "nevents", "rname", "scalingfactor"]
        names += ["FIELD_%d_NAME" % i for i in range(len(members) + 1)]
        with h5records.RecordInput(out_path, pc.FIXTURE_TABLES[kind]) as u:
            assert u.members == t.members and u.item_size == t.item_size and u.n_rows == t.n_rows
            for a in names:
                x, y = t.read_attr(a), u.read_attr(a)
                assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), a
        with h5records.RecordInput(out_path, "Chanmap") as c:
            assert _records(c).tobytes() == pc.chanmap_rows().tobytes() and c.read_attr("TITLE") == "channel map"
    _assert_members_equal(out_path, pc.FIXTURE_TABLES[kind], feat, rec)


def test_bad_arguments_fail_with_a_message(tmp_path):
    from waveformml_amd.psd import h5records
    from waveformml_amd.psd.h5records import H5RecordError
    with pytest.raises(H5RecordError, match="cannot open"):
        h5records.RecordInput(str(tmp_path / "missing.h5"), "WaveformPairCal")
    with pytest.raises(H5RecordError, match="no table"):
        h5records.RecordInput(_fixture("cal"), "WaveformPairNorm")
    # a table that is not of a compound type: the group-layout fixture's coordinate dataset
    plain = os.path.join(GOLD, "h5", "combined", "Combined_0_WaveformPairSim.h5")
    with pytest.raises(H5RecordError, match="compound"):
        h5records.RecordInput(plain, "WaveformPairs/coord")
    with pytest.raises(H5RecordError, match="not a dataset"):
        h5records.RecordInput(plain, "WaveformPairs")
    with h5records.RecordInput(_fixture("cal"), "WaveformPairCal") as t:
        buf = np.zeros((t.n_rows, t.item_size), np.uint8)
        for r0, r1 in ((-1, 3), (5, 2), (0, t.n_rows + 1), (t.n_rows, t.n_rows + 1)):
            with pytest.raises(H5RecordError, match="rows"):
                t.read_records(r0, r1, buf)
        with pytest.raises(H5RecordError, match="buffer"):
            t.read_records(0, 4, buf[:3])
        t.read_records(t.n_rows, t.n_rows, buf)                       # an empty range is fine
        with pytest.raises(KeyError):
            t.member("phys")
        with h5records.RecordOutput(str(tmp_path / "o.h5")) as out:
            with pytest.raises(H5RecordError, match="no table"):
                out.append(buf, 1)
            with pytest.raises(H5RecordError, match="no dataset"):
                out.copy_dataset(t, "NoSuchMap")
            with pytest.raises(H5RecordError, match="overlap"):
                out.create_table("x", [("a", 0, pc.I32, 2), ("b", 4, pc.I32, 1)], 12)
            with pytest.raises(H5RecordError, match="not described inside"):
                out.create_table("x", [("a", 8, pc.F64, 1)], 12)
            out.create_table_like(t)
            with pytest.raises(H5RecordError, match="buffer"):
                out.append(buf[:2], 3)


def test_chunks_equal_the_references_next_chunk(gold):
    from waveformml_amd.psd.PredictionWriter import chunk_bounds, chunk_events
    checked = 0
    for name, events in pc.chunk_columns().items():
        np.testing.assert_array_equal(events, gold["chunkcol_%s" % name])
        n = len(events)
        sizes = pc.chunk_sizes(n)
        assert {1, 7, n - 1, n, n + 1} <= set(sizes)
        for nrows in sizes:
            got = chunk_bounds(events, nrows)
            want = [tuple(int(v) for v in r) for r in gold["chunks_%s_%d" % (name, nrows)]]
            assert got == want, (name, nrows)
            counts = chunk_events(events, got)
            assert counts == [pc.n_events(events[a:b]) for a, b in got]
            checked += 1
    assert checked >= 25
    tail = gold["chunks_tail_16"]
    assert tail[-1].tolist() == [16, 40]                               # the last event spans the final boundary
    assert chunk_bounds(np.zeros(0, np.int32), 8) == []
    with pytest.raises(ValueError):
        chunk_bounds(np.zeros(3, np.int32), 0)


def test_host_restatements_equal_the_reference_goldens(gold):
    """host_renumber / host_normalize / host_swap (tests/prediction_cases.py) against what the reference's own functions
    recorded, bit for bit: the GPU end-to-end tests compose them with a module's forward."""
    assert float(gold["z_scale"]) == 1200.0
    assert pc.host_renumber(np.array([5, 5, 9, 9, 5])).tolist() == [0, 0, 1, 1, 2]
    for name, lay, width, n, pattern, gkind, seed in pc.PREPARE_CASES:
        rec = pc.make_records(lay, width, n, pattern, seed)
        coords = np.array(rec["coord"]).reshape(n, 3)
        np.testing.assert_array_equal(pc.host_renumber(coords[:, 2]), gold["prep_%s_coords" % name][:, 2], err_msg=name)
        np.testing.assert_array_equal(coords[:, :2], gold["prep_%s_coords" % name][:, :2])
        if "waveform" in rec.dtype.names:
            got = pc.host_normalize(coords, np.asarray(rec["waveform"]).reshape(n, width), pc.gains_table(gkind))
            assert got.tobytes() == gold["prep_%s_feats" % name].tobytes(), name
    for case in pc.SCATTER_CASES:
        name, lay, width, n, pattern, seed, mode, L, member, col0, affine = case
        if mode == "rows":
            continue
        rec = pc.make_records(lay, width, n, pattern, seed)
        coords = np.array(rec["coord"]).reshape(n, 3)
        for dt in pc.scatter_dtypes(case):
            src = pc.scatter_source(mode, L, n, pc.n_events(coords[:, 2]), seed, dt).float().numpy()
            if affine:
                src = (src - np.float32(0.5)) * np.float32(gold["z_scale"])
            got = pc.host_swap(mode, np.zeros((n, L), np.float32), src, coords)
            assert got.tobytes() == gold["scat_%s_%s" % (name, dt)].tobytes(), (name, dt)


def test_writer_library_survives_damaged_files_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "waveformml_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asan_writer"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "waveformml_amd", "lib", "h5writer_sanitize_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("h5writer_sanitize:")][-1]
    assert "2500 rows round trip" in line
    ok = int(line.split("calls (")[1].split(" ok")[0])
    refused = int(line.split(" ok, ")[1].split(" refused")[0])
    damaged = int(line.split("round trip, ")[1].split(" damaged")[0])
    assert ok > 500 and refused > 500 and damaged >= 25, line


def test_writer_library_exports_and_ctypes_table_mirror_its_header():
    from waveformml_amd.psd import h5records
    text = open(os.path.join(ROOT, "include", "wfh5w.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(wfh5w_[a-z0-9_]+)\s*\(", text)))
    assert len(names) == 17 and sorted(h5records.SIGNATURES) == names
    lib = ctypes.CDLL(h5records.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "libwfh5w.so does not export %s" % n
    assert ctypes.sizeof(h5records.Member) == 80                     # struct wfh5w_member: char[64] + int64 + 2 x int32
    # the reader's header is untouched: the writer shares no symbol with it
    reader = open(os.path.join(ROOT, "include", "wfh5.h")).read()
    assert "wfh5w_" not in reader


def test_prediction_kernels_are_declared_exported_and_bound():
    from waveformml_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("wfs_predict_prepare", "wfs_predict_scatter", "wfs_predict_workspace_ints"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert _lib.WFS_PREDICT_ROWS_PER_BLOCK == pc.T
    assert _lib.load().wfs_predict_workspace_ints(3 * pc.T + 7) == 4
    header = open(os.path.join(ROOT, "include", "wfsparse.h")).read()
    assert "#define WFS_PREDICT_ROWS_PER_BLOCK %d" % pc.T in header and "#define WFS_ABI_VERSION 6" in header


def test_calgroup_and_foreign_datatypes_raise():
    from waveformml_amd.psd.PredictionWriter import ZPredictionWriter, gain_factors
    cfg = {"system_config": {}, "net_config": {}}
    with pytest.raises(NotImplementedError, match="calibration database"):
        ZPredictionWriter("o.h5", _fixture("cal"), cfg, "none.ckpt", calgroup="x")
    with pytest.raises(NotImplementedError, match="PhysPulse"):
        ZPredictionWriter("o.h5", _fixture("cal"), cfg, "none.ckpt", datatype="PhysPulse")
    with pytest.raises(IOError, match="unrecognized datatype"):
        ZPredictionWriter("o.h5", _fixture("cal"), cfg, "none.ckpt", datatype="Waveform")
    g = np.full((14, 11, 2), 2.0)
    assert gain_factors(g).dtype == np.float64 and gain_factors(g, 1.5).dtype == np.float32
    assert gain_factors(g)[0, 0, 0] == 690.0 / 16383 / 2.0
    with pytest.raises(ValueError):
        gain_factors(np.ones((14, 11)))
