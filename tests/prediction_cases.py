"""Shared by the prediction-writer tests and their golden generator (tests/golden/make_prediction_goldens.py): record
layouts, seeded raw-record buffers and the case lists.  Inputs are rebuilt from seeds on both sides; the golden file holds
only what the reference's functions made of them.

T is the kernel's workgroup size in rows (WFS_PREDICT_ROWS_PER_BLOCK).  Event patterns and row counts sit on its
boundaries; row widths 2L are 2, 130 (L = 65: the PMT-side boundary falls inside an aligned int16 pair) and 300."""
import numpy as np

T = 256
NX, NY = 14, 11
I16, I32, I64, F32, F64 = 0, 1, 2, 3, 4                  # include/wfh5w.h element kinds
_FMT = {I16: "<i2", I32: "<i4", I64: "<i8", F32: "<f4", F64: "<f8"}

# (name, offset, kind, count): reference src/datasets/H5CompoundTypes.py WaveformPairCal (packed, 324 bytes) and
# WaveformPairNorm (explicit offsets, 584 bytes)
CAL_MEMBERS = [("evt", 0, I64, 1), ("t", 8, F64, 1), ("dt", 16, F32, 1), ("z", 20, F32, 1), ("E", 24, F32, 1),
               ("PSD", 28, F32, 1), ("PE", 32, F32, 2), ("coord", 40, I32, 3), ("waveform", 52, I16, 130),
               ("EZ", 312, F32, 2), ("PID", 320, I32, 1)]
CAL_ITEM = 324
NORM_MEMBERS = [("t", 560, F64, 1), ("coord", 520, I32, 3), ("pulse", 0, F32, 130), ("phys", 532, F32, 7),
                ("EZ", 572, F32, 2), ("PID", 568, I32, 1)]
NORM_ITEM = 584


def odd_layout(width, pulse=False):
    """A synthetic layout whose item size is 2 mod 4 and whose members sit at offsets that are 2 mod 4: alignment shifts
    from row to row, every record access takes the 2-byte path."""
    members, off = [("tag", 0, I16, 1)], 2
    members.append(("coord", off, I32, 3))
    off += 12
    members.append(("waveform" if not pulse else "pulse", off, F32 if pulse else I16, width))
    off += width * (4 if pulse else 2)
    members.append(("phys", off, F32, 7))
    off += 28
    members.append(("EZ", off, F32, 2))
    off += 8
    if off % 4 == 0:
        members.append(("pad", off, I16, 1))
        off += 2
    assert off % 4 == 2
    return members, off


def dtype_of(members, item):
    return np.dtype({"names": [m[0] for m in members],
                     "formats": [(_FMT[m[2]], (m[3],)) if m[3] > 1 else _FMT[m[2]] for m in members],
                     "offsets": [m[1] for m in members], "itemsize": item})


def layout(name, width=130):
    """(members, item size) of "cal", "norm", "odd" (waveform) or "oddp" (pulse)."""
    if name == "cal":
        assert width == 130
        return CAL_MEMBERS, CAL_ITEM
    if name == "norm":
        assert width == 130
        return NORM_MEMBERS, NORM_ITEM
    return odd_layout(width, pulse=(name == "oddp"))


def member(members, name):
    return [m for m in members if m[0] == name][0]


def event_numbers(pattern, n, rng):
    """int32 [n] event numbers of a named pattern."""
    if pattern == "one":
        return np.full(n, 7, np.int32)
    if pattern == "each":
        return (np.arange(n, dtype=np.int64) * 3 + 11).astype(np.int32)
    if pattern == "59955":
        base = np.array([5, 5, 9, 9, 5], np.int32)
        return np.resize(base, n)
    if pattern == "extremes":
        lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
        runs = np.array([lo, lo, hi, hi, hi, lo, 0, hi, lo + 1, hi - 1], np.int32)
        return np.repeat(np.resize(runs, (n + 2) // 3), 3)[:n]
    if pattern in ("at", "before", "after"):
        # one change exactly at / one row before / one row after every workgroup boundary, and nowhere else
        shift = {"at": 0, "before": -1, "after": 1}[pattern]
        ev = np.zeros(n, np.int64)
        for b in range(T, n + T, T):
            if 0 < b + shift < n:
                ev[b + shift:] += 1
        return (ev * 2 + 40).astype(np.int32)
    assert pattern == "runs"
    ev, out, e = [], 0, 100
    while out < n:
        k = int(rng.integers(1, 7))
        ev += [e] * k
        out += k
        e += int(rng.integers(1, 4)) if rng.random() > 0.1 else -int(rng.integers(1, 3))     # numbers may go back
    return np.array(ev[:n], np.int32)


def make_records(layout_name, width, n, pattern, seed):
    """Seeded structured array [n] of the layout, every byte defined (padding bytes too: they must survive)."""
    members, item = layout(layout_name, width)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(max(n, 1), item), dtype=np.uint8)[:n]
    rec = raw.view(dtype_of(members, item)).reshape(n)
    ev = event_numbers(pattern, n, rng)
    rec["coord"][:, 0] = rng.integers(0, NX, n)
    rec["coord"][:, 1] = rng.integers(0, NY, n)
    corners = [(0, 0), (0, NY - 1), (NX - 1, 0), (NX - 1, NY - 1)]
    for i in range(min(n, 4)):
        rec["coord"][(i * 7) % n, :2] = corners[i]
    rec["coord"][:, 2] = ev
    if "waveform" in rec.dtype.names:
        wf = rng.integers(-2000, 12000, size=(n, width)).astype(np.int16)
        wf[0, 0], wf[0, -1], wf[-1, width // 2 - 1], wf[-1, width // 2] = -32768, 32767, 32767, -32768
        rec["waveform"] = wf if width > 1 else wf[:, 0]
    else:
        rec["pulse"] = rng.random((n, width), dtype=np.float32) * 2 - 0.5
    for name in ("phys", "EZ"):
        if name in rec.dtype.names:
            rec[name] = rng.standard_normal(rec[name].shape).astype(np.float32)
    return rec


def gains_table(kind, seed=5):
    """gain_factors [NX, NY, 2] as the writers form them: float64-born (no scale factor) or float32-born."""
    rng = np.random.default_rng(seed)
    gains = 0.6 + 0.8 * rng.random((NX, NY, 2))
    if kind == "f32":
        return np.divide(np.full((NX, NY, 2), 1.3 * 690.0 / (2 ** 14 - 1), dtype=np.float32), gains.astype(np.float32))
    return np.divide(np.full((NX, NY, 2), 690.0 / (2 ** 14 - 1)), gains)


# name, layout, width, n, event pattern, gains kind, seed
PREPARE_CASES = (
    [("n%d" % n, "odd", 2, n, "runs", "f64", 100 + n) for n in (1, 2, T - 1, T, T + 1, 3 * T + 7)]
    + [("p_%s" % p, lay, 2, 3 * T + 7, p, "f32", 200 + i)
       for i, (p, lay) in enumerate([("one", "odd"), ("each", "oddp"), ("at", "odd"), ("before", "oddp"), ("after", "odd"),
                                     ("59955", "odd"), ("extremes", "oddp")])]
    + [("p5", "odd", 2, 5, "59955", "f64", 300),
       ("cal_f64", "cal", 130, T + 1, "runs", "f64", 301), ("cal_f32", "cal", 130, 65, "runs", "f32", 302),
       ("norm", "norm", 130, T + 1, "runs", "f64", 303), ("odd130", "odd", 130, 37, "runs", "f32", 304),
       ("odd300", "odd", 300, 40, "runs", "f64", 305), ("oddp300", "oddp", 300, 19, "each", "f64", 306)])

# name, layout, width, n, pattern, seed, mode, L, member, col0, affine
SCATTER_CASES = []
for _lay, _w in (("cal", 130), ("norm", 130), ("odd", 2)):
    for _n, _p in ((1, "runs"), (2, "runs"), (T - 1, "at"), (T, "before"), (T + 1, "after"), (3 * T + 7, "runs"),
                   (5, "59955"), (T + 1, "one"), (T + 1, "each"), (T + 1, "extremes")):
        _tag = "%s_%d_%s" % (_lay, _n, _p)
        SCATTER_CASES.append(("dense1_" + _tag, _lay, _w, _n, _p, 400 + _n, "dense", 1, "EZ", 1, True))
        if _lay != "cal":                                  # WaveformPairCal has no phys member
            SCATTER_CASES.append(("dense5_" + _tag, _lay, _w, _n, _p, 500 + _n, "dense", 5, "phys", 2, False))
            SCATTER_CASES.append(("event3_" + _tag, _lay, _w, _n, _p, 600 + _n, "event", 3, "phys", 4, False))
            SCATTER_CASES.append(("rows5_" + _tag, _lay, _w, _n, _p, 700 + _n, "rows", 5, "phys", 2, False))


# 16-bit sources: the cases whose pattern crosses a workgroup boundary, and the smallest one
def scatter_dtypes(case):
    return ("f32", "bf16", "f16") if case[4] in ("after", "59955") else ("f32",)


def n_events(ev):
    ev = np.asarray(ev)
    return int(1 + np.count_nonzero(ev[1:] != ev[:-1])) if len(ev) else 0


def scatter_source(mode, L, n, B, seed, dtype="f32"):
    """The model output of a scatter case: float32 VALUES representable in ``dtype`` (so every dtype shares one golden
    per dtype tag)."""
    import torch
    rng = np.random.default_rng(seed + 9000)
    shape = {"dense": (B, L, NX, NY), "event": (B, L), "rows": (n, L)}[mode]
    v = torch.from_numpy(rng.random(shape, dtype=np.float32) * 1.5 - 0.25)
    td = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)[dtype]
    return v.to(td)


# event columns for the chunking test: name -> int32 array; `tail` ends in an event that spans the final boundary
def chunk_columns():
    rng = np.random.default_rng(77)
    cols = {"runs": event_numbers("runs", 131, rng), "59955": event_numbers("59955", 23, rng),
            "one": event_numbers("one", 17, rng), "each": event_numbers("each", 19, rng)}
    tail = event_numbers("runs", 40, rng)
    tail[-9:] = tail[-10] + 50                       # the last event is 9 rows long
    cols["tail"] = tail
    return cols


def chunk_sizes(n):
    return sorted({1, 7, 16, n - 1, n, n + 1} - {0})


# ---- the fixture files ----
N_ROWS = 130
FIXTURE_FILES = {"cal": "pred_1_WFCal.h5", "norm": "pred_1_WFNorm.h5"}
FIXTURE_TABLES = {"cal": "WaveformPairCal", "norm": "WaveformPairNorm"}
CHANMAP = [("chan", 0, I32, 1), ("seg", 4, I32, 1), ("pmt", 8, I32, 1), ("pos", 12, F32, 2)]


def chanmap_rows():
    chan = np.zeros(28, dtype=dtype_of(CHANMAP, 20))
    chan["chan"], chan["seg"], chan["pmt"] = np.arange(28), np.arange(28) // 2, np.arange(28) % 2
    chan["pos"] = np.stack([np.arange(28) * 0.5, np.arange(28) * -1.25], 1)
    return chan


def fixture_records(kind):
    """(records, events) of the fixture files under tests/golden/h5/pred/ (tests/golden/make_prediction_fixtures.py)."""
    rec = make_records(kind, 130, N_ROWS, "runs", 902 if kind == "cal" else 901)
    rng = np.random.default_rng(903)
    ev = rec["coord"][:, 2].copy()
    ev[-6:] = ev[-7] + 4
    rec["coord"][:, 2] = ev
    starts = np.flatnonzero(np.concatenate([[True], ev[1:] != ev[:-1]]))
    for s, e in zip(starts, list(starts[1:]) + [N_ROWS]):
        cells = rng.permutation(NX * NY)[:e - s]
        rec["coord"][s:e, 0], rec["coord"][s:e, 1] = cells // NY, cells % NY
    if kind == "cal":
        rec["evt"] = ev
        rec["waveform"] = np.clip(rec["waveform"], -200, 9000)
        rec["waveform"][0, 0], rec["waveform"][0, -1] = -32768, 32767
    rec["PID"] = rng.integers(0, 6, N_ROWS)
    rec["t"] = np.cumsum(rng.random(N_ROWS))
    return rec, len(starts)


# ---- vectorised restatements of the reference's row walks (checked against the goldens in tests/test_prediction_io.py;
# the end-to-end GPU tests compose them with the module's eager forward) ----
def host_renumber(ev):
    """normalize_waveforms' event column: +1 wherever the number changes, from 0."""
    ev = np.asarray(ev)
    return np.concatenate([[0], np.cumsum(ev[1:] != ev[:-1])]).astype(np.int32) if len(ev) else np.zeros(0, np.int32)


def host_normalize(coords, wf, gain_factors):
    """normalize_waveforms' output: the product formed in the gain table's own dtype promotion, stored as float32."""
    half = wf.shape[1] // 2
    g = gain_factors[coords[:, 0], coords[:, 1]]                       # [n, 2]
    side = (np.arange(wf.shape[1]) >= half).astype(np.int64)
    return (wf.astype(np.float64) * g[:, side].astype(np.float64)).astype(np.float32)


def host_swap(mode, target, src, coords):
    """swap_sparse_from_dense (per plane) / swap_sparse_from_event / plain assignment into ``target`` [n, L]."""
    e = host_renumber(coords[:, 2])
    if mode == "dense":
        target[:] = src[e[:, None], np.arange(src.shape[1])[None, :], coords[:, 0:1], coords[:, 1:2]]
    elif mode == "event":
        target[:] = src[e]
    else:
        target[:] = src[:len(target)]
    return target
