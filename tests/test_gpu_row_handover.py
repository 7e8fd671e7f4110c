"""wfs_load_rows_batch (csrc/optim.hip), the one-launch hand-over of a per-row batch into a captured step, against the
torch composition it replaces in psd/graph._CapturedRunner._load: slice copies, ``fill_`` of the whole target buffer,
``coords[:, perm]``, the row-count fill and the existing wfs_event_offsets entry.  Every destination buffer is compared
BIT FOR BIT as bytes.  Both sides start from buffers pre-filled with a sentinel byte, so the comparison also shows that
feature and coordinate rows at and beyond ``n`` are not written while every target row there holds the pad element."""
import ctypes

import numpy as np
import pytest
import torch

from waveformml_amd import _lib
from waveformml_amd.psd.graph import _pad_element

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0xA5
N_CAP, B = 64, 40

# (dtype, trailing shape, pad value): the criterion's ignore_index as labels.fill_ stores it
TARGETS = [(torch.int64, (), -100), (torch.float32, (), -100), (torch.float32, (2,), -100), (torch.float32, (7,), -100)]
# (cols, permutation or None, source offset in ints)
COORDS = [(1, None, 0), (3, [2, 0, 1], 0), (4, [3, 0, 1, 2], 0), (4, [3, 0, 1, 2], 1)]


def sentinel(nbytes):
    return torch.full((max(int(nbytes), 1),), SENTINEL, dtype=torch.uint8, device=DEV)[:int(nbytes)]


def offset_view(values, offset_bytes):
    """``values`` (a host uint8 array) on the device, starting ``offset_bytes`` into a fresh allocation."""
    buf = torch.zeros((len(values) + offset_bytes + 16,), dtype=torch.uint8, device=DEV)
    view = buf[offset_bytes:offset_bytes + len(values)]
    view.copy_(torch.from_numpy(values))
    return view


def event_column(rng, n, pattern):
    """A batch column of n rows over at most B events: every event with rows ("full"), empty events in the middle and
    at the end ("gaps"), or "full" with the LAST row stepping down (the one disorder that leaves no table word to two
    writers, so the two sides can be compared word for word)."""
    if n == 0:
        return np.zeros((0,), np.int32)
    if pattern == "gaps":
        used = np.sort(rng.choice(np.arange(0, B - 5), size=min(n, 9), replace=False))     # the last 5 stay empty too
        ev = np.sort(used[rng.integers(0, len(used), size=n)])
    else:
        ev = np.sort(np.r_[np.arange(min(n, B)), rng.integers(0, min(n, B), size=max(0, n - B))])
    ev = ev.astype(np.int32)
    if pattern == "decreasing" and n > 2:
        assert ev[n - 2] >= 1
        ev[n - 1] = ev[n - 2] - 1
    return ev


class Case(object):
    def __init__(self, n, n_cap, coords, row_bytes, target, seed, feat_offset=0, pattern="full", images=0):
        rng = np.random.default_rng(seed)
        self.n, self.n_cap, self.row_bytes = n, n_cap, row_bytes
        self.cols, self.perm, coord_offset = coords
        c = rng.integers(0, 14, size=(n, self.cols)).astype(np.int32)
        self.ev_col = self.perm[0] if self.perm is not None else 0
        c[:, self.ev_col] = event_column(rng, n, pattern)
        self.coords = offset_view(c.reshape(-1).view(np.uint8), 4 * coord_offset).view(torch.int32).view(n, self.cols)
        self.feats = offset_view(rng.integers(0, 256, size=n * row_bytes, dtype=np.uint8), feat_offset)
        self.t_dtype, self.t_trail, self.pad = target
        shape = (n,) + self.t_trail
        if self.t_dtype == torch.int64:
            t = torch.from_numpy(rng.integers(-5, 5, size=shape))
        else:
            t = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
        self.targets = t.to(DEV)
        self.t_row_bytes = int(np.prod(self.t_trail, dtype=np.int64)) * t.element_size()
        self.events = B if self.perm is not None else 0
        self.n_images = images
        if images:
            self.W = torch.from_numpy(rng.standard_normal((3, 32, 32)).astype(np.float32)).to(DEV)

    def destinations(self):
        lib = _lib.load()
        d = {"coords": sentinel(self.n_cap * self.cols * 4), "feats": sentinel(self.n_cap * self.row_bytes),
             "targets": sentinel(self.n_cap * self.t_row_bytes), "n_valid": sentinel(8)}
        if self.perm is not None:
            d["indices"] = sentinel(self.n_cap * self.cols * 4)
            d["events"] = sentinel(4 * int(lib.wfs_event_offsets_ints(self.events)))
        if self.n_images:
            d["img_fwd"] = sentinel(int(lib.wfs_filter_image_bytes(3)))
            d["img_t"] = sentinel(int(lib.wfs_filter_image_bytes(3)))
        return d

    def jobs(self, d):
        jobs = (_lib.FilterImageJob * 1)()
        if self.n_images:
            jobs[0].W, jobs[0].img_fwd, jobs[0].img_t = self.W.data_ptr(), d["img_fwd"].data_ptr(), d["img_t"].data_ptr()
            jobs[0].K, jobs[0].dtype = 3, _lib.WFS_BF16
        return jobs

    def entry(self, d=None, n=None, n_cap=None, elem=None, perm=None, null=()):
        """The one launch; returns (status, destinations).  ``null``: destinations passed as NULL."""
        d = d if d is not None else self.destinations()
        ptr = lambda k: None if (k in null or k not in d) else _lib.ptr(d[k])          # noqa: E731
        perm = perm if perm is not None else self.perm
        rc = _lib.load().wfs_load_rows_batch(
            _lib.ptr(self.coords), self.n if n is None else n, self.n_cap if n_cap is None else n_cap, self.cols,
            _lib.i32_array(perm) if perm is not None else None, ptr("coords"), ptr("indices"), _lib.ptr(self.feats),
            ptr("feats"), self.row_bytes, _lib.ptr(self.targets), ptr("targets"), self.t_row_bytes,
            self.targets.element_size() if elem is None else elem, _pad_element(self.t_dtype, self.pad), ptr("n_valid"),
            ptr("events"), self.events, self.jobs(d) if self.n_images else None, self.n_images, _lib.stream_ptr())
        return rc, d

    def composition(self):
        """What _CapturedRunner._load does for a per-row batch without the entry."""
        lib, d, n = _lib.load(), self.destinations(), self.n
        d["coords"].view(torch.int32).view(self.n_cap, self.cols)[:n].copy_(self.coords)
        if self.row_bytes:
            d["feats"].view(self.n_cap, self.row_bytes)[:n].copy_(self.feats.view(n, self.row_bytes))
        labels = d["targets"].view(self.t_dtype).view((self.n_cap,) + self.t_trail)
        labels.fill_(self.pad)
        labels[:n].copy_(self.targets)
        n_valid = d["n_valid"].view(torch.int64)
        n_valid.fill_(n)
        if self.perm is not None:
            indices = d["indices"].view(torch.int32).view(self.n_cap, self.cols)
            indices[:n].copy_(self.coords[:, self.perm])
            # the event table of the VALID rows: the sentinel rows beyond n are never read (n_valid)
            _lib.check(lib.wfs_event_offsets(_lib.ptr(indices), self.n_cap, self.cols - 1, self.events, _lib.ptr(n_valid),
                                             _lib.ptr(d["events"]), _lib.stream_ptr()))
        if self.n_images:
            _lib.check(lib.wfs_conv_filter_images(_lib.ptr(self.W), 3, _lib.WFS_BF16, _lib.ptr(d["img_fwd"]),
                                                  _lib.ptr(d["img_t"]), _lib.stream_ptr()))
        return d

    def check(self, what):
        rc, got = self.entry()
        assert rc == _lib.WFS_OK, (what, _lib.last_error())
        want = self.composition()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(got[k], want[k]), (what, k)
        n = self.n
        assert bool((got["feats"][n * self.row_bytes:] == SENTINEL).all()), what
        assert bool((got["coords"][n * self.cols * 4:] == SENTINEL).all()), what
        pads = got["targets"].view(self.t_dtype).view((self.n_cap,) + self.t_trail)[n:]
        assert bool((pads == self.pad).all()), what
        return got


def test_every_shape_matches_the_composition_bit_for_bit():
    """n in {0, 1, 63, 64} of a capacity of 64 x the four coordinate forms x feature rows of 4, 28, 260 and 520 bytes,
    the four target forms taken in turn."""
    k = 0
    for n in (0, 1, 63, 64):
        for ci, coords in enumerate(COORDS):
            for ri, row_bytes in enumerate((4, 28, 260, 520)):
                target = TARGETS[(ci + ri + k) % 4]
                Case(n, N_CAP, coords, row_bytes, target, seed=1000 + k).check((n, coords, row_bytes, target))
                k += 1


@pytest.mark.parametrize("target", TARGETS, ids=["int64", "f32", "f32x2", "f32x7"])
def test_every_target_form_at_every_row_count(target):
    for n in (0, 1, 63, 64):
        Case(n, N_CAP, COORDS[1], 28, target, seed=7 + n).check((n, target))


@pytest.mark.parametrize("row_bytes", [28, 260, 520])
def test_feature_source_offset_by_four_bytes(row_bytes):
    """A slice of a packed buffer that starts 4 bytes off a 16-byte boundary: the byte path."""
    for n in (1, 63, 64):
        case = Case(n, N_CAP, COORDS[1], row_bytes, TARGETS[1], seed=50 + n, feat_offset=4)
        assert case.feats.data_ptr() % 16 == 4
        case.check((n, row_bytes))


@pytest.mark.parametrize("pattern", ["full", "gaps", "decreasing"])
def test_event_offsets_and_flag_words(pattern):
    """The table and the flag words are wfs_event_offsets': every event with rows, empty events in the middle and at the
    end, and a batch column that steps down once (a flag word is set -- the same one)."""
    lib = _lib.load()
    for coords in COORDS[1:3]:
        for n in (0, 63):
            got = Case(n, N_CAP, coords, 28, TARGETS[0], seed=90 + n, pattern=pattern).check((pattern, coords, n))
            table = got["events"].view(torch.int32).cpu().numpy()
            assert len(table) == int(lib.wfs_event_offsets_ints(B))
            assert bool(table[B + 1:].any()) == (pattern == "decreasing" and n > 0), (pattern, n, table[B + 1:])
            if pattern != "decreasing" or n == 0:      # (the row that steps down is the one that would write the tail)
                assert np.all(np.diff(table[:B + 1]) >= 0) and table[0] == 0 and table[B] == n


def test_one_image_job_in_the_same_launch():
    got = Case(63, N_CAP, COORDS[2], 260, TARGETS[0], seed=3, images=1).check("images")
    assert not bool((got["img_fwd"] == SENTINEL).all()) and not bool((got["img_t"] == SENTINEL).all())
    Case(0, N_CAP, COORDS[1], 260, TARGETS[1], seed=4, images=1).check("images, no rows")


def test_grid_stride_loops_take_more_than_one_pass():
    """8200 rows of 520 bytes: 266500 16-byte lanes and 8256 x 7 target elements against a grid capped at 1024 blocks of
    256 threads."""
    Case(8200, 8256, COORDS[2], 520, TARGETS[3], seed=11).check("large")
    Case(8200, 8256, COORDS[1], 520, TARGETS[0], seed=12, feat_offset=4).check("large, byte path")


def test_bad_arguments_return_einval_and_launch_nothing():
    case = Case(63, N_CAP, COORDS[1], 28, TARGETS[1], seed=5)
    bad = [dict(n=65), dict(elem=3), dict(perm=[2, 0, 3]), dict(perm=[-1, 0, 1]), dict(null=("feats",)),
           dict(null=("targets",)), dict(n_cap=62)]
    for kw in bad:
        rc, d = case.entry(**kw)
        assert rc == _lib.WFS_EINVAL and _lib.last_error(), kw
        torch.cuda.synchronize()
        for k, buf in d.items():
            assert bool((buf == SENTINEL).all()), (kw, k)
    # the coordinate destinations alone MAY be NULL
    rc, d = case.entry(null=("coords", "indices"))
    torch.cuda.synchronize()
    assert rc == _lib.WFS_OK and bool((d["coords"] == SENTINEL).all()) and bool((d["indices"] == SENTINEL).all())
    assert torch.equal(d["feats"], case.composition()["feats"])
    assert isinstance(_pad_element(torch.float32, -100), ctypes.Array) and _pad_element(torch.float16, -100) is None
