"""The record arm of the event-local strided rulebook build (csrc/evconv.hip, `Rec`): a thread keeps three rows of its
event digested in two registers each and every phase walks those records; rows past the 1536th of an event are digested
again in every phase.  Every case runs the device-count build (capacities for N and M, the valid counts in device memory:
what a captured step runs) against the exact-size build, which takes the chip-wide kernels of rulebook.hip, bit for bit:
output coordinates in first-seen order, both tables, the output set's event offsets and the cell -> row map.  The PSD
geometry is also held against the CPU oracle directly (oracle.ref.get_indice_pairs).  Event sizes sit on both sides of
every boundary of the row cache (512, 1024, 1536 rows); the geometries the record arm refuses (a leading stride, a
strided last dimension that does not pack) pin the path that was kept for them.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THREADS, R = 512, 3                       # evconv.hip: threads of a workgroup, EC_REC_PER_THREAD
PSD = ((14, 11, 256), (3, 3, 3), (1, 1, 4), (0, 0, 0))
SIZES_SMALL = (0, 1, 511, 512, 513)
SIZES_LARGE = (1024, 1025, R * THREADS, R * THREADS + 1, R * THREADS + 600)


def _events(rng, shape, sizes):
    """Distinct random sites, sizes[b] of them in event b, grouped by event, random order inside an event."""
    vol = int(np.prod(shape))
    rows = []
    for b, s in enumerate(sizes):
        assert s <= vol
        pos = rng.choice(vol, size=s, replace=False)
        cols = [np.full(s, b)]
        for d in range(len(shape)):
            cols.append((pos // int(np.prod(shape[d + 1:]))) % shape[d])
        rows.append(np.stack(cols, 1))
    return np.ascontiguousarray(np.concatenate(rows).astype(np.int32))


def _exact(t, B, shape, ksize, stride, padding):
    from waveformml_amd.spconv import ops
    return ops.build_rulebook(t, B, list(shape), list(ksize), list(stride), list(padding), [1] * len(shape), False,
                              known_unique=True)


def _device_count(t, n_dev, B, shape, ksize, stride, padding, cap_m, events=None):
    from waveformml_amd.spconv import ops
    rb = ops.build_rulebook(t, B, list(shape), list(ksize), list(stride), list(padding), [1] * len(shape), False,
                            n_dev=n_dev, out_capacity=cap_m, events=events)
    torch.cuda.synchronize()
    assert rb.events_out is not None              # the event-local build ran
    return rb


def _padded(t, extra=313):
    pad = torch.cat([t, torch.full((extra, t.shape[1]), 99999, dtype=torch.int32, device=DEV)])
    return pad, torch.tensor([t.shape[0]], dtype=torch.int64, device=DEV)


def _assert_equal(rb, exact, B, N):
    M = int(rb.m_dev)
    assert M == exact.M and int(rb.overflow) == 0 and not rb.event_flags.any()
    assert torch.equal(rb.out_indices[:M], exact.out_indices)
    assert torch.equal(rb.nbr_out[:, :N], exact.nbr_out)
    assert torch.equal(rb.nbr_in[:, :M], exact.nbr_in)
    oi = exact.out_indices.cpu().numpy().astype(np.int64)
    assert np.array_equal(rb.events_out[:B + 1].cpu().numpy(), np.searchsorted(oi[:, 0], np.arange(B + 1)))
    assert not rb.events_out[B + 1:].any()
    lin = oi[:, 0]
    for d in range(oi.shape[1] - 1):
        lin = lin * rb.out_spatial_shape[d] + oi[:, 1 + d]
    want = np.full(B * int(np.prod(rb.out_spatial_shape)), -1, np.int32)
    want[lin] = np.arange(M, dtype=np.int32)
    assert np.array_equal(rb.cell_map[2].cpu().numpy(), want)


def _build_both(idx, B, shape, ksize, stride, padding):
    t = torch.from_numpy(idx).to(DEV)
    exact = _exact(t, B, shape, ksize, stride, padding)
    pad, nv = _padded(t)
    rb = _device_count(pad, nv, B, shape, ksize, stride, padding, exact.M + 77)
    _assert_equal(rb, exact, B, idx.shape[0])
    return exact, rb


def _pair_sets(table):
    """[K, n] table of partners (-1: none) -> per offset the sorted (column, partner) pairs."""
    out = []
    for k in range(table.shape[0]):
        j = np.nonzero(table[k] >= 0)[0]
        out.append(np.stack([j, table[k, j]], 1))
    return out


@pytest.mark.parametrize("sizes", [SIZES_SMALL, SIZES_LARGE], ids=["to_513_rows", "to_2136_rows"])
def test_psd_geometry_across_the_row_cache_boundaries(sizes):
    """Events of 0 .. 513 rows, and of 1024 .. R * 512 + 600 rows (M_e in the thousands: a few offsets per image pass),
    then the second layer on the first one's output rows and event offsets; both against the exact builds, and the first
    against the CPU oracle: same out_indices, and per kernel offset the same set of (input row, output row) pairs in the
    by-input and in the by-output table."""
    from oracle import ref
    shape, ksize, stride, padding = PSD
    B = len(sizes)
    idx = _events(np.random.default_rng(31), shape, sizes)
    N = idx.shape[0]
    exact, rb = _build_both(idx, B, shape, ksize, stride, padding)
    out, pairs, num = ref.get_indice_pairs(idx, B, list(shape), list(ksize), list(stride), list(padding), 1, 0, False)
    M = int(rb.m_dev)
    assert np.array_equal(rb.out_indices[:M].cpu().numpy(), out)
    by_in = _pair_sets(rb.nbr_out[:, :N].cpu().numpy())
    by_out = _pair_sets(rb.nbr_in[:, :M].cpu().numpy())
    for k in range(pairs.shape[1]):
        want = pairs[:, k, :int(num[k])].T
        want = want[np.argsort(want[:, 0], kind="stable")]
        assert np.array_equal(by_in[k], want), k
        assert np.array_equal(by_out[k][:, ::-1], want[np.argsort(want[:, 1], kind="stable")]), k
    # the second layer: input = the first build's output rows (a capacity of them), counts and offsets from the device
    shape2 = tuple(rb.out_spatial_shape)
    assert shape2 == (12, 9, 64)
    exact2 = _exact(exact.out_indices, B, shape2, ksize, stride, padding)
    rb2 = _device_count(rb.out_indices, rb.m_dev, B, shape2, ksize, stride, padding, exact2.M + 77, events=rb.events_out)
    _assert_equal(rb2, exact2, B, M)


def test_capacity_that_cuts_inside_an_event_of_three_rows_per_thread():
    """out_capacity in the middle of the outputs of the 1537-row event: flagged, the first m_dev output rows and their
    table columns are the exact build's, partners that do not exist read -1."""
    shape, ksize, stride, padding = PSD
    B = len(SIZES_LARGE)
    idx = _events(np.random.default_rng(32), shape, SIZES_LARGE)
    N = idx.shape[0]
    t = torch.from_numpy(idx).to(DEV)
    exact = _exact(t, B, shape, ksize, stride, padding)
    ev = np.searchsorted(exact.out_indices[:, 0].cpu().numpy(), np.arange(B + 1))
    cap = int(ev[3] + ev[4]) // 2
    assert ev[3] < cap < ev[4]
    pad, nv = _padded(t)
    rb = _device_count(pad, nv, B, shape, ksize, stride, padding, cap)
    assert int(rb.overflow) == 1 and int(rb.m_dev) == cap and not rb.event_flags.any()
    assert torch.equal(rb.out_indices[:cap], exact.out_indices[:cap])
    assert torch.equal(rb.nbr_in[:, :cap], exact.nbr_in[:, :cap])
    want = torch.where(exact.nbr_out < cap, exact.nbr_out, torch.full_like(exact.nbr_out, -1))
    assert torch.equal(rb.nbr_out[:, :N], want)
    assert np.array_equal(rb.events_out[:B + 1].cpu().numpy(), np.minimum(ev, cap))
    cells = rb.cell_map[2].cpu().numpy()
    assert cells.max() == cap - 1 and np.array_equal(np.sort(cells[cells >= 0]), np.arange(cap))


@pytest.mark.parametrize("shape,ksize,stride,padding,sizes", [
    # record arm, dense form (last stride 1); an event holds 154 sites at most
    ((14, 11), (3, 3), (1, 1), (0, 0), (154, 0, 1, 153, 77, 20)),
    # record arm, padding variant of the PSD geometry
    ((14, 11, 256), (3, 3, 3), (1, 1, 4), (0, 0, 1), (513, 0, 1025, 2, 1537)),
    # record arm, 4-D (five-column rows: no 16-byte row load), packed
    ((6, 5, 4, 12), (1, 2, 2, 3), (1, 1, 1, 3), (0, 0, 0, 0), (700, 3, 1440, 0, 1100)),
    # record arm, more than 9 slots: dense 27 and packed 12
    ((6, 5, 40), (3, 3, 3), (1, 1, 1), (1, 1, 1), (600, 1, 1200, 1100)),
    ((8, 9, 40), (3, 4, 2), (1, 1, 2), (0, 1, 0), (1300, 513, 0, 1700)),
    # refused: strides on leading dimensions / a strided last dimension under a longer kernel.  (12, 30) holds 360 sites
    ((12, 30), (3, 3), (2, 2), (1, 1), (360, 0, 200, 359, 1)),
    ((10, 7, 33), (3, 2, 3), (2, 1, 3), (1, 0, 2), (513, 1100, 0, 512, 1600)),
    # refused, 4-D, from the parametrisation of test_device_count_conv_build_equals_exact_build; one event above 512 rows
    ((6, 5, 4, 12), (1, 2, 2, 3), (1, 1, 2, 2), (0, 0, 1, 1), (100, 700, 0, 30)),
], ids=["dense_2d", "psd_padded", "packed_4d", "dense_27_slots", "packed_12_slots", "refused_2d_s2", "refused_3d", "refused_4d"])
def test_other_geometries_equal_the_exact_build(shape, ksize, stride, padding, sizes):
    idx = _events(np.random.default_rng(33), shape, sizes)
    _build_both(idx, len(sizes), shape, ksize, stride, padding)


@pytest.mark.parametrize("local_row", [5, THREADS + 88, 2 * THREADS + 88, R * THREADS + 88],
                         ids=["first", "second", "third", "uncached"])
def test_out_of_range_coordinates_are_flagged_in_every_cached_row(local_row):
    """flags[2] for a row that a thread holds as its first, second or third record, and for one past the cache."""
    shape, ksize, stride, padding = PSD
    sizes = (40, R * THREADS + 200, 7)
    idx = _events(np.random.default_rng(34), shape, sizes)
    idx[sizes[0] + local_row, 3] = shape[2]
    t = torch.from_numpy(idx).to(DEV)
    pad, nv = _padded(t)
    rb = _device_count(pad, nv, len(sizes), shape, ksize, stride, padding, 2 * idx.shape[0])
    f = rb.event_flags.cpu().numpy()
    assert f[2] == 1 and f[0] == 0
