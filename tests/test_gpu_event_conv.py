"""The event-local build of regular (strided) convolutions (csrc/evconv.hip, k_ev_conv) against the CPU oracle
(oracle/spconv_ref.c) directly, bit for bit, at the edges of the kernel: empty events (first, interior,
last), batches past 512 events (a second look-back pass, a larger look-back state), events of more rows than a
workgroup has threads, by-output images of several passes, the packed table with more than 9 leading slots, the two
dense slot layouts, grids at the LDS limit, output capacities below the output count and the 65534-row limit of an
event.  Every build goes through ``ops.build_rulebook`` in device-count mode as a captured step runs it: index rows
padded past the valid count with junk, an output capacity above the output count, a per-layer flag store (built three
times on it: three epochs of the look-back state).

Also the captured runners around the build: GraphedEvalStep.check() reports an ungrouped batch, the look-back state of
a live train graph survives an eval runner captured on the other side of the 512-event step, and three captured C2
steps at the bench's size against the CPU oracle.
"""
import copy
import gc
import json
import os
import weakref

import numpy as np
import pytest
import torch

from helpers import rand_coords

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSD_GEO = ([3, 3, 3], [1, 1, 4], [0, 0, 0], [1, 1, 1])


def _listify(v, ndim):
    return [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)] * ndim


def _oracle(idx, B, shape, ksize, stride, padding, dilation):
    """(out_indices [M, D+1], by-input table [K, N], by-output table [K, M]) of the oracle's regular conv rulebook."""
    from oracle import ref
    out, pairs, num = ref.get_indice_pairs(idx, B, list(shape), ksize, stride, padding, dilation, 0, False)
    out = np.asarray(out)
    K, N, M = pairs.shape[1], idx.shape[0], out.shape[0]
    by_in = np.full((K, N), -1, np.int32)
    by_out = np.full((K, M), -1, np.int32)
    for k in range(K):
        n = int(num[k])
        by_in[k, pairs[0, k, :n]] = pairs[1, k, :n]
        by_out[k, pairs[1, k, :n]] = pairs[0, k, :n]
    return out, by_in, by_out


def _decode_packed(packed, kl):
    """Dense [K, N] from the packed [K / kl, N] table, in numpy: entry = output row << 3 | offset along the last kernel
    dim, -1 = none (independent of the library's k_unpack_table)."""
    Kq, N = packed.shape
    dense = np.full((Kq * kl, N), -1, np.int32)
    for q in range(Kq):
        e = packed[q]
        for o in range(kl):
            hit = (e >= 0) & ((e & 7) == o)
            dense[q * kl + o, hit] = e[hit] >> 3
    return dense


def _by_input(rb, N):
    """The by-input table [K, N] of a build, decoded from the packed form when there is one (and then also checked
    against the unpack kernel's expansion)."""
    if rb.nbr_out_packed is not None:
        mine = _decode_packed(rb.nbr_out_packed[:, :N].cpu().numpy(), rb.packed_kl)
        assert np.array_equal(rb.nbr_out[:, :N].cpu().numpy(), mine), "k_unpack_table"
        return mine
    return rb.nbr_out[:, :N].cpu().numpy()


def _device_build(idx, B, shape, ksize, stride, padding=0, dilation=1, store=None, out_capacity=None, n_pad=313,
                  want_cell_map=True, rows=None, events=None):
    """ops.build_rulebook in device-count mode: ``idx`` (numpy or a device tensor) padded with junk rows past the valid
    count, the output capacity above the output count (or ``out_capacity``)."""
    from waveformml_amd.spconv import ops
    ndim = len(shape)
    t = idx if torch.is_tensor(idx) else torch.from_numpy(np.ascontiguousarray(idx)).to(DEV)
    N = int(t.shape[0]) if rows is None else int(rows)
    nv = torch.tensor([N], dtype=torch.int64, device=DEV) if rows is None or not torch.is_tensor(rows) else rows
    if n_pad:
        junk = torch.full((n_pad, ndim + 1), 99999, dtype=torch.int32, device=DEV)
        junk[::3, 0] = 0                                  # junk that would land in event 0 / in range if it were read
        junk[1::3, 1:] = 1
        t = torch.cat([t[:N], junk])
    rb = ops.build_rulebook(t, B, list(shape), _listify(ksize, ndim), _listify(stride, ndim), _listify(padding, ndim),
                            _listify(dilation, ndim), False, n_dev=nv, out_capacity=out_capacity, flags=store,
                            want_cell_map=want_cell_map, events=events)
    torch.cuda.synchronize()
    return rb


def _check_against_oracle(rb, idx, B, shape, ksize, stride, padding=0, dilation=1, want=None, event_local=True):
    """Bit-exact comparison of a device-count build with the oracle; returns the oracle's result."""
    ndim = len(shape)
    N = idx.shape[0]
    if want is None:
        want = _oracle(idx, B, shape, _listify(ksize, ndim), _listify(stride, ndim), _listify(padding, ndim),
                       _listify(dilation, ndim))
    out, by_in, by_out = want
    M = out.shape[0]
    assert (rb.events_out is not None) == event_local
    assert int(rb.m_dev) == M and M < rb.M
    assert int(rb.overflow) == 0
    assert np.array_equal(rb.out_indices[:M].cpu().numpy(), out)
    assert np.array_equal(rb.nbr_in[:, :M].cpu().numpy(), by_out)
    assert np.array_equal(_by_input(rb, N), by_in)
    if event_local:
        assert not rb.event_flags.any(), rb.event_flags.cpu().numpy()
        ev = rb.events_out.cpu().numpy()
        assert np.array_equal(ev[:B + 1], np.searchsorted(out[:, 0], np.arange(B + 1)))
        assert not ev[B + 1:].any()
        if rb.cell_map is not None:
            V = int(np.prod(rb.out_spatial_shape))
            lin = out[:, 0].astype(np.int64)
            for d in range(ndim):
                lin = lin * rb.out_spatial_shape[d] + out[:, 1 + d]
            cells = np.full(B * V, -1, np.int32)
            cells[lin] = np.arange(M, dtype=np.int32)
            assert np.array_equal(rb.cell_map[2].cpu().numpy(), cells)
    return want


def _state(store):
    st = [v for k, v in store.items() if isinstance(k, tuple) and k[0] == "conv_state"]
    assert len(st) == 1 and st[0] is store["conv_state"]
    return st[0]


def _three_times(idx, B, shape, ksize, stride, padding=0, dilation=1, **kw):
    """Builds three times on one flag store (epochs 1, 2, 3 of the look-back state), each oracle-exact; the output
    capacity 77 rows above the output count."""
    ndim = len(shape)
    want = _oracle(idx, B, shape, _listify(ksize, ndim), _listify(stride, ndim), _listify(padding, ndim),
                   _listify(dilation, ndim))
    store = {}
    for _rep in range(3):
        rb = _device_build(idx, B, shape, ksize, stride, padding, dilation, store=store,
                           out_capacity=want[0].shape[0] + 77, **kw)
        want = _check_against_oracle(rb, idx, B, shape, ksize, stride, padding, dilation, want=want)
    assert int(_state(store)[0]) == 3
    return rb, want


def _events(rng, counts, shape):
    """Rows grouped by event, ``counts[e]`` distinct sites in event e (0: an empty event)."""
    parts = []
    for e, n in enumerate(counts):
        if n:
            p = rand_coords(rng, 1, shape, n)
            p[:, 0] = e
            parts.append(p)
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, len(shape) + 1), np.int32)


@pytest.mark.parametrize("case", ["one_event", "empty_first_interior_last", "one_of_forty"])
def test_event_conv_small_batches_and_empty_events(case):
    rng = np.random.default_rng({"one_event": 1, "empty_first_interior_last": 2, "one_of_forty": 3}[case])
    shape = (14, 11, 64)
    if case == "one_event":
        B, counts = 1, [700]
    elif case == "empty_first_interior_last":
        B, counts = 7, [0, 300, 41, 0, 1, 520, 0]
    else:
        B = 40
        counts = [0] * B
        counts[17] = 450
    idx = _events(rng, counts, shape)
    _three_times(idx, B, shape, *PSD_GEO)


def test_event_conv_no_valid_rows():
    """n_dev = 0: no outputs, no flags, nothing reachable but "none"."""
    rng = np.random.default_rng(4)
    B, shape = 5, (14, 11, 64)
    idx = _events(rng, [30, 30, 30, 30, 30], shape)
    t = torch.from_numpy(idx).to(DEV)
    store = {}
    for _rep in range(3):
        rb = _device_build(t, B, shape, *PSD_GEO, store=store, rows=0, out_capacity=64)
        assert int(rb.m_dev) == 0 and int(rb.overflow) == 0 and not rb.event_flags.any()
        assert not rb.events_out.any()
        assert bool((rb.cell_map[2] == -1).all())
    assert int(_state(store)[0]) == 3


@pytest.mark.parametrize("B", [513, 1024])
def test_event_conv_past_512_events(B):
    """A second look-back pass per thread (events > 512) and the look-back state past one page per replica."""
    from waveformml_amd.psd import synthetic
    T = 64
    c, _f, _y = synthetic.generate(B, T, 3, seed=B)
    idx = np.ascontiguousarray(c[:, [3, 0, 1, 2]])
    _three_times(idx, B, (14, 11, T), *PSD_GEO)


def test_event_conv_chain_at_2048_events():
    """The bench's large-batch mode: both strided layers at 2048 events x 256 samples, the second built from the first
    one's output rows, output count and output event offsets, three times on the same stores."""
    from waveformml_amd.psd import synthetic
    B, T = 2048, 256
    c, _f, _y = synthetic.generate(B, T, 3, seed=2048)
    idx = np.ascontiguousarray(c[:, [3, 0, 1, 2]])
    N = idx.shape[0]
    w1 = _oracle(idx, B, (14, 11, T), *PSD_GEO)
    shape2 = (12, 9, T // 4)
    w2 = _oracle(w1[0], B, shape2, *PSD_GEO)
    M1, M2 = w1[0].shape[0], w2[0].shape[0]
    t = torch.from_numpy(idx).to(DEV)
    store1, store2 = {}, {}
    for _rep in range(3):
        r1 = _device_build(t, B, (14, 11, T), *PSD_GEO, store=store1, out_capacity=M1 + 1000, n_pad=2048,
                           want_cell_map=False)
        _check_against_oracle(r1, idx, B, (14, 11, T), *PSD_GEO, want=w1)
        r2 = _device_build(r1.out_indices, B, list(r1.out_spatial_shape), *PSD_GEO, store=store2, out_capacity=M2 + 500,
                           n_pad=0, rows=r1.m_dev, events=r1.events_out)
        assert r2.N == r1.M
        _check_against_oracle(r2, w1[0], B, shape2, *PSD_GEO, want=w2)
        assert r1.packed_kl == 3 and N > 0
    assert int(_state(store1)[0]) == 3 and int(_state(store2)[0]) == 3


def test_event_conv_large_events():
    """An event of more rows than a workgroup has threads (several ticket / scan passes, rows beyond the first pass
    digested again) and an event filling most of a large output grid (the by-output image in several passes)."""
    rng = np.random.default_rng(6)
    idx = _events(rng, [40, 3000, 12, 0, 77], (14, 11, 64))
    _three_times(idx, 5, (14, 11, 64), *PSD_GEO)
    # 14 x 11 x 256 -> 12 x 9 x 64 = 6912 output cells; 30000 of the 39424 input cells of event 1 reach nearly all
    idx = _events(rng, [100, 30000, 5], (14, 11, 256))
    rb, want = _three_times(idx, 3, (14, 11, 256), *PSD_GEO)
    m1 = int(np.sum(want[0][:, 0] == 1))
    assert m1 > 6000


@pytest.mark.parametrize("shape,ksize,stride,padding,packed_kl", [
    ((14, 11, 64), (4, 3, 2), (1, 1, 2), (0, 0, 0), 2),      # packed, 12 leading slots: k_ev_conv<true, 32, 512>
    ((14, 11, 64), (4, 4, 2), (1, 1, 2), (1, 1, 0), 2),      # packed, 16 leading slots, kl 2
    ((9, 7, 40), (3, 3, 2), (1, 2, 3), (1, 0, 1), 2),        # packed, kl 2
    ((14, 11), (3, 3), (1, 1), (0, 0), 0),                   # dense, 9 slots
    ((14, 11, 64), (1, 3, 3), (1, 1, 2), (0, 1, 1), 0),      # dense, 9 slots, 3-D
    ((14, 11, 64), (3, 3, 3), (1, 1, 2), (0, 0, 0), 0),      # dense, 27 slots: k_ev_conv<false, 32, 512>
    ((10, 9, 30), (3, 3, 3), (2, 1, 1), (1, 1, 1), 0),       # dense, 27 slots, padding
])
def test_event_conv_slot_layouts(shape, ksize, stride, padding, packed_kl):
    """The packed form with more than 9 leading slots needs kl = 2 (K <= 32, leading kernel sizes <= 4), the dense form
    takes the register cache up to 9 slots and streams its candidates beyond."""
    rng = np.random.default_rng(7)
    B = 6
    counts = [int(v) for v in rng.integers(1, int(np.prod(shape)) // 3, B)]
    counts[2] = 0
    idx = _events(rng, counts, shape)
    rb, _ = _three_times(idx, B, shape, list(ksize), list(stride), list(padding), 1)
    assert rb.packed_kl == packed_kl


@pytest.mark.parametrize("T,event_local", [(256, True), (260, False)])
def test_event_conv_at_the_lds_grid_limit(T, event_local):
    """18 x 18 x 256 -> 16 x 16 x 64 = 16384 output cells per event (EC_MAXCELLS): built event-locally; 18 x 18 x 260 ->
    16 x 16 x 65 = 16640 cells: the chip-wide build takes it, and it is oracle-exact too."""
    rng = np.random.default_rng(8)
    shape = (18, 18, T)
    B = 3
    idx = _events(rng, [2000, 9000, 700], shape)
    from waveformml_amd.spconv import ops
    assert int(np.prod(ops.get_conv_output_size(shape, PSD_GEO[0], PSD_GEO[1], PSD_GEO[2], PSD_GEO[3]))) == (
        16384 if event_local else 16640)
    want = _oracle(idx, B, shape, *PSD_GEO)
    store = {}
    for _rep in range(3):
        rb = _device_build(idx, B, shape, *PSD_GEO, store=store, out_capacity=want[0].shape[0] + 77)
        _check_against_oracle(rb, idx, B, shape, *PSD_GEO, want=want, event_local=event_local)


@pytest.fixture(params=[True, False], ids=["event_local_conv", "chip_wide_conv"])
def conv_build(request):
    from waveformml_amd.spconv import ops
    old = ops.EVENT_LOCAL_CONV
    ops.EVENT_LOCAL_CONV = request.param
    yield request.param
    ops.EVENT_LOCAL_CONV = old


def test_event_conv_capacity_below_the_output_count():
    """out_capacity < M: the first M_cap outputs exist, in order; every table, the output event offsets and the cell
    map stay inside the capacity -- what no longer exists reads "none"."""
    rng = np.random.default_rng(9)
    B, shape = 7, (14, 11, 64)
    idx = _events(rng, [300, 0, 450, 200, 350, 0, 280], shape)
    out, by_in, by_out = _oracle(idx, B, shape, *PSD_GEO)
    M = out.shape[0]
    N = idx.shape[0]
    for cap in (M // 2, int(np.searchsorted(out[:, 0], 3)), 1):         # mid-event, at an event boundary, one row
        store = {}
        for _rep in range(2):
            rb = _device_build(idx, B, shape, *PSD_GEO, store=store, out_capacity=cap)
            assert int(rb.m_dev) == cap and int(rb.overflow) == 1 and not rb.event_flags.any()
            assert np.array_equal(rb.out_indices[:cap].cpu().numpy(), out[:cap])
            assert np.array_equal(_by_input(rb, N), np.where(by_in >= cap, -1, by_in))
            assert np.array_equal(rb.nbr_in[:, :cap].cpu().numpy(), by_out[:, :cap])
            ev = rb.events_out.cpu().numpy()
            assert np.array_equal(ev[:B + 1], np.minimum(np.searchsorted(out[:, 0], np.arange(B + 1)), cap))
            V = int(np.prod(rb.out_spatial_shape))
            lin = out[:cap, 0].astype(np.int64)
            for d in range(3):
                lin = lin * rb.out_spatial_shape[d] + out[:cap, 1 + d]
            cells = np.full(B * V, -1, np.int32)
            cells[lin] = np.arange(cap, dtype=np.int32)
            assert np.array_equal(rb.cell_map[2].cpu().numpy(), cells)
            rb.overflow.zero_()


def test_conv_build_capacity_below_the_output_count_stays_in_bounds(conv_build):
    """Both device-count builds: with out_capacity < M no table entry points past what exists."""
    rng = np.random.default_rng(10)
    B, shape = 6, (14, 11, 64)
    idx = _events(rng, [260, 410, 0, 330, 120, 500], shape)
    N = idx.shape[0]
    M = _oracle(idx, B, shape, *PSD_GEO)[0].shape[0]
    cap = M // 3
    rb = _device_build(idx, B, shape, *PSD_GEO, out_capacity=cap)
    assert (rb.events_out is not None) == conv_build
    assert int(rb.m_dev) == cap and int(rb.overflow) == 1
    t_in = rb.nbr_out[:, :N].cpu().numpy()
    t_out = rb.nbr_in[:, :cap].cpu().numpy()
    assert t_in.min() >= -1 and t_in.max() < cap
    assert t_out.min() >= -1 and t_out.max() < N
    oi = rb.out_indices[:cap].cpu().numpy()
    assert oi[:, 0].min() >= 0 and oi[:, 0].max() < B


def test_event_conv_row_limit():
    """An event of 65534 rows (the most a workgroup's uint16 local rows can name) is oracle-exact; one of 65535 sets
    flags[0] and leaves every by-input entry of its rows at -1, everything else in bounds."""
    rng = np.random.default_rng(11)
    shape = (8, 8, 1100)                                  # -> 6 x 6 x 275 = 9900 output cells: event-local
    idx = _events(rng, [500, 65534, 300], shape)
    _three_times(idx, 3, shape, *PSD_GEO, n_pad=64)
    idx = _events(rng, [500, 65535, 300], shape)
    N = idx.shape[0]
    rb = _device_build(idx, 3, shape, *PSD_GEO, store={}, n_pad=64)
    assert int(rb.event_flags[0]) == 1
    m = int(rb.m_dev)
    assert 0 < m <= rb.M
    t_in = _by_input(rb, N)
    assert bool((t_in[:, 500:500 + 65535] == -1).all())
    assert t_in.min() >= -1 and t_in.max() < m
    t_out = rb.nbr_in[:, :m].cpu().numpy()
    assert t_out.min() >= -1 and t_out.max() < N
    assert np.all((t_out < 500) | (t_out >= 500 + 65535))                 # no output gathers from the failed event
    ev = rb.events_out[:4].cpu().numpy()
    assert ev[0] == 0 and np.all(np.diff(ev) >= 0) and ev[3] == m


# ---------------------------------------------------------------------------------------------------------------------
# the captured runners around the build


def _cfg(T):
    with open(os.path.join(ROOT, "config", "psd_c2_3d.json")) as f:
        cfg = json.load(f)
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["algorithm"][-1] = [32 * 10 * 7 * (T // 16), 3]
    return cfg


def _batch(B, T, seed, device=DEV):
    from waveformml_amd.psd import synthetic
    c, f, y = synthetic.generate(B, T, 3, seed=seed)
    return ([torch.from_numpy(c).to(device), torch.from_numpy(f).to(device)], torch.from_numpy(y).to(device))


def _ungrouped(batch):
    (c, f), y = batch
    c2, f2 = c.clone(), f.clone()
    i, j = 3, c.shape[0] - 5                  # rows of the first and the last event change places
    c2[[i, j]], f2[[i, j]] = c2[[j, i]], f2[[j, i]]
    return ([c2, f2], y)


def _module(cfg, seed=0):
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    torch.manual_seed(seed)
    return LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg))).to(DEV)


def _train_step(mod, batch):
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.graph import GraphedTrainStep
    red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
    mod.optimizer_parameters = red.optimizer_parameters()
    opt = mod.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, tuple) else opt
    return GraphedTrainStep(mod, opt, red, batch), red, opt


def test_captured_eval_step_raises_on_an_ungrouped_batch():
    """ADVICE: GraphedEvalStep replays of a batch that is not grouped by event return bias-only logits; check() must say
    so, as GraphedTrainStep.check() does, and a good batch afterwards checks clean."""
    from waveformml_amd.psd.graph import GraphedEvalStep
    T, B = 64, 32
    mod = _module(_cfg(T))
    good = _batch(B, T, 5)
    bad = _ungrouped(good)
    step = GraphedEvalStep(mod, good)
    assert step._event_flags
    ref = step(good).clone()
    assert torch.isfinite(ref).all()
    step.check()
    assert torch.isfinite(step(bad)).all()
    assert torch.equal(step(good), ref)       # sticky: the good replay in between does not hide the failure
    with pytest.raises(RuntimeError, match="grouped by event"):
        step.check()
    assert torch.equal(step(good), ref)
    step.check()
    step.close()


def test_captured_evaluation_raises_on_an_ungrouped_batch():
    from waveformml_amd.psd.evaluate import test_loop
    T, B = 64, 32
    mod = _module(_cfg(T))
    good = _batch(B, T, 6)
    other = _batch(B, T, 7)
    res = test_loop(mod, [good, other], DEV, capture=True)
    assert res["events"] == 2 * B and np.isfinite(res["test_loss"])
    with pytest.raises(RuntimeError, match="grouped by event"):
        test_loop(mod, [good, _ungrouped(other), good], DEV, capture=True)


def test_eval_runner_across_512_events_keeps_the_train_graphs_state():
    """A GraphedEvalStep captured at 600 events beside a live GraphedTrainStep captured at 256 (look-back states of two
    sizes in one layer's store): the train graph's state tensors stay alive, memory handed out afterwards is never
    written by its replays, and its steps are bit-identical to a twin's that never met the eval runner."""
    from waveformml_amd.psd.graph import GraphedEvalStep
    T = 64
    cfg = _cfg(T)
    b256 = [_batch(256, T, s) for s in (31, 32, 33)]
    b600 = _batch(600, T, 34)
    results = []
    for with_eval in (True, False):
        mod = _module(cfg, seed=1)
        step, red, _opt = _train_step(mod, b256[0])
        # the state each strided layer's latest build (the train graph's) was handed
        convs = [m for m in mod.modules() if "conv_state" in m.__dict__.get("_flag_store", {})]
        assert len(convs) == 2
        states = [m.__dict__["_flag_store"]["conv_state"] for m in convs]
        sizes = {int(s.numel()) for s in states}
        refs = [weakref.ref(s) for s in states]
        del states
        losses = [float(step(b256[0]))]
        canaries = []
        if with_eval:
            ev = GraphedEvalStep(mod, b600)
            assert torch.isfinite(ev(b600)).all()
            ev.check()
            # the eval runner's builds took states of another size (600 events: past one page per replica) ...
            assert all(int(m.__dict__["_flag_store"]["conv_state"].numel()) not in sizes for m in convs)
            gc.collect()
            # ... and the train graph's, which its replays keep writing, are still alive
            assert all(r() is not None for r in refs), "the train graph's look-back state was freed"
            canaries = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) for n in sizes for _ in range(8)]
        for bt in b256[1:] + b256[:1]:
            losses.append(float(step(bt)))
        step.check()
        torch.cuda.synchronize()
        for c in canaries:
            assert bool((c == 0x5A5A5A5A).all()), "a train replay wrote memory it no longer owns"
        if with_eval:
            assert torch.isfinite(ev(b600)).all()
            ev.check()
            ev.close()
        results.append((losses, red.flat_param.detach().clone()))
    assert results[0][0] == results[1][0], results
    assert torch.equal(results[0][1], results[1][1])


def test_three_captured_c2_steps_at_bench_size_match_the_cpu_oracle():
    """Three replays of the captured C2 step (256 events x 256 samples, fp32 rows), each on another seeded batch,
    against the oracle-backed CPU twin stepping the same batches from the same weights.

    Bars: losses within 1e-5 relative and every parameter tensor after the last step within 1e-5 of its scale -- of the
    oracle run in FLOAT64, the exact value of the reference's arithmetic, or, where fp32 arithmetic itself cannot get
    there, within a small multiple of the fp32 oracle's own error (the convention of test_gpu_fullsize.py).  With the
    config's SGD (momentum 0.98, nesterov) the fp32 oracle's gradient error (up to ~7e-3 of scale on the SubM layers'
    gradients at this size) compounds: after three steps its BatchNorm biases are ~2e-2 of scale away from float64,
    its third loss ~2e-4, so "1e-5 of the fp32 oracle" alone is no bar a correct implementation could meet."""
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    with open(os.path.join(ROOT, "config", "psd_c2_3d.json")) as f:
        cfg = json.load(f)
    cfg["optimize_config"].pop("scheduler_class", None)
    B, T = 256, 256
    gpu = _module(cfg, seed=2)
    cpu_cfg = copy.deepcopy(cfg)
    cpu_cfg["net_config"]["imports"] = ["oracle.spconv" if m == "waveformml_amd.spconv" else m
                                        for m in cpu_cfg["net_config"]["imports"]]
    host = [_batch(B, T, s, device="cpu") for s in (41, 42, 43)]
    dev = [([c.to(DEV), f.to(DEV)], y.to(DEV)) for (c, f), y in host]
    step, _red, opt = _train_step(gpu, dev[0])
    # the capture's calibration and warm-up steps moved the weights and the momentum: the twins start from the weights as
    # they are, and every side from zero momentum (with dampening 0 the same as torch's first step, buf = g)
    with torch.no_grad():
        for st in opt.state.values():
            for v in st.values():
                if torch.is_tensor(v) and v.is_floating_point():
                    v.zero_()
    start = {k: v.detach().cpu() for k, v in gpu.state_dict().items()}
    twins = []
    for dtype in (torch.float32, torch.float64):
        m = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cpu_cfg))).to(dtype)
        m.load_state_dict(start)
        m.train()
        o = m.configure_optimizers()
        assert isinstance(o, torch.optim.SGD)
        twins.append((m, o, dtype))
    for i, (gb, ((c, f), y)) in enumerate(zip(dev, host)):
        lg = float(step(gb))
        ls = []
        for m, o, dtype in twins:
            o.zero_grad()
            loss = m.training_step(([c, f.to(dtype)], y), i)
            loss.backward()
            o.step()
            ls.append(float(loss.detach()))
        l32, l64 = ls
        assert abs(lg - l64) <= 1e-5 * abs(l64) + 3 * abs(l32 - l64), (i, lg, l32, l64)
        assert abs(lg - l32) <= 1e-5 * abs(l64) + 4 * abs(l32 - l64), (i, lg, l32, l64)
    step.check()
    for (name, a), b, t in zip(gpu.model.named_parameters(), twins[0][0].model.parameters(),
                               twins[1][0].model.parameters()):
        a, b, t = a.detach().double().cpu().numpy(), b.detach().double().numpy(), t.detach().numpy()
        scale = max(float(np.abs(t).max()), 1e-30)
        e32 = float(np.abs(b - t).max())
        assert float(np.abs(a - t).max()) <= 1e-5 * scale + 3 * e32, (name, float(np.abs(a - t).max()), e32, scale)
        assert float(np.abs(a - b).max()) <= 1e-5 * scale + 4 * e32, (name, float(np.abs(a - b).max()), e32, scale)
