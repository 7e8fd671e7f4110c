"""GPU checks of the fused segment loss of LitZ / LitEZ (csrc/segloss.hip, spconv.functional.SegmentMapLossFunction)
against a float64 torch composition over the same counted rows, and of the two modules with ``net_config.fused_segment_loss``
against themselves without it.

Bounds, the conventions of tests/test_gpu_masked_loss.py: losses within 1e-5 relative (fp64 sums, one rounding to fp32 at
the end); dmap of an fp32 map within 1e-6 of the gradient's scale; dmap of a 16-bit map within one correctly rounded
store of the value -- 2^-8 (bf16) / 2^-11 (fp16) of it -- on top of that fp32 bar, and for fp16 half the spacing of its
subnormals (2^-25) where the value lies below its normal range.

Row counts: 1, 65, 1000, and 1023 / 1024 / 1025 around the forward's chunk of 1024 rows; the backward takes 4 events per
workgroup, so the map's B runs over 1, 3, 4, 5, 8, 9 in a test of its own (B = 1, 3, 5, 9 end in a partial workgroup whose
span is no multiple of 16 bytes: the element-wise store).

The forward is the fold of csrc/wfs_lossfold.h that the masked regression loss shares: on an equivalent problem the two
losses agree bit for bit (a test of its own)."""
import copy

import numpy as np
import pytest
import torch

from test_host_mirror import _z_config
from test_segment_callers import ez_config, segment_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NX, NY = 14, 11
U_ROUND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
WORST = {"loss": 0.0, "dmap_f32": 0.0, "dmap_16": 0.0}
PAD = -100.0                                                   # the captured step's fill value for per-row targets
POISON = [float("nan"), float("inf"), -float("inf"), PAD]
TARGETS = {1: [("n", (0,)), ("n2", (0,)), ("n7", (4,))], 2: [("n2", (0, 1)), ("n7", (4, 2))]}


def _mask():
    from waveformml_amd.psd.segments import segment_status, single_ended_mask
    return single_ended_mask(segment_status())                  # [1, 1, 14, 11], CPU


def _rows(n, rng, events_of=5):
    """n rows (x, y, event) grouped by event, segments unique within an event: event 1 holds all 154 segments when the
    rows allow it, event 2 has none.  Returns the rows and the last event id."""
    rows, e = [], 0
    while len(rows) < n:
        if e == 2:
            e += 1
            continue
        left = n - len(rows)
        k = NX * NY if (e == 1 and left >= NX * NY) else min(left, 1 + int(rng.integers(0, events_of)))
        cells = sorted(int(v) for v in rng.permutation(NX * NY)[:k])
        rows += [(cell // NY, cell % NY, e) for cell in cells]
        e += 1
    return rows, e - 1


def _inputs(n, planes, dtype, tkind, seed, n_valid=None, mask=None, b_extra=3, poison=True):
    """map [B, planes, 14, 11], coords [n, 3], target [n] / [n, 2] / [n, 7], the counted rows.  ``poison``: NaN / Inf /
    the padding value in every row that is not counted and in every map cell that belongs to no counted row, and
    coordinates outside the map beyond the valid count."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    rows, last = _rows(n, rng)
    B = last + 1 + b_extra
    c = torch.tensor(rows, dtype=torch.int32)
    if n == 1 and mask is not None:
        c[0, 0], c[0, 1] = 1, 0                                 # segment 1 is single-ended
    m = torch.rand((B, planes, NX, NY), generator=g).to(dtype)
    shape = {"n": (n,), "n2": (n, 2), "n7": (n, 7)}[tkind]
    target = torch.rand(shape, generator=g).to(dtype)
    counted = torch.ones(n, dtype=torch.bool)
    if n_valid is not None:
        counted &= torch.arange(n) < n_valid
    if mask is not None:
        counted &= mask[0, 0, c[:, 0].long(), c[:, 1].long()] == 1.0
    if poison:
        vals = torch.tensor(POISON)[torch.arange(n) % 4].to(dtype)
        bad = (~counted).reshape(-1, *([1] * (target.dim() - 1)))
        target = torch.where(bad, vals.reshape(-1, *([1] * (target.dim() - 1))), target)
        live = torch.zeros((B, NX, NY), dtype=torch.bool)
        cc = c[counted].long()
        live[cc[:, 2], cc[:, 0], cc[:, 1]] = True
        fill = torch.tensor(POISON)[torch.arange(m.numel()) % 4].reshape(m.shape).to(dtype)
        m = torch.where(live[:, None], m, fill)
        if n_valid is not None:
            c[n_valid:] = torch.tensor([-7, 400, 2 ** 30], dtype=torch.int32)    # beyond the valid rows: never read
    return m, c, target, counted, B


def _reference(m, c, target, cols, counted, kind, g=1.0):
    """float64: per-plane losses, their sum, the gradient map (duplicated segments add up) and the count."""
    cc = c[counted].long()
    t = target.double().reshape(target.shape[0], -1)[counted]
    cnt = int(counted.sum())
    grad = torch.zeros(m.shape, dtype=torch.float64)
    per = []
    for p, col in enumerate(cols):
        d = m.double()[cc[:, 2], p, cc[:, 0], cc[:, 1]] - t[:, col]
        v = d.abs() if kind == 0 else d * d
        per.append(float(v.sum() / cnt) if cnt else float("nan"))
        if cnt:
            s = torch.sign(d) if kind == 0 else 2 * d
            grad.index_put_((cc[:, 2], torch.full_like(cc[:, 2], p), cc[:, 0], cc[:, 1]), g * s / cnt, accumulate=True)
    return per, sum(per), grad, cnt


def _run(m, c, target, cols, kind, mask=None, n_valid=None, max_blocks=0, g=1.0):
    from waveformml_amd.spconv import functional as Fsp
    x = m.to(DEV).requires_grad_(True)
    nv = torch.tensor([n_valid], dtype=torch.int64, device=DEV) if n_valid is not None else None
    total, per = Fsp.segment_map_loss(x, c.to(DEV), target.to(DEV), cols, kind,
                                      se_mask=mask.to(DEV) if mask is not None else None, n_valid=nv, max_blocks=max_blocks)
    assert total.dtype == torch.float32 and total.shape == () and total.requires_grad
    assert per.shape == (len(cols),) and not per.requires_grad
    (total * g).backward()
    return total.detach(), per.detach(), x.grad


def _check(m, c, target, cols, counted, kind, mask, n_valid, what, zero_row=None):
    dtype = m.dtype
    want_per, want_total, want_grad, cnt = _reference(m, c, target, cols, counted, kind, g=3.0)
    assert cnt > 0, what
    total, per, grad = _run(m, c, target, cols, kind, mask, n_valid, g=3.0)
    for got, want in [(float(total), want_total)] + list(zip(per.tolist(), want_per)):
        rel = abs(got - want) / abs(want)
        WORST["loss"] = max(WORST["loss"], rel)
        assert rel <= 1e-5, (what, got, want)
    got = grad.double().cpu()
    assert grad.dtype == dtype and grad.shape == m.shape and torch.isfinite(got).all(), what
    live = torch.zeros(m.shape, dtype=torch.bool)
    cc = c[counted].long()
    live[cc[:, 2], :, cc[:, 0], cc[:, 1]] = True
    assert (got[~live] == 0).all(), what                        # exactly 0 in every cell outside the counted rows
    scale = float(want_grad.abs().max())
    err = (got - want_grad).abs()
    bound = U_ROUND[dtype] * want_grad.abs() + 1e-6 * scale + (2.0 ** -25 if dtype == torch.float16 else 0.0)
    assert (err <= bound).all(), (what, float((err - bound).max()))
    key = "dmap_f32" if dtype == torch.float32 else "dmap_16"
    WORST[key] = max(WORST[key], float(err.max()) / scale)
    if zero_row is not None and kind == 0 and counted[zero_row]:
        x, y, e = (int(v) for v in c[zero_row])
        assert (got[e, :, x, y] == 0).all(), what               # d = 0 under L1: sign(0) = 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [1, 65, 1000, 1023, 1024, 1025])
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("kind", [0, 1], ids=["L1", "MSE"])
def test_losses_and_gradient_map_against_the_float64_composition(kind, planes, n, dtype):
    mask = _mask()
    valid_counts = sorted({1, max(1, n - 37), n})
    arms = [(True, None)] + [(False, nv) for nv in valid_counts] + [(True, max(1, n - 37))]
    for k, (use_mask, n_valid) in enumerate(arms):
        tkind, cols = TARGETS[planes][k % len(TARGETS[planes])]
        m, c, target, counted, B = _inputs(n, planes, dtype, tkind, 1000 * n + 10 * kind + k, n_valid,
                                           mask if use_mask else None)
        if use_mask and not counted.any():
            continue                                             # n_valid = 1 on a segment that is not single-ended
        zero_row = None
        if n > 2 and counted[1]:
            x, y, e = (int(v) for v in c[1])
            tt = target.reshape(n, -1)
            for p, col in enumerate(cols):
                m[e, p, x, y] = tt[1, col]                       # d = 0 in every plane
            zero_row = 1
        _check(m, c, target, cols, counted, kind, mask if use_mask else None, n_valid,
               (use_mask, n_valid, tkind, cols, B), zero_row)
    print("largest relative error of a loss, largest dmap error / scale (fp32, 16-bit):", WORST)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 8, 9])
def test_every_event_count_around_the_backward_workgroup(B, dtype):
    """B events of 1 .. 3 rows, the last two (B > 2) without rows: full workgroups of 4 events and partial ones."""
    rng = np.random.default_rng(B)
    rows = []
    for e in range(max(1, B - 2)):
        cells = sorted(int(v) for v in rng.permutation(NX * NY)[:1 + e % 3])
        rows += [(cell // NY, cell % NY, e) for cell in cells]
    c = torch.tensor(rows, dtype=torch.int32)
    n = len(rows)
    g = torch.Generator().manual_seed(B)
    for planes, cols in ((1, (0,)), (2, (0, 1))):
        m = torch.rand((B, planes, NX, NY), generator=g).to(dtype)
        target = torch.rand((n, 2), generator=g).to(dtype)
        _check(m, c, target, cols, torch.ones(n, dtype=torch.bool), 1, None, None, (B, planes))


@pytest.mark.parametrize("kind", [0, 1], ids=["L1", "MSE"])
def test_no_counted_row_gives_nan_losses_a_zero_count_and_a_zero_map(kind):
    from waveformml_amd import _lib
    m, c, target, _counted, B = _inputs(65, 2, torch.float32, "n2", 7, poison=False)
    total, per, grad = _run(m, c, target, (0, 1), kind, None, 0)
    assert torch.isnan(total).item() and torch.isnan(per).all().item() and (grad == 0).all().item()
    c[:, 0], c[:, 1], c[:, 2] = 0, 0, torch.arange(65, dtype=torch.int32)     # segment 0 is dead, not single-ended
    m = torch.rand((65, 2, NX, NY))
    total, per, grad = _run(m, c, target, (0, 1), kind, _mask(), None)
    assert torch.isnan(total).item() and torch.isnan(per).all().item() and (grad == 0).all().item()
    # the count itself, through the C entry point
    lib, p = _lib.load(), _lib.ptr
    md, cd, td, mk = m.to(DEV), c.to(DEV), target.to(DEV), _mask().reshape(NX, NY).to(DEV)
    nbytes = int(lib.wfs_segment_map_loss_workspace_bytes(65, 2))
    work = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    _lib.check(lib.wfs_segment_map_loss(p(md), _lib.dtype_code(md), 65, 2, NX, NY, p(cd), p(td), _lib.dtype_code(td), 2,
                                        _lib.i32_array((0, 1)), p(mk), 65, None, kind, 0, p(work), nbytes, p(out),
                                        p(count), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(count) == 0 and torch.isnan(out).all().item() and int(work[0]) == 0


@pytest.mark.parametrize("n", [1000, 5000])
def test_result_repeats_bit_for_bit_and_does_not_depend_on_the_launch_shape(n):
    mask = _mask()
    m, c, target, _counted, B = _inputs(n, 2, torch.float32, "n7", 11, n - 37, mask)
    runs = [_run(m, c, target, (4, 2), 1, mask, n - 37, max_blocks=mb) for mb in (0, 0, 1, 2, 3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # nor on the rows' capacity or the map's B: the same rows in longer, padded buffers and a larger map
    extra, more = 3000, 2500
    m2 = torch.cat([m, torch.full((more, 2, NX, NY), float("nan"))])
    target2 = torch.cat([target, torch.full((extra, 7), PAD)])
    c2 = torch.cat([c, torch.zeros((extra, 3), dtype=torch.int32)])
    padded = _run(m2, c2, target2, (4, 2), 1, mask, n - 37)
    assert torch.equal(padded[0], runs[0][0]) and torch.equal(padded[1], runs[0][1])
    assert torch.equal(padded[2][:B], runs[0][2]) and (padded[2][B:] == 0).all().item()


@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("n", [1025, 5000])
def test_map_loss_and_masked_loss_agree_bit_for_bit_on_an_equivalent_problem(n, max_blocks):
    """L1, fp32, one plane, ``map[event, 0, x, y] = pred[row]``: the same counted rows, and no product in the term, so
    both kernels add the same fp64 terms in the same order through the same fold -- loss, count and the gradient at the
    rows are the same bits.  (MSE is left out: ``d * d`` may be contracted into the sum in one kernel and not in the
    other.)"""
    from waveformml_amd.spconv import functional as Fsp
    rng = np.random.default_rng(n)
    g = torch.Generator().manual_seed(n)
    rows, last = _rows(n, rng)
    c = torch.tensor(rows, dtype=torch.int32).to(DEV)
    x, y, e = (c[:, k].long() for k in range(3))
    pred = torch.rand(n, generator=g).to(DEV).requires_grad_(True)
    target = torch.rand((n, 7), generator=g).to(DEV)
    m = torch.zeros((last + 1, 1, NX, NY), device=DEV)
    m[e, 0, x, y] = pred.detach()
    m.requires_grad_(True)
    mask = _mask().to(DEV)
    nv = torch.tensor([n - 37], dtype=torch.int64, device=DEV)   # padding rows behind the valid ones
    total, _per = Fsp.segment_map_loss(m, c, target, (4,), 0, se_mask=mask, n_valid=nv, max_blocks=max_blocks)
    loss, _mse = Fsp.masked_regression_loss(pred, target, 0, col=4, coords=c, se_mask=mask, n_valid=nv,
                                            max_blocks=max_blocks)
    counts = [int(t.grad_fn.saved_tensors[-1]) for t in (total, loss)]
    total.backward()
    loss.backward()
    assert torch.isfinite(loss).item() and 0 < counts[0] < n - 37
    assert torch.equal(total.detach().view(torch.int32), loss.detach().view(torch.int32))
    assert counts[0] == counts[1]
    assert torch.equal(m.grad[e, 0, x, y].view(torch.int32), pred.grad.view(torch.int32))
    assert int((pred.grad != 0).sum()) == counts[0]


def test_duplicated_segments_count_each_row_and_add_up_in_the_cell():
    """Outside the contract of the callers (segments are unique within an event), defined all the same: every row counts,
    the cell's gradient is the sum of its rows' values."""
    rows = [(3, 4, 0), (3, 4, 0), (5, 1, 0), (3, 4, 0), (0, 0, 1), (7, 7, 1), (7, 7, 1)]
    c = torch.tensor(rows, dtype=torch.int32)
    g = torch.Generator().manual_seed(5)
    m, target = torch.rand((3, 2, NX, NY), generator=g), torch.rand((len(rows), 2), generator=g)
    for kind in (0, 1):
        _check(m, c, target, (0, 1), torch.ones(len(rows), dtype=torch.bool), kind, None, None, ("duplicates", kind))
        a, b = _run(m, c, target, (0, 1), kind), _run(m, c, target, (0, 1), kind)
        assert torch.equal(a[2], b[2])


def _module_pair(cls, cfg, batch, seed):
    """(loss, parameter gradients, logged validation values) of ``cls`` with and without the key, same weights."""
    from waveformml_amd.psd.config import load_config
    out = []
    for key in (True, False):
        cfg_k = copy.deepcopy(cfg)
        if key:
            cfg_k["net_config"]["fused_segment_loss"] = True
        torch.manual_seed(seed)
        mod = cls(load_config(cfg_k)).to(DEV)
        assert mod.fused_segment_loss is key and mod.per_row_targets is key
        (c, f), y = batch
        loss = mod.training_step(([c.to(DEV), f.to(DEV)], y.to(DEV)), 0)
        loss.backward()
        grads = [q.grad.detach().cpu() for q in mod.model.parameters()]
        with torch.no_grad():
            mod.validation_step(([c.to(DEV), f.to(DEV)], y.to(DEV)), 0)
        out.append((float(loss.detach()), grads, {k: float(v) for k, v in mod.logged.items()}))
    return out


def _assert_parity(on, off):
    assert np.isfinite(off[0]) and abs(on[0] - off[0]) <= 1e-5 * abs(off[0]), (on[0], off[0])
    assert len(on[1]) == len(off[1])
    for a, b in zip(on[1], off[1]):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), (a.shape, float((a - b).abs().max()))


@pytest.mark.parametrize("se_loss", [False, True], ids=["plain", "SELoss"])
def test_litz_with_the_key_matches_the_composition(se_loss):
    from waveformml_amd.psd.litz import LitZ
    cfg = _z_config(["waveformml_amd.spconv"])
    if se_loss:
        cfg["net_config"]["SELoss"] = True
    rng = np.random.default_rng(41)
    rows, c, f = segment_rows(rng, 12, 6, 40)
    y = torch.from_numpy(rng.random(len(rows)).astype(np.float32))
    on, off = _module_pair(LitZ, cfg, ([c, f], y), 5)
    _assert_parity(on, off)
    assert set(on[2]) == set(off[2]) == {"train_loss", "val_loss"}
    assert on[2]["val_loss"] == off[2]["val_loss"]


@pytest.mark.parametrize("version", [0, 2])
def test_litez_with_the_key_matches_the_composition(version):
    from waveformml_amd.psd.litz import LitEZ
    cfg = ez_config(["waveformml_amd.spconv"], version=version)
    rng = np.random.default_rng(43)
    rows, c, f = segment_rows(rng, 12, 6, 40)
    y = torch.from_numpy(rng.random((len(rows), 2)).astype(np.float32))
    on, off = _module_pair(LitEZ, cfg, ([c, f], y), 6)
    _assert_parity(on, off)
    assert set(on[2]) == set(off[2]) == {"train_loss", "val_loss", "val_MAE_E", "val_MAE_z"}
    for k in ("val_loss", "val_MAE_E", "val_MAE_z"):
        assert on[2][k] == off[2][k], k                          # validation stays on the composition: unchanged by the key


def test_litez_fused_step_leaves_the_callers_features_unscaled():
    """``algorithm == "features"`` with ``e_factor != 1``: the fused training route scales a copy (a captured step's
    calibration runs on the trainer's own first batch, which is then trained on: an in-place factor would be applied
    twice), and its loss is the composition's, which scales in place as the reference does."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitEZ
    cfg = ez_config(["waveformml_amd.spconv"])
    cfg["net_config"].update(algorithm="features", escale=24.0)
    rng = np.random.default_rng(47)
    rows, c, f = segment_rows(rng, 12, 6, 20)
    y = torch.from_numpy(rng.random((len(rows), 2)).astype(np.float32))
    losses = {}
    for key in (True, False):
        cfg_k = copy.deepcopy(cfg)
        cfg_k["net_config"]["fused_segment_loss"] = key
        torch.manual_seed(8)
        mod = LitEZ(load_config(cfg_k)).to(DEV)
        assert mod.phys_coord and mod.e_factor == 2.0
        fd = f.to(DEV)
        first = float(mod.training_step(([c.to(DEV), fd], y.to(DEV)), 0).detach())
        if key:
            assert torch.equal(fd.cpu(), f)                       # untouched: a second step sees the same batch
            assert float(mod.training_step(([c.to(DEV), fd], y.to(DEV)), 0).detach()) == first
        else:
            assert torch.equal(fd.cpu()[:, [0, 2, 3]], 2.0 * f[:, [0, 2, 3]])    # the reference's in-place factor
        losses[key] = first
    assert abs(losses[True] - losses[False]) <= 1e-5 * abs(losses[False]), losses
