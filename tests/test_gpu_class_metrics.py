"""GPU ClassificationMetrics (csrc/classmetrics.hip, psd/class_metrics.py) against the float64 restatement of
tests/class_metrics_cases.py and the curves RECORDED from the reference's ROCCurve (tests/golden/class_metrics_cases.npz).
Nothing here reads the reference tree.

Bounds: every integer table equals the restatement (the builder keeps every drawn row outside the margin within which two
correct softmaxes may differ; the crafted rows are exact).  The mean loss lies within 2^-32 absolute of the float64 value:
a row's fixed-point image is off by at most 2^-33, so the mean of the images is, and the fp64 terms themselves (below
2^15) differ from the restatement's by a few ulps, under 2^-37 each.  ``roc_curve`` equals the recording exactly: both
are float32 quotients of the same integers.  Shapes are small: the workgroup takes 256 rows per pass, so 255 / 256 / 257
rows and a ragged last pass of one and of two workgroups are all below 1500 rows."""
import numpy as np
import pytest
import torch

import class_metrics_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS = 256                      # CM_THREADS: rows per workgroup pass
REG = 8                         # CM_REG: the last class count held in registers
LOSS_TOL = 2.0 ** -32


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


def dev_logits(x, dtype):
    return torch.from_numpy(x).to(DEV).to(cc.TORCH_DTYPE[dtype])


def make(C, T=100, **kw):
    from waveformml_amd.psd.class_metrics import ClassificationMetrics
    return ClassificationMetrics(DEV, C, T, **kw)


def add(ev, x, labels, dtype="f32", n_valid=None, mask=None, **kw):
    ev.add(dev_logits(x, dtype), torch.from_numpy(labels).to(DEV),
           n_valid=None if n_valid is None else torch.tensor(n_valid, dtype=torch.int64, device=DEV),
           loss_mask=None if mask is None else torch.from_numpy(mask).to(DEV), **kw)


def check(res, host, what=""):
    n, correct, loss_rows, ignored = host["head"]
    got = (res["n"], res["correct"], res["loss_rows"], res["ignored"])
    print(what, "head", got, "expected", host["head"], "loss", res["loss"], "expected", host["loss"])
    assert got == host["head"], what
    assert res["confusion"].dtype == np.int64 and np.array_equal(res["confusion"], host["confusion"]), what
    assert res["roc_bins"].dtype == np.int64 and np.array_equal(res["roc_bins"], host["roc"]), what
    assert res["confusion"].sum() == n and (res["acc"] == correct / n if n else np.isnan(res["acc"]))
    if loss_rows:
        assert abs(res["loss"] - host["loss"]) <= LOSS_TOL, (what, res["loss"] - host["loss"])
    else:
        assert np.isnan(res["loss"]), what


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1])
def test_row_counts(n):
    x, labels, _n, _r = cc.make_case(n, 5, seed=100 + n, crafted=False)
    ev = make(5)
    add(ev, x.reshape(n, 5), labels)
    check(ev.results(), cc.host_tables(x.reshape(n, 5), labels, 5, ev.thresholds), n)


@pytest.mark.parametrize("max_blocks,n", [(1, 2 * ROWS + 37), (2, 5 * ROWS + 5), (2, 3 * ROWS), (0, 5 * ROWS + 5)])
def test_ragged_last_pass_of_the_grid_stride_loop(max_blocks, n):
    x, labels, _n, _r = cc.make_case(n, 3, seed=n, crafted=False)
    ev = make(3)
    add(ev, x, labels, max_blocks=max_blocks)
    check(ev.results(), cc.host_tables(x, labels, 3, ev.thresholds), (max_blocks, n))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [2, 3, 4, 5, REG, REG + 1, 10, 32])
def test_class_counts_and_row_types_with_the_crafted_rows(C, dtype):
    x, labels, n, _r = cc.make_case(150, C, 100, dtype, seed=C)
    assert len(x) > n                                              # the crafted rows are in
    ev = make(C)
    add(ev, x, labels, dtype)
    res = ev.results()
    host = cc.host_tables(x, labels, C, ev.thresholds)
    check(res, host, (C, dtype))
    if C in (2, 4, 5, 10):
        # all-equal logits: p = 1 / C lies ON threshold 100 / C and counts as >=; the tie goes to index 0
        assert host["roc"][:, :, 100 // C].sum() >= 4 * C
    for k, name in enumerate(ev.class_names):
        for a, b in zip((res["classes"][name][r] for r in ("tn", "fp", "fn", "tp")), cc.rates(host["roc"][k])):
            assert a.dtype == np.int64 and np.array_equal(a, b)


@pytest.mark.parametrize("C,T", [(2, 1), (5, 1), (2, 1024), (7, 1024), (5, 7)])
def test_threshold_counts(C, T):
    x, labels, _n, _r = cc.make_case(120, C, T, "f32", seed=T + C)
    ev = make(C, T)
    assert np.array_equal(ev.thresholds, cc.thresholds(T))
    add(ev, x, labels)
    check(ev.results(), cc.host_tables(x, labels, C, ev.thresholds), (C, T))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_row_stride_above_c_and_a_view_from_an_odd_element(dtype):
    C, pad = 5, 3
    x, labels, _n, _r = cc.make_case(ROWS + 9, C, 100, dtype, seed=21)
    N = len(labels)
    flat = torch.full((N * (C + pad) + 1,), float("nan"), device=DEV, dtype=cc.TORCH_DTYPE[dtype])
    view = flat[1:].view(N, C + pad)[:, :C]                        # starts at element 1, rows C + pad apart
    view.copy_(dev_logits(x, dtype))
    assert view.storage_offset() == 1 and view.stride() == (C + pad, 1)
    ev = make(C)
    ev.add(view, torch.from_numpy(labels).to(DEV))
    check(ev.results(), cc.host_tables(x, labels, C, ev.thresholds), dtype)


def test_ignore_index_valid_count_and_loss_mask():
    C = 5
    x, labels, _n, _r = cc.make_case(2 * ROWS + 20, C, seed=31)
    N = len(labels)
    labels[::7] = -100
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)
    nv = ROWS + 40
    x[nv:] = np.nan                                                # beyond the valid count: never read into a result
    labels[nv + 3] = 77
    for kw in (dict(n_valid=nv), dict(n_valid=nv, mask=mask), dict(n_valid=0), dict(n_valid=N + 50, mask=mask)):
        ev = make(C)
        xx = np.where(np.isnan(x), 0.0, x).astype(np.float32) if kw["n_valid"] > nv else x
        ll = np.where(labels == 77, 0, labels) if kw["n_valid"] > nv else labels
        add(ev, xx, ll, **kw)
        check(ev.results(), cc.host_tables(xx, ll, C, ev.thresholds, **kw), kw)
    ev = make(C, ignore_index=3)                                   # another ignore_index; a bool mask
    ev.add(dev_logits(x[:nv], "f32"), torch.from_numpy(labels[:nv].clip(0)).to(DEV), loss_mask=torch.from_numpy(mask[:nv] != 0).to(DEV))
    check(ev.results(), cc.host_tables(x[:nv], labels[:nv].clip(0), C, ev.thresholds, ignore=3, mask=mask[:nv]), "ignore 3")


def test_three_adds_equal_one_and_runs_repeat_bit_for_bit():
    C = 5
    x, labels, _n, _r = cc.make_case(3 * ROWS + 11, C, seed=41)
    cuts = [0, 100, ROWS + 150, len(labels)]
    one, three, again, single = make(C), make(C), make(C), make(C)
    add(one, x, labels)
    for a, b in zip(cuts[:-1], cuts[1:]):
        add(three, x[a:b], labels[a:b])
    add(again, x, labels)
    add(single, x, labels, max_blocks=1)
    tables = one.tables.cpu()
    for other in (three, again, single):
        assert torch.equal(other.tables.cpu(), tables)             # the fixed-point loss sum included
    check(one.results(), cc.host_tables(x, labels, C, one.thresholds), "one add")
    one.reset()
    assert int(one.tables.abs().sum()) == 0 and int(one.flags[0]) == 0
    assert one.results()["n"] == 0 and np.isnan(one.results()["acc"])
    add(one, x, labels)
    assert torch.equal(one.tables.cpu(), tables)
    assert one.state_tensors()[0] is one.tables


@pytest.mark.parametrize("name", sorted(cc.RECORDED))
def test_roc_curve_equals_the_reference_recording(gold, name):
    x, labels, C, T, dtype = cc.recorded_case(name)
    assert np.array_equal(x, gold[name + "_logits"]) and np.array_equal(labels, gold[name + "_labels"])
    ev = make(C, T)
    half = len(labels) // 2
    add(ev, x[:half], labels[:half], dtype)
    add(ev, x[half:], labels[half:], dtype)
    res = ev.results()
    check(res, cc.host_tables(x, labels, C, ev.thresholds), name)
    assert res["roc_curve"]().dtype == np.float32
    assert np.array_equal(res["roc_curve"](0), gold[name + "_roc0"], equal_nan=True)
    assert np.array_equal(res["roc_curve"](C - 1), gold[name + "_rocl"], equal_nan=True)


@pytest.mark.parametrize("what", ["nan", "inf", "label_high", "label_negative", "loss_range"])
def test_flags_fire_and_the_flagged_row_is_in_no_table(what):
    C = 3
    x, labels, _n, _r = cc.make_case(ROWS + 30, C, seed=51, crafted=False)
    row = 77
    if what == "nan":
        x[row, 1], match = np.nan, "not finite"
    elif what == "inf":
        x[row, 2], match = -np.inf, "not finite"
    elif what == "label_high":
        labels[row], match = C, "outside"
    elif what == "label_negative":
        labels[row], match = -1, "outside"
    else:
        x[row], labels[row], match = np.array([1e5, 0.0, 0.0], np.float32), 1, "2\\^15"
    ev = make(C)
    add(ev, x, labels)
    with pytest.raises(RuntimeError, match=match):
        ev.results()
    assert int(ev.flags[0]) == dict(nan=1, inf=1, label_high=2, label_negative=2, loss_range=4)[what]
    skip = np.arange(len(labels)) == row
    host = cc.host_tables(np.where(skip[:, None], 0.0, x).astype(np.float32), np.where(skip, 0, labels), C, ev.thresholds,
                          skip=skip)
    tabs = ev.tables.cpu().numpy()
    assert (tabs[0], tabs[1], tabs[2], tabs[4]) == host["head"]
    assert np.array_equal(tabs[5:5 + C * C].reshape(C, C), host["confusion"])
    assert np.array_equal(tabs[5 + C * C:].reshape(C, 2, 101), host["roc"])
    assert abs(tabs[3] / 2.0 ** 32 / tabs[2] - host["loss"]) <= LOSS_TOL
    if what == "loss_range":
        # the same row outside the loss mask is counted: its term is never formed
        ev.reset()
        add(ev, x, labels, mask=(~skip).astype(np.uint8))
        check(ev.results(), cc.host_tables(x, labels, C, ev.thresholds, mask=(~skip).astype(np.uint8)), "masked out")


def test_argument_checks():
    ev = make(5)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.add(torch.zeros(4, 5), lab)
    with pytest.raises(RuntimeError, match=r"\[N, 5\]"):
        ev.add(torch.zeros(4, 4, device=DEV), lab)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        ev.add(torch.zeros(5, 4, device=DEV).t(), lab)
    with pytest.raises(RuntimeError, match="int64"):
        ev.add(torch.zeros(4, 5, device=DEV), lab.int())
    with pytest.raises(RuntimeError, match="loss_mask"):
        ev.add(torch.zeros(4, 5, device=DEV), lab, loss_mask=torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="n_valid"):
        ev.add(torch.zeros(4, 5, device=DEV), lab, n_valid=torch.tensor(4))
    with pytest.raises(ValueError, match="LDS"):
        make(8, 1024)
    assert ev.results()["n"] == 0
