"""GPU checks of psd/quantifier_evaluator.SegEvaluator (csrc/segquant.hip) against tests/golden/seg_quantifier_cases.npz,
recorded from the reference's own functions: every count (error_hist, error_2d, the n tables) exactly, error_edges bit
for bit, the real-valued tables within 1e-5 of each output's largest magnitude; then determinism and a LitSegQuantifier
test loop against the NumPy restatement of tests/seg_quantifier_cases.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import seg_quantifier_cases as sc
from test_segment_callers import segment_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "config", "segment_quantifier_z.json")
WORST = {}
BAD_CLASS = {"max_zero": 0, "nan_first_target": 0, "nan_first_results": 1}     # the class whose first subset fails


@pytest.fixture(scope="module")
def gold():
    return sc.load_golden()


def make(gold, name, **over):
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    kw = sc.constructor_kwargs(gold, name)
    kw.update(over)
    return SegEvaluator(DEV, seg_status=gold["seg_status"], **kw)


def feed(ev, bt, dtype, pid_dtype=torch.int64, pad=0):
    """One ``add``; ``pad`` rows of NaN / out-of-range padding behind the batch, cut off by a device ``n_valid``."""
    td = getattr(torch, sc.TORCH_DTYPES[dtype])
    c, res, tg, pid = (torch.from_numpy(np.ascontiguousarray(bt[k])) for k in ("coords", "results", "target", "pid"))
    nv = int(bt["n_valid"])
    if pad:
        assert nv < 0
        nv = len(c)
        c = torch.cat([c, torch.tensor([[-3, 99, 7]] * pad, dtype=torch.int32)])
        res = torch.cat([res, torch.full((pad,), float("nan"))])
        tg = torch.cat([tg, torch.full((pad, tg.shape[1]), float("inf"))])
        pid = torch.cat([pid, torch.full((pad,), 6, dtype=torch.int64)])
    n_valid = torch.tensor([nv], dtype=torch.int64, device=DEV) if nv >= 0 else None
    fields = [pid.to(pid_dtype).to(DEV)] if ev.has_PID else None
    ev.add(res.to(td).to(DEV), tg.to(td).to(DEV), c.to(DEV), fields, n_valid=n_valid)


def test_every_case_against_the_recorded_tables(gold):
    checked = nans = 0
    for name in sc.case_names(gold):
        m = sc.meta_of(gold, name)
        ev = make(gold, name)
        for bt in sc.batches_of(gold, name):
            feed(ev, bt, m["dtype"])
        if m["raises"]:
            with pytest.raises(RuntimeError, match="largest .error. of 0 or one that is not finite"):
                ev.results()
            bad = BAD_CLASS[name]                                # until then the class's edges stay unset
            assert int(ev.error_flags.item()) == 1 << bad and not ev.error_edges_set[bad].item()
            continue
        if m["nan_rows"]:
            # a NaN error has no fixed-point image: results() raises for the metric tables; the error tables hold the row
            # where the reference's walk leaves it
            with pytest.raises(RuntimeError, match="no fixed-point image"):
                ev.results()
            state = {"error_hist": ev.error_hist.cpu().numpy(), "error_2d": ev.error_2d.cpu().numpy(),
                     "error_edges": ev.error_edges.cpu().numpy(), "error_edges_set": ev.error_edges_set.cpu().numpy()}
            sc.compare(sc.expected(gold, name), name, state, errors_only=True)
            nans += 1
            continue
        res = ev.results()
        sc.compare(sc.expected(gold, name), name, res, worst=WORST)
        assert res["scale_factor"] == (1200.0 if m["target_index"] == 4 else 12.0)
        checked += 1
    assert checked >= 20 and nans == 2
    print("largest error / largest magnitude of the real-valued tables:", WORST)
    assert WORST and max(WORST.values()) <= sc.TOL


def test_per_row_outputs_equal_the_recorded_walks(gold):
    for name in ("rows_257", "padded", "pid_outside", "no_pid"):
        ev = make(gold, name)
        for b, bt in enumerate(sc.batches_of(gold, name)):
            feed(ev, bt, "f32")
            rec = gold["%s_b%d_rows" % (name, b)]
            n = rec.shape[1]
            got = [ev.multiplicity, ev.se_mask, ev.category, ev.slot]
            for g, r in zip(got, rec):
                assert np.array_equal(g[:n].cpu().numpy(), r), name
            assert (ev.category[n:] == -1).all().item() and torch.isfinite(ev.mae).all().item()
            err = bt["results"][:n].astype(np.float64) - bt["target"][:n, ev.target_index].astype(np.float64)
            assert np.array_equal(ev.error[:n].cpu().numpy(), err)           # fp64 from the stored values


@pytest.mark.parametrize("name", ["rows_65", "c2_both", "no_pid"])
def test_padding_rows_behind_a_device_row_count_change_nothing(gold, name):
    """The captured form: NaN results, Inf targets and coordinates off the grid behind ``n_valid`` (and past a row-block
    boundary); int32 PIDs."""
    ev = make(gold, name)
    for bt in sc.batches_of(gold, name):
        feed(ev, bt, "f32", pid_dtype=torch.int32, pad=300)
    sc.compare(sc.expected(gold, name), name, ev.results())


def test_two_adds_and_one_add_of_the_concatenation_hold_the_same_integers(gold):
    a, b = make(gold, "two_adds_f32"), make(gold, "concat_f32")
    for bt in sc.batches_of(gold, "two_adds_f32"):
        feed(a, bt, "f32")
    feed(b, sc.batches_of(gold, "concat_f32")[0], "f32")
    for x, y in zip([a.error_hist, a.error_2d, a.error_edges_set, a.error_edges.view(torch.int64), a.metric_pairs.tables],
                    [b.error_hist, b.error_2d, b.error_edges_set, b.error_edges.view(torch.int64), b.metric_pairs.tables]):
        assert torch.equal(x, y)


def test_two_runs_give_bit_identical_state_and_reset_clears(gold):
    states = []
    for _ in range(2):
        ev = make(gold, "two_adds_f32")
        for name in ("two_adds_f32", "rows_257", "padded", "c2_both"):
            for bt in sc.batches_of(gold, name):
                feed(ev, bt, "f32")
        states.append([t.clone() for t in ev.state_tensors() + [ev.error_hist, ev.error_edges.view(torch.int64)]])
    assert len(ev.state_tensors()) == 2                       # metric tables and error_2d: data-dependent edges
    for a, b in zip(*states):
        assert torch.equal(a, b)
    ev.reset()
    assert not ev.error_edges_set.any().item() and ev.error_hist.sum().item() == 0 and ev.error_2d.sum().item() == 0
    for bt in sc.batches_of(gold, "c2_both"):                 # after a reset the first batch fixes the ranges again
        feed(ev, bt, "f32")
    sc.compare(sc.expected(gold, "c2_both"), "c2_both after reset", ev.results())
    fixed = make(gold, "fixed_edges")
    assert len(fixed.state_tensors()) == 3
    fixed.reset()
    assert fixed.error_edges_set.all().item()
    for bt in sc.batches_of(gold, "fixed_edges"):
        feed(fixed, bt, "f32")
    sc.compare(sc.expected(gold, "fixed_edges"), "fixed_edges after reset", fixed.results())


def test_flags_and_argument_checks(gold):
    ev = make(gold, "rows_64")
    bt = dict(sc.batches_of(gold, "rows_64")[0])
    bad = dict(bt, coords=bt["coords"][::-1].copy())          # event column descending
    feed(ev, bad, "f32")
    with pytest.raises(RuntimeError, match="not sorted"):
        ev.results()
    ev.reset()
    off = dict(bt, coords=bt["coords"].copy())
    off["coords"][3, 0] = 14
    feed(ev, off, "f32")
    with pytest.raises(RuntimeError, match="outside the detector grid"):
        ev.results()
    ev.reset()
    c = torch.from_numpy(bt["coords"]).to(DEV)
    r, t = torch.from_numpy(bt["results"]).to(DEV), torch.from_numpy(bt["target"]).to(DEV)
    with pytest.raises(RuntimeError, match="no additional fields"):
        ev.add(r, t, c)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ev.add(r.cpu(), t, c, [torch.from_numpy(bt["pid"]).to(DEV)])
    with pytest.raises(RuntimeError, match="n_phys"):
        ev.add(r, t[:, :4].contiguous(), c, [torch.from_numpy(bt["pid"]).to(DEV)])
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    with pytest.raises(RuntimeError, match="calgroup"):
        SegEvaluator(DEV, calgroup="x")


def test_lit_seg_quantifier_test_loop_fills_the_tables(gold):
    """LitSegQuantifier + SPConvPreserveNet through evaluate.segment_test_loop over two synthetic batches, held against
    the NumPy restatement fed the module's own last_test_outputs."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litsegq import LitSegQuantifier
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    cfg = json.load(open(CONFIG))
    cfg["evaluation_config"] = {"bin_overrides": {"4": [-600.0, 600.0, 20]}}
    torch.manual_seed(5)
    mod = LitSegQuantifier(load_config(cfg)).to(DEV)
    rng = np.random.default_rng(21)
    loader = []
    for B in (12, 9):
        rows, c, f = segment_rows(rng, B, 7, 130)
        t = torch.from_numpy(rng.random((len(rows), 8)).astype(np.float32))
        pid = torch.from_numpy(np.array([1, 4, 6, 258, 256, 512, 3])[rng.integers(0, 7, len(rows))])
        loader.append(([c, [f, pid]], t))
    ev = mod.evaluator
    assert isinstance(ev, SegEvaluator) and ev is mod.evaluator and ev.has_PID and ev.target_index == 4
    assert ev.additional_field_names == ["PID"] and ev.n_bins == 20      # evaluation_config merged over the field names
    plain = segment_test_loop(mod, copy.deepcopy(loader), DEV)
    out = segment_test_loop(mod, copy.deepcopy(loader), DEV, evaluator=ev)
    assert sorted(plain) == ["rows", "test_loss", "test_mse"] and sorted(out) == sorted(list(plain) + ["evaluation"])
    assert abs(out["test_loss"] - plain["test_loss"]) <= 1e-6 * abs(plain["test_loss"])
    host = sc.HostSegTables(ev.seg_status.cpu().numpy(), 4, {4: [-600.0, 600.0, 20]}, True)
    with torch.no_grad():
        for i, ((c, f), y) in enumerate(copy.deepcopy(loader)):
            mod.test_step(([c.to(DEV), [t.to(DEV) for t in f]], y.to(DEV)), i)
            pred, target, cc, fields = mod.last_test_outputs
            assert pred.shape == (len(c),) and len(fields) == 1
            host.add(pred.cpu().numpy(), target.cpu().numpy(), cc.cpu().numpy(), fields[0].cpu().numpy())
    res = out["evaluation"]
    assert res["error_hist"].sum() > 10 and res["error_edges_set"].sum() >= 3
    sc.compare(sc.as_expected(host.results()), "test loop", res)
