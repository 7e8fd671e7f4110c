"""GPU checks of psd/real_z_evaluator.ZEvaluatorRealWFNorm (csrc/zreal.hip) against
tests/golden/z_real_evaluator_cases.npz, recorded from the reference's own functions: pulse alignment (start index and
aligned samples) and the neighbour-average baseline bit for bit, every count exactly, the real-valued tables within 1e-5
of each output's largest magnitude; then the rule for samples beyond a row, concatenation, padding, determinism, flags,
and a LitZ test loop on phys targets."""
import copy

import numpy as np
import pytest
import torch

import z_real_evaluator_cases as zc
from test_host_mirror import _z_config
from waveformml_amd.psd import real_z_evaluator  # noqa: F401  (the module under test: no test here runs without it)
from test_segment_callers import segment_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}
P = 5


@pytest.fixture(scope="module")
def gold():
    return zc.load_golden()


def make(gold, name, **over):
    from waveformml_amd.psd.real_z_evaluator import ZEvaluatorRealWFNorm
    m = zc.meta_of(gold, name)
    kw = {}
    if m["has_pid"]:
        kw["additional_field_names"] = ["PID"]
    if m["wf"]:
        kw["wf_analysis"] = True
    kw.update(over)
    return ZEvaluatorRealWFNorm(DEV, **kw)


def tensors(bt, dtype, pid_dtype=torch.int64):
    td = getattr(torch, zc.TORCH_DTYPES[dtype])
    c = torch.from_numpy(np.ascontiguousarray(bt["coords"])).to(DEV)
    pred, targ, f = (torch.from_numpy(bt[k].astype(np.float32)).to(td).to(DEV) for k in ("pred", "targ", "feats"))
    pid = torch.from_numpy(bt["pid"]).to(pid_dtype).to(DEV)
    nv = int(bt["n_valid"])
    n_valid = torch.tensor([nv], dtype=torch.int64, device=DEV) if nv >= 0 else None
    return pred, targ, c, f, pid, n_valid


def feed(ev, bt, dtype, pid_dtype=torch.int64):
    pred, targ, c, f, pid, n_valid = tensors(bt, dtype, pid_dtype)
    ev.add(pred, targ, c, f, [pid] if ev.has_PID else None, n_valid=n_valid)
    return pid


def align(rows, dtype, L, n_valid=None):
    """csrc/zreal.hip's wfs_align_pulses on its own: (samples [2, P, N], start [N, 2]); the outputs start out as junk."""
    from waveformml_amd import _lib
    td = getattr(torch, zc.TORCH_DTYPES[dtype])
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(td).to(DEV)
    N = t.shape[0]
    samples = torch.full((2, P, N), 7.0, dtype=torch.float32, device=DEV)
    start = torch.full((N, 2), 99, dtype=torch.int32, device=DEV)
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().wfs_align_pulses(_lib.ptr(t), _lib.dtype_code(t), N, _lib.ptr(nv), L, P, _lib.ptr(samples),
                                            _lib.ptr(start), _lib.stream_ptr()))
    return samples.cpu().numpy(), start.cpu().numpy()


def test_alignment_is_bit_identical_to_the_recorded_walks(gold):
    """A clean pulse, flat tops (plateau centre), two equal maxima (the first wins), monotone and constant rows (peak
    index 0), an all-zero row, a peak at sample 0 and at 1 (zero padding), a crossing that runs to the row's start, a
    negative peak (tx = 0), plateaus and falls across the kernel's 64-sample chunks, and noisy pulses; L = 8, 65, 150."""
    seen = set()
    for name in (str(n) for n in gold["align_names"]):
        L, dt = int(gold[name + "_L"]), str(gold[name + "_dtype"])
        samples, start = align(gold[name + "_rows"], dt, L)
        assert np.array_equal(start, gold[name + "_start"]), name
        assert np.array_equal(np.transpose(samples, (2, 0, 1)).astype(np.float64), gold[name + "_samples"]), name
        seen.add((L, dt))
        pats = [str(p) for p in gold["al_patterns_L%d" % L]]
        assert start[pats.index("peak_at_1"), 0] == -1 and samples[0, 0, pats.index("peak_at_1")] == 0.0
        assert start[pats.index("all_zero"), 0] == -1 and start[pats.index("negative_peak"), 0] == 0
    assert seen == {(8, "f32"), (8, "bf16"), (8, "f16"), (65, "f32"), (65, "bf16"), (65, "f16"), (150, "f32")}


def _rule(v):
    """start of one side by the stated rule, in fp64: plateau-centred local maxima, the first strictly above the running
    best (index 0 if none beats v[0]); down the rising edge to half height with linear interpolation, 0 when the result
    leaves the row; round half to even, minus one sample."""
    v = np.asarray(v, np.float64)
    best, rise = 0, None
    for i in range(1, len(v)):
        if v[i] > v[i - 1]:
            rise = i
        elif v[i] < v[i - 1] and rise is not None:
            centre = (rise + i - 1) // 2
            if v[centre] > v[best]:
                best = centre
            rise = None
    half, s = 0.5 * v[best], best
    while s > 0 and not v[s] < half:
        s -= 1
    if s == 0:
        tx = -float(best)
    else:
        prev = v[s + 1] if s < best else v[best]
        with np.errstate(all="ignore"):
            tx = -((best - s - 1) + (prev - half) / (prev - v[s]))
    if not 0 <= best + tx < len(v):
        tx = 0.0
    return int(np.round(best + tx)) - 1


@pytest.mark.parametrize("L", [8, 65])
def test_samples_beyond_the_row_are_zero(L):
    """A peak in the last two samples: the reference indexes past the row there; here those samples are 0."""
    rows = np.zeros((3, 2 * L), np.float32)
    rows[0, L - 3:L] = [0.2, 1.0, 0.4]                  # start = L - 4: one sample beyond
    rows[1, L - 3:L] = [-0.5, 1.0, 0.4]                 # a steep edge, start = L - 3: two beyond
    rows[2, L:][L - 4:] = [0.1, 0.45, 1.0, 0.3]         # the right side
    samples, start = align(rows, "f32", L)
    want_start = np.array([[_rule(r[:L]), _rule(r[L:])] for r in rows])
    assert want_start[0, 0] == L - 4 and want_start[1, 0] == L - 3 and want_start[2, 1] == L - 4
    assert np.array_equal(start, want_start)
    for i in range(3):
        for side in range(2):
            v = np.concatenate([np.zeros(1, np.float32), rows[i, side * L:(side + 1) * L], np.zeros(P + 1, np.float32)])
            s = want_start[i, side] + 1
            assert np.array_equal(samples[side, :, i], v[s:s + P]), (i, side)
    assert samples[0, -1, 0] == 0.0 and np.array_equal(samples[0, -2:, 1], [0.0, 0.0])


def test_alignment_never_reads_rows_behind_the_valid_count(gold):
    name = "al_L65_f32"
    rows = gold[name + "_rows"].copy()
    rows[20:] = np.nan
    samples, start = align(rows, "f32", 65, n_valid=20)
    assert np.array_equal(start[:20], gold[name + "_start"][:20]) and not start[20:].any()
    assert np.array_equal(np.transpose(samples, (2, 0, 1))[:20].astype(np.float64), gold[name + "_samples"][:20])
    assert not samples[:, :, 20:].any()


def test_every_case_against_the_recorded_tables(gold):
    """Both blind-PMT orientations, double-ended double entry, dead segments, multiplicities n_mult and n_mult + 1, z at
    -600, 600 and the slice edge 0, E under and over range, PID present and absent, an unmapped PID, a batch without
    class 3, a target of exactly 0, a padded batch; fp32 / bf16 / fp16 maps and rows, L = 8, 65, 150."""
    for name in zc.case_names(gold):
        m = zc.meta_of(gold, name)
        ev = make(gold, name)
        for bt in zc.batches_of(gold, name):
            pid = feed(ev, bt, m["dtype"])
            assert np.array_equal(pid.cpu().numpy(), bt["pid"])              # the caller's PID is not mapped in place
            nv = len(bt["coords"]) if bt["n_valid"] < 0 else int(bt["n_valid"])
            # the baseline prediction bit for bit (float32, as the reference's map)
            assert np.array_equal(ev.baseline[:nv].cpu().numpy(), bt["baseline"]), name
            if m["wf"]:
                assert np.array_equal(ev.start[:nv].cpu().numpy(), bt["start"]), name
                got = ev.samples[:, :, :nv].permute(2, 0, 1).cpu().numpy().astype(np.float64)
                assert np.array_equal(got, bt["samples"]), name
                assert not ev.samples[:, :, nv:].any().item() and (ev.sample_category[nv:] == -1).all().item()
        res = ev.results()
        assert res["class_out_of_range"] is False
        zc.compare(gold, name, res, ev, worst=WORST)
        if name == "special":
            n = res["seg_mult_zmae"][1]
            assert n[:, :, 5].sum() > 0 and n[:, :, 6].sum() > 0             # multiplicity n_mult and the overflow column
            assert res["E_mult_dual"][1][0].sum() + res["E_mult_single"][1][0].sum() >= 2     # E under range
            assert res["E_mult_dual"][1][-1].sum() + res["E_mult_single"][1][-1].sum() >= 2   # E over range
    print("largest error / largest magnitude of the real-valued tables:", WORST)
    assert WORST and max(WORST.values()) <= zc.TOL


def test_retrieve_error_metrics_follow_the_tables(gold):
    ev = make(gold, "two_adds_f32", namespace="real")
    for bt in zc.batches_of(gold, "two_adds_f32"):
        feed(ev, bt, "f32", pid_dtype=torch.int32)
    res = ev.results()
    zc.compare(gold, "two_adds_f32", res, ev)
    out = ev.retrieve_error_metrics(res)
    assert sorted(out) == ["evaluation/real_dual_z_MAE_cal_vs_E", "evaluation/real_dual_z_MAE_vs_E",
                           "evaluation/real_single_z_MAE_cal_vs_E", "evaluation/real_single_z_MAE_vs_E"]
    for tag, key in (("single_z_MAE_vs_E", "E_mult_single"), ("dual_z_MAE_vs_E", "E_mult_dual"),
                     ("single_z_MAE_cal_vs_E", "E_mult_single_cal")):
        s, n = gold["two_adds_f32_%s_sum" % key], gold["two_adds_f32_%s_n" % key]
        want = [1200. * s[i].sum() / n[i].sum() if n[i].sum() > 0 else 0 for i in range(1, 101)]
        assert len(out["evaluation/real_" + tag]) == 100
        assert np.allclose(out["evaluation/real_" + tag], want, rtol=0, atol=1e-5 * max(want))
        assert max(want) > 0


def test_two_adds_equal_one_add_of_the_concatenation(gold):
    """The network's tables, the class tables and the sample tables; the baseline's look-behind stops in front of row 0
    of the BATCH, so its tables depend on where a batch starts and are left out."""
    b0, b1 = zc.batches_of(gold, "two_adds_f32")
    a, b = make(gold, "two_adds_f32"), make(gold, "two_adds_f32")
    feed(a, b0, "f32")
    feed(a, b1, "f32")
    c1 = b1["coords"].copy()
    c1[:, 2] += b0["pred"].shape[0]
    both = dict(coords=np.concatenate([b0["coords"], c1]), pred=np.concatenate([b0["pred"], b1["pred"]]),
                targ=np.concatenate([b0["targ"], b1["targ"]]), feats=np.concatenate([b0["feats"], b1["feats"]]),
                pid=np.concatenate([b0["pid"], b1["pid"]]), n_valid=np.int64(-1))
    feed(b, both, "f32")
    assert torch.equal(a.tables[0], b.tables[0]) and a.tables[0].sum().item() > 0
    assert torch.equal(a.metric_pairs.tables, b.metric_pairs.tables)
    assert torch.equal(a.sample_pairs.tables, b.sample_pairs.tables)
    assert a.results()["seg_mult_zmae_cal"][1].sum() == b.results()["seg_mult_zmae_cal"][1].sum()


def test_two_runs_give_bit_identical_state_and_reset_clears(gold):
    states = []
    for _ in range(2):
        ev = make(gold, "two_adds_f32")
        for name in ("two_adds_f32", "special", "padded"):
            for bt in zc.batches_of(gold, name):
                feed(ev, bt, "f32")
        states.append([t.clone() for t in ev.state_tensors()])
    assert len(states[0]) == 3
    for x, y in zip(*states):
        assert torch.equal(x, y)
    ev.reset()
    assert all(t.sum().item() == 0 for t in ev.state_tensors())
    for bt in zc.batches_of(gold, "special"):
        feed(ev, bt, "f32")
    zc.compare(gold, "special", ev.results(), ev)


def test_flags_and_argument_checks(gold):
    from waveformml_amd.psd.real_z_evaluator import ZEvaluatorRealWFNorm
    bt = zc.batches_of(gold, "no_class3")[0]
    ev = make(gold, "no_class3")
    feed(ev, dict(bt, coords=bt["coords"][::-1].copy()), "f32")               # event column descending
    with pytest.raises(RuntimeError, match="not sorted"):
        ev.results()
    ev.reset()
    off = dict(bt, coords=bt["coords"].copy())
    off["coords"][3, 0] = 14
    feed(ev, off, "f32")
    with pytest.raises(RuntimeError, match="outside the detector grid"):
        ev.results()
    ev.reset()
    # a NaN prediction has no fixed-point image: the row is left out and results() raises
    nan = dict(bt, pred=bt["pred"].copy())
    co = bt["coords"][2]
    nan["pred"][co[2], 0, co[0], co[1]] = np.nan
    feed(ev, nan, "f32")
    assert ev.tables[0].sum().item() > 0
    with pytest.raises(RuntimeError, match="not finite|no fixed-point image"):
        ev.results()
    ev.reset()
    # an unmapped PID on a single-ended row: left out of the class tables and reported, the other tables hold the row
    se = np.flatnonzero(gold["seg_status"][bt["coords"][:, 0], bt["coords"][:, 1]] == 0.5)
    odd = dict(bt, pid=bt["pid"].copy())
    odd["pid"][se[0]] = 7
    feed(ev, odd, "f32")
    res = ev.results()
    assert res["class_out_of_range"] is True
    assert res["metric_pairs"]["metrics"]["energy"][1].sum() == len(se) - 1
    assert res["metric_pairs"]["metrics"]["z"][1].sum() == 3 * (len(se) - 1)
    assert res["z_binned_metric_pairs"][-1]["metrics"]["sample 0"][1].sum() == 2 * len(bt["coords"])
    assert np.array_equal(res["seg_mult_zmae"][1], gold["no_class3_seg_mult_zmae_n"])
    once = make(gold, "no_class3", count_last_metric_once=True)
    feed(once, bt, "f32")
    r1 = once.results()["metric_pairs"]["metrics"]
    assert r1["z"][1].sum() == r1["energy"][1].sum() == len(se)
    pred, targ, c, f, pid, _ = tensors(bt, "f32")
    with pytest.raises(RuntimeError, match="no additional fields"):
        ev.add(pred, targ, c, f)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ev.add(pred.cpu(), targ, c, f, [pid])
    with pytest.raises(RuntimeError, match="target must be"):
        ev.add(pred, targ[:, :4].contiguous(), c, f, [pid])
    with pytest.raises(RuntimeError, match="2 L"):
        ev.add(pred, targ, c, f[:, :15].contiguous(), [pid])
    with pytest.raises(RuntimeError, match="calgroup"):
        ZEvaluatorRealWFNorm(DEV, calgroup="x")
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        ZEvaluatorRealWFNorm("cpu")


def test_litz_test_loop_on_phys_targets_fills_the_tables():
    """A tiny LitZ whose test targets are the seven phys planes, through evaluate.segment_test_loop, eager: the module's
    evaluator holds what a direct ``add`` on ``last_test_outputs`` gives."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litz import LitZ
    from waveformml_amd.psd.real_z_evaluator import ZEvaluatorRealWFNorm
    cfg = copy.deepcopy(_z_config(["waveformml_amd.spconv"]))
    cfg["dataset_config"]["test_dataset_params"] = {"label_name": "phys", "additional_fields": ["PID"]}
    cfg["evaluation_config"] = {"wf_analysis": True}
    torch.manual_seed(3)
    mod = LitZ(load_config(cfg)).to(DEV)
    assert mod.test_has_phys
    rng = np.random.default_rng(14)
    batches = []
    for B in (9, 6):
        rows, c, f = segment_rows(rng, B, 4, 40)
        t = torch.from_numpy(rng.random((len(rows), 7)).astype(np.float32))
        pid = torch.from_numpy(np.array([1, 4, 6, 258, 256, 512, 3])[rng.integers(0, 7, len(rows))])
        batches.append(([c, [f * 0.05, pid]], t))
    plain = segment_test_loop(mod, copy.deepcopy(batches), DEV)
    assert "evaluation" not in plain and plain["rows"] == sum(len(b[0][0]) for b in batches)
    ev = mod.evaluator
    assert isinstance(ev, ZEvaluatorRealWFNorm) and mod.evaluator is ev
    assert ev.has_PID and ev.analyze_waveforms and ev.additional_field_names == ["PID"]
    out = segment_test_loop(mod, copy.deepcopy(batches), DEV, evaluator=ev)
    assert out["test_loss"] == plain["test_loss"]
    direct = ZEvaluatorRealWFNorm(DEV, additional_field_names=["PID"], wf_analysis=True)
    mod.eval()
    with torch.no_grad():
        for i, ((c, f), t) in enumerate(copy.deepcopy(batches)):
            mod.test_step(([c.to(DEV), [x.to(DEV) for x in f]], t.to(DEV)), i)
            assert len(mod.last_test_outputs) == 5 and tuple(mod.last_test_outputs[1].shape[1:]) == (7, 14, 11)
            direct.add(*mod.last_test_outputs)
    for x, y in zip(ev.state_tensors(), direct.state_tensors()):
        assert torch.equal(x, y)
    res = out["evaluation"]
    assert res["seg_mult_zmae"][1].sum() >= out["rows"] and res["seg_mult_zmae_cal"][1].sum() == res["seg_mult_zmae"][1].sum()
    assert res["z_binned_metric_pairs"][-1]["metrics"]["sample 0"][1].sum() == 2 * out["rows"]
    assert len(ev.retrieve_error_metrics(res)) == 4
