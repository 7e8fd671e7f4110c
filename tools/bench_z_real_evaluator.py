"""Cost of the real-data z evaluator inside the LitZ test loop on phys targets (psd/evaluate.segment_test_loop, a
SingleEndedZConv on 65-sample waveform pairs, PID as the additional field, waveform analysis on; fp32 rows, synthetic
batches of 256 events / about 770 rows), of its ``add`` alone, and of the pulse-alignment kernel alone; no kernel trace:

  none     the loop without an evaluator
  gpu      the loop + psd/real_z_evaluator.ZEvaluatorRealWFNorm (csrc/zreal.hip + metricpairs.hip, nine launches per batch,
           no read-back)
  host     the loop + the path the reference takes: predictions, targets, coordinates, feature rows and PID to the host,
           the tables there.  The CPU side is VECTORISED NumPy (argmax peaks, masked crossings, np.add.at tables; only
           the order-dependent baseline walks the events in Python), which is far more favourable to the host than the
           reference's row-by-row walks would be, and it bins by floor division instead of the reference's edge walks.
  add      ZEvaluatorRealWFNorm.add alone (HIP events around back-to-back calls) at about 770 and 86.5 k rows, and
           results() after it (wall clock of five calls: the read-back of every table and the split on the host)
  align    wfs_align_pulses alone on the same rows, with the bytes per second it achieves against the row bytes it must
           read (rows x 2 L x 4)

The loop arms run in ONE process, alternating, `rounds` times; the figure per arm is the median over rounds and the
spread is (max - min) over rounds.  The kernel figures are the median and spread of `rounds` windows of 100 calls (20 at
86.5 k rows).  Every timed window ends in a device synchronise.

The tool also measures the error of the evaluator's tables against the goldens (``errors`` in the result).

usage: python tools/bench_z_real_evaluator.py [--batches 8] [--loops 4] [--rounds 7] [--out FILE] [--profile FILE]
prints one JSON line; --out appends it to FILE; --profile writes profiles/z_real_evaluator_ab.txt's text to FILE"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PIDS = [1, 4, 6, 258, 256, 512]
L = 65


def z_config():
    return {"system_config": {"model_name": "SingleEndedZConv", "n_samples": L, "gpu_enabled": True, "half_precision": 0},
            "net_config": {"criterion_class": "L1Loss", "criterion_params": [],
                           "imports": ["torch.nn", "waveformml_amd.spconv"], "net_type": "2DConvolution",
                           "algorithm": "conv", "hparams": {"conv": {"kernel_size": 3, "n_layers": 3},
                                                            "point": {"pointwise_layers": 2}}},
            "optimize_config": {"imports": ["torch.optim"], "lr": 0.01, "optimizer_class": "optim.SGD",
                                "optimizer_params": {"momentum": 0.9}},
            "dataset_config": {"imports": [], "test_dataset_params": {"label_name": "phys", "additional_fields": ["PID"]}},
            "evaluation_config": {"wf_analysis": True}}


class HostZRealEvaluator:
    """add() as the reference's: five tensors to the host, the tables there (vectorised NumPy)."""

    def __init__(self, ev):
        import numpy as np
        self.np, self.ev = np, ev
        self.seg, self.blind = ev.seg_status.cpu().numpy(), ev.blind_detl.cpu().numpy()
        shapes = [s for _n, s in ev._layout]
        self.tables = [[(np.zeros(s), np.zeros(s, np.int64)) for s in shapes] for _ in range(2)]
        nb = [int(p[2]) + 2 for p in ev.metric_params]
        self.cls1 = [np.zeros((5, n)) for n in nb]
        self.cls2 = {(i, j): np.zeros((5, nb[i], nb[j])) for i in range(4) for j in range(i + 1, 4)}
        self.smp1 = [np.zeros((61, 102)) for _ in range(5)]
        self.smp2 = {(i, j): np.zeros((61, 102, 102)) for i in range(5) for j in range(i + 1, 5)}

    @staticmethod
    def _bins(np, v, lo, hi, nb, w=None):
        w = (hi - lo) / nb if w is None else w
        b = np.floor((v - lo) / w).astype(np.int64) + 1
        return np.where(v < lo, 0, np.where(v >= hi, nb + 1, np.clip(b, 1, nb)))

    def _walk(self, tab, co, mult, p, t, E):
        np, ev = self.np, self.ev
        dev = np.abs(p - t)
        z = (t - 0.5) * ev.z_scale
        st, bl = self.seg[co[:, 0], co[:, 1]], self.blind[co[:, 0], co[:, 1]]
        eb = self._bins(np, E, ev.E_low, ev.E_high, ev.n_E)
        col = np.where(mult <= ev.n_mult, mult - 1, ev.n_mult)
        single = st > 0
        for dist, rows in ((np.where((st == 0.5) & (bl == 1), 588. - z, 588. + z), (st == 0.5) | (st == 0)),
                           (588. - z, st == 0)):
            zb = self._bins(np, dist, 0., 1176., ev.n_z, ev.z_scale / ev.n_z)
            for k, idx, sel in ((0, (co[:, 0], co[:, 1], col), rows), (1, (zb, col), rows & single), (2, (zb, col), rows & ~single),
                                (3, (zb, eb), rows & single), (4, (zb, eb), rows & ~single)):
                i = tuple(a[sel] for a in idx)
                np.add.at(tab[k][0], i, dev[sel])
                np.add.at(tab[k][1], i, 1)
        for k, sel in ((5, single), (6, ~single)):
            np.add.at(tab[k][0], (eb[sel], col[sel]), dev[sel])
            np.add.at(tab[k][1], (eb[sel], col[sel]), 1)

    def add(self, predictions, target, c, f, additional_fields=None):
        np, ev = self.np, self.ev
        pred, targ, co = predictions.detach().cpu().numpy(), target.detach().cpu().numpy(), c.detach().cpu().numpy()
        wf, pid = f.detach().cpu().numpy(), additional_fields[ev.PID_index].detach().cpu().numpy()
        from waveformml_amd.psd.real_z_evaluator import map_pid, sample_category
        e, x, y = co[:, 2], co[:, 0], co[:, 1]
        p, t, E, psd = pred[e, 0, x, y], targ[e, ev.z_index, x, y], targ[e, ev.E_index, x, y], targ[e, ev.PSD_index, x, y]
        mult = np.bincount(e)[e]
        cls = map_pid(pid)
        se = self.seg[x, y] == 0.5
        # class tables: single-ended rows, the multiplicity among them
        mult_se = np.bincount(e, weights=se)[e]
        mae = np.where(t == 0, 0., np.abs(p - t))
        sel = se & (cls >= 0) & (cls < 5)
        par = [E, psd, mult_se, t]
        b = [self._bins(np, v[sel], r[0], r[1], int(q[2])) for v, r, q in zip(par, ev.normalized_ranges, ev.metric_params)]
        for i in range(4):
            np.add.at(self.cls1[i], (cls[sel], b[i]), mae[sel])
            for j in range(i + 1, 4):
                np.add.at(self.cls2[(i, j)], (cls[sel], b[i], b[j]), mae[sel])
        # alignment: argmax peak, the last sample below half height in front of it, five samples from there
        N, rows = len(co), np.arange(len(co))
        dmm = np.abs((t - p) * ev.z_scale)
        cat = sample_category((t - 0.5) * ev.z_scale, cls, 5)
        for side in range(2):
            v = wf[:, side * L:(side + 1) * L].astype(np.float64)
            pk = v.argmax(axis=1)
            below = (v < 0.5 * v[rows, pk][:, None]) & (np.arange(L)[None, :] <= pk[:, None])
            s = np.where(below.any(axis=1), L - 1 - below[:, ::-1].argmax(axis=1), 0)
            nxt = np.minimum(s + 1, L - 1)
            with np.errstate(all="ignore"):
                frac = (v[rows, nxt] - 0.5 * v[rows, pk]) / (v[rows, nxt] - v[rows, s])
            arrival = np.where(below.any(axis=1), s + 1 - np.nan_to_num(frac), 0.)
            start = np.rint(arrival).astype(np.int64) - 1
            idx = start[:, None] + np.arange(5)[None, :]
            smp = np.where((idx >= 0) & (idx < L), v[rows[:, None], np.clip(idx, 0, L - 1)], 0.)
            sb = [self._bins(np, smp[:, k], r[0], r[1], 100) for k, r in enumerate(ev.sample_pairs.ranges)]
            for i in range(5):
                np.add.at(self.smp1[i], (cat, sb[i]), dmm)
                for j in range(i + 1, 5):
                    np.add.at(self.smp2[(i, j)], (cat, sb[i], sb[j]), dmm)
        self._walk(self.tables[0], co, mult, p, t, E)
        # the baseline: order dependent, event by event
        base = np.where(se, np.float32(0.5), t.astype(np.float32))
        bounds = np.flatnonzero(np.diff(e, prepend=-1, append=-1))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if not (base[lo:hi] != 0.5).any():
                continue
            for r in range(lo, hi):
                if base[r] != 0.5:
                    continue
                q = np.r_[r + 1:hi, r - 1:max(lo, 1) - 1:-1]
                q = q[(base[q] != 0.5) & (np.abs(x[q] - x[r]) == 1) & (np.abs(y[q] - y[r]) == 1)]
                if len(q):
                    base[r] = base[q].astype(np.float64).sum() / len(q)
        self._walk(self.tables[1], co, mult, base.astype(np.float64), t, E)

    def state_tensors(self):
        return []

    def results(self):
        return {"seg_mult_zmae": self.tables[0][0]}


def time_calls(torch, fn, rounds, warm=10, n=100):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / n)
    return us


def summary(us):
    return {"us_per_call": round(statistics.median(us), 2), "spread_us": round(max(us) - min(us), 2)}


def phys_batch(torch, g, events, per_event, dev):
    """About ``events * per_event * 0.98`` distinct active segments, grouped by event; pulses of amplitude <= 0.06."""
    rows = sorted({(int(x), int(y), e) for e in range(events)
                   for x, y in zip(torch.randint(0, 14, (per_event,), generator=g).tolist(),
                                   torch.randint(0, 11, (per_event,), generator=g).tolist())}, key=lambda r: r[2])
    n = len(rows)
    c = torch.tensor(rows, dtype=torch.int32)
    pid = torch.tensor(PIDS)[torch.randint(0, len(PIDS), (n,), generator=g)]
    t = torch.arange(L, dtype=torch.float32)[None, :]
    pk = torch.randint(5, L - 10, (n, 2), generator=g).float()
    amp = torch.rand(n, 2, generator=g) * 0.06
    sides = [amp[:, s:s + 1] * torch.exp(-0.5 * ((t - pk[:, s:s + 1]) / 2.0) ** 2) + 1e-4 * torch.rand(n, L, generator=g)
             for s in range(2)]
    return ([c.to(dev), [torch.cat(sides, dim=1).to(dev), pid.to(dev)]], torch.rand(n, 7, generator=g).to(dev))


def measure_errors(torch, dev):
    import z_real_evaluator_cases as zc
    from waveformml_amd.psd.real_z_evaluator import ZEvaluatorRealWFNorm
    gold, worst, cases = zc.load_golden(), {}, 0
    for name in zc.case_names(gold):
        m = zc.meta_of(gold, name)
        kw = dict(additional_field_names=["PID"]) if m["has_pid"] else {}
        if m["wf"]:
            kw["wf_analysis"] = True
        ev = ZEvaluatorRealWFNorm(dev, **kw)
        td = getattr(torch, zc.TORCH_DTYPES[m["dtype"]])
        for bt in zc.batches_of(gold, name):
            nv = int(bt["n_valid"])
            pred, targ, f = (torch.from_numpy(bt[k]).float().to(td).to(dev) for k in ("pred", "targ", "feats"))
            ev.add(pred, targ, torch.from_numpy(bt["coords"]).to(dev), f,
                   [torch.from_numpy(bt["pid"]).to(dev)] if m["has_pid"] else None,
                   n_valid=torch.tensor([nv], dtype=torch.int64, device=dev) if nv >= 0 else None)
        zc.compare(gold, name, ev.results(), ev, worst=worst)
        cases += 1
    return {"table_cases": cases, "tables": {k: float("%.2g" % v) for k, v in worst.items()}}


def render_profile(d, line):
    """The text of profiles/z_real_evaluator_ab.txt from one result of this tool."""
    e = d["errors"]
    rows = ["GPU ZEvaluatorRealWFNorm against the host path (tools/bench_z_real_evaluator.py --profile; MI355X, no kernel trace).",
            "Written by the tool; method: its docstring.",
            "",
            "evaluate.segment_test_loop of LitZ on phys targets (SingleEndedZConv, 65-sample waveform pairs, PID, waveform",
            "analysis on); synthetic batches of %d events / %s rows on average, %d batches per timed window; the three arms"
            % (d["events_per_batch"], d["rows_per_batch"], d["batches_per_window"]),
            "alternate in one process, %d rounds; median over rounds, spread = max - min over rounds." % d["rounds"],
            "",
            "arm                                                          ms per batch   spread"]
    for key, label in (("none", "loop, no evaluator"), ("gpu", "loop + GPU evaluator (nine launches, no read-back per batch)"),
                       ("host", "loop + host path (5 D2H copies + vectorised NumPy)")):
        rows.append("%-60s %-14s %s" % (label, d[key]["ms_per_batch"], d[key]["spread_ms"]))
    rows += ["added by the GPU evaluator: %+.4f ms per batch; by the host path: %+.4f ms per batch"
             % (d["gpu_added_ms"], d["host_added_ms"]),
             "(the host arm is vectorised NumPy with floor-division bins and argmax peaks, which flatters the host against the",
             "reference's row-by-row walks; only its baseline walks the events in Python)",
             "Every timed window ends in ONE results(): the GPU arm then reads back its 102 MB of int64 tables (61 categories x",
             "ten 102 x 102 sample pairs are 101 MB of them) and splits them on the host.  That is inside the GPU arm's figure,",
             "spread over the window's %d batches: results() alone takes %s ms (spread %s), i.e. %.2f ms per batch of such a"
             % (d["batches_per_window"], d["results_770"]["ms_per_call"], d["results_770"]["spread_ms"],
                d["results_770"]["ms_per_call"] / d["batches_per_window"]),
             "window; the device work per batch is the `add` below.",
             "",
             "entry points alone (HIP events around back-to-back calls, 10 warm-up calls; median of %d windows)" % d["rounds"],
             "                                                                     us per call  spread"]
    for tag in ("770", "86500"):
        n = d["add_" + tag]["rows"]
        rows.append("%-68s %-12s %s" % ("ZEvaluatorRealWFNorm.add, %d rows" % n, d["add_" + tag]["us_per_call"],
                                        d["add_" + tag]["spread_us"]))
        a = d["align_" + tag]
        rows.append("%-68s %-12s %s" % ("wfs_align_pulses alone, %d rows (%.1f GB/s of %d row bytes)"
                                        % (n, a["gbytes_per_s"], a["row_bytes"]), a["us_per_call"], a["spread_us"]))
    rows += ["The alignment kernel's rate is the row bytes it must read (rows x 2 L x 4) over its time; at 770 rows the call is",
             "bound by its launch, not by memory.",
             "",
             "Measured error.  Tables against tests/golden/z_real_evaluator_cases.npz (%d cases; every count, the start indices, the"
             % e["table_cases"],
             "aligned samples and the baseline exact), largest error relative to each output's largest magnitude: %s (bar 1e-5)."
             % ", ".join("%s %.2g" % kv for kv in sorted(e["tables"].items())),
             "",
             "raw line of the tool:", line, ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--loops", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--events", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None, help="write the profile text (profiles/z_real_evaluator_ab.txt) there")
    args = ap.parse_args()
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litz import LitZ
    from waveformml_amd.psd.real_z_evaluator import PULSE_ANALYSIS_SAMPLES, ZEvaluatorRealWFNorm
    if not torch.cuda.is_available():
        raise SystemExit("bench_z_real_evaluator: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "events_per_batch": args.events, "rounds": args.rounds}

    mod = LitZ(DictionaryUtility.to_object(z_config())).to(dev)
    batches = [phys_batch(torch, g, args.events, 3, dev) for _ in range(args.batches)]
    out["rows_per_batch"] = round(sum(b[1].shape[0] for b in batches) / len(batches), 1)
    out["batches_per_window"] = args.batches * args.loops
    arms = {"none": None, "gpu": mod.evaluator, "host": HostZRealEvaluator(mod.evaluator)}
    with torch.no_grad():
        for ev in arms.values():                                                      # warm every arm
            segment_test_loop(mod, batches, dev, evaluator=ev)
        arms["gpu"].reset()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for name, ev in arms.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = segment_test_loop(mod, batches * args.loops, dev, evaluator=ev)    # ends in a read-back
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t) / (args.loops * len(batches)) * 1e3)
                out.setdefault("test_loss", res["test_loss"])
                if name == "gpu":
                    ev.reset()
    for name, v in times.items():
        out[name] = {"ms_per_batch": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
    out["gpu_added_ms"] = round(out["gpu"]["ms_per_batch"] - out["none"]["ms_per_batch"], 4)
    out["host_added_ms"] = round(out["host"]["ms_per_batch"] - out["none"]["ms_per_batch"], 4)

    # add alone, and the alignment kernel alone
    for tag, events in (("770", 256), ("86500", 28800)):
        (c, (f, pid)), target = phys_batch(torch, g, events, 3, dev)
        rows = int(c.shape[0])
        n = 100 if rows < 10000 else 20
        tdense = torch.zeros((events, 7, 14, 11), device=dev)
        tdense[c[:, 2].long(), :, c[:, 0].long(), c[:, 1].long()] = target
        pdense = (tdense[:, 4:5] + 0.05 * (torch.rand(events, 1, 14, 11, generator=g).to(dev) - 0.5)).contiguous()
        ev = ZEvaluatorRealWFNorm(dev, additional_field_names=["PID"], wf_analysis=True)
        out["add_" + tag] = dict(summary(time_calls(torch, lambda: ev.add(pdense, tdense, c, f, [pid]), args.rounds, n=n)),
                                 rows=rows)
        ms = []
        for _ in range(5):                                                            # raises if a flag was set
            torch.cuda.synchronize()
            t = time.perf_counter()
            ev.results()
            ms.append((time.perf_counter() - t) * 1e3)
        out["results_" + tag] = {"ms_per_call": round(statistics.median(ms), 2), "spread_ms": round(max(ms) - min(ms), 2)}
        samples = torch.zeros((2, PULSE_ANALYSIS_SAMPLES, rows), device=dev)
        start = torch.zeros((rows, 2), dtype=torch.int32, device=dev)
        lib, p = _lib.load(), _lib.ptr

        def align():
            _lib.check(lib.wfs_align_pulses(p(f), _lib.dtype_code(f), rows, None, L, PULSE_ANALYSIS_SAMPLES, p(samples),
                                            p(start), _lib.stream_ptr()))

        a = summary(time_calls(torch, align, args.rounds, n=n))
        a["row_bytes"] = rows * 2 * L * 4
        a["gbytes_per_s"] = round(a["row_bytes"] / a["us_per_call"] / 1e3, 2)
        out["align_" + tag] = a
    out["errors"] = measure_errors(torch, dev)
    line = json.dumps(out)
    print(line)
    if args.profile:
        with open(args.profile, "w") as f:
            f.write(render_profile(out, line))
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
