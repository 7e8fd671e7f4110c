"""Cost of the SegEvaluator tables inside the LitSegQuantifier test loop (psd/evaluate.segment_test_loop,
config/segment_quantifier_z.json: SPConvPreserveNet, 4 metrics, 6 pairs and the error tables at the default 100 bins; fp32
rows, synthetic batches of 256 events / about 770 rows), of its ``add`` alone, and of the fused masked regression loss
against the torch composition it replaces; no kernel trace:

  none     the loop without an evaluator
  gpu      the loop + psd/quantifier_evaluator.SegEvaluator (csrc/segquant.hip + metricpairs.hip, five launches per
           batch plus seven fills whenever the row count changes, no read-back)
  host     the loop + the path the reference takes: predictions, target, coordinates and PID to the host, the binning
           there.  The CPU side is the VECTORISED NumPy restatement of tests/seg_quantifier_cases.py, which is more
           favourable to the host than the reference's row-by-row walks would be.
  add      SegEvaluator.add alone (HIP events around back-to-back calls) at about 770 and 86.5 k rows, with the batch's
           event count (n_events) and without it, and the RealMetricPairTables accumulate it contains alone on the same
           rows
  loss     forward + backward of spconv.functional.masked_regression_loss (csrc/segloss.hip, one launch each way) against
           psd/litsegq.masked_regression_composition over the same masks (single-ended mask, valid-row count, target
           column 4; L1) at 1024 and 86.5 k rows, with the number of kernel launches of each (torch.profiler, one pass)

The loop arms run in ONE process, alternating, `rounds` times; the figure per arm is the median over rounds and the
spread is (max - min) over rounds.  The loss arms alternate in the same way.  The kernel figures are the median and spread
of `rounds` windows of 100 calls.  Every timed window ends in a device synchronise.

The tool also measures the error of the evaluator's tables against the goldens and of the fused loss against a float64
composition (``errors`` in the result).

usage: python tools/bench_seg_quantifier.py [--batches 8] [--loops 4] [--rounds 7] [--out FILE] [--profile FILE]
prints one JSON line; --out appends it to FILE; --profile writes profiles/seg_quantifier_ab.txt's text to FILE"""
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


class HostSegEvaluator:
    """add() as the reference's: everything to the host, the binning there."""

    def __init__(self, gpu_evaluator):
        import seg_quantifier_cases as sc
        ev = gpu_evaluator
        self.tables = sc.HostSegTables(ev.seg_status.cpu().numpy(), ev.target_index, None, ev.has_PID)
        self.pid_index = ev.PID_index

    def add(self, results, target, c, additional_fields=None):
        self.tables.add(results.detach().cpu().numpy(), target.detach().cpu().numpy(), c.detach().cpu().numpy(),
                        additional_fields[self.pid_index].detach().cpu().numpy())

    def state_tensors(self):
        return []

    def results(self):
        return self.tables.results()


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


def segment_batch(torch, g, events, per_event, channels, dev):
    """About ``events * per_event * 0.98`` distinct active segments, grouped by event."""
    rows = sorted({(int(x), int(y), e) for e in range(events)
                   for x, y in zip(torch.randint(0, 14, (per_event,), generator=g).tolist(),
                                   torch.randint(0, 11, (per_event,), generator=g).tolist())}, key=lambda r: r[2])
    n = len(rows)
    c = torch.tensor(rows, dtype=torch.int32)
    pid = torch.tensor(PIDS)[torch.randint(0, len(PIDS), (n,), generator=g)]
    return ([c.to(dev), [torch.rand(n, channels, generator=g).to(dev), pid.to(dev)]], torch.rand(n, 8, generator=g).to(dev))


def count_launches(torch, fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)      # kernels, fills, copies


def measure_errors(torch, dev):
    """Largest error of the evaluator's real-valued tables against tests/golden/seg_quantifier_cases.npz (relative to each
    output's largest magnitude; counts and edges are compared exactly by ``compare``), and of the fused loss against a
    float64 torch composition (loss and mse relative, fp32 dpred relative to the gradient's scale)."""
    import numpy as np
    import seg_quantifier_cases as sc
    from waveformml_amd import _lib
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    from waveformml_amd.psd.segments import segment_status, single_ended_mask
    from waveformml_amd.spconv import functional as Fsp
    gold, worst, cases = sc.load_golden(), {}, 0
    for name in sc.case_names(gold):
        m = sc.meta_of(gold, name)
        if m["raises"] or m["nan_rows"]:
            continue
        ev = SegEvaluator(dev, seg_status=gold["seg_status"], **sc.constructor_kwargs(gold, name))
        td = getattr(torch, sc.TORCH_DTYPES[m["dtype"]])
        for bt in sc.batches_of(gold, name):
            nv = int(bt["n_valid"])
            ev.add(torch.from_numpy(bt["results"]).to(td).to(dev), torch.from_numpy(bt["target"]).to(td).to(dev),
                   torch.from_numpy(bt["coords"]).to(dev), [torch.from_numpy(bt["pid"]).to(dev)] if ev.has_PID else None,
                   n_valid=torch.tensor([nv], dtype=torch.int64, device=dev) if nv >= 0 else None)
        sc.compare(sc.expected(gold, name), name, ev.results(), worst=worst)
        cases += 1
    out = {"table_cases": cases, "tables": {k: float("%.2g" % v) for k, v in worst.items()}}
    mask = single_ended_mask(segment_status()).to(dev)
    g = torch.Generator().manual_seed(5)
    loss_err = {"loss": 0.0, "mse": 0.0, "dpred_f32": 0.0}
    for kind in (_lib.WFS_LOSS_L1, _lib.WFS_LOSS_MSE):
        for n in (65, 1000, 86500):
            pred = torch.rand(n, generator=g).to(dev).requires_grad_(True)
            target = torch.rand(n, 8, generator=g).to(dev)
            c = torch.stack([torch.randint(0, 14, (n,), generator=g), torch.randint(0, 11, (n,), generator=g),
                             torch.arange(n) // 3], dim=1).to(torch.int32).to(dev)
            n_valid = torch.tensor([n - n // 10], dtype=torch.int64, device=dev)
            loss, mse = Fsp.masked_regression_loss(pred, target, kind, col=4, coords=c, se_mask=mask, n_valid=n_valid)
            loss.backward()
            counted = (torch.arange(n, device=dev) < n_valid.reshape(())) & (mask[0, 0, c[:, 0].long(), c[:, 1].long()] == 1.0)
            d = (pred.detach().double() - target[:, 4].double())[counted]
            per = d.abs() if kind == _lib.WFS_LOSS_L1 else d * d
            want = torch.zeros(n, dtype=torch.float64, device=dev)
            want[counted] = (torch.sign(d) if kind == _lib.WFS_LOSS_L1 else 2 * d) / d.numel()
            loss_err["loss"] = max(loss_err["loss"], abs(float(loss) - float(per.mean())) / float(per.mean()))
            loss_err["mse"] = max(loss_err["mse"], abs(float(mse) - float((d * d).mean())) / float((d * d).mean()))
            loss_err["dpred_f32"] = max(loss_err["dpred_f32"],
                                        float((pred.grad.double() - want).abs().max() / want.abs().max()))
    out["loss"] = {k: float("%.2g" % v) for k, v in loss_err.items()}
    return out


def render_profile(d, line):
    """The text of profiles/seg_quantifier_ab.txt from one result of this tool."""
    e = d["errors"]
    rows = ["GPU SegEvaluator against the host path, and the fused masked regression loss against the torch composition it",
            "replaces (tools/bench_seg_quantifier.py --profile; MI355X, no kernel trace).  Written by the tool; method: its docstring.",
            "",
            "Evaluator: evaluate.segment_test_loop of LitSegQuantifier (config/segment_quantifier_z.json), PID as the additional",
            "field, default 100 bins; synthetic batches of %d events / %s rows on average, %d batches per timed window; the"
            % (d["events_per_batch"], d["rows_per_batch"], d["batches_per_window"]),
            "three arms alternate in one process, %d rounds; median over rounds, spread = max - min over rounds." % d["rounds"],
            "",
            "arm                                                          ms per batch   spread"]
    for key, label in (("none", "loop, no evaluator"), ("gpu", "loop + GPU SegEvaluator (no read-back per batch)"),
                       ("host", "loop + host path (4 D2H copies + vectorised NumPy)")):
        rows.append("%-60s %-14s %s" % (label, d[key]["ms_per_batch"], d[key]["spread_ms"]))
    rows += ["added by the GPU evaluator: %+.4f ms per batch; by the host path: %+.4f ms per batch"
             % (d["gpu_added_ms"], d["host_added_ms"]),
             "(the host arm is the vectorised float64 NumPy restatement of tests/seg_quantifier_cases.py, which flatters the host",
             "against the reference's row-by-row walks)",
             "",
             "entry points alone (HIP events around 100 back-to-back calls, 10 warm-up calls; median of %d windows)" % d["rounds"],
             "                                                                     us per call  spread"]
    for tag in ("770", "86500"):
        n = d["add_" + tag]["rows"]
        for key, label in (("add_", "SegEvaluator.add with n_events, %d rows"), ("add_no_n_events_", "SegEvaluator.add without n_events, %d rows"),
                           ("accumulate_real_", "RealMetricPairTables accumulate alone, %d rows")):
            rows.append("%-68s %-12s %s" % (label % n, d[key + tag]["us_per_call"], d[key + tag]["spread_us"]))
    rows += ["n_events is the batch's event count, as a loader knows it.  Without it the row count bounds the event indices and the",
             "thread of the last row in k_eval_offsets (wfs_evoffsets.h) fills the offsets of the events that do not exist one after",
             "the other.  The pairwise accumulate takes its direct-atomics route here: 5 classes x four 100-bin metrics are 1570 1-D",
             "cells, above the 1024 of its LDS image.  The rest of an `add` (rows, edge fix-up, error bins) is not broken down.",
             "",
             "Loss: forward + backward of masked_regression_loss (one launch each way) against masked_regression_composition with",
             "the same masks (single-ended mask, device-side valid-row count at 90 % of the rows, column 4 of [N, 8]; L1), fp32;",
             "windows of 100 back-to-back EAGER calls, the variants alternating window by window, %d windows each; launches ="
             % d["rounds"],
             "device events of one pass under torch.profiler (kernels, fills, copies, autograd's own included).",
             "",
             "rows      variant              us per forward + backward   spread   device launches"]
    for tag, n in (("1024", "1 024"), ("86500", "86 500")):
        for key, label in (("loss_fused_", "fused"), ("loss_torch_", "torch composition")):
            v = d[key + tag]
            rows.append("%-9s %-20s %-27s %-8s %s" % (n, label, v["us_per_call"], v["spread_us"], v["launches"]))
    rows += ["ratio of the medians, torch composition / fused: %.1f at 1 024 rows, %.1f at 86 500 rows."
             % (d["loss_torch_1024"]["us_per_call"] / d["loss_fused_1024"]["us_per_call"],
                d["loss_torch_86500"]["us_per_call"] / d["loss_fused_86500"]["us_per_call"]),
             "Eager calls are bound by the host's enqueue time, not by the device: read the figures with their spreads.  The device",
             "time of the two kernels alone is not measured; inside a captured step the launch count is what remains.",
             "",
             "Measured error.  Tables against tests/golden/seg_quantifier_cases.npz (%d cases; counts, error_hist, error_2d and"
             % e["table_cases"],
             "error_edges exact), largest error relative to each output's largest magnitude: %s (bar 1e-5)."
             % ", ".join("%s %.2g" % kv for kv in sorted(e["tables"].items())),
             "Loss against a float64 torch composition over the same counted rows (L1 and MSE, 65 / 1000 / 86 500 rows, fp32): loss",
             "%.2g and mse %.2g relative (bar 1e-5), dpred %.2g of the gradient's scale (bar 1e-6)."
             % (e["loss"]["loss"], e["loss"]["mse"], e["loss"]["dpred_f32"]),
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
    ap.add_argument("--profile", default=None, help="write the profile text (profiles/seg_quantifier_ab.txt) there")
    args = ap.parse_args()
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litsegq import LitSegQuantifier, masked_regression_composition
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    from waveformml_amd.psd.segments import segment_status, single_ended_mask
    from waveformml_amd.spconv import functional as Fsp
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_quantifier: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "events_per_batch": args.events, "rounds": args.rounds}

    with open(os.path.join(ROOT, "config", "segment_quantifier_z.json")) as f:
        cfg = json.load(f)
    cfg["optimize_config"].pop("scheduler_class", None)
    mod = LitSegQuantifier(DictionaryUtility.to_object(cfg)).to(dev)
    batches = [segment_batch(torch, g, args.events, 3, 130, dev) for _ in range(args.batches)]
    out["rows_per_batch"] = round(sum(b[1].shape[0] for b in batches) / len(batches), 1)
    out["batches_per_window"] = args.batches * args.loops
    arms = {"none": None, "gpu": mod.evaluator, "host": HostSegEvaluator(mod.evaluator)}
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

    # add alone
    for tag, events in (("770", 256), ("86500", 28800)):
        (c, (_f, pid)), target = segment_batch(torch, g, events, 3, 1, dev)
        results = (target[:, 4] + 0.1 * (torch.rand(target.shape[0], generator=g).to(dev) - 0.5)).contiguous()
        ev = SegEvaluator(dev, additional_field_names=["PID"])
        # n_events: the batch's event count, as a loader knows it.  Without it the row count bounds the event indices and
        # the offset launch fills the offsets of the events that do not exist one after the other
        out["add_" + tag] = dict(summary(time_calls(
            torch, lambda: ev.add(results, target, c, [pid], n_events=events), args.rounds)), rows=int(target.shape[0]))
        out["add_no_n_events_" + tag] = summary(time_calls(torch, lambda: ev.add(results, target, c, [pid]), args.rounds))
        mp = ev.metric_pairs
        out["accumulate_real_" + tag] = summary(time_calls(
            torch, lambda: mp.add(ev.parameters, ev.mae, ev.category, ranges=ev.normalized_ranges), args.rounds))
        ev.results()                                                                  # no flag was raised

    # the loss: forward + backward, fused against the torch composition over the same masks
    mask = single_ended_mask(segment_status()).to(dev)
    crit_none = torch.nn.L1Loss(reduction="none")
    for tag, n in (("1024", 1024), ("86500", 86500)):
        pred = torch.rand(n, generator=g).to(dev).requires_grad_(True)
        target = torch.rand(n, 8, generator=g).to(dev)
        c = torch.stack([torch.randint(0, 14, (n,), generator=g), torch.randint(0, 11, (n,), generator=g),
                         torch.arange(n) // 3], dim=1).to(torch.int32).to(dev)
        n_valid = torch.tensor([n - n // 10], dtype=torch.int64, device=dev)

        def fused():
            pred.grad = None
            loss, _mse = Fsp.masked_regression_loss(pred, target, _lib.WFS_LOSS_L1, col=4, coords=c, se_mask=mask,
                                                    n_valid=n_valid)
            loss.backward()

        def composed():
            pred.grad = None
            counted = (torch.arange(n, device=dev) < n_valid.reshape(())) & \
                (mask[0, 0, c[:, 0].long(), c[:, 1].long()] == 1.0)
            loss, _mse = masked_regression_composition(crit_none, pred, target[:, 4], counted)
            loss.backward()

        fused(), composed()
        fu, co = [], []
        for _ in range(args.rounds):                                                  # alternating windows
            fu += time_calls(torch, fused, 1, warm=2)
            co += time_calls(torch, composed, 1, warm=2)
        out["loss_fused_" + tag], out["loss_torch_" + tag] = summary(fu), summary(co)
        out["loss_fused_" + tag]["launches"] = count_launches(torch, fused)
        out["loss_torch_" + tag]["launches"] = count_launches(torch, composed)
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
