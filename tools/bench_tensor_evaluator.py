"""Cost of the TensorEvaluator tables inside the LitWaveform test loop (psd/evaluate.segment_test_loop,
config/waveform_tcn_z.json with a phys test target: 8 metrics, 28 pairs, the default 100 bins; fp32 rows, synthetic batches
of 1024 rows, the config's batch), and of its entry points alone; no kernel trace:

  none     the loop without an evaluator
  gpu      the loop + psd/tensor_evaluator.TensorEvaluator (csrc/metricpairs.hip, two launches per batch, no read-back)
  host     the loop + the path the reference takes: detector numbers, target and per-row loss to the host, the binning
           there.  The CPU side is the VECTORISED NumPy restatement of tests/tensor_evaluator_cases.py, which is more
           favourable to the host than the reference's 308 masks and row-by-row walks would be.
  kernels  TensorEvaluator.add alone (HIP events around back-to-back calls) at 1024 and at 16384 rows, and
           wfs_metric_pairs_accumulate_real alone on those rows

The loop arms run in ONE process, alternating, `rounds` times; the figure per arm is the median over rounds and the
spread is (max - min) over rounds.  The kernel figures are the median and spread of `rounds` windows of 100 calls.  Every
timed window ends in a device synchronise.  WFS_LIB selects another build of the library: `make -C waveformml_amd/csrc
knock_mp` builds tools/exp/mp_direct/libwfsparse.so, in which the 1-D tables take direct global atomics instead of the
LDS image (the launch-shape A/B; run it with --kernels-only).

usage: python tools/bench_tensor_evaluator.py [--batches 8] [--loops 4] [--rounds 7] [--kernels-only] [--out FILE]
prints one JSON line; --out appends it to FILE"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class HostTensorEvaluator:
    """add() as the reference's: everything to the host, the binning there."""

    def __init__(self, gpu_evaluator):
        import tensor_evaluator_cases as tc
        ev = gpu_evaluator
        self.tables = tc.HostTensorTables(ev.metric_pairs.n_bins, ev.normalized_ranges, ev.metric_names, ev.metric_name)

    def add(self, c, f, target, results):
        self.tables.add(c.detach().cpu().numpy(), target.detach().cpu().numpy(), results.detach().cpu().numpy())

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
    return {"us_per_call": round(statistics.median(us), 2), "spread_us": round(max(us) - min(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--loops", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litwaveform import LitWaveform
    from waveformml_amd.psd.tensor_evaluator import TensorEvaluator
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensor_evaluator: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "rows_per_batch": args.rows, "rounds": args.rounds}

    if not args.kernels_only:
        with open(os.path.join(ROOT, "config", "waveform_tcn_z.json")) as f:
            cfg = json.load(f)
        cfg["optimize_config"].pop("scheduler_class", None)
        cfg["dataset_config"]["test_dataset_params"] = {"label_name": "phys"}
        mod = LitWaveform(DictionaryUtility.to_object(cfg)).to(dev)
        batches = []
        for _ in range(args.batches):
            c = torch.randint(0, 308, (args.rows,), generator=g, dtype=torch.int32)
            batches.append(([c.to(dev), torch.rand(args.rows, 59, generator=g).to(dev)],
                            torch.rand(args.rows, 8, generator=g).to(dev)))
        out["batches_per_window"] = args.batches * args.loops
        arms = {"none": None, "gpu": mod.evaluator, "host": HostTensorEvaluator(mod.evaluator)}
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

    # the entry points alone: 8 metrics + 28 pairs at the default 100 bins, and a single metric
    for tag, n in (("1024", 1024), ("16384", 16384)):
        c = torch.randint(0, 308, (n,), generator=g, dtype=torch.int32).to(dev)
        target = torch.rand(n, 8, generator=g).to(dev)
        results = torch.rand(n, generator=g).to(dev)
        ev = TensorEvaluator(dev, target_has_phys=True, target_index=7, metric_name="mean absolute error")
        out["add_phys_" + tag] = time_calls(torch, lambda: ev.add(c, None, target, results), args.rounds)
        mp = ev.metric_pairs
        out["accumulate_real_phys_" + tag] = time_calls(
            torch, lambda: mp.add(ev.parameters, results, ev.category, ranges=ev.normalized_ranges), args.rounds)
        ev.results()                                                                  # no flag was raised
        one = TensorEvaluator(dev, target_index=7, metric_name="mean absolute error")
        single = target[:, 7].contiguous()
        out["add_single_" + tag] = time_calls(torch, lambda: one.add(c, None, single, results), args.rounds)
        one.results()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
