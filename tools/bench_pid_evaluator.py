"""Cost of the PID evaluation tables inside the LitSegClassifier test loop (psd/evaluate.segment_test_loop,
SPConvPreserveNet at config/examples/IoniClassifierCNN.json's shape, fp32 rows, 130 features, synthetic 256-event batches),
and of the pairwise metric tables PSDEvaluator gains with metric_pairs=True; no kernel trace:

  none     the loop without an evaluator
  gpu      the loop + psd/pid_evaluator.PIDEvaluator (csrc/metricpairs.hip, three launches per batch, no read-back)
  host     the loop + the path the reference takes: predictions, targets, coordinates and phys to the host, the walks and
           the binning there.  The CPU side is the VECTORISED NumPy restatement of tests/pid_evaluator_cases.py, which is
           more favourable to the host than the reference's row-by-row loops would be.
  kernels  PIDEvaluator.add alone (HIP events around back-to-back calls) at the loop's row count and at 86.5 k rows
           (256 events x 338 rows; with the event count given, and with the row count as its bound), and
           wfs_metric_pairs_accumulate alone on those rows
  psd      PSDEvaluator.add with and without metric_pairs at 256 events (T = 150, 5 rows per event)

The loop arms run in ONE process, alternating, `rounds` times; the figure per arm is the median over rounds and the
spread is (max - min) over rounds.  The kernel figures are the median and spread of `rounds` windows of 100 calls.  Every
timed window ends in a device synchronise.  WFS_LIB selects another build of the library (the launch-shape A/B).

usage: python tools/bench_pid_evaluator.py [--batches 8] [--loops 8] [--rounds 7]      prints one JSON line"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

IONI_CONFIG = {
    "system_config": {"model_name": "SegClassifierCNN", "n_type": 5, "n_samples": 65, "gpu_enabled": True,
                      "half_precision": 0},
    "net_config": {"criterion_class": "CrossEntropyLoss", "criterion_params": [],
                   "imports": ["torch.nn", "waveformml_amd.psd.SPConvNet", "waveformml_amd.spconv"],
                   "net_class": "SPConvNet.SPConvPreserveNet",
                   "hparams": {"n_conv": 6, "conv_params": {"pointwise_factor": 0, "pad_factor": 1.00, "size_factor": 3,
                                                             "stride_factor": 1.2, "n_expansion": 3, "expansion_factor": 1.2}}},
    "optimize_config": {"imports": ["torch.optim"], "lr": 0.01, "optimizer_class": "optim.SGD",
                        "optimizer_params": {"momentum": 0.9}},
    "dataset_config": {"imports": [], "test_dataset_params": {"additional_fields": ["phys"]}},
}


class HostPIDEvaluator:
    """add() as the reference's: everything to the host, the walks there."""

    def __init__(self, gpu_evaluator):
        import pid_evaluator_cases as pc
        ev = gpu_evaluator
        self.tables = pc.HostPIDTables(ev.seg_status.cpu().numpy(), ev.metric_pairs.n_bins, ev.normalized_ranges, ev.E_scale)

    def add(self, pred, target, c, additional_fields=None):
        self.tables.add(c.detach().cpu().numpy(), pred.detach().cpu().numpy(), target.detach().cpu().numpy(),
                        additional_fields[0].detach().cpu().numpy())

    def results(self):
        t = self.tables
        return {"SE_confusion": t.SE_confusion, "confusion_SE": t.confusion_SE, "confusion_energy": t.confusion_energy}


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
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--config", default=None, help="a LitSegClassifier config (JSON) instead of the built-in one")
    args = ap.parse_args()
    import numpy as np
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.evaluator import PSDEvaluator
    from waveformml_amd.psd.litseg import LitSegClassifier
    from waveformml_amd.psd.pid_evaluator import PIDEvaluator
    if not torch.cuda.is_available():
        raise SystemExit("bench_pid_evaluator: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = copy.deepcopy(IONI_CONFIG)
    if args.config:
        with open(args.config) as f:
            cfg = json.load(f)
    mod = LitSegClassifier(load_config(cfg)).to(dev)
    rng = np.random.default_rng(5)

    def phys_rows(n):
        ph = rng.random((n, 8)).astype(np.float32)
        ph[:, 5] *= 0.6
        return torch.from_numpy(ph)

    batches = []
    for s in range(args.batches):
        c, f, _y = synthetic.generate(256, 65, 3, seed=900 + s, layout="2d")
        y = torch.from_numpy(rng.integers(0, 5, len(c)))
        batches.append(([torch.from_numpy(c).to(dev), [torch.from_numpy(f).to(dev), phys_rows(len(c)).to(dev)]], y.to(dev)))
    rows = sum(int(b[0][0].shape[0]) for b in batches) / len(batches)
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "events_per_batch": 256, "rows_per_batch": round(rows),
           "rounds": args.rounds, "batches_per_window": args.batches * args.loops}
    arms = {"none": None, "gpu": mod.evaluator, "host": HostPIDEvaluator(mod.evaluator)}
    for ev in arms.values():                                                      # warm every arm
        segment_test_loop(mod, batches, dev, evaluator=ev)
    arms["gpu"].reset()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, ev in arms.items():
            loops = 1 if name == "host" else args.loops                          # the host arm is slow
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = segment_test_loop(mod, batches * loops, dev, evaluator=ev)     # ends in a read-back
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) / (loops * len(batches)) * 1e3)
            out.setdefault("test_loss", res["test_loss"])
    for name, v in times.items():
        out[name] = {"ms_per_batch": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
    out["gpu_added_ms"] = round(out["gpu"]["ms_per_batch"] - out["none"]["ms_per_batch"], 4)
    out["host_added_ms"] = round(out["host"]["ms_per_batch"] - out["none"]["ms_per_batch"], 4)

    # the entry points alone
    g = torch.Generator().manual_seed(1)
    for tag, n, per in (("small", None, None), ("large", 256 * 338, 338)):
        if n is None:
            c = batches[0][0][0]
            n = int(c.shape[0])
        else:
            # more rows per event than the detector has segments, so cells repeat -- which the tables do not mind
            c = torch.stack([torch.randint(0, 14, (n,), generator=g), torch.randint(0, 11, (n,), generator=g),
                             torch.arange(n) // per], 1).int().to(dev)
        pred, targ = torch.randint(0, 5, (n,), generator=g).to(dev), torch.randint(0, 5, (n,), generator=g).to(dev)
        fields = [phys_rows(n).to(dev)]
        ev = PIDEvaluator(dev)
        out[tag + "_rows"] = n
        out[tag + "_pid_add"] = time_calls(torch, lambda: ev.add(pred, targ, c, fields), args.rounds)
        out[tag + "_pid_add_events_given"] = time_calls(torch, lambda: ev.add(pred, targ, c, fields, n_events=256), args.rounds)
        mp = ev.metric_pairs
        out[tag + "_metric_pairs_accumulate"] = time_calls(
            torch, lambda: mp.add(ev.parameters, ev.accuracy, ev.category, ranges=ev.normalized_ranges), args.rounds)
        out[tag + "_single_ended_rows"] = int((ev.category >= 0).sum())
        ev.results()                                                              # no flag was raised

    # PSDEvaluator.add with and without the pairwise tables, 256 events
    T = 150
    c = torch.stack([torch.randint(0, 14, (1280,), generator=g), torch.randint(0, 11, (1280,), generator=g),
                     torch.arange(1280) // 5], 1).int().to(dev)
    f = torch.rand((1280, 2 * T), generator=g).to(dev)
    labels, preds = torch.randint(0, 2, (256,), generator=g).to(dev), torch.randint(0, 2, (256,), generator=g).to(dev)
    for tag, flag in (("psd_add", False), ("psd_add_metric_pairs", True)):
        pe = PSDEvaluator(["Gamma", "Neutron"], dev, n_samples=T, metric_pairs=flag)
        out[tag] = time_calls(torch, lambda: pe.add(([c, f], labels), None, preds), args.rounds)
        pe.results()
    out["psd_metric_pairs_added_us"] = round(out["psd_add_metric_pairs"]["us_per_call"] - out["psd_add"]["us_per_call"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
