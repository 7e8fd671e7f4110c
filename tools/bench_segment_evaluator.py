"""Cost of the per-segment evaluation tables inside the LitZ test loop (psd/evaluate.segment_test_loop, SingleEndedZConv
with a 3-layer 3x3 conv stack, fp32 rows, 40 features, synthetic 256-event batches of about 765 rows), no kernel trace:

  none     the loop without an evaluator
  gpu      the loop + psd/segment_evaluator.ZEvaluator (csrc/segstats.hip, two launches per batch, no read-back)
  host     the loop + the path the reference takes: predictions, targets and coordinates to the host, the row walks there.
           The CPU side is the VECTORISED NumPy restatement of tests/segment_evaluator_cases.py, which is more
           favourable to the host than the reference's row-by-row loops would be.
  kernels  wfs_seg_z_accumulate (with an energy map) and wfs_seg_energy_accumulate alone, HIP events around back-to-back
           calls, at 765 rows and at 86.5 k rows (256 events x 338 rows)

The loop arms run in ONE process, alternating, `rounds` times; the figure per arm is the median over rounds and the
spread is (max - min) over rounds.  Every timed window ends in a device synchronise.

usage: python tools/bench_segment_evaluator.py [--batches 8] [--loops 8] [--rounds 7]      prints one JSON line"""
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

Z_CONFIG = {
    "system_config": {"model_name": "SingleEndedZConv", "n_samples": 20, "gpu_enabled": True, "half_precision": 0},
    "net_config": {"criterion_class": "L1Loss", "criterion_params": [], "imports": ["torch.nn", "waveformml_amd.spconv"],
                   "net_type": "2DConvolution", "algorithm": "conv",
                   "hparams": {"conv": {"kernel_size": 3, "n_layers": 3}, "point": {"pointwise_layers": 2}}},
    "optimize_config": {"imports": ["torch.optim"], "lr": 0.01, "optimizer_class": "optim.SGD",
                        "optimizer_params": {"momentum": 0.9}},
    "dataset_config": {"imports": []},
}


class HostZEvaluator:
    """add() as the reference's: everything to the host, the row walks there."""

    def __init__(self):
        import segment_evaluator_cases as sc
        from waveformml_amd.psd.segments import segment_status
        self.tables = sc.HostZTables(segment_status())

    def add(self, predictions, target, c, f, E=None):
        pred, targ, coo = predictions.detach().cpu().numpy(), target.detach().cpu().numpy(), c.detach().cpu().numpy()
        self.tables.add(coo, pred[:, 0], targ[:, 0])

    def results(self):
        return self.tables.results()


def time_calls(torch, fn, warm, n):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3 / n, 2)                                  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--loops", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litz import LitZ
    from waveformml_amd.psd.segment_evaluator import EnergyEvaluator, ZEvaluator
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment_evaluator: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mod = LitZ(load_config(copy.deepcopy(Z_CONFIG))).to(dev)
    rng = np.random.default_rng(5)
    batches = []
    for s in range(args.batches):
        c, f, _y = synthetic.generate(256, 20, 3, seed=900 + s, layout="2d")
        z = torch.from_numpy(rng.random(len(c)).astype(np.float32))
        batches.append(([torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev)], z.to(dev)))
    rows = sum(int(b[0][0].shape[0]) for b in batches) / len(batches)
    out = {"events_per_batch": 256, "rows_per_batch": round(rows), "rounds": args.rounds,
           "batches_per_window": args.batches * args.loops}
    arms = {"none": None, "gpu": ZEvaluator(dev), "host": HostZEvaluator()}
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
        pred = torch.rand((256, 2, 14, 11), generator=g).to(dev)
        targ = (torch.rand((256, 2, 14, 11), generator=g) * 0.9 + 0.05).to(dev)
        zev, eev = ZEvaluator(dev, use_energy=True), EnergyEvaluator(dev)
        out[tag + "_rows"] = n
        out[tag + "_seg_z_accumulate_us"] = time_calls(
            torch, lambda: zev.add_planes(pred, 1, targ, 1, c, targ, 0), 10, 100)
        out[tag + "_seg_energy_accumulate_us"] = time_calls(torch, lambda: eev.add_planes(pred, 0, targ, 0, c), 10, 100)
        zev.results(), eev.results()                                              # no flag was raised
    print(json.dumps(out))


if __name__ == "__main__":
    main()
