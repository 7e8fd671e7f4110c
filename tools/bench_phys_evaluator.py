"""Cost of the extracted-feature evaluation statistics (psd/phys_evaluator.PhysEvaluator, csrc/physstats.hip) inside the
captured test loop of config/psd_features_det.json (ExtractedFeatureConvNet, fp32 rows of 7 quantities; synthetic batches
of 256 events and 3 rows per event on average), and of one ``add`` alone.

  none   captured eval, no evaluator
  gpu    captured eval + PhysEvaluator (three launches per batch, no read-back until results())
  host   captured eval + the path the reference takes: device-to-host copies of the batch, then the statistics on the CPU.
         The CPU side here is VECTORISED NumPy (segment sums with np.add.reduceat, a cumulative sum for the running
         energy, vectorised bin search), which FLATTERS the host: the reference walks rows and events one by one under
         numba on one core, and its float32 sums are sequential, which a vectorised sum does not reproduce bit for bit.

The three arms alternate in one process; every timed window ends in one results().  Median over rounds, spread = max - min
over rounds.  ``add`` alone: HIP events around back-to-back calls, at 768 rows and at 256 x 338 = 86 528 rows.

usage: python tools/bench_phys_evaluator.py [--rounds 7] [--batches 32] [--profile]
       --profile writes profiles/phys_evaluator_ab.txt"""
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


def det_batch(rng, events, rows_per_event, n_classes):
    """A synthetic PulseDatasetDet batch: `rows_per_event` distinct segments per event on average (at least one)."""
    import numpy as np
    if rows_per_event <= 8:
        counts = np.maximum(rng.poisson(rows_per_event - 1, events) + 1, 1)
    else:
        counts = np.full(events, rows_per_event)
    ev = np.repeat(np.arange(events), counts)
    n = len(ev)
    coords = np.column_stack([rng.integers(0, 14, n), rng.integers(0, 11, n), ev]).astype(np.int32)
    feats = rng.uniform(0.02, 0.6, (n, 7)).astype(np.float32)
    return coords, feats, rng.integers(0, n_classes, events).astype(np.int64)


class HostEvaluator:
    """add() as the reference's: everything to the host, averages and tables there (vectorised; see the docstring)."""

    def __init__(self, n_classes):
        import numpy as np
        import phys_evaluator_cases as pc
        self.np, self.pc = np, pc
        self.tables = pc.HostTables(n_classes)

    def add(self, batch, output, predictions):
        np = self.np
        inputs, labels = batch
        n = int(inputs[2].item()) if len(inputs) > 2 else inputs[0].shape[0]
        c, f = inputs[0][:n].cpu().numpy(), inputs[1][:n].float().cpu().numpy()
        y, p, _o = labels.cpu().numpy(), predictions.cpu().numpy(), output.cpu().numpy()
        E = len(y)
        q = self.pc.derived(f)
        first = np.searchsorted(c[:, 2], np.arange(E))
        has = np.diff(np.append(first, n)) > 0
        starts = first[has]
        q0 = q[0].astype(np.float64)
        ene = np.zeros(E)
        ene[has] = np.add.reduceat(q0, starts)
        cs = np.cumsum(q0)
        base = np.zeros(n)
        base[:] = np.repeat((cs[starts] - q0[starts]), np.diff(np.append(starts, n)))
        running = cs - base
        coo = np.zeros((E, 2))
        coo[has] = np.add.reduceat(c[:, :2] * running[:, None], starts, axis=0)
        feat = np.zeros((8, E), np.float32)
        sums = np.zeros((7, E))
        sums[:, has] = np.add.reduceat((q * q[0]).astype(np.float64), starts, axis=1)
        pos = ene > 0
        safe = np.where(pos, ene, 1.0)
        feat[1:7] = np.where(pos, sums[1:] / safe, sums[1:])
        feat[0] = np.where(pos, ene, 0.0)
        coo = np.where(pos[:, None], coo / safe[:, None], coo)
        mult = np.where(pos, np.diff(np.append(first, n)), 0).astype(np.int32)
        feat[7] = mult
        self.tables.add(coo, feat, mult, p, y)

    def reset(self):
        self.tables = self.pc.HostTables(self.tables.p["C"])

    def results(self):
        return self.tables.t


def add_alone(torch, ev, batch, pred, windows=7, calls=100):
    for _ in range(10):
        ev.add(batch, None, pred)
    us = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            ev.add(batch, None, pred)
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(us), max(us) - min(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import test_loop
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.phys_evaluator import PhysEvaluator
    from waveformml_amd.spconv import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream())
    ops.ASSUME_VALID_UNIQUE_INDICES = True
    cfg = json.load(open(os.path.join(ROOT, "config", "psd_features_det.json")))
    names = list(cfg["system_config"]["type_names"])
    torch.manual_seed(0)
    mod = LitPSD(load_config(copy.deepcopy(cfg))).to(dev)
    rng = np.random.default_rng(900)

    def on_device(c, f, y):
        return ([torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev)], torch.from_numpy(y).to(dev))
    batches = [on_device(*det_batch(rng, 256, 3, len(names))) for _ in range(args.batches)]
    batches.sort(key=lambda b: -b[0][0].shape[0])                  # the capture sizes itself on its first batch
    rows = sum(int(b[0][0].shape[0]) for b in batches) / len(batches)
    arms = {"none": None, "gpu": PhysEvaluator(names, dev, spectra=True), "host": HostEvaluator(len(names))}
    times = {k: [] for k in arms}
    for k, ev in arms.items():                                     # warm-up: capture, allocations
        test_loop(mod, batches[:2], dev, capture=True, evaluator=ev)
    for _ in range(args.rounds):
        for k, ev in arms.items():
            if ev is not None:
                ev.reset()
            torch.cuda.synchronize()
            t = time.perf_counter()
            test_loop(mod, batches, dev, capture=True, evaluator=ev)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) / len(batches) * 1e3)
    out = {"events_per_batch": 256, "rows_per_batch": round(rows, 1), "batches_per_window": len(batches),
           "rounds": args.rounds}
    for k in arms:
        out[k + "_ms_per_batch"] = round(statistics.median(times[k]), 4)
        out[k + "_spread"] = round(max(times[k]) - min(times[k]), 4)
    alone = {}
    for label, per_event in (("small", 3), ("large", 338)):
        c, f, y = det_batch(np.random.default_rng(7), 256, per_event, len(names))
        batch = on_device(c, f, y)
        for spectra in (False, True):
            ev = PhysEvaluator(names, dev, spectra=spectra)
            med, spread = add_alone(torch, ev, batch, torch.zeros_like(batch[1]))
            alone[(label, spectra)] = (len(c), med, spread)
            out["add_%s%s_us" % (label, "_spectra" if spectra else "")] = round(med, 2)
        out["rows_" + label] = len(c)
    print(json.dumps(out))
    if args.profile:
        lines = [
            "GPU PhysEvaluator against the host path (tools/bench_phys_evaluator.py --profile; MI355X, no kernel trace).",
            "Written by the tool; method: its docstring.", "",
            "evaluate.test_loop(capture=True) of LitPSD on config/psd_features_det.json (ExtractedFeatureConvNet, fp32);",
            "synthetic batches of 256 events / %.1f rows on average, %d batches per timed window; the three arms" % (
                rows, len(batches)),
            "alternate in one process, %d rounds; median over rounds, spread = max - min over rounds." % args.rounds, "",
            "%-62s %-14s %s" % ("arm", "ms per batch", "spread")]
        text = {"none": "loop, no evaluator", "gpu": "loop + GPU evaluator with spectra (three launches, no read-back)",
                "host": "loop + host path (5 D2H copies + vectorised NumPy)"}
        for k in arms:
            lines.append("%-62s %-14s %s" % (text[k], out[k + "_ms_per_batch"], out[k + "_spread"]))
        lines += ["added by the GPU evaluator: %+.4f ms per batch; by the host path: %+.4f ms per batch" % (
            out["gpu_ms_per_batch"] - out["none_ms_per_batch"], out["host_ms_per_batch"] - out["none_ms_per_batch"]),
            "(the host arm is vectorised NumPy -- segment sums, a cumulative sum for the running energy, a vectorised bin",
            "search -- which flatters the host against the reference's row-by-row walks under numba)", "",
            "PhysEvaluator.add alone (HIP events around 100 back-to-back calls, 10 warm-up calls; median of 7 windows)",
            "%-62s %-14s %s" % ("", "us per call", "spread")]
        for (label, spectra), (n, med, spread) in alone.items():
            lines.append("%-62s %-14s %s" % ("add, %d rows, 256 events%s" % (n, ", with spectra" if spectra else ""),
                                             round(med, 2), round(spread, 2)))
        lines += ["A call is two library entries = three launches; at 768 rows it is bound by its launches, at 86 528 rows by",
                  "the sequential row walk of the longest events (338 rows each, one wavefront per event).", ""]
        with open(os.path.join(ROOT, "profiles", "phys_evaluator_ab.txt"), "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
