"""Cost of the per-batch evaluation statistics inside the captured test loop (psd/evaluate.test_loop, 2-D GEP net, fp32 rows,
T = 150, synthetic 256-event batches), one process per arm and no kernel trace:

  none     captured eval, no evaluator
  gpu      captured eval + psd/evaluator.PSDEvaluator (csrc/evalstats.hip)
  host     captured eval + the path the reference takes: device-to-host copy of the batch, then the statistics on the CPU.
           The CPU side here is the VECTORISED NumPy restatement of tests/evaluator_cases.py, which is more favourable
           to the host than the reference's sample-by-sample loops under numba would be on one core.
  kernels  the two entry points alone (HIP events around back-to-back launches), with the bytes (a) has to stream

usage: python tools/bench_evaluator.py            (runs every arm in a child process, prints one JSON line)
       python tools/bench_evaluator.py --arm gpu  (one arm in this process)"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARMS = ["none", "gpu", "host", "kernels"]


class HostEvaluator:
    """add() as the reference's: everything to the host, statistics and tables there."""

    def __init__(self, n_classes, T):
        import evaluator_cases as ec
        import numpy as np
        self.ec, self.np = ec, np
        self.tables = ec.HostTables(n_classes, T)
        self.gains, self.seg = np.ones((14, 11, 2)), np.zeros((14, 11), np.float32)

    def add(self, batch, output, predictions):
        inputs, labels = batch
        n = int(inputs[2].item()) if len(inputs) > 2 else inputs[0].shape[0]
        c, f = inputs[0][:n].cpu().numpy(), inputs[1][:n].float().cpu().numpy()
        y, p, _o = labels.cpu().numpy(), predictions.cpu().numpy(), output.cpu().numpy()
        self.tables.add(self.ec.average_pulse(c, f, self.gains, self.seg, len(y)), p, y)

    def results(self):
        return self.tables.t


def run_arm(arm, n_batches, loops):
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import test_loop
    from waveformml_amd.psd.evaluator import PSDEvaluator
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.spconv import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream())
    ops.ASSUME_VALID_UNIQUE_INDICES = True
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "gep_config.json")))
    names = list(cfg["system_config"]["type_names"])
    torch.manual_seed(0)
    mod = LitPSD(load_config(copy.deepcopy(cfg))).to(dev)
    batches = []
    for s in range(n_batches):
        c, f, y = synthetic.generate(256, 150, len(names), seed=900 + s, layout="2d")
        batches.append(([torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev)], torch.from_numpy(y).to(dev)))
    rows = sum(int(b[0][0].shape[0]) for b in batches) / len(batches)
    out = {"arm": arm, "events_per_batch": 256, "rows_per_batch": round(rows)}
    if arm == "kernels":
        ev = PSDEvaluator(names, dev, n_samples=150)
        (c, f), y = batches[0]
        pred = torch.zeros_like(y)
        ev.add(batches[0], None, pred)
        lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr()

        def stats():
            _lib.check(lib.wfs_event_pulse_stats(
                p(c), p(f), c.shape[0], 150, _lib.WFS_F32, None, 256, p(ev.gain_factor), p(ev.seg_status), 14, 11, 0,
                p(ev._offsets), p(ev._rowstats), p(ev.avg_coo), p(ev.summed_pulses), p(ev.output_stats),
                p(ev.multiplicity), p(ev.n_SE), p(ev.psdl), p(ev.psdr), p(ev.energy), p(ev.features), p(ev.flags), st))

        def accumulate():
            _lib.check(lib.wfs_eval_accumulate(
                256, 150, len(names), p(ev.avg_coo), p(ev.summed_pulses), p(ev.multiplicity), p(ev.n_SE), p(ev.psdl),
                p(ev.psdr), p(ev.energy), p(pred), p(y), ev.n_bins, ev.n_mult, ev.n_confusion, ev.n_SE_max, 14, 11,
                ev.emin, ev.emax, ev.psd_min, ev.psd_max, p(ev.tables), p(ev.sum_wf), p(ev.sum_labelled), p(ev.flags), st))
        for name, fn in (("event_pulse_stats", stats), ("eval_accumulate", accumulate)):
            for _ in range(10):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(100):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name + "_us"] = round(a.elapsed_time(b) * 10.0, 2)              # ms per 100 -> us per call
        row_bytes = c.shape[0] * 300 * 4
        out["waveform_bytes"] = row_bytes
        out["event_pulse_stats_GBps"] = round(row_bytes / (out["event_pulse_stats_us"] * 1e-6) / 1e9, 1)
        # the same launches over 256 events x 338 rows (86.5 k rows, 104 MB of fp32 waveforms): more rows per event than
        # the detector has segments, so cells repeat -- which the statistics do not mind
        g = torch.Generator().manual_seed(1)
        n = 256 * 338
        c = torch.stack([torch.randint(0, 14, (n,), generator=g), torch.randint(0, 11, (n,), generator=g),
                         torch.arange(n) // 338], 1).int().to(dev)
        f = torch.rand((n, 300), generator=g).to(dev)
        ev.add(([c, f], y), None, pred)
        for _ in range(5):
            stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            stats()
        b.record()
        torch.cuda.synchronize()
        out["large_rows"] = n
        out["large_event_pulse_stats_us"] = round(a.elapsed_time(b) * 50.0, 1)
        out["large_waveform_bytes"] = n * 300 * 4
        out["large_event_pulse_stats_GBps"] = round(n * 1200 / (out["large_event_pulse_stats_us"] * 1e-6) / 1e9, 1)
        return out
    ev = {"none": None, "gpu": PSDEvaluator(names, dev, n_samples=150), "host": HostEvaluator(len(names), 150)}[arm]
    test_loop(mod, batches[:2], dev, capture=True, evaluator=ev)
    if arm == "gpu":
        ev.reset()
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = test_loop(mod, batches * loops, dev, capture=True, evaluator=ev)
    torch.cuda.synchronize()
    out["ms_per_batch"] = round((time.perf_counter() - t) / (loops * len(batches)) * 1e3, 3)
    out["test_acc"] = res["test_acc"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--loops", type=int, default=8)
    args = ap.parse_args()
    if args.arm:
        print(json.dumps(run_arm(args.arm, args.batches, args.loops)))
        return
    out = {}
    for arm in ARMS:
        loops = 1 if arm == "host" else args.loops                              # the host arm is slow
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--batches", str(args.batches),
                            "--loops", str(loops)], capture_output=True, text=True, timeout=420)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit("arm %s failed with status %d" % (arm, r.returncode))
        out[arm] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
