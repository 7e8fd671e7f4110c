"""Cost of psd/class_metrics.ClassificationMetrics (csrc/classmetrics.hip):

  add      ``add`` alone (one launch, no read-back) at 256 x 2 (a LitPSD batch), 768 x 5 (a segment-classifier batch)
           and 86.5 k x 5 rows, fp32 logits, 100 thresholds
  torch    the torch composition that produces the same numbers at the same shapes: evaluate._score (criterion, softmax,
           argmax, compare, mean), the bincount confusion matrix, and the reference's ROCCurve for ONE class index (100
           threshold comparisons, each with its bincount) -- the tables keep the ROC bins of EVERY class; its kernel
           launches per call are counted from a torch.profiler trace of one call (``null`` when the trace is unavailable)
  loop     evaluate.test_loop(capture=True) on the GEP fixture config (tests/golden/gep_config.json), 256-event synthetic
           batches resident on the device, per batch: without ``metrics`` (the parent commit's code path: every change to
           the loop sits behind ``metrics is not None``) and with ``module.metrics`` (one launch per batch, ``_score`` not
           run).  Each call builds and captures its step once; both arms pay that alike.

All arms of a group run in ONE process, alternating, ``rounds`` times; the figure is the median over rounds and the spread
(max - min) over rounds.  A kernel window is 100 back-to-back calls; every timed window ends in a device synchronise.

usage: python tools/bench_class_metrics.py [--rounds 7] [--batches 64] [--no-trace]      prints one JSON line"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(256, 2), (768, 5), (86528, 5)]
CALLS = 100


def window(fn, calls=CALLS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def summary(values):
    return {"median_us": round(statistics.median(values), 2), "spread_us": round(max(values) - min(values), 2)}


def torch_composition(C, T):
    """The same numbers from torch ops; accumulators persistent, as the tables are."""
    crit, softmax = torch.nn.CrossEntropyLoss(), torch.nn.Softmax(dim=1)
    state = dict(tot=torch.zeros((), device=DEV), acc=torch.zeros((), device=DEV),
                 confusion=torch.zeros(C * C, dtype=torch.int64, device=DEV),
                 roc=torch.zeros(T, 4, dtype=torch.int64, device=DEV))
    thr = [(i + 1.0) / T for i in range(T)]

    def call(logits, labels):
        b = logits.shape[0]
        prob = softmax(logits)
        pred = torch.argmax(prob, dim=1)
        state["tot"] += crit(logits, labels) * b
        state["acc"] += (pred == labels).float().mean() * b
        state["confusion"] += torch.bincount(labels * C + pred, minlength=C * C)
        binary = (labels == 0).long() * 2
        for i in range(T):
            state["roc"][i] += torch.bincount(binary + (prob[:, 0] >= thr[i]).long(), minlength=4)
    return call


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if str(getattr(e, "device_type", "")).endswith("CUDA")
                   and not e.key.startswith(("Memcpy", "Memset")))
    except Exception as exc:  # the figure is optional; the timings are not
        print("trace unavailable: %r" % (exc,), file=sys.stderr)
        return None


def bench_add(rounds, trace):
    from waveformml_amd.psd.class_metrics import ClassificationMetrics
    out = {}
    for n, C in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(n)
        logits = (torch.randn(n, C, generator=g) * 2).to(DEV)
        labels = torch.randint(0, C, (n,), generator=g).to(DEV)
        ev = ClassificationMetrics(DEV, C)
        comp = torch_composition(C, 100)
        arms = {"add": lambda: ev.add(logits, labels), "torch": lambda: comp(logits, labels)}
        for fn in arms.values():
            window(fn, 5)
        times = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                times[k].append(window(fn, CALLS if k == "add" else 10))
        res = {k: summary(v) for k, v in times.items()}
        if trace:
            res["add"]["launches"] = count_launches(arms["add"])
            res["torch"]["launches"] = count_launches(arms["torch"])
        ev.results()                           # the flags are clean
        out["%dx%d" % (n, C)] = res
    return out


def bench_loop(rounds, n_batches):
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.evaluate import test_loop
    from waveformml_amd.psd.lit import LitPSD
    with open(os.path.join(ROOT, "tests", "golden", "gep_config.json")) as fh:
        cfg = json.load(fh)
    torch.manual_seed(0)
    mod = LitPSD(load_config(copy.deepcopy(cfg))).to(DEV)
    mod.eval()
    base = []
    for s in range(8):
        c, f, y = synthetic.generate(256, 150, len(cfg["system_config"]["type_names"]), seed=s, layout="2d")
        base.append(([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV)], torch.from_numpy(y).to(DEV)))
    batches = [base[i % 8] for i in range(n_batches)]
    metrics = mod.metrics

    def arm(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = test_loop(mod, batches, DEV, capture=True, metrics=m)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_batches * 1e6, out
    arms = {"without_metrics": None, "with_metrics": metrics}
    for m in arms.values():
        arm(m)
    times, last = {k: [] for k in arms}, {}
    for _ in range(rounds):
        for k, m in arms.items():
            metrics.reset()
            t, last[k] = arm(m)
            times[k].append(t)
    res = {k: summary(v) for k, v in times.items()}
    res["per_batch_of"] = n_batches
    res["test_loss"] = {k: v["test_loss"] for k, v in last.items()}
    res["test_acc"] = {k: v["test_acc"] for k, v in last.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    out = {"tool": "bench_class_metrics", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "add": bench_add(args.rounds, not args.no_trace), "loop": bench_loop(args.rounds, args.batches)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
