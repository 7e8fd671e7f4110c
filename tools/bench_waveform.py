"""A/B timing of the per-pulse TCN (config/waveform_tcn_z.json's plan, TemporalConvNet(1, [8, 16, 8], 3)) at L = 59.

Arm ``fused``: this tree's TemporalConvNet(fused=True) -- the wfs_tcnc_* kernels.  Arm ``torch``: the TemporalConvNet of
another tree given by ``--parent`` (a worktree of the parent commit), which runs the torch composition for multi-channel
plans.  Each measurement is one fresh process (warm-up, then the median of --iters forward+backward calls timed with
HIP events); the two arms alternate, --reps measurements each, in one run.  The captured LitWaveform training step
(psd/graph.GraphedTrainStep, fused path) is timed in the same run.

    python tools/bench_waveform.py --parent /path/to/parent/worktree --out profiles/waveform_tcn_ab.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN, K, L = [8, 16, 8], 3, 59


def _events_ms(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def measure_tcn(arm, n, warmup, iters):
    import torch
    from waveformml_amd.psd.tcn import TemporalConvNet
    torch.manual_seed(0)
    net = (TemporalConvNet(1, PLAN, K, 0.0, fused=True) if arm == "fused" else TemporalConvNet(1, PLAN, K, 0.0))
    net = net.cuda().train()
    x = torch.rand(n, 1, L, device="cuda")
    dy = torch.randn(n, PLAN[-1], L, device="cuda")

    def step():
        net.zero_grad(set_to_none=True)
        net(x).backward(dy)
    ms = _events_ms(step, warmup, iters)
    if arm == "fused":
        from waveformml_amd.psd import tcn
        assert tcn.TCNC_CALLS[0] > 0
    return ms


def measure_captured(n, warmup, iters):
    import copy
    import torch
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.graph import GraphedTrainStep
    from waveformml_amd.psd.litwaveform import LitWaveform
    with open(os.path.join(HERE, "config", "waveform_tcn_z.json")) as f:
        cfg = json.load(f)
    cfg["optimize_config"].pop("scheduler_class", None)
    torch.manual_seed(0)
    mod = LitWaveform(DictionaryUtility.to_object(copy.deepcopy(cfg))).cuda()
    red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
    mod.optimizer_parameters = red.optimizer_parameters()
    opt = mod.configure_optimizers()
    c = torch.randint(0, 616, (n, 1), dtype=torch.int32, device="cuda")
    batch = ([c, torch.rand(n, L, device="cuda")], torch.rand(n, device="cuda"))
    step = GraphedTrainStep(mod, opt, red, batch, warmup=2)
    ms = _events_ms(lambda: step(batch), warmup, iters)
    step.check()
    step.close()
    return ms


def _child(root, args):
    env = dict(os.environ)
    root = os.path.abspath(root)
    env["PYTHONPATH"] = root
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, cwd=root,
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("%s %s failed:\n%s" % (root, args, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=["fused", "torch", "captured"])
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--parent", help="root of the parent commit's tree (the torch arm)")
    ap.add_argument("--sizes", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.measure:
        ms = (measure_captured(a.n, a.warmup, a.iters) if a.measure == "captured"
              else measure_tcn(a.measure, a.n, a.warmup, a.iters))
        print(json.dumps({"ms": ms}))
        return
    common = ["--warmup", str(a.warmup), "--iters", str(a.iters)]
    lines = ["TCN forward+backward, plan %s k=%d L=%d fp32, dropout 0; median of %d calls per measurement, %d "
             "measurements per arm, arms alternating, one process per measurement" % (PLAN, K, L, a.iters, a.reps)]
    for n in [int(s) for s in a.sizes.split(",")]:
        arms = {"fused": [], "parent torch": [], "captured LitWaveform step": []}
        for _ in range(a.reps):
            arms["fused"].append(_child(HERE, ["--measure", "fused", "--n", str(n)] + common))
            arms["parent torch"].append(_child(a.parent, ["--measure", "torch", "--n", str(n)] + common))
            arms["captured LitWaveform step"].append(_child(HERE, ["--measure", "captured", "--n", str(n)] + common))
        med = {k: statistics.median(v) for k, v in arms.items()}
        spread = {k: max(v) - min(v) for k, v in arms.items()}
        margin = max(spread["fused"], spread["parent torch"])
        lines.append("N=%d rows:" % n)
        for k, v in arms.items():
            lines.append("  %-27s median %.4f ms  spread %.4f ms  runs %s" % (k, med[k], spread[k],
                                                                             " ".join("%.4f" % t for t in v)))
        lines.append("  parent / fused = %.2f;  parent - fused = %.4f ms vs margin (larger spread) %.4f ms: %s"
                     % (med["parent torch"] / med["fused"], med["parent torch"] - med["fused"], margin,
                        "faster" if med["parent torch"] - med["fused"] > margin else "NOT faster beyond the spread"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
