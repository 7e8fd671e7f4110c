"""A/B timing of the dense C1 net (config/psd_c1_dense.json: DenseConvNet, block 300 -> 221 -> 142 -> 63 on the 14 x 11
map, each layer Conv2d + BatchNorm2d + ReLU) at batch 32 and batch 256, in fp32 and bf16, training mode.

Arm ``kernels``: this tree's Conv2DBlock(fused=True) -- the wfs_conv2d_* kernels -- and wfs_densify_rows.  Arm ``torch``:
the same modules as the torch composition of nn.Conv2d / nn.BatchNorm2d / nn.ReLU (MIOpen) on the same tensors (for bf16
rows: the block's parameters in bf16 for the stack, autocast for the step), and ``sparse_coo_tensor(...).to_dense()`` +
``permute`` (+ the copy that makes the map contiguous) for the densify.  Three measurements per arm:

  stack      forward + backward of the block on a dense map
  step       the captured LitPSD training step (psd/graph.GraphedTrainStep) on capacity-padded rows; the torch arm keeps
             the densify launch (nothing else honours the padded rows) and runs the block and the linears as torch does
  densify    rows -> map

Each (arm, batch, dtype) is one fresh process under its own time limit (warm-up, then the median of --iters calls timed
with HIP events); the arms alternate, --reps processes each, in one run.  A Python error of an arm is recorded in place of
a time.  A child that dies of a signal or runs out of time ends the whole run: nothing more is started on the GPU.

    python tools/bench_dense.py --out profiles/dense_conv2d_ab.txt
"""
import argparse
import copy
import json
import os
import platform
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 14, 11
ROWS_PER_EVENT = 31          # BASELINE C1: 1 k rows at batch 32


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


def _config():
    with open(os.path.join(HERE, "config", "psd_c1_dense.json")) as f:
        cfg = json.load(f)
    cfg["optimize_config"].pop("scheduler_class", None)
    return cfg


def _rows(batch, C, dtype, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    n = batch * ROWS_PER_EVENT
    cells = torch.randperm(batch * H * W, generator=g)[:n].sort().values
    coords = torch.stack([(cells % (H * W)) // W, cells % W, cells // (H * W)], 1).to(torch.int32)
    coords[-1, 2] = batch - 1
    return coords.cuda(), torch.rand(n, C, generator=g).to(dtype).cuda()


def measure_stack(arm, batch, dtype, warmup, iters):
    import torch
    from waveformml_amd.psd import convnet2d
    cfg = _config()
    hp = cfg["net_config"]["hparams"]
    C = 2 * cfg["system_config"]["n_samples"]
    torch.manual_seed(0)
    net = convnet2d.Conv2DBlock(C, hp["out_planes"], hp["n_conv"], [H, W, C], fused=arm == "kernels", **hp["conv_params"])
    net = net.cuda().train()
    if arm == "torch" and dtype != torch.float32:
        net = net.to(dtype)
    coords, feats = _rows(batch, C, dtype)
    x = convnet2d.densify_rows(feats, coords, batch, H, W)              # channels_last, for both arms
    with torch.no_grad():
        shape = net(x).shape
    dy = torch.randn(shape, device="cuda").to(dtype)
    calls = convnet2d.CONV2D_CALLS[0]

    def step():
        net.zero_grad(set_to_none=True)
        net(x).backward(dy)
    ms = _events_ms(step, warmup, iters)
    assert (convnet2d.CONV2D_CALLS[0] > calls) == (arm == "kernels")
    return ms


def measure_step(arm, batch, dtype, warmup, iters):
    import torch
    from waveformml_amd.psd import convnet2d
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.densenet import DenseConvNet
    from waveformml_amd.psd.graph import GraphedTrainStep
    from waveformml_amd.psd.lit import LitPSD
    cfg = _config()
    C = 2 * cfg["system_config"]["n_samples"]
    torch.manual_seed(0)
    mod = LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))
    if arm == "torch":
        def forward(x, net=mod.model):
            dense = convnet2d.densify_rows(x[1], x[0], int(net.batch_size_hint), H, W, x[2] if len(x) > 2 else None)
            with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
                out = net.model.model(dense).reshape(-1, net.n_linear)
                return net.linear(out).float()
        assert isinstance(mod.model, DenseConvNet)
        mod.model.forward = forward
    mod = mod.cuda()
    red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
    mod.optimizer_parameters = red.optimizer_parameters()
    opt = mod.configure_optimizers()
    coords, feats = _rows(batch, C, dtype)
    labels = torch.randint(0, 2, (batch,), device="cuda")
    data = ([coords, feats], labels)
    calls = convnet2d.CONV2D_CALLS[0]
    step = GraphedTrainStep(mod, opt, red, data, warmup=2)
    ms = _events_ms(lambda: step(data), warmup, iters)
    step.check()
    step.close()
    assert (convnet2d.CONV2D_CALLS[0] > calls) == (arm == "kernels")
    return ms


def measure_densify(arm, batch, dtype, warmup, iters):
    import torch
    from waveformml_amd.psd import convnet2d
    C = 2 * _config()["system_config"]["n_samples"]
    coords, feats = _rows(batch, C, dtype)
    if arm == "kernels":
        return _events_ms(lambda: convnet2d.densify_rows(feats, coords, batch, H, W), warmup, iters)
    index = coords[:, [2, 0, 1]].long().t().contiguous()

    def dense():
        return torch.sparse_coo_tensor(index, feats, size=[batch, H, W, C]).to_dense().permute(0, 3, 1, 2).contiguous()
    return _events_ms(dense, warmup, iters)


def _child(args, limit):
    """One (arm, batch, dtype) in a fresh process: {measurement: milliseconds or the last line of a Python error}."""
    env = dict(os.environ)
    env["PYTHONPATH"] = HERE
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, cwd=HERE, capture_output=True,
                         text=True, timeout=limit)
    if out.returncode != 0:
        raise RuntimeError("%s ended with status %d:\n%s" % (args, out.returncode, out.stderr[-3000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def _header(a):
    import torch
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    return ["Dense C1 net (config/psd_c1_dense.json: block 300 -> 221 -> 142 -> 63, kernels 3 2 2, 14 x 11 map), training mode",
            "box: %s, %s, torch %s; commit %s (+ the working tree of this change)"
            % (platform.node(), torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__,
               commit or "unknown"),
            "protocol: one process per (arm, batch, dtype), arms alternating, %d processes each; per measurement %d warm-up "
            "calls, then the median of %d calls timed with HIP events" % (a.reps, a.warmup, a.iters)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=["kernels", "torch"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=150, help="seconds per process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.measure:
        import torch
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[a.dtype]
        res = {}
        for name, fn in (("stack", measure_stack), ("step", measure_step), ("densify", measure_densify)):
            try:
                res[name] = fn(a.measure, a.batch, dtype, a.warmup, a.iters)
            except (RuntimeError, AssertionError, TypeError, ValueError) as e:       # recorded in place of a time
                res[name] = "error: %s: %s" % (type(e).__name__, str(e).strip().splitlines()[-1][:160] if str(e) else "")
                torch.cuda.synchronize()
        print(json.dumps(res))
        return
    assert a.warmup >= 3 and a.iters >= 20
    lines = _header(a)
    common = ["--warmup", str(a.warmup), "--iters", str(a.iters)]
    for batch in [int(s) for s in a.batches.split(",")]:
        for dt in a.dtypes.split(","):
            runs = {"kernels": [], "torch": []}
            for _ in range(a.reps):
                for arm in ("kernels", "torch"):
                    runs[arm].append(_child(["--measure", arm, "--batch", str(batch), "--dtype", dt] + common, a.limit))
            lines.append("batch %d (%d rows), %s:" % (batch, batch * ROWS_PER_EVENT, dt))
            for what in ("stack", "step", "densify"):
                med = {}
                for arm in ("kernels", "torch"):
                    v = [r[what] for r in runs[arm]]
                    errs = [t for t in v if isinstance(t, str)]
                    if errs:
                        lines.append("  %-8s %-8s %s" % (what, arm, errs[0]))
                        continue
                    med[arm] = statistics.median(v)
                    lines.append("  %-8s %-8s median %.4f ms  runs %s" % (what, arm, med[arm], " ".join("%.4f" % t for t in v)))
                if len(med) == 2:
                    lines.append("  %-8s torch / kernels = %.2f" % (what, med["torch"] / med["kernels"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
