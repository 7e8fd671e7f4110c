"""The optimizer update of one flat fp32 parameter buffer as a captured training step runs it, and the C2 step with SGD
against Adam.  One JSON line per measurement.
    usage: python tools/microbench_optim.py [update|step|all] [rounds]
update: FlatSGD (wfs_sgd_step, the C2 config's momentum 0.98 + nesterov), FlatAdam (wfs_adam_step; amsgrad off / on) and
  torch's single-tensor Adam with capturable=True (its elementwise launches), each captured as 20 steps in one HIP graph
  and replayed, timed with device events; buffers of the parameter counts of C2 (config/psd_c2_3d.json), GEP
  (tests/golden/gep_config.json, T = 150) and the C5 2-D hybrid net (the same config, T = 1024, n_dil = 3).  Bytes moved
  per element: SGD with momentum 20 (p, buf read + written, g read), Adam 28 (p, m, v read + written, g read), amsgrad 36.
step: the C2 training step at the bench's size (256 events, T = 256, bf16 rows) captured once with SGD (the config) and
  once with Adam (lr 1e-3), replayed alternately ``rounds`` x 100 times each.
WFS_LIB=<another build> times another variant of the kernels."""
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from waveformml_amd.psd.config import DictionaryUtility, load_config  # noqa: E402
from waveformml_amd.psd.lit import LitPSD  # noqa: E402
from waveformml_amd.psd.optim import FlatAdam, FlatSGD  # noqa: E402

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12        # MI355X: spec peak; float4 copy measured (MI355X_MICROARCH.md)
REPS, ITERS = 20, 10
dev = torch.device("cuda:0")
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
torch.cuda.set_stream(torch.cuda.Stream())


def c2_cfg():
    with open(os.path.join(ROOT, "config", "psd_c2_3d.json")) as f:
        return json.load(f)


def gep_cfg(T, n_dil):
    with open(os.path.join(ROOT, "tests", "golden", "gep_config.json")) as f:
        cfg = json.load(f)
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["hparams"]["n_dil"] = n_dil
    return cfg


def n_params(cfg, loader=DictionaryUtility.to_object):
    torch.manual_seed(0)
    return sum(p.numel() for p in LitPSD(loader(copy.deepcopy(cfg))).model.parameters())


def graph_us(step):
    """Device time of one ``step()`` inside a replayed graph of REPS steps (warmed up eagerly first)."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.current_stream()):
        for _ in range(REPS):
            step()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        a.record()
        for _ in range(ITERS):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / (ITERS * REPS))
    g.reset()
    return best


def update():
    sizes = {"C2": n_params(c2_cfg()), "GEP": n_params(gep_cfg(150, 0), load_config),
             "C5_2d_hybrid": n_params(gep_cfg(1024, 3), load_config)}
    for net, n in sizes.items():
        gen = torch.Generator(device=dev).manual_seed(1)
        w0 = torch.randn(n, device=dev, generator=gen)
        grad = torch.randn(n, device=dev, generator=gen) * 1e-2
        variants = [("FlatSGD", 20, lambda p: FlatSGD([p], lr=1e-3, momentum=0.98, nesterov=True)),
                    ("FlatAdam", 28, lambda p: FlatAdam([p], lr=1e-3)),
                    ("FlatAdam_amsgrad", 36, lambda p: FlatAdam([p], lr=1e-3, amsgrad=True)),
                    ("torch_Adam_capturable", 28, lambda p: torch.optim.Adam([p], lr=1e-3, capturable=True,
                                                                             foreach=False))]
        for name, bpe, make in variants:
            p = torch.nn.Parameter(w0.clone())
            p.grad = grad
            opt = make(p)
            us = graph_us(opt.step)
            bytes_ = bpe * n
            print(json.dumps({"net": net, "elements": n, "optimizer": name, "us_per_step": round(us, 2),
                              "bytes_per_element": bpe, "GB_per_s": round(bytes_ / us / 1e3, 1),
                              "share_of_hbm_spec": round(bytes_ / (us * 1e-6) / HBM_SPEC, 3),
                              "share_of_hbm_measured": round(bytes_ / (us * 1e-6) / HBM_MEASURED, 3),
                              "lib": os.environ.get("WFS_LIB", "in-tree")}), flush=True)
            del opt, p


def step():
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.graph import GraphedTrainStep
    c, f, y = synthetic.generate(256, 256, 3, seed=1)
    batch = ([torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev).to(torch.bfloat16)], torch.from_numpy(y).to(dev))
    steps = {}
    for name in ("SGD", "Adam"):
        cfg = c2_cfg()
        if name == "Adam":
            oc = cfg["optimize_config"]
            oc["optimizer_class"], oc["optimizer_params"], oc["lr"] = "optim.Adam", {}, 1e-3
        torch.manual_seed(0)
        mod = LitPSD(DictionaryUtility.to_object(cfg)).to(dev)
        red = FlatGradAllReducer(mod.model.parameters())
        mod.optimizer_parameters = red.optimizer_parameters()
        opt = mod.configure_optimizers()
        opt = opt[0][0] if isinstance(opt, tuple) else opt
        steps[name] = (GraphedTrainStep(mod, opt, red, batch), type(opt).__name__)
    times = {k: [] for k in steps}
    for _ in range(rounds):
        for name, (g, _) in steps.items():
            for _ in range(10):
                g(batch)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(100):
                g(batch)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) / 100 * 1e3)
    for name, (g, cls) in steps.items():
        g.check()
        print(json.dumps({"c2_captured_step": name, "optimizer_class": cls, "events": 256, "rows": int(len(c)),
                          "ms_per_step_median": round(float(np.median(times[name])), 4),
                          "ms_per_step_rounds": [round(v, 4) for v in times[name]]}), flush=True)
    print(json.dumps({"adam_minus_sgd_us_median": round((float(np.median(times["Adam"])) -
                                                          float(np.median(times["SGD"]))) * 1e3, 1)}), flush=True)
    for g, _ in steps.values():
        g.close()


if mode in ("update", "all"):
    update()
if mode in ("step", "all"):
    step()
