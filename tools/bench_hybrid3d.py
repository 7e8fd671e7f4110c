"""BASELINE.json configs[4] ("C5") as BASELINE.md 3 writes it -- feat [n, 1, 2T] -> TCN -> voxelise on the GPU -> C2-style
SubM3d head (config/psd_c5_hybrid3d.json, psd/net.SPConvHybrid3DNet) -- one card.  Prints one JSON line: eager and
captured ms / step, events / s and voxels / s of the hybrid net; in the same run the captured step of the same head fed
the host-voxelised batch (psd/synthetic layout "3d", same seed) and the fused TCN forward + backward alone on the same
rows (captured as well); fp32 logits / loss parity against the CPU twin (torch TCN + torch voxeliser + oracle.spconv
head, as tests/test_gpu_hybrid3d.py assembles it) on the same batch and weights; the voxeliser's algorithmic bytes.
    usage: python tools/bench_hybrid3d.py [events=256] [steps=50] [dtype=bf16] [captured-only]
``captured-only``: the captured hybrid step alone (a run under rocprofv3 --kernel-trace --stats)."""
import copy
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from waveformml_amd.psd import synthetic  # noqa: E402
from waveformml_amd.psd.config import DictionaryUtility  # noqa: E402
from waveformml_amd.psd.ddp import FlatGradAllReducer  # noqa: E402
from waveformml_amd.psd.graph import GraphedTrainStep  # noqa: E402
from waveformml_amd.psd.lit import LitPSD  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
dname = sys.argv[3] if len(sys.argv) > 3 else "bf16"
only_captured = len(sys.argv) > 4 and sys.argv[4] == "captured-only"
dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dname]
T = 1024
dev = torch.device("cuda:0")
torch.cuda.set_stream(torch.cuda.Stream())
with open(os.path.join(ROOT, "config", "psd_c5_hybrid3d.json")) as fh:
    CFG = json.load(fh)
CFG["system_config"]["n_samples"] = T


def module(cfg, seed=0):
    torch.manual_seed(seed)
    return LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg))).to(dev)


def optimised(mod):
    red = FlatGradAllReducer(mod.model.parameters())
    mod.optimizer_parameters = red.optimizer_parameters()
    opt = mod.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, tuple) else opt
    return red, opt


def time_fn(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


c2, f2, y = synthetic.generate(E, T, 3, seed=1, layout="2d")
rows_dev = torch.from_numpy(f2).to(dev).to(dtype)
batch = ([torch.from_numpy(c2).to(dev), rows_dev], torch.from_numpy(y).to(dev))
n_rows = int(c2.shape[0])
V = int(((f2[:, :T] > 0) | (f2[:, T:] > 0)).sum())

# ---- the hybrid net: captured (and eager) step
hyb = module(CFG)
red, opt = optimised(hyb)


def eager():
    red.reset()
    loss = hyb.training_step(batch, 0)
    loss.backward()
    red.finish()
    opt.step()


eager_ms = None if only_captured else time_fn(eager, max(5, steps // 5))
g = GraphedTrainStep(hyb, opt, red, batch)
graph_ms = time_fn(lambda: g(batch), steps)
g.check()
if only_captured:
    print(json.dumps({"events": E, "voxels": V, "captured_ms_per_step": round(graph_ms, 4)}))
    sys.exit(0)
# which rulebook build / head route each layer took in the captured step's device-count mode
paths = []
for name, m in hyb.model.sparseModel.named_children():
    rb = getattr(m, "last_rulebook", None)
    if rb is None:
        continue
    if getattr(rb, "events_out", None) is not None:
        p = "event-local strided (evconv.hip)"
    elif getattr(rb, "event_flags", None) is not None:
        p = "event-local SubM (evrulebook.hip)"
    else:
        p = "chip-wide (rulebook.hip)"
    paths.append("%s %s: %s" % (name, type(m).__name__, p))
head_route = hyb.model.head_route            # what SPConvNet._head decided when the step was captured

# ---- the same head fed the host-voxelised batch (3-D layout, same seed)
c3, f3, y3 = synthetic.generate(E, T, 3, seed=1, layout="3d")
assert len(c3) == V
head_cfg = copy.deepcopy(CFG)
head_cfg["net_config"]["net_class"] = "SPConvNet.SPConvNet"
head_cfg["net_config"].pop("hparams")
hmod = module(head_cfg)
hred, hopt = optimised(hmod)
hbatch = ([torch.from_numpy(c3).to(dev), torch.from_numpy(f3).to(dev).to(dtype)], torch.from_numpy(y3).to(dev))
hg = GraphedTrainStep(hmod, hopt, hred, hbatch)
head_ms = time_fn(lambda: hg(hbatch), steps)
hg.check()

# ---- the fused TCN forward + backward alone on the same rows, captured
tcn = hyb.model.waveformLayer
params = [p for p in tcn.parameters()]
x_static = rows_dev.unsqueeze(1).clone()
gy = torch.randn_like(x_static)


def tcn_step():
    red.reset()                         # the parameters' gradient slots in the flat buffer: stable addresses
    tcn(x_static).backward(gy)


s = torch.cuda.current_stream()
for _ in range(3):
    tcn_step()
torch.cuda.synchronize()
tg = torch.cuda.CUDAGraph()
with torch.cuda.graph(tg, stream=s):
    tcn_step()
tcn_ms = time_fn(tg.replay, steps)

# ---- fp32 parity against the CPU twin on the same batch and weights (dropout off on both sides)


def twin_forward(self, x, batch_size=None):
    coords, feats = x[0], x[1]
    if batch_size is None:
        batch_size = int(coords[-1, -1]) + 1
    yv = self.waveformLayer(feats.unsqueeze(1)).squeeze(1)
    thr = self.voxelizer.threshold
    r, t = torch.nonzero((feats[:, :T] > thr) | (feats[:, T:] > thr), as_tuple=True)
    c = coords.long()
    idx = torch.stack([c[r, 2], c[r, 0], c[r, 1], t], 1).int()
    st = self.spconv.SparseConvTensor(torch.stack([yv[r, t], yv[r, T + t]], 1), idx, self.spatial_size, batch_size)
    return self._head(st)


pcfg = copy.deepcopy(CFG)
pcfg["net_config"]["hparams"]["wf_params"]["dropout"] = 0.0
pg = module(pcfg, seed=5)
ccfg = copy.deepcopy(pcfg)
ccfg["net_config"]["imports"] = ["oracle.spconv" if m == "waveformml_amd.spconv" else m for m in ccfg["net_config"]["imports"]]
torch.manual_seed(5)
pc = LitPSD(DictionaryUtility.to_object(ccfg))
pc.model.forward = types.MethodType(twin_forward, pc.model)
pc.load_state_dict({k: v.cpu() for k, v in pg.state_dict().items()})
with torch.no_grad():
    lg = pg.model([batch[0][0], torch.from_numpy(f2).to(dev)]).double().cpu().numpy()
    lc = pc.model([torch.from_numpy(c2), torch.from_numpy(f2)]).double().numpy()
loss_g = float(pg.training_step(([batch[0][0], torch.from_numpy(f2).to(dev)], batch[1]), 0))
loss_c = float(pc.training_step(([torch.from_numpy(c2), torch.from_numpy(f2)], torch.from_numpy(y)), 0))

sz = rows_dev.element_size()
n_off = n_rows * ((T + 63) // 64) + 1
# forward: the rows read twice for the mask (count and emit pass), the values at active positions, indices + features
# written, slice offsets written and read; backward: dfeat + the indices' t read, every row written whole
fwd_bytes = 2 * n_rows * 2 * T * sz + V * 2 * sz + V * (16 + 2 * sz) + 3 * 4 * n_off
bwd_bytes = V * (2 * sz + 16) + n_rows * 2 * T * sz + 4 * n_off
print(json.dumps({
    "config": "psd_c5_hybrid3d.json: TCN (n_dil 3, k 3, dropout 0.2) -> voxelise -> 3 SubM3d + 3 SparseConv3d(1,1,4) -> "
              "Linear(20480, 3), %s rows, T = %d" % (dname, T),
    "events": E, "rows": n_rows, "voxels": V, "voxel_fraction": round(V / (n_rows * T), 4),
    "eager_ms_per_step": round(eager_ms, 4), "captured_ms_per_step": round(graph_ms, 4),
    "events_per_s": round(E / (graph_ms * 1e-3)), "voxels_per_s": round(V / (graph_ms * 1e-3)),
    "head_on_host_voxels_captured_ms_per_step": round(head_ms, 4), "tcn_fwd_bwd_alone_captured_ms": round(tcn_ms, 4),
    "bar_captured_le_head_plus_tcn_plus_30us": bool(graph_ms <= head_ms + tcn_ms + 0.030),
    "excess_over_head_plus_tcn_us": round((graph_ms - head_ms - tcn_ms) * 1e3, 1),
    "fp32_parity": {"logits_max_abs_rel_to_scale": float(np.abs(lg - lc).max() / max(np.abs(lc).max(), 1e-30)),
                    "loss_rel": abs(loss_g - loss_c) / abs(loss_c)},
    "voxelizer_algorithmic_bytes": {"forward_plan_plus_emit": int(fwd_bytes), "backward": int(bwd_bytes)},
    "head_route_captured": head_route, "rulebook_paths_captured": paths,
    "voxel_capacity": hyb.model.voxelizer.out_capacity,
}))
