"""Micro-benchmark of the max-pool kernels (csrc/pool.hip) on the rulebook of C2's first strided layer (3 x 3 x 3, stride
[1, 1, 4]) next to the conv kernels that gather through the same tables (run on the GPU box).
usage: python tools/microbench_pool.py [iters] [f32|bf16] [events] [samples]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from waveformml_amd.psd import synthetic
from waveformml_amd.spconv import ops, functional as Fsp

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
DT = torch.bfloat16 if (len(sys.argv) > 2 and sys.argv[2] == "bf16") else torch.float32
NB = int(sys.argv[3]) if len(sys.argv) > 3 else 256
TS = int(sys.argv[4]) if len(sys.argv) > 4 else 256
dev = torch.device("cuda:0")
c, f, y = synthetic.generate(NB, TS, 3, seed=1234)
torch.cuda.set_stream(torch.cuda.Stream())
idx = torch.from_numpy(np.ascontiguousarray(c[:, [3, 0, 1, 2]])).to(dev)
GEO = ([14, 11, TS], [3] * 3, [1, 1, 4], [0] * 3, [1] * 3)
rb = ops.build_rulebook(idx, NB, *GEO, False, known_unique=True)
N, M = rb.N, rb.M
# the same rulebook as a captured step builds it: capacity rows, counts on the device, the packed by-input table
nv = torch.tensor([N], dtype=torch.int64, device=dev)
rbd = ops.build_rulebook(idx, NB, *GEO, False, n_dev=nv, out_capacity=int(M * 1.25), flags={})
X = torch.randn(N, 32, device=dev).clamp_(min=0).to(DT)          # rows behind a ReLU
dY = torch.randn(M, 32, device=dev).to(DT)
dYd = torch.randn(rbd.M, 32, device=dev).to(DT)
ES = X.element_size()
W = torch.randn(27, 32, 32, device=dev) * 0.1
Y = Fsp.maxpool_fwd(rb.nbr_in, None, 27, M, X)
Yd = Fsp.maxpool_fwd(rbd.nbr_in, None, 27, rbd.M, X, rbd.m_dev)


def timeit(name, fn, nbytes, reps=10, rounds=9):
    """`reps` launches captured into a HIP graph; `rounds` timed batches of `iters` replays each, warm; the MEDIAN batch
    gives GPU time per launch including the in-graph launch gap, free of Python / ctypes overhead."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) / (iters * reps) * 1e3)
    med = float(np.median(us))
    print("%-40s %8.2f us (min %.2f max %.2f)  %7.1f GB/s  %.3f of 8 TB/s" % (name, med, min(us), max(us), nbytes / med / 1e3,
                                                                              nbytes / med / 1e3 / 8000.0), flush=True)


P = int((rb.nbr_out >= 0).sum())
print("%s  events %d  N %d  M %d  pairs %d" % (str(DT).split(".")[-1], NB, N, M, P))
# bytes = table + gathered rows + written rows (the table at its stored size: 4 bytes per entry)
timeit("pool fwd 32ch (by-output table)", lambda: Fsp.maxpool_fwd(rb.nbr_in, None, 27, M, X), 27 * M * 4 + P * 32 * ES + M * 32 * ES)
timeit("pool bwd 32ch (dense by-input table)", lambda: Fsp.maxpool_bwd(rb.nbr_out, 27, 0, N, X, Y, dY),
       27 * N * 4 + N * 32 * ES + 2 * P * 32 * ES + N * 32 * ES)
if rbd.nbr_out_packed is not None:
    kl = rbd.packed_kl
    timeit("pool bwd 32ch (packed table, counts)", lambda: Fsp.maxpool_bwd(rbd.nbr_out_packed, 27, kl, N, X, Yd, dYd, rbd.n_dev),
           27 // kl * N * 4 + N * 32 * ES + 2 * P * 32 * ES + N * 32 * ES)
timeit("pool fwd 32ch (capacity rows, counts)", lambda: Fsp.maxpool_fwd(rbd.nbr_in, None, 27, rbd.M, X, rbd.m_dev),
       27 * M * 4 + P * 32 * ES + M * 32 * ES)
# the yardstick: the convolution through the same tables (tools/microbench_conv.py's "conv s4" lines), same byte formula
# plus its filters
timeit("conv s4 fwd 32->32 (yardstick)", lambda: Fsp.gather_conv(rb.nbr_in, None, 27, -1, M, X, W, False, None),
       27 * M * 4 + P * 32 * ES + M * 32 * ES + 27 * 4096)
timeit("conv s4 dX (yardstick)", lambda: Fsp.gather_conv(rb.nbr_out, None, 27, -1, N, dY, W, True, None),
       27 * N * 4 + P * 32 * ES + N * 32 * ES + 27 * 4096)
