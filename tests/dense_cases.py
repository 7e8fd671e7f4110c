"""Shared by tests/test_dense_cases_host.py and tests/test_gpu_dense_edges.py: the edge cases of the dense
Conv2d + BatchNorm2d + ReLU (+ Dropout) stack kernels (csrc/conv2d.hip: wfs_conv2d_fwd / wfs_conv2d_bwd), their inputs,
the float64 reference, a plain-Python statement of the planning arm every case is there for, and the reference of
wfs_densify_rows.  (Not a test module: nothing here is collected.)

Reference: the torch composition nn.Conv2d -> nn.BatchNorm2d -> nn.ReLU, times the dropout multipliers where a layer
has some, in float64 on the CPU, layer by layer, on the X and dY the kernels see (rounded to the row type first), with
the gradient kept at every conv output.  Parameters are drawn as tests/test_gpu_densenet.py draws them (taps of order
1 / sqrt(fan), BN scale in [0.5, 1.5], shift ~ N(0, 0.3), running statistics away from (0, 1)); the dropout masks come
from waveform_cases.hash_masks with the documented counter (layer << 44 | flat index of the element in the layer's
output as NCHW).

The seed of a case (per row type and mode: the conditions are properties of the rounded inputs) is the first of
0 .. MAX_TRIES - 1 at which, in float64,
  * no pre-ReLU value of a layer lies within the case's margin (seq_cases.RELU_MARGIN = 1e-5 unless the table says
    otherwise) of that layer's largest magnitude,
  * every layer has between 5 % and 95 % of its ReLUs on,
  * torch's own fp32 CPU run is within seq_cases.E32_MAX = 3e-6 of the float64 run on every tensor,
  * for 16-bit rows, the float64 run with the operands the header says the backward rounds to the row type (dz, the
    filters of the dX product, the activation the dW product reads, Y and dX themselves) so rounded -- and nothing else
    changed -- is within E16_SHARE = 0.5 of the row type's bar (2e-2 / 3e-3) on every tensor: half the bar for
    the number format, half for the kernels (rounding Y and dX to the row type alone costs 0.1 .. 0.2 of it).  A tensor that is a small difference of large terms (d bn.weight of an eval-mode layer whose
    running statistics sit far from the data's: sum g xhat with xhat nearly constant) carries the 2^-9 of a bf16 dz
    at the size of its TERMS, whatever kernel computes it; such a draw is ill-posed for a bar taken against the
    tensor's own magnitude, exactly as a draw that fails the fp32 condition is.
These are conditions on the inputs, proven on the CPU by the host test; nothing on the GPU relaxes them.

Two rows (case `m2`): with M = 2, xhat = +-1 / sqrt(1 + eps / var) and dz = gamma invstd g (1 - xhat^2) / 2 is a
difference of terms 1 + var / eps times its size (tests/bn_cases.py, "Two rows"), so no fp32 evaluation holds it at
eps = 1e-5 and var of order one.  The case takes eps = 0.5, where the difference is of the order of its terms.

The planning constants of csrc/conv2d.hip that decide an arm are copied below; arms_py restates wfs_conv2d_arms, and
the host test holds the two against each other.
"""
import collections
import functools

import numpy as np
import torch
from torch import nn

import waveform_cases as wc
from seq_cases import E32_MAX, KINDS, RELU_MARGIN

DROP_P = 0.3
DROP_SEED = 0x2545F4914F6CDD1D        # the int64 the GPU test puts in device memory
MAX_TRIES = 40
E16_SHARE = 0.5                       # of the 16-bit bar: what the documented 16-bit operands alone may cost
RL, NRB_MAX, EW_MAXBLK = 4, 256, 1024
TM, TN, TK, DW_CHUNK = 64, 64, 32, 2048

Layer = collections.namedtuple("Layer", "cout fs st pd dil bias mom eps")
# kinds: the row types the case runs in; modes: "train" / "eval"; drop: dropout p per layer or None (NULL); dx: dX
# wanted; nbt0: the layers whose num_batches_tracked address is 0; margin: the case's ReLU margin; arm: the tags
# (tags_of) the case is in the table for
Case = collections.namedtuple("Case", "name B H W c0 layers kinds modes drop dx nbt0 margin arm why")

ALL = ("f32", "bf16", "f16")
F32 = ("f32",)


def L(cout, fs=3, st=1, pd=0, dil=1, bias=False, mom=0.1, eps=1e-5):
    return Layer(cout, fs, st, pd, dil, bias, mom, eps)


def _c(name, B, H, W, c0, layers, arm, why, kinds=F32, modes=("train",), drop=None, dx=True, nbt0=(), margin=RELU_MARGIN):
    return Case(name, B, H, W, c0, tuple(layers), kinds, modes, drop, dx, tuple(nbt0), margin, set(arm), why)


CASES = [
    # ------------------------------------------------------------------------------------------------ row passes
    _c("m2", 2, 1, 1, 3, [L(4, 1, eps=0.5)], {"M=2", "layers=1"},
       "the smallest training call: unbiased factor 2, one partial for four folding lanes"),
    _c("nrb-exact", 4, 32, 32, 2, [L(3, 3, pd=1)], {"nrb=256 exact", "dw slices=2 full"},
       "M = 4096: 256 row blocks of 16 rows, nothing strides"),
    _c("nrb-over", 5, 32, 32, 3, [L(4, 3, pd=1), L(2, 3, pd=1)], {"nrb strided", "dw slices=3", "dw last=1024"},
       "M = 5120 on both layers: the statistics, g-sum and dz blocks stride; 3 dW slices, the last 1024 positions",
       kinds=ALL, modes=("train", "eval")),
    _c("ew-exact", 16, 32, 32, 2, [L(3, 3, pd=1)], {"ew=1024 exact"}, "M = 16384: 1024 blocks in the BN + ReLU pass"),
    _c("ew-over", 17, 32, 32, 2, [L(3, 3, pd=1)], {"ew strided"}, "M = 17408: the BN + ReLU blocks stride"),
    _c("b2048", 2048, 1, 1, 3, [L(4, 1)], {"B=2048"}, "B = MAX_BATCH on a 1 x 1 map"),
    _c("chunk-64", 2, 6, 5, 3, [L(64, 3, pd=1)], {"cout=64"}, "one full channel chunk of the row passes"),
    _c("chunk-65", 2, 6, 5, 3, [L(65, 3, pd=1)], {"cout=65"}, "a second channel chunk with one live lane",
       modes=("train", "eval")),
    # ------------------------------------------------------------------------------------------------- dW slices
    _c("dw-2048", 2, 32, 32, 2, [L(3, 3, pd=1)], {"dw slices=1 full"}, "exactly one full dW slice"),
    _c("dw-2052", 4, 27, 19, 5, [L(3, 3, pd=1)], {"dw slices=2", "dw last=4"}, "the second dW slice holds 4 positions",
       kinds=ALL),
    # -------------------------------------------------------------------------------------------- GEMM tile edges
    _c("edge-63", 7, 3, 3, 63, [L(63, 1)], {"fwd M=63", "fwd N=63", "dx N=63", "dw M=63", "dw N=63"},
       "fs 1, 63 -> 63 on 63 positions: M, N and K of all three products one below a tile edge", kinds=ALL),
    _c("edge-64", 1, 8, 8, 64, [L(64, 1)], {"fwd M=64", "fwd N=64", "dx N=64", "dw M=64", "dw N=64"},
       "fs 1, 64 -> 64 on 64 positions: M, N of all three products on a tile edge (K two steps)", kinds=ALL),
    _c("edge-65", 5, 13, 1, 65, [L(65, 1)], {"fwd M=65", "fwd N=65", "dx N=65", "dw M=65", "dw N=65"},
       "fs 1, 65 -> 65 on 65 positions: one past a tile edge everywhere", kinds=ALL),
    _c("k1-n63", 2, 6, 5, 1, [L(63, 1), L(1, 1)], {"fwd K=1", "fwd N=1", "fwd N=63", "dx K=1", "dx N=1", "dw N=1", "dw M=1"},
       "1 -> 63 -> 1 pointwise: K = 1 and N = 1 in every product", kinds=ALL),
    _c("chain-31-33", 2, 6, 5, 31, [L(64, 1), L(33, 1, bias=True), L(65, 1)],
       {"fwd K=31", "fwd K=33", "dx N=31", "dx N=33", "dx K=33", "dw N=31", "dw N=33", "bias on some layers"},
       "31 -> 64 -> 33 -> 65 pointwise: K = 31 (a short only step) and 33 (one past a step)", kinds=ALL),
    _c("k32", 2, 7, 5, 2, [L(2, 4, pd=1)], {"fwd K=32", "dx K=32", "dw N=32", "fs=4"},
       "cin 2, cout 2, fs 4: K = 32 forward and in dX, N = 32 in dW", kinds=ALL),
    _c("maxc", 2, 3, 3, 512, [L(512, 1), L(1, 3, pd=2)], {"cin=512", "cout=512", "pd=reach"},
       "512 -> 512 -> 1: the channel bound in both places, 8 channel chunks", kinds=ALL),
    _c("k12800", 2, 5, 5, 512, [L(3, 5, pd=2)], {"K=12800", "fs=5"}, "the longest contraction, 400 steps"),
    # --------------------------------------------------------------------------------------------------- geometry
    _c("g-max", 3, 32, 29, 3, [L(4, 5, st=3, pd=16, dil=4), L(3, 3, pd=1)],
       {"fs=5", "st=3", "dil=4", "pd=16", "pd=reach", "unread rows", "H=32"},
       "fs 5, dilation 4, padding 16 = the reach, stride 3 with rows and columns no tap reads; then 3 x 3",
       kinds=ALL, modes=("train", "eval")),
    _c("g-st3-d3", 2, 17, 14, 3, [L(3, 2, st=3, pd=0, dil=3), L(4, 4, st=2, pd=3)],
       {"fs=2", "fs=4", "st=3", "st=2", "dil=3", "pd=0", "pd=reach", "unread rows"},
       "fs 2 at dilation 3 and stride 3 without padding, then fs 4 at stride 2 with the largest padding", kinds=ALL),
    _c("g-d2-k5", 2, 20, 18, 3, [L(3, 5, st=2, pd=4, dil=2), L(2, 2, pd=0, dil=4)],
       {"fs=5", "st=2", "dil=2", "dil=4", "unread rows"}, "fs 5 at dilation 2 and stride 2, then fs 2 at dilation 4",
       kinds=ALL),
    _c("to-1x1", 3, 7, 5, 3, [L(4, 3, st=2), L(3, 2), L(3, 2, st=3, pd=1)], {"ends 1x1", "st=3", "unread rows"},
       "7 x 5 -> 3 x 2 -> 2 x 1 -> 1 x 1: the last layer's statistics over 3 values", kinds=ALL),
    _c("row-1x32", 2, 1, 32, 3, [L(3, 3, pd=1), L(2, 3, st=2, pd=2)], {"map 1x32", "pd=reach"}, "a 1 x 32 map", kinds=ALL),
    _c("col-32x1", 2, 32, 1, 3, [L(3, 3, pd=2, dil=2), L(2, 2, st=3, pd=1)], {"map 32x1", "st=3", "unread rows"},
       "a 32 x 1 map", kinds=ALL),
    _c("single-st2", 3, 8, 6, 3, [L(5, 3, st=2)], {"layers=1", "st=2", "unread rows", "unread cells of dX"},
       "one layer at stride 2: input row 7 and column 5 are read by no tap, dX is exactly zero there", kinds=ALL),
    _c("eight", 2, 6, 5, 3,
       [L(4, 3, pd=1), L(5, 1, bias=True), L(6, 2, pd=1), L(7, 2), L(8, 3, pd=1, bias=True), L(9, 3, pd=2, dil=2), L(6, 1),
        L(3, 3, pd=1, bias=True)], {"layers=8", "bias on some layers", "fs=1", "fs=2", "fs=3"},
       "eight layers of 3 .. 9 channels, mixed fs / pd, bias on three of them", kinds=ALL, modes=("train", "eval")),
    # ------------------------------------------------------------------------------------------ records and modes
    _c("drop-0-p-0", 3, 7, 5, 4, [L(5, 3, pd=1), L(6, 3, pd=1), L(3, 3, pd=1)], {"dropout [0, p, 0]"},
       "dropout on the middle layer only", drop=(0.0, DROP_P, 0.0)),
    _c("bn-records", 3, 7, 5, 4, [L(5, 3, pd=1, mom=0.0), L(4, 2, mom=0.1, eps=1e-3, bias=True), L(3, 3, pd=1, mom=1.0, eps=0.1)],
       {"momentum 0", "momentum 1", "eps per layer", "nbt=0", "bias on some layers"},
       "momentum 0 / 0.1 / 1 and eps 1e-5 / 1e-3 / 0.1 per layer, num_batches_tracked absent on the middle one",
       modes=("train", "eval"), nbt0=(1,)),
    _c("no-dx", 3, 7, 5, 4, [L(5, 3, pd=1), L(3, 2, st=2)], {"no dX"}, "dX NULL: the first layer's input gradient is skipped",
       kinds=ALL, dx=False),
    _c("odd-act", 3, 5, 3, 3, [L(3, 3, pd=1), L(2, 3, pd=1)], {"odd 16-bit activation"},
       "135 elements between the layers: the 16-bit buffers end in a padded 8-byte granule", kinds=ALL),
]
BY_NAME = {c.name: i for i, c in enumerate(CASES)}
assert len(BY_NAME) == len(CASES)

# every arm of the table; the host test holds the union of tags_of over the cases against it
REQUIRED = set().union(*[c.arm for c in CASES])


def case_params():
    """(case index, kind, mode) of every run of the table."""
    return [(i, kind, mode) for i, c in enumerate(CASES) for kind in c.kinds for mode in c.modes]


def run_id(i, kind, mode):
    return "%s-%s-%s" % (CASES[i].name, kind, mode)


# ----------------------------------------------------------------------------------------------- plan arithmetic
def shapes(c):
    """Per layer (cin, hin, win, hout, wout), the reference's size formula."""
    out, cin, h, w = [], c.c0, c.H, c.W
    for ly in c.layers:
        reach = ly.dil * (ly.fs - 1)
        ho, wo = (h + 2 * ly.pd - reach - 1) // ly.st + 1, (w + 2 * ly.pd - reach - 1) // ly.st + 1
        out.append((cin, h, w, ho, wo))
        cin, h, w = ly.cout, ho, wo
    return out


def plan_arrays(c):
    """(channels, fs, st, pd, dil) as the entry points take them."""
    return tuple([getattr(ly, f) for ly in c.layers] for f in ("cout", "fs", "st", "pd", "dil"))


def _row_blocks(M, cap):
    return max(1, min(cap, (M + 4 * RL - 1) // (4 * RL)))


def arms_py(c):
    """wfs_conv2d_arms in plain Python: per layer [M, row blocks of the statistics / g-sum / dz passes, row blocks of the
    BN + ReLU pass, forward tiles along M, along N, K steps, dW slices, positions in the last slice]."""
    out = []
    for ly, (cin, _h, _w, ho, wo) in zip(c.layers, shapes(c)):
        M, K = c.B * ho * wo, cin * ly.fs * ly.fs
        ns = (M + DW_CHUNK - 1) // DW_CHUNK
        out.append([M, _row_blocks(M, NRB_MAX), _row_blocks(M, EW_MAXBLK), (M + TM - 1) // TM, (ly.cout + TN - 1) // TN,
                    (K + TK - 1) // TK, ns, M - (ns - 1) * DW_CHUNK])
    return out


def products(c):
    """(M, N, K) of the three GEMMs of every layer (header comment of csrc/conv2d.hip): {"fwd": [...], "dx": [...],
    "dw": [...]}; dX of layer 0 only when the case wants it."""
    out = {"fwd": [], "dx": [], "dw": []}
    for i, (ly, (cin, h, w, ho, wo)) in enumerate(zip(c.layers, shapes(c))):
        taps = ly.fs * ly.fs
        out["fwd"].append((c.B * ho * wo, ly.cout, cin * taps))
        if i > 0 or c.dx:
            out["dx"].append((c.B * h * w, cin, ly.cout * taps))
        out["dw"].append((ly.cout, cin * taps, c.B * ho * wo))
    return out


EDGES = (1, 31, 32, 33, 63, 64, 65)


def tags_of(c, arms):
    """The arms of the issue's list that the case reaches, from `arms` (wfs_conv2d_arms' answer, or arms_py) and plain
    arithmetic on the plan.  Only tags of REQUIRED are reported."""
    t = set()
    sh = shapes(c)
    for ly, (cin, h, w, ho, wo), a in zip(c.layers, sh, arms):
        M, nrb, ew, _tm, _tn, _ks, ns, last = a
        reach = ly.dil * (ly.fs - 1)
        t |= {"M=2"} if M == 2 else set()
        t |= {"nrb=256 exact"} if (nrb == NRB_MAX and M == NRB_MAX * 4 * RL) else set()
        t |= {"nrb strided"} if (nrb == NRB_MAX and M > NRB_MAX * 4 * RL) else set()
        t |= {"ew=1024 exact"} if (ew == EW_MAXBLK and M == EW_MAXBLK * 4 * RL) else set()
        t |= {"ew strided"} if (ew == EW_MAXBLK and M > EW_MAXBLK * 4 * RL) else set()
        t |= {"dw slices=1 full"} if (ns == 1 and last == DW_CHUNK) else set()
        t |= {"dw slices=2 full"} if (ns == 2 and last == DW_CHUNK) else set()
        t |= {"dw slices=%d" % ns, "dw last=%d" % last} if ns > 1 else set()
        t |= {"cout=%d" % ly.cout, "cin=%d" % cin, "K=%d" % (cin * ly.fs * ly.fs)}
        t |= {"fs=%d" % ly.fs, "st=%d" % ly.st, "dil=%d" % ly.dil, "H=%d" % h}
        t |= {"pd=0"} if ly.pd == 0 and ly.fs > 1 else set()
        t |= {"pd=reach"} if ly.pd == reach and reach > 0 else set()
        t |= {"pd=%d" % ly.pd}
        t |= {"unread rows"} if ((h + 2 * ly.pd - reach - 1) % ly.st and (w + 2 * ly.pd - reach - 1) % ly.st) else set()
        t |= {"momentum 0"} if ly.mom == 0 else set()
        t |= {"momentum 1"} if ly.mom == 1 else set()
    for name, prods in products(c).items():
        for M, N, K in prods:
            t |= {"%s M=%d" % (name, M)} if M in EDGES else set()
            t |= {"%s N=%d" % (name, N)} if N in EDGES else set()
            t |= {"%s K=%d" % (name, K)} if K in EDGES else set()
    ly0, (_cin, h, w, _ho, _wo) = c.layers[0], sh[0]
    reach = ly0.dil * (ly0.fs - 1)
    if len(c.layers) == 1 and c.dx and ly0.pd == 0 and (h - reach - 1) % ly0.st and (w - reach - 1) % ly0.st:
        t.add("unread cells of dX")
    t |= {"B=%d" % c.B, "layers=%d" % len(c.layers)}
    t |= {"ends 1x1"} if sh[-1][3:] == (1, 1) and (c.H, c.W) != (1, 1) else set()
    t |= {"map %dx%d" % (c.H, c.W)}
    t |= {"bias on some layers"} if 0 < sum(ly.bias for ly in c.layers) < len(c.layers) else set()
    t |= {"dropout [0, p, 0]"} if c.drop is not None and c.drop[0] == 0 and c.drop[-1] == 0 and max(c.drop) > 0 else set()
    t |= {"eps per layer"} if len({ly.eps for ly in c.layers}) == len(c.layers) > 1 else set()
    t |= {"nbt=0"} if c.nbt0 else set()
    t |= {"no dX"} if not c.dx else set()
    if len(c.layers) > 1 and "bf16" in c.kinds:
        t |= {"odd 16-bit activation"} if any((c.B * ho * wo * ly.cout) % 2 for ly, (_a, _b, _c2, ho, wo) in
                                              list(zip(c.layers, sh))[:-1]) else set()
    return t & REQUIRED


# ------------------------------------------------------------------------------- problems and float64 references
def make_net(c, seed):
    """[(nn.Conv2d, nn.BatchNorm2d)] per layer in fp32 with live parameters, drawn as tests/test_gpu_densenet.py's
    _randomise draws them."""
    g = torch.Generator().manual_seed(seed)
    net, cin = [], c.c0
    with torch.no_grad():
        for ly in c.layers:
            conv = nn.Conv2d(cin, ly.cout, (ly.fs, ly.fs), (ly.st, ly.st), ly.pd, (ly.dil, ly.dil), 1, ly.bias)
            bn = nn.BatchNorm2d(ly.cout, eps=ly.eps, momentum=ly.mom)
            fan = cin * ly.fs * ly.fs
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / fan ** 0.5)
            if ly.bias:
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.5)
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.3)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.2)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
            bn.num_batches_tracked.fill_(41)
            net.append((conv, bn))
            cin = ly.cout
    return net


def drop_masks(c):
    """The dropout multipliers of every layer's output [B, C, H', W'] in float64 (None: the layer has none), rebuilt
    from DROP_SEED with the counter of include/wfsparse.h: layer << 44 | flat NCHW index."""
    masks = []
    for i, (ly, (_cin, _h, _w, ho, wo)) in enumerate(zip(c.layers, shapes(c))):
        if c.drop is None or c.drop[i] == 0:
            masks.append(None)
            continue
        shape = (c.B, ly.cout, ho, wo)
        ctr = (np.uint64(i) << np.uint64(44)) + np.arange(int(np.prod(shape)), dtype=np.uint64)
        masks.append(wc.hash_masks(DROP_SEED, c.drop[i], ctr).reshape(shape))
    return masks


def _twin(net, dtype, training):
    out = []
    for conv, bn in net:
        c2, b2 = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.dilation,
                           1, conv.bias is not None).to(dtype), nn.BatchNorm2d(bn.num_features, eps=bn.eps,
                                                                              momentum=bn.momentum).to(dtype)
        c2.load_state_dict({k: v.to(dtype) for k, v in conv.state_dict().items()})
        b2.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in bn.state_dict().items()})
        out.append((c2.train(training), b2.train(training)))
    return out


def forward(net, x, masks, training, dtype, pre=None):
    """The composition layer by layer on a twin of `net` in `dtype`: (y, [conv outputs], twin); `pre` (a list)
    receives every layer's pre-ReLU values.  Eval mode applies no dropout."""
    twin = _twin(net, dtype, training)
    h, zs = x, []
    for i, (conv, bn) in enumerate(twin):
        z = conv(h)
        if z.requires_grad:
            z.retain_grad()
        zs.append(z)
        v = bn(z)
        if pre is not None:
            pre.append(v.detach())
        h = torch.relu(v)
        if training and masks[i] is not None:
            h = h * masks[i].to(dtype)
    return h, zs, twin


def run(net, x, dy, masks, training, dtype):
    """Forward and backward in `dtype`: ([(name, tensor)], {conv.bias name: summed |dz| scale}, pre-ReLU values).
    Names: y, dx, then per layer L<i>.conv.weight, .conv.bias (where present), .bn.weight, .bn.bias (gradients),
    .running_mean, .running_var (after the call)."""
    xr = x.detach().to(dtype).requires_grad_(True)
    pre = []
    y, zs, twin = forward(net, xr, masks, training, dtype, pre)
    y.backward(dy.to(dtype))
    out, bias_scale = [("y", y.detach()), ("dx", xr.grad)], {}
    for i, ((conv, bn), z) in enumerate(zip(twin, zs)):
        out.append(("L%d.conv.weight" % i, conv.weight.grad))
        if conv.bias is not None:
            out.append(("L%d.conv.bias" % i, conv.bias.grad))
            bias_scale["L%d.conv.bias" % i] = float(z.grad.abs().sum((0, 2, 3)).max())
        out += [("L%d.bn.weight" % i, bn.weight.grad), ("L%d.bn.bias" % i, bn.bias.grad),
                ("L%d.running_mean" % i, bn.running_mean.detach().clone()), ("L%d.running_var" % i, bn.running_var.detach().clone())]
        assert int(bn.num_batches_tracked) == (42 if training else 41)
    return out, bias_scale, pre


def scale_of(name, ref_tensor, bias_scale, training):
    """What a tensor's error is taken against: its largest float64 magnitude -- for a conv bias in front of a
    training-mode BatchNorm, whose exact gradient is zero, the summed |dz| of the reference
    (tests/test_gpu_densenet.py)."""
    if training and name in bias_scale:
        return bias_scale[name]
    return float(ref_tensor.abs().max())


def relu_state(pre):
    """(smallest min|v| / max|v| over the layers, smallest and largest share of ReLUs on)."""
    margin = min(float(v.abs().min()) / float(v.abs().max()) for v in pre)
    on = [float((v > 0).double().mean()) for v in pre]
    return margin, min(on), max(on)


def rounded_backward(c, net, x, dy, masks, training, rnd):
    """The stack's backward written out in float64 on the float64 forward, with the operands of the backward products
    passed through `rnd` where the header says the kernels round them to the row type: dz, the filters of the dX
    product, the activation the dW product reads, and the outputs Y and dX.  Everything else -- the forward, the
    statistics, the sums of g and g xhat, the bias sums -- stays float64.  With rnd = identity this is autograd's answer
    (the host test holds it to 1e-10).  [(name, tensor)] in run()'s order."""
    from torch.nn import grad as G
    f64 = torch.float64
    twin = _twin(net, f64, training)
    acts, layers, h = [x.double()], [], x.double()
    with torch.no_grad():
        for i, (conv, bn) in enumerate(twin):
            z = conv(h)
            if training:
                mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
            else:
                mean, var = bn.running_mean, bn.running_var
            inv = 1.0 / torch.sqrt(var + bn.eps)
            xh = (z - mean[None, :, None, None]) * inv[None, :, None, None]
            v = bn.weight[None, :, None, None] * xh + bn.bias[None, :, None, None]
            m = (v > 0).double()
            if training and masks[i] is not None:
                m = m * masks[i]
            h = v * m
            layers.append((xh, m, inv))
            acts.append(h)
        out = {"y": rnd(acts[-1])}
        dA = dy.double()
        for i in range(len(twin) - 1, -1, -1):
            conv, bn = twin[i]
            xh, m, inv = layers[i]
            g = dA * m
            dbe, dga = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
            n = float(g.numel() // g.shape[1])
            k1, k2 = (dbe / n, dga / n) if training else (torch.zeros_like(dbe), torch.zeros_like(dga))
            dz = (bn.weight * inv)[None, :, None, None] * (g - k1[None, :, None, None] - xh * k2[None, :, None, None])
            dzr = rnd(dz)
            geo = dict(stride=conv.stride, padding=conv.padding, dilation=conv.dilation)
            out["L%d.conv.weight" % i] = G.conv2d_weight(rnd(acts[i]), conv.weight.shape, dzr, **geo)
            if conv.bias is not None:
                out["L%d.conv.bias" % i] = dz.sum((0, 2, 3))
            out["L%d.bn.weight" % i], out["L%d.bn.bias" % i] = dga, dbe
            dA = G.conv2d_input(acts[i].shape, rnd(conv.weight), dzr, **geo)
        out["dx"] = rnd(dA)
    return out


def e16_of(c, p_ref, net, x, dy, masks, bias_scale, training, kind):
    """What the documented 16-bit operands alone cost on this input: rounded_backward with rounding to the row type
    against the float64 reference, |error| over each tensor's scale.  A property of the input and the number format."""
    dt = KINDS[kind]
    got = rounded_backward(c, net, x, dy, masks, training, lambda t: t.to(dt).double())
    out = {}
    for n, b in p_ref:
        if n in got:
            scale = scale_of(n, b, bias_scale, training)
            out[n] = float((got[n] - b).abs().max()) / scale
    return out


Problem = collections.namedtuple("Problem", "seed net x dy masks ref r32 bias_scale pre e32 e16")


def _draw(c, kind, seed):
    net = make_net(c, seed)
    g = torch.Generator().manual_seed(10000 + seed)
    ho, wo = shapes(c)[-1][3:]
    x = torch.randn(c.B, c.c0, c.H, c.W, generator=g).to(KINDS[kind])          # the rounded inputs both sides see
    dy = torch.randn(c.B, c.layers[-1].cout, ho, wo, generator=g).to(KINDS[kind])
    return net, x, dy


def e32_of(c, ref, r32, bias_scale, training):
    out = {}
    for (n, b), (_n, a) in zip(ref, r32):
        err, scale = wc.max_err(a, b)[0], scale_of(n, b, bias_scale, training)
        out[n] = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
    return out


@functools.lru_cache(maxsize=None)
def problem(i, kind, mode):
    """Case CASES[i] in row type `kind` and mode "train" / "eval" at its seed (module docstring): the fp32 modules
    holding the parameters as the call finds them, X and dY rounded to the row type, the masks, the float64 reference
    [(name, tensor)], torch's fp32 run of the same, the conv-bias scales, the float64 pre-ReLU values and e32 per
    tensor.  Computed once; nothing in it may be written."""
    c, training = CASES[i], mode == "train"
    masks = drop_masks(c)
    for seed in range(MAX_TRIES):
        net, x, dy = _draw(c, kind, seed)
        with torch.no_grad():
            pre = []
            forward(net, x.double(), masks, training, torch.float64, pre)
        margin, lo, hi = relu_state(pre)
        if margin < c.margin or lo < 0.05 or hi > 0.95:
            continue
        ref, bias_scale, pre = run(net, x, dy, masks, training, torch.float64)
        r32, _b, _p = run(net, x, dy, masks, training, torch.float32)
        e32 = e32_of(c, ref, r32, bias_scale, training)
        if max(e32.values()) > E32_MAX:
            continue
        e16 = {}
        if kind != "f32":
            e16 = e16_of(c, ref, net, x, dy, masks, bias_scale, training, kind)
            if max(e16.values()) > E16_SHARE * wc.TOL[KINDS[kind]]:
                continue
        return Problem(seed, net, x, dy, masks, ref, r32, bias_scale, pre, e32, e16)
    raise AssertionError("%s: no seed below %d gives a well-posed, conditioned problem" % (run_id(i, kind, mode), MAX_TRIES))


# --------------------------------------------------------------------------------------------- wfs_densify_rows
# (name, B, H, W, C, rows, kind, three rows on one cell, device-side row count)
DensifyCase = collections.namedtuple("DensifyCase", "name B H W C n kind triple counted")
DENSIFY_CASES = [
    DensifyCase("1x32-c1", 3, 1, 32, 1, 40, "f32", False, False),
    DensifyCase("32x1-c512", 2, 32, 1, 512, 30, "f16", False, False),
    DensifyCase("32x32-c3", 2, 32, 32, 3, 700, "f32", False, True),
    DensifyCase("32x32-c512-bf16", 1, 32, 32, 512, 90, "bf16", True, True),
    DensifyCase("triple-bf16", 2, 5, 4, 37, 25, "bf16", True, False),
]


def densify_problem(d):
    """(coords int32 [n_cap, 3] = (x, y, event), rows [n_cap, C], n_valid, want [B, H, W, C]).  `want` is the header's
    statement: the valid rows added cell by cell in row order in fp32, rounded once.  With a device-side count the rows
    behind it hold NaN and coordinates of live cells.  Without equal coordinates `want` is to_dense's answer, asserted
    here."""
    g = torch.Generator().manual_seed(len(d.name) + d.C)
    cells = torch.randperm(d.B * d.H * d.W, generator=g)[:d.n]
    if d.triple:                                   # rows 3 and the last land on row 0's cell: three rows on one cell
        cells[3] = cells[-1] = cells[0]
    sp = d.H * d.W
    coords = torch.stack([(cells % sp) // d.W, cells % d.W, cells // sp], 1).to(torch.int32)
    rows = torch.randn(d.n, d.C, generator=g).to(KINDS[d.kind])
    n_valid = d.n
    if d.counted:
        extra = 9
        coords = torch.cat([coords, coords[:extra]])
        rows = torch.cat([rows, torch.full((extra, d.C), float("nan")).to(rows.dtype)])
    want = torch.zeros(d.B, d.H, d.W, d.C, dtype=torch.float32)
    for r in range(n_valid):
        x, y, b = coords[r].tolist()
        want[b, x, y] += rows[r].float()
    want = want.to(rows.dtype)
    if not d.triple:
        idx = coords[:n_valid][:, [2, 0, 1]].long().t()
        dense = torch.sparse_coo_tensor(idx, rows[:n_valid].float(), size=[d.B, d.H, d.W, d.C]).to_dense().to(rows.dtype)
        assert torch.equal(dense, want)
    return coords, rows, n_valid, want
