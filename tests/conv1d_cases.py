"""Shared by tests/test_conv1d_cases_host.py and tests/test_gpu_conv1d_edges.py: the edge cases of the dense
Conv1d + BatchNorm1d + ReLU stack kernels (csrc/conv1d.hip: wfs_conv1d_fwd / wfs_conv1d_bwd), their inputs, the float64
reference and a plain-Python statement of the planning arm every case is there for.  (Not a test module: nothing here
is collected.)

Reference: the torch composition nn.Conv1d -> nn.BatchNorm1d -> nn.ReLU in float64 on the CPU, layer by layer, on the
X and dY the kernels see (rounded to the row type first), with the gradient kept at every conv output.  Parameters are
drawn as tests/test_gpu_convnet.py's _randomise draws them (taps of order 1 / sqrt(fan), conv bias ~ N(0, 0.5), BN
scale in [0.5, 1.5], shift ~ N(0, 0.3), running statistics away from (0, 1)).

The seed of a (case, row type, mode, rows that count) is the first of 0 .. MAX_TRIES - 1 at which, in float64,
  * no pre-ReLU value of a layer lies within seq_cases.RELU_MARGIN = 1e-5 of that layer's largest magnitude,
  * every layer has between 5 % and 95 % of its ReLUs on,
  * torch's own fp32 CPU run is within seq_cases.E32_MAX = 3e-6 of the float64 run on every compared tensor.
These are conditions on the inputs, proven on the CPU by the host test; no case has a margin of its own and nothing on
the GPU relaxes them.

Grid inputs (the cap cases, more than 131072 positions): X is drawn from the multiples of 1/16 in [-2, 2], exact in all
three row types, and every layer has fs = 1, st = 1.  Every activation at a position is then a function of that
position's c0 = 2 input values alone, at most 65^2 distinct values per channel, so the margin condition is a condition
on 4225 values and not on 135168 (with continuous inputs a value within 1e-5 of zero is expected about four times per
channel at this size, and no seed would pass).  dY stays continuous.

Two tensors are zero, or nearly, by algebra, and are held to the same bars against what they are summed from:
  * d conv.bias in front of a training-mode BatchNorm (exactly zero): scale max_c sum |dz|, as
    tests/test_gpu_convnet.py does;
  * d conv.weight of a layer with cin x fs = 1 in training mode: BatchNorm removes the scale of z = w x + b, so the
    exact gradient is of order eps / (var + eps) of its terms, and torch's own fp32 run misses it by 1e-3 .. 1 of its
    own magnitude.  Scale: max_c sum |dz a|.  ONLY layer 0 of case `c1` is such a layer (the host test asserts it).
In eval mode both are ordinary tensors.

Two rows (case `m2`): eps = 0.5, for the reason tests/dense_cases.py gives under "Two rows".

Rows that count: a case runs at capacity N; with a device-side count n_valid the rows that count are
min(max(n_valid, 0), N), the reference is the composition on those rows alone, and the GPU test fills the others with
NaN and 3e30.

The planning constants of csrc/conv1d.hip that decide an arm are copied below; arms_py restates wfs_conv1d_arms, and the
host test holds the two against each other.
"""
import collections
import functools

import torch
from torch import nn

import waveform_cases as wc
from seq_cases import E32_MAX, KINDS, RELU_MARGIN

MAX_TRIES = 40
TB, CH, ST_MAXBLK, DW_TP, DW_MAXBLK, EW_MAXBLK = 256, 8, 512, 32, 256, 2048
MAXC, MAXK, MAXS, MAXLY, MAXL = 64, 16, 8, 8, 4096
ST_CAP, EW_CAP, DW_CAP = ST_MAXBLK * TB, EW_MAXBLK * TB, DW_MAXBLK * DW_TP        # 131072, 524288, 8192
NBT0 = 41                                 # num_batches_tracked before the call

Layer = collections.namedtuple("Layer", "cout fs st pd bias mom eps")
# kinds: the row types the case runs in; modes: "train" / "eval"; grid: X from the multiples of 1/16; nbt0: the layers
# whose num_batches_tracked address is 0; nvalid: the device-side row counts the case runs with (None: NULL); arm: the
# tags (tags_of) the case is in the table for
Case = collections.namedtuple("Case", "name N L c0 layers kinds modes grid nbt0 nvalid arm why")

ALL = ("f32", "bf16", "f16")
F32 = ("f32",)
BOTH = ("train", "eval")


def Ly(cout, fs, st, pd, bias=True, mom=0.1, eps=1e-5):
    return Layer(cout, fs, st, pd, bias, mom, eps)


def _c(name, N, L, c0, layers, arm, why, kinds=F32, modes=("train",), grid=False, nbt0=(), nvalid=(None,)):
    layers = tuple(ly if isinstance(ly, Layer) else Ly(*ly) for ly in layers)
    return Case(name, N, L, c0, layers, kinds, modes, grid, tuple(nbt0), tuple(nvalid), set(arm), why)


DW8193 = [(3, 3, 1, 1), (2, 2, 1, 0)]
NV_PLAN = [(5, 3, 2, 1), (3, 4, 1, 2)]

CASES = [
    # --------------------------------------------------------------------------------------- position passes and caps
    _c("st-exact", 32, 4096, 2, [(2, 1, 1, 0)], {"pos=131072 exact", "L=4096", "fold nblk=512"},
       "131072 positions: 512 blocks, nothing strides; L = 4096", grid=True),
    _c("st-over", 33, 4096, 2, [(3, 1, 1, 0), (2, 1, 1, 0)],
       {"fwd strided", "head strided", "role A strided", "role A strided to dX", "fold nblk=512", "BN on load strided",
        "nv=6"},
       "135168 positions: forward of both layers, the head and role A of both layers stride; fold of 512 partials; "
       "BN on load under a stride", kinds=ALL, modes=BOTH, grid=True),
    _c("ew-exact", 64, 4096, 2, [(2, 1, 1, 0)], {"ew=2048 exact"}, "k_c1d_out at exactly 2048 blocks", grid=True),
    _c("ew-over", 65, 4096, 2, [(2, 1, 1, 0)], {"ew strided"}, "k_c1d_out strides", kinds=ALL, grid=True),
    _c("dw-8160", 3, 2720, 2, [(3, 3, 1, 1)], {"dw blocks=256, last idle"},
       "256 dW blocks, the last owns no tile and must write zeros"),
    _c("dw-8192", 2, 4096, 2, [(3, 3, 1, 1)], {"dw tiles=256 exact"}, "256 full tiles, one each"),
    _c("dw-8193", 3, 2731, 2, DW8193, {"dw second tile=1", "dw last tile=30", "dw tiles cross rows"},
       "layer 0: block 0's second tile holds one position; layer 1 (8190): last tile of 30; tiles cross row ends",
       kinds=ALL),
    # --------------------------------------------------------------------- dW columns, groups, CO, channel chunks
    _c("c1", 6, 40, 1, [(1, 1, 1, 0), (1, 3, 1, 1)], {"ncol=2", "groups=128", "nv=2", "single-tap weight"},
       "ncol = 2, 128 groups; fold nv = 2; single-tap weight rule"),
    _c("g3-85", 3, 20, 12, [(7, 7, 1, 3)], {"ncol=85", "groups=3", "idle=1", "cout=7"},
       "ncol = 85: 3 groups, one idle thread; cout 7"),
    _c("g2-86", 3, 20, 17, [(8, 5, 1, 2)], {"ncol=86", "groups=2", "cout=8", "cin=17"},
       "ncol = 86: 2 groups; cout 8 = CO edge; cin 17 = third CH chunk with one lane"),
    _c("g2-127", 3, 20, 9, [(9, 14, 1, 13)], {"ncol=127", "groups=2", "idle=2", "cout=9", "CO=16", "cin=9"},
       "ncol = 127: 2 groups, two idle threads; cout 9 -> CO = 16; cin 9", kinds=ALL),
    _c("g1-129", 3, 20, 16, [(17, 8, 1, 4)], {"ncol=129", "groups=1", "cout=17", "CO=32"},
       "ncol = 129: one group; cout 17 -> CO = 32", kinds=ALL),
    _c("one-256", 2, 20, 51, [(16, 5, 1, 2)], {"ncol=256", "chunks=1", "cout=16"},
       "ncol = 256: one full column chunk; cout 16"),
    _c("two-257", 2, 20, 64, [(33, 4, 1, 0)], {"ncol=257", "chunks=2", "last chunk=1", "groups=256", "CO=64", "CW passes=2",
                                                "nv=66", "cout=33"},
       "second chunk of one column (the bias column), 256 groups, CO = 64: two CW passes; fold nv = 66", kinds=ALL),
    _c("max-1025", 2, 4, 64, [(64, 16, 1, 15)], {"ncol=1025", "chunks=5", "cin chunks=8", "cout=64", "fs=16", "pd=fs-1",
                                                  "nv=128", "taps=8192"},
       "every bound: 5 column chunks, 8 channel chunks, both LDS tap images full (8192 floats), nv = 128",
       kinds=ALL, modes=BOTH),
    _c("co-32-64", 3, 20, 3, [(32, 3, 1, 1), (64, 2, 1, 0), (3, 1, 1, 0)],
       {"cout=32", "cout=64", "ncol=65", "groups=3", "CW passes=2", "cin=64", "nv=6"},
       "cout 32 edge; cout 64 at ncol = 65: 3 groups x two CW passes; cin 64 at fs = 1; nv = 6", kinds=ALL, modes=BOTH),
    # ------------------------------------------------------------------------------------------------------ geometry
    _c("st8-k16", 5, 59, 1, [(4, 16, 8, 0), (3, 6, 1, 0)], {"st=8", "fs=16", "pd=0", "unread samples", "lout=1"},
       "st = 8, fs = 16, pd = 0; samples 56 .. 58 unread (dX exactly 0); ends at L_out = 1, statistics over 5 values",
       kinds=ALL),
    _c("st-gt-fs", 3, 30, 2, [(3, 2, 5, 0)], {"st>fs", "unread samples"},
       "stride above the kernel: three of every five samples unread", kinds=ALL),
    _c("pd-max", 3, 4, 2, [(3, 16, 1, 15), (2, 16, 8, 15)], {"row shorter than kernel", "pd=fs-1", "st=8"},
       "row shorter than the kernel, pd = fs - 1, then st = 8", kinds=ALL, modes=BOTH),
    _c("L1", 7, 1, 3, [(5, 1, 1, 0), (2, 1, 1, 0)], {"L=1"}, "L = 1", kinds=ALL),
    _c("eight", 3, 200, 2, [(3, 3, 1, 1), (9, 2, 2, 0), (8, 5, 1, 4), (17, 1, 1, 0), (16, 4, 2, 3), (33, 3, 1, 1), (5, 2, 1, 1),
                           (4, 3, 3, 0)], {"layers=8", "CO=8", "CO=16", "CO=32", "CO=64"},
       "eight layers, both ping-pong halves, every CO, L_out 200 -> 18", kinds=ALL, modes=BOTH),
    _c("odd-16", 3, 5, 3, [(3, 3, 1, 1), (1, 2, 2, 0)], {"odd 16-bit rows"}, "odd 16-bit element counts", kinds=ALL),
    # ------------------------------------------------------------------------------ statistics, counts and records
    _c("m2", 2, 1, 3, [Ly(4, 1, 1, 0, eps=0.5)], {"M=2", "L=1"}, "the smallest training call: unbiased factor 2"),
    _c("nv", 9, 37, 2, NV_PLAN, {"n_valid NULL", "n_valid=N", "n_valid<N", "n_valid>N"},
       "n_valid on the device in {NULL, 9, 6, 12} at capacity 9", kinds=ALL, nvalid=(None, 9, 6, 12)),
    _c("nv-dw", 4, 2731, 2, DW8193, {"n_valid<N", "dw strided"},
       "dw-8193 at capacity 4 with n_valid = 3: whole tiles of padding rows add nothing", nvalid=(3,)),
    _c("bn-records", 3, 20, 2, [Ly(4, 3, 1, 1, bias=False, mom=0.0), Ly(5, 2, 1, 0, mom=0.1, eps=1e-3),
                               Ly(3, 3, 1, 1, mom=1.0, eps=0.1)],
       {"momentum 0", "momentum 1", "eps per layer", "nbt=0", "no conv bias"},
       "momentum 0 / 0.1 / 1 and eps 1e-5 / 1e-3 / 0.1, num_batches_tracked absent on the middle layer, no conv bias on "
       "the first", modes=BOTH, nbt0=(1,)),
    # the plan Conv1DNet builds for tests/test_gpu_convnet.py's `stride-3` (the host test holds it against conv1d_plan).
    # N = 150 and not 300: layer 0 has 146400 continuous pre-ReLU values at 300 rows, about four of them expected
    # within the margin, and none of the 40 seeds passes at 300 or 200 rows (150 rows: seed 21); the dW blocks still
    # stride (286 tiles on 256 blocks).
    _c("module", 150, 62, 2, [(8, 6, 1, 2), (6, 3, 2, 0), (5, 2, 3, 0)], {"module plan", "dw strided"},
       "`stride-3` of tests/test_gpu_convnet.py at N = 150, also run through Conv1DNet(fused=True)", kinds=("bf16",)),
]
MODULE_KW = dict(num_channels=2, out_size=5, num_expand=1, num_contract=2, expand_factor=4, size_factor=6, pad_factor=1,
                 stride_factor=3)
BY_NAME = {c.name: i for i, c in enumerate(CASES)}
assert len(BY_NAME) == len(CASES)

# every arm of the table; the host test holds the union of tags_of over the cases against it
REQUIRED = set().union(*[c.arm for c in CASES])


def rows_of(c, nv):
    """The rows that count of case `c` run with the device-side count `nv` (None: NULL)."""
    return c.N if nv is None else min(max(nv, 0), c.N)


def case_params():
    """(case index, kind, mode, n_valid) of every run of the table."""
    return [(i, kind, mode, nv) for i, c in enumerate(CASES) for kind in c.kinds for mode in c.modes for nv in c.nvalid]


def run_id(i, kind, mode, nv=None):
    return "%s-%s-%s%s" % (CASES[i].name, kind, mode, "" if nv is None else "-nv%d" % nv)


# ----------------------------------------------------------------------------------------------- plan arithmetic
def shapes(c):
    """Per layer (cin, lin, lout), the reference's size formula."""
    out, cin, lin = [], c.c0, c.L
    for ly in c.layers:
        lout = (lin + 2 * ly.pd - ly.fs) // ly.st + 1
        out.append((cin, lin, lout))
        cin, lin = ly.cout, lout
    return out


def plan_arrays(c):
    """(channels, fs, st, pd) as the entry points take them."""
    return tuple([getattr(ly, f) for ly in c.layers] for f in ("cout", "fs", "st", "pd"))


def _pos_blocks(P):
    return max(1, min(ST_MAXBLK, (P + TB - 1) // TB))


def arms_py(c):
    """wfs_conv1d_arms in plain Python: per layer [L_in, L_out, position blocks over N L_out, position blocks of role A
    over N L_in, input-channel chunks, dW blocks, column chunks, columns of the last chunk, its thread groups, CO], then
    [blocks of k_c1d_out]."""
    out = []
    for ly, (cin, lin, lout) in zip(c.layers, shapes(c)):
        ncol = cin * ly.fs + 1
        chunks = (ncol + TB - 1) // TB
        mycols = min(TB, ncol - (chunks - 1) * TB)
        groups = TB // mycols if mycols <= TB // 2 else 1
        co = 8 if ly.cout <= 8 else 16 if ly.cout <= 16 else 32 if ly.cout <= 32 else 64
        out.append([lin, lout, _pos_blocks(c.N * lout), _pos_blocks(c.N * lin), (cin + CH - 1) // CH,
                    min(DW_MAXBLK, c.N * lout // DW_TP + 1), chunks, mycols, groups, co])
    total = c.N * c.layers[-1].cout * shapes(c)[-1][2]
    out.append([min(EW_MAXBLK, (total + TB - 1) // TB)])
    return out


def tags_of(c, arms):
    """The arms of the issue's list that the case reaches, from `arms` (wfs_conv1d_arms' answer, or arms_py) and plain
    arithmetic on the plan.  Only tags of REQUIRED are reported."""
    t = set()
    sh = shapes(c)
    n = len(c.layers)
    for i, (ly, (cin, lin, lout), a) in enumerate(zip(c.layers, sh, arms)):
        _lin, _lout, pb, pa, nchunk, dwb, chunks, mycols, groups, co = a
        P, Pin, ncol = c.N * lout, c.N * lin, cin * ly.fs + 1
        tiles = (P + DW_TP - 1) // DW_TP
        t |= {"pos=131072 exact"} if (pb == ST_MAXBLK and P == ST_CAP) else set()
        t |= {"fold nblk=512"} if pb == ST_MAXBLK else set()
        t |= {"fwd strided"} if (pb == ST_MAXBLK and P > ST_CAP) else set()
        t |= {"head strided"} if (i == n - 1 and pb == ST_MAXBLK and P > ST_CAP) else set()
        t |= {"role A strided"} if (i > 0 and pa == ST_MAXBLK and Pin > ST_CAP) else set()
        t |= {"role A strided to dX"} if (i == 0 and pa == ST_MAXBLK and Pin > ST_CAP) else set()
        t |= {"BN on load strided"} if (i > 0 and pb == ST_MAXBLK and P > ST_CAP) else set()
        t |= {"dw blocks=256, last idle"} if (dwb == DW_MAXBLK and tiles == DW_MAXBLK - 1) else set()
        t |= {"dw tiles=256 exact"} if (dwb == DW_MAXBLK and P == DW_CAP) else set()
        t |= {"dw second tile=1"} if (dwb == DW_MAXBLK and P == DW_CAP + 1) else set()
        t |= {"dw last tile=30"} if (dwb == DW_MAXBLK and tiles == DW_MAXBLK and P % DW_TP == 30) else set()
        t |= {"dw strided"} if (dwb == DW_MAXBLK and tiles > DW_MAXBLK + 1) else set()
        t |= {"dw tiles cross rows"} if (c.N > 1 and lout % DW_TP and P > DW_TP) else set()
        t |= {"ncol=%d" % ncol, "groups=%d" % groups, "chunks=%d" % chunks, "last chunk=%d" % mycols, "CO=%d" % co,
              "cout=%d" % ly.cout, "cin=%d" % cin, "cin chunks=%d" % nchunk, "nv=%d" % (2 * ly.cout),
              "fs=%d" % ly.fs, "st=%d" % ly.st, "L=%d" % lin, "lout=%d" % lout}
        t |= {"idle=%d" % (TB - groups * mycols)} if chunks == 1 else set()
        t |= {"CW passes=2"} if (co == 64 and groups > 1) else set()
        t |= {"taps=8192"} if (CH * cin * ly.fs == 8192 and ly.cout * CH * ly.fs == 8192) else set()
        t |= {"single-tap weight"} if (cin * ly.fs == 1 and "train" in c.modes) else set()
        t |= {"pd=0"} if (ly.pd == 0 and ly.fs > 1) else set()
        t |= {"pd=fs-1"} if (ly.pd == ly.fs - 1 and ly.fs > 1) else set()
        t |= {"row shorter than kernel"} if lin < ly.fs else set()
        t |= {"st>fs"} if ly.st > ly.fs else set()
        t |= {"unread samples"} if (i == 0 and ly.pd == 0 and (lout - 1) * ly.st + ly.fs < lin) else set()
        t |= {"M=2"} if P == 2 else set()
        t |= {"momentum 0"} if ly.mom == 0 else set()
        t |= {"momentum 1"} if ly.mom == 1 else set()
    total = c.N * c.layers[-1].cout * sh[-1][2]
    t |= {"ew=2048 exact"} if (arms[n][0] == EW_MAXBLK and total == EW_CAP) else set()
    t |= {"ew strided"} if (arms[n][0] == EW_MAXBLK and total > EW_CAP) else set()
    t |= {"layers=%d" % n}
    t |= {"odd 16-bit rows"} if ((c.N * c.c0 * c.L) % 2 and "bf16" in c.kinds and "f16" in c.kinds) else set()
    t |= {"eps per layer"} if len({ly.eps for ly in c.layers}) == n > 1 else set()
    t |= {"nbt=0"} if c.nbt0 else set()
    t |= {"no conv bias"} if 0 < sum(not ly.bias for ly in c.layers) < n else set()
    for nv in c.nvalid:
        t |= {"n_valid NULL"} if nv is None else {"n_valid=N"} if nv == c.N else {"n_valid<N"} if nv < c.N else {"n_valid>N"}
    t |= {"module plan"} if c.name == "module" else set()
    return t & REQUIRED


# ------------------------------------------------------------------------------- problems and float64 references
def make_net(c, seed):
    """[(nn.Conv1d, nn.BatchNorm1d)] per layer in fp32 with live parameters, drawn as tests/test_gpu_convnet.py's
    _randomise draws them; num_batches_tracked = NBT0."""
    g = torch.Generator().manual_seed(seed)
    net, cin = [], c.c0
    with torch.no_grad():
        for ly in c.layers:
            conv = nn.Conv1d(cin, ly.cout, ly.fs, stride=ly.st, padding=ly.pd, bias=ly.bias)
            bn = nn.BatchNorm1d(ly.cout, eps=ly.eps, momentum=ly.mom)
            fan = cin * ly.fs
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / fan ** 0.5)
            if ly.bias:
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.5)
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.3)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.2)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
            bn.num_batches_tracked.fill_(NBT0)
            net.append((conv, bn))
            cin = ly.cout
    return net


def twin(net, dtype, training):
    """A copy of `net` in `dtype` and the given mode."""
    out = []
    for conv, bn in net:
        c2 = nn.Conv1d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                       bias=conv.bias is not None).to(dtype)
        b2 = nn.BatchNorm1d(bn.num_features, eps=bn.eps, momentum=bn.momentum).to(dtype)
        c2.load_state_dict({k: v.to(dtype) for k, v in conv.state_dict().items()})
        b2.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in bn.state_dict().items()})
        out.append((c2.train(training), b2.train(training)))
    return out


def forward(net, x, training, dtype):
    """The composition layer by layer on a twin of `net` in `dtype`: (y, [conv outputs], [each layer's input],
    [pre-ReLU values], twin)."""
    tw = twin(net, dtype, training)
    h, zs, ins, pre = x, [], [], []
    for conv, bn in tw:
        ins.append(h)
        z = conv(h)
        if z.requires_grad:
            z.retain_grad()
        zs.append(z)
        v = bn(z)
        pre.append(v.detach())
        h = torch.relu(v)
    return h, zs, ins, pre, tw


def run(net, x, dy, training, dtype):
    """Forward and backward in `dtype`: ([(name, tensor)], {name: scale of a tensor that is zero by algebra}, pre-ReLU
    values).  Names: y, dx, then per layer L<i>.conv.weight, .conv.bias (where present), .bn.weight, .bn.bias
    (gradients), .running_mean, .running_var (after the call)."""
    xr = x.detach().to(dtype).requires_grad_(True)
    y, zs, ins, pre, tw = forward(net, xr, training, dtype)
    y.backward(dy.to(dtype))
    out, summed = [("y", y.detach()), ("dx", xr.grad)], {}
    for i, ((conv, bn), z, a) in enumerate(zip(tw, zs, ins)):
        out.append(("L%d.conv.weight" % i, conv.weight.grad))
        if conv.in_channels * conv.kernel_size[0] == 1:
            # one tap of one channel (pd = 0): the sample position t reads is t st
            read = a.detach()[:, :, ::conv.stride[0]][:, :, :z.shape[2]]
            summed["L%d.conv.weight" % i] = float((z.grad * read).abs().sum((0, 2)).max())
        if conv.bias is not None:
            out.append(("L%d.conv.bias" % i, conv.bias.grad))
            summed["L%d.conv.bias" % i] = float(z.grad.abs().sum((0, 2)).max())
        out += [("L%d.bn.weight" % i, bn.weight.grad), ("L%d.bn.bias" % i, bn.bias.grad),
                ("L%d.running_mean" % i, bn.running_mean.detach().clone()), ("L%d.running_var" % i, bn.running_var.detach().clone())]
        assert int(bn.num_batches_tracked) == NBT0 + int(training)
    return out, summed, pre


def scale_of(name, ref_tensor, summed, training):
    """What a tensor's error is taken against: its largest float64 magnitude -- for the two tensors a training-mode
    BatchNorm makes zero by algebra (module docstring), what they are summed from."""
    if training and name in summed:
        return summed[name]
    return float(ref_tensor.abs().max())


def relu_state(pre):
    """(smallest min|v| / max|v| over the layers, smallest and largest share of ReLUs on)."""
    margin = min(float(v.abs().min()) / float(v.abs().max()) for v in pre)
    on = [float((v > 0).double().mean()) for v in pre]
    return margin, min(on), max(on)


Problem = collections.namedtuple("Problem", "seed rows net x dy ref r32 summed pre e32")


def _draw(c, kind, seed, rows):
    net = make_net(c, seed)
    g = torch.Generator().manual_seed(10000 + seed)
    if c.grid:
        x = torch.randint(-32, 33, (rows, c.c0, c.L), generator=g).double() / 16.0
    else:
        x = torch.randn(rows, c.c0, c.L, generator=g)
    x = x.to(KINDS[kind])                                                   # the rounded inputs both sides see
    dy = torch.randn(rows, c.layers[-1].cout, shapes(c)[-1][2], generator=g).to(KINDS[kind])
    return net, x, dy


def e32_of(ref, r32, summed, training):
    out = {}
    for (n, b), (_n, a) in zip(ref, r32):
        err, scale = wc.max_err(a, b)[0], scale_of(n, b, summed, training)
        out[n] = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
    return out


@functools.lru_cache(maxsize=None)
def problem(i, kind, mode, rows=None):
    """Case CASES[i] in row type `kind` and mode "train" / "eval" on `rows` rows (None: the case's N) at its seed (module
    docstring): the fp32 modules holding the parameters as the call finds them, X and dY rounded to the row type, the
    float64 reference [(name, tensor)], torch's fp32 run of the same, the scales of the tensors that are zero by
    algebra, the float64 pre-ReLU values and e32 per tensor.  Computed once; nothing in it may be written."""
    c, training = CASES[i], mode == "train"
    rows = c.N if rows is None else rows
    for seed in range(MAX_TRIES):
        net, x, dy = _draw(c, kind, seed, rows)
        with torch.no_grad():
            pre = forward(net, x.double(), training, torch.float64)[3]
        margin, lo, hi = relu_state(pre)
        if margin < RELU_MARGIN or lo < 0.05 or hi > 0.95:
            continue
        ref, summed, pre = run(net, x, dy, training, torch.float64)
        r32, _s, _p = run(net, x, dy, training, torch.float32)
        e32 = e32_of(ref, r32, summed, training)
        if max(e32.values()) > E32_MAX:
            continue
        return Problem(seed, rows, net, x, dy, ref, r32, summed, pre, e32)
    raise AssertionError("%s on %d rows: no seed below %d gives a well-posed, conditioned problem"
                         % (run_id(i, kind, mode), rows, MAX_TRIES))
