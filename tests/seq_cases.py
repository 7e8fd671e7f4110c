"""Shared by tests/test_seq_cases_host.py, tests/test_gpu_seq_edges.py, tests/test_gpu_waveform.py and
tests/test_gpu_recurrent.py: the live-parameter recipe of the multi-channel TCN, the dropout references of the two
waveform front ends (csrc/tcnc.hip, csrc/rnn.hip), the edge cases of their row kernels, a plain-Python statement of the
dispatch arm every case is there for, and the float64 references.  (Not a test module: nothing here is collected.)

The arm statements restate the dispatch arithmetic of the two sources (their constants are copied below); the host test
holds them against the table and against the list of arms no other test reaches.  Inputs of a case are fixed by its
seed (one per row dtype where no seed serves all three): the first seed from 0 on the CPU at which every tensor is
live, torch's own fp32 run stays within 2e-6 of float64 and no ReLU pre-activation other than an exact zero lies within
2e-5 of its layer's largest -- the bounds the host test asserts are 3e-6 and 1e-5.  (A ReLU that close to zero may fall
on the other side in fp32, which is a property of the input, not of a kernel; see relu_margin for the exact zeros.)
"""
import collections
import functools

import numpy as np
import torch

import waveform_cases as wc
from recurrent_cases import case_id, make_inputs, make_rnn, run_torch

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DROP_P = 0.3
DROP_SEED = 0x2545F4914F6CDD1D        # the int64 the GPU test puts in device memory; the masks below are rebuilt from it
E32_MAX = 3e-6                        # torch's fp32 CPU run against float64, every tensor (tests/test_bn_cases_host.py)
RELU_MARGIN = 1e-5                    # smallest |pre-activation| of a ReLU over its layer's largest


# ------------------------------------------------------------------------------------------------------------ TCN
def make_tcn(c0, channels, k, dropout=0.0, seed=0):
    """TemporalConvNet(fused=True) in fp32 on the CPU with live parameters, and its float64 twin."""
    from waveformml_amd.psd.tcn import TemporalConvNet
    torch.manual_seed(seed)
    net = TemporalConvNet(c0, channels, kernel_size=k, dropout=dropout, fused=True)
    with torch.no_grad():
        for name, p in net.named_parameters():  # N(0, 0.01) taps would leave the net almost linear
            p.copy_(torch.randn_like(p) * 0.5)
            if name.endswith(("bias", "weight_g", "downsample.weight")):
                p.abs_().add_(0.1)              # ... and a narrow level can die (all ReLUs off): keep the residuals live
    return net, tcn_twin(net, torch.float64)


def tcn_twin(net, dtype):
    """The torch composition (fused off) holding net's parameters in `dtype`."""
    from waveformml_amd.psd.tcn import TemporalConvNet
    ref = TemporalConvNet(net.num_inputs, net.channels, kernel_size=net.kernel_size, dropout=net.dropout).to(dtype)
    ref.load_state_dict({k_: v.to(dtype) for k_, v in net.state_dict().items()})
    return ref


def tcn_hash_masks(seed, p, N, C, L, conv):
    """The kernels' dropout multipliers of conv `conv` (= 2 level + {0, 1}), [N, C, L] in float64, computed here from the
    documented scheme (csrc/tcnc.hip drop_mult: splitmix64 finaliser over seed + counter * golden ratio, counter =
    (((row << 4 | conv) << 5 | channel) << 12) | t; dropped when the high 32 bits are below p 2^32, else 1 / (1 - p) in
    fp32)."""
    row = np.arange(N, dtype=np.uint64)[:, None, None]
    ch = np.arange(C, dtype=np.uint64)[None, :, None]
    t = np.arange(L, dtype=np.uint64)[None, None, :]
    return wc.hash_masks(seed, p, ((((row << np.uint64(4)) | np.uint64(conv)) << np.uint64(5) | ch) << np.uint64(12)) | t)


def tcn_masked_reference(ref, x, masks, pre=None):
    """The torch composition with the given dropout multipliers in place of nn.Dropout (None: no mask), in ref's dtype.
    `pre` (a list) receives (level, name, pre-activation) of every ReLU."""
    h = x
    for lv, blk in enumerate(ref.network):
        L = h.shape[2]
        c1, c2 = blk.convs
        z1 = c1(h)[:, :, :L]
        h1 = torch.relu(z1)
        if masks[2 * lv] is not None:
            h1 = h1 * masks[2 * lv].to(h1.dtype)
        z2 = c2(h1)[:, :, :L]
        h2 = torch.relu(z2)
        if masks[2 * lv + 1] is not None:
            h2 = h2 * masks[2 * lv + 1].to(h2.dtype)
        res = h if blk.downsample is None else blk.downsample(h)
        if pre is not None:
            pre += [(lv, "conv1", z1.detach()), (lv, "conv2", z2.detach()), (lv, "out", (h2 + res).detach())]
        h = torch.relu(h2 + res)
    return h


# ------------------------------------------------------------------------------------------------------------ RNN
def rnn_hash_masks(seed, p, N, C, T, layer):
    """The kernels' dropout multipliers of layer `layer`'s outputs, [N, T, C] in float64, from the documented scheme
    (include/wfsparse.h, recurrent front end): splitmix64 finaliser over seed + counter * golden ratio, counter =
    (((row << 3 | layer) << 6 | channel) << 12) | t; dropped when the high 32 bits are below p 2^32, else 1 / (1 - p) in
    fp32."""
    row = np.arange(N, dtype=np.uint64)[:, None, None]
    t = np.arange(T, dtype=np.uint64)[None, :, None]
    ch = np.arange(C, dtype=np.uint64)[None, None, :]
    return wc.hash_masks(seed, p, ((((row << np.uint64(3)) | np.uint64(layer)) << np.uint64(6) | ch) << np.uint64(12)) | t)


def elman(rnn, x, masks, dtype=torch.float64, pre=None, hidden=None):
    """The Elman recurrence written out (autograd, `dtype`) on rnn's parameters, `masks[l]` multiplying layer l's
    outputs (None: no mask).  Returns (y, leaf parameters in named_parameters order).  `pre` (a list) receives
    (layer, direction, pre-activations [N, T, H]); `hidden` (a list) the last state [N, H] of every chain, in nn.RNN's
    order."""
    params = {n: p.detach().to(dtype).requires_grad_(True) for n, p in rnn.named_parameters()}
    act = torch.relu if rnn.nonlinearity == "relu" else torch.tanh
    N, T, _ = x.shape
    inp = x
    for l in range(rnn.num_layers):
        outs = []
        for d, sfx in enumerate(("", "_reverse") if rnn.bidirectional else ("",)):
            wi, wh = params["weight_ih_l%d%s" % (l, sfx)], params["weight_hh_l%d%s" % (l, sfx)]
            b = (params["bias_ih_l%d%s" % (l, sfx)] + params["bias_hh_l%d%s" % (l, sfx)]) if rnn.bias else 0
            pre_in = inp @ wi.t() + b
            h = torch.zeros(N, rnn.hidden_size, dtype=dtype)
            hs, zs = [None] * T, [None] * T
            for t in (range(T - 1, -1, -1) if d else range(T)):
                zs[t] = pre_in[:, t] + h @ wh.t()
                h = act(zs[t])
                hs[t] = h
            outs.append(torch.stack(hs, 1))
            if pre is not None:
                pre.append((l, d, torch.stack(zs, 1).detach()))
            if hidden is not None:
                hidden.append(h.detach())
        inp = torch.cat(outs, 2)
        if masks[l] is not None:
            inp = inp * masks[l].to(dtype)
    return inp, [params[n] for n, _ in rnn.named_parameters()]


# ------------------------------------------------------------------------------------------------- the case tables
# constants of csrc/rnn.hip and csrc/tcnc.hip that decide an arm
RNN_MAXI, RNN_MAXH, RNN_MAXLY, RNN_MAXT = 32, 32, 8, 4096
SCAN_TB, MIX_TB, MIX_CH, TT, DW_TB = 64, 256, 8, 32, 256
TCN_MAXC, TCN_MAXK, TCN_MAXLV, TCN_MAXL, TCN_TB, TCN_CH = 32, 8, 8, 4096, 256, 8

# case = (T, I, H, layers, directions, nonlinearity, bias); dropout: DROP_P between the layers; dx: x requires grad;
# zero: the gradients that are identically zero; arms: what rnn_arms must say
RnnCase = collections.namedtuple("RnnCase", "case N seed dropout dx zero arms why")
# case = (c0, channels, k, L); arms: per convolution (ncol, groups, slot 1 live, CO, live channels of the last chunk)
TcnCase = collections.namedtuple("TcnCase", "case N seed dropout arms why")


def _r(case, N, seed, arms, why, dropout=False, dx=True, zero=()):
    return RnnCase(case, N, seed, dropout, dx, zero, arms, why)


def _arms(HP, matvec, CO, ncol, groups, scan, mix, tiles):
    return dict(HP=HP, matvec=matvec, CO=CO, ncol=ncol, groups=groups, scan_blocks=scan, mix_blocks=mix, tiles_n=tiles)


RNN_CASES = [
    _r((1, 1, 4, 2, 2, "relu", True), 3, 0, _arms(4, "registers", 8, [6, 13], [42, 19], 1, 1, 1),
       "T = 1: dW_hh is identically zero", zero=("weight_hh",)),
    _r((2, 2, 1, 2, 1, "tanh", True), 5, 0, _arms(4, "registers", 8, [4, 3], [64, 85], 1, 1, 1), "H = 1, T = 2"),
    _r((33, 1, 8, 2, 2, "relu", False), 64, (20, 345, 11), _arms(8, "registers", 8, [10, 25], [25, 10], 1, 1, 2),
       "top of HP = 8, N = Npad, no bias with two directions"),
    _r((33, 1, 9, 2, 1, "relu", True), 65, 20, _arms(16, "parked", 16, [11, 19], [23, 13], 2, 1, 3),
       "bottom of HP = 16, parked matvec, a second scan block with one live lane"),
    _r((17, 5, 16, 2, 2, "tanh", True), 63, 0, _arms(16, "parked", 16, [22, 49], [11, 5], 1, 1, 2),
       "top of HP = 16, I = 5 with a Q tail in the transposed mix"),
    _r((17, 1, 17, 2, 1, "relu", True), 33, 6, _arms(32, "parked", 32, [19, 35], [13, 7], 1, 1, 2),
       "bottom of HP = 32, k_rnn_dw<32>, N one past a transpose tile"),
    _r((9, 32, 32, 2, 2, "tanh", True), 257, 0, _arms(32, "parked", 32, [65, 97], [3, 2], 5, 2, 9),
       "I = MAXI, C = MAXC, ncol = 97, N one past MIX_TB"),
    _r((5, 32, 32, 1, 2, "relu", False), 31, 1, _arms(32, "parked", 32, [65], [3], 1, 1, 1), "single layer at full width"),
    _r((12, 3, 5, 8, 2, "relu", True), 40, 3, _arms(8, "registers", 8, [9] + [16] * 7, [28] + [16] * 7, 1, 1, 2),
       "deepest stack, two directions"),
    _r((4096, 1, 4, 2, 1, "tanh", True), 2, 2, _arms(4, "registers", 8, [6, 9], [42, 28], 1, 1, 1), "T = MAX_T"),
    # outside the table of shapes: the no-dX route and the dropout counter's field edges
    _r((33, 1, 9, 2, 1, "relu", True), 65, 20, _arms(16, "parked", 16, [11, 19], [23, 13], 2, 1, 3),
       "the twin without dX: every parameter gradient bit-identical", dx=False),
    _r((4096, 1, 4, 2, 1, "tanh", True), 2, 0, _arms(4, "registers", 8, [6, 9], [42, 28], 1, 1, 1),
       "dropout at t = 4095", dropout=True),
    _r((6, 2, 32, 8, 2, "tanh", True), 3, 0, _arms(32, "parked", 32, [35] + [97] * 7, [7] + [2] * 7, 1, 1, 1),
       "dropout at layer = 6, channel = 63", dropout=True),
]

TCN_CASES = [
    TcnCase((1, [32, 32], 8, 40), 3, 4, False,
            [(9, 28, False, 32, 0), (257, 1, True, 32, 0), (2, 128, False, 32, 0), (257, 1, True, 32, 0), (257, 1, True, 32, 0)],
            "ncol = 257, slot r = 1, LDS full"),
    TcnCase((32, [32], 8, 33), 2, 1, False, [(257, 1, True, 32, 0), (257, 1, True, 32, 0)],
            "c0 = MAXC, identity residual in the row dtype"),
    TcnCase((1, [16, 16], 8, 64), 1, 0, False,
            [(9, 28, False, 16, 0), (129, 1, False, 16, 0), (2, 128, False, 16, 0), (129, 1, False, 16, 0), (129, 1, False, 16, 0)],
            "ncol = 129, groups == 1 at its lower edge"),
    TcnCase((1, [24, 24], 5, 31), 3, 0, False,
            [(6, 42, False, 32, 0), (121, 2, False, 32, 0), (2, 128, False, 32, 0), (121, 2, False, 32, 0), (121, 2, False, 32, 0)],
            "ncol = 121, groups = 2; N L = 93, tile tail"),
    TcnCase((5, [9, 17, 16, 8], 3, 31), 9, 11, False,
            [(16, 16, False, 16, 1), (28, 9, False, 16, 1), (6, 42, False, 16, 1),
             (28, 9, False, 32, 1), (52, 4, False, 32, 1), (10, 25, False, 32, 1),
             (52, 4, False, 16, 0), (49, 5, False, 16, 0), (18, 14, False, 16, 0),
             (49, 5, False, 8, 0), (25, 10, False, 8, 0), (17, 15, False, 8, 0)],
            "CO edges, one-channel chunk tails, downsample over several 16-bit channels"),
    TcnCase((2, [4] * 8, 2, 20), 3, 0, False,
            [(5, 51, False, 8, 4), (9, 28, False, 8, 4), (3, 85, False, 8, 4)] + [(9, 28, False, 8, 4)] * 14,
            "8 levels, dilation > L"),
    TcnCase((3, [5], 2, 1), 4, 0, False, [(7, 36, False, 8, 5), (11, 23, False, 8, 5), (4, 64, False, 8, 5)],
            "L = 1: the gradient of every tap but the last is identically zero"),
    TcnCase((4, [4, 4], 3, 7), 5, 0, False, [(13, 19, False, 8, 4)] * 4, "c0 == cout, no downsample anywhere"),
    TcnCase((1, [4], 2, 4096), 2, (34, 126, 34), False, [(3, 85, False, 8, 4), (9, 28, False, 8, 4), (2, 128, False, 8, 4)], "L = MAX_L"),
    # the dropout counter's field edges
    TcnCase((2, [32] * 8, 2, 64), 2, 777, True,
            [(5, 51, False, 32, 0), (65, 3, False, 32, 0), (3, 85, False, 32, 0)] + [(65, 3, False, 32, 0)] * 14,
            "dropout at conv = 15, channel = 31"),
    TcnCase((1, [4], 2, 4096), 2, 151, True, [(3, 85, False, 8, 4), (9, 28, False, 8, 4), (2, 128, False, 8, 4)],
            "dropout at t = 4095"),
]


def rnn_id(c):
    return "%s-N%d%s%s" % (case_id(c.case), c.N, "-drop" if c.dropout else "", "" if c.dx else "-nodx")


def tcn_id(c):
    c0, channels, k, L = c.case
    return "%s-N%d%s" % ("-".join(map(str, [c0] + list(channels) + [k, L])), c.N, "-drop" if c.dropout else "")


def seed_of(c, kind):
    """The seed of the case's parameters and inputs in row dtype `kind`: one for all three, or one each."""
    return c.seed if isinstance(c.seed, int) else c.seed[list(KINDS).index(kind)]


def kinds_of(c):
    """Row dtypes of a case: all three, fp32 alone for the dropout cases."""
    return ("f32",) if c.dropout else tuple(KINDS)


# ------------------------------------------------------------------------------------------- the arms, in plain Python
def rnn_arms(case, N):
    """What csrc/rnn.hip does with the case: the scan's padded width HP and the form of its matvec, the dW kernel's CO,
    per layer the dW tile's columns and thread groups, and the blocks along the rows of the scan, the mix and the
    output transpose."""
    _T, I, H, layers, dirs, _nl, _b = case
    HP = 4 if H <= 4 else 8 if H <= 8 else 16 if H <= 16 else 32
    ncol = [(I if l == 0 else dirs * H) + H + 1 for l in range(layers)]
    Npad = (N + SCAN_TB - 1) // SCAN_TB * SCAN_TB
    return _arms(HP, "registers" if HP <= 8 else "parked", 8 if H <= 8 else 16 if H <= 16 else 32, ncol,
                 [DW_TB // c for c in ncol], Npad // SCAN_TB, (N + MIX_TB - 1) // MIX_TB, (N + TT - 1) // TT)


def rnn_tags(c):
    """The untested arms (the module docstring of tests/test_seq_cases_host.py lists them) that the case reaches."""
    T, I, H, layers, dirs, _nl, bias = c.case
    a = rnn_arms(c.case, c.N)
    tags = {"HP=%d" % a["HP"], "matvec=" + a["matvec"], "CO=%d" % a["CO"]}
    tags |= {"H=%d" % H} & {"H=1", "H=9", "H=17"}
    tags |= {"T=%d" % T} & {"T=1", "T=2", "T=%d" % RNN_MAXT}
    tags |= {"top of HP=%d" % a["HP"]} if H == a["HP"] and H > 4 else set()      # (H = 4 is the committed config)
    tags |= {"C=MAXC"} if dirs * H == 2 * RNN_MAXH else set()
    tags |= {"ncol=97"} if 97 in a["ncol"] else set()
    tags |= {"I=MAXI"} if I == RNN_MAXI else set()
    tags |= {"Q tail"} if I > 1 and I % MIX_CH else set()
    tags |= {"scan blocks > 1"} if a["scan_blocks"] > 1 else set()
    tags |= {"one live lane in the last scan block"} if c.N % SCAN_TB == 1 else set()
    tags |= {"N=Npad"} if c.N % SCAN_TB == 0 else set()
    tags |= {"mix blocks > 1"} if a["mix_blocks"] > 1 else set()
    tags |= {"transpose tiles > 1"} if a["tiles_n"] > 1 else set()
    tags |= {"two directions without bias"} if dirs == 2 and not bias else set()
    tags |= {"layers=MAXLY"} if layers == RNN_MAXLY else set()
    tags |= {"single layer"} if layers == 1 else set()
    tags |= {"no dX"} if not c.dx else set()
    if c.dropout:
        tags |= {"drop layer=6"} if layers - 2 == 6 else set()
        tags |= {"drop channel=63"} if dirs * H == 64 else set()
        tags |= {"drop t=4095"} if T == 4096 else set()
    return tags


RNN_REQUIRED = {"HP=4", "HP=8", "HP=16", "HP=32", "matvec=registers", "matvec=parked", "CO=8", "CO=16", "CO=32",
                "H=1", "H=9", "H=17", "T=1", "T=2", "T=4096", "top of HP=8", "top of HP=16", "top of HP=32", "C=MAXC",
                "ncol=97", "I=MAXI", "Q tail", "scan blocks > 1", "one live lane in the last scan block", "N=Npad",
                "mix blocks > 1", "transpose tiles > 1", "two directions without bias", "layers=MAXLY", "single layer",
                "no dX", "drop layer=6", "drop channel=63", "drop t=4095"}


def tcn_convs(case):
    """The convolutions of the plan in the kernels' order (per level conv1, conv2, the downsample when cin != cout):
    (level, cin, cout, taps, dilation)."""
    c0, channels, k, _L = case
    out = []
    for lv, cout in enumerate(channels):
        cin = c0 if lv == 0 else channels[lv - 1]
        out += [(lv, cin, cout, k, 1 << lv), (lv, cout, cout, k, 1 << lv)]
        if cin != cout:
            out.append((lv, cin, cout, 1, 0))
    return out


def tcn_arms(case):
    """What k_tcnc_dw does with every convolution of the plan: the tile's columns, its thread groups, whether the second
    column slot carries a live column, CO (chosen by the level's cout), and the live channels of the last 8-channel
    chunk of the conv passes (0: the chunk is full)."""
    out = []
    for _lv, cin, cout, kk, _d in tcn_convs(case):
        ncol = cin * kk + 1
        out.append((ncol, TCN_TB // ncol if ncol <= TCN_TB // 2 else 1, ncol > TCN_TB,
                    8 if cout <= 8 else 16 if cout <= 16 else 32, cout % TCN_CH))
    return out


def tcn_tags(c):
    c0, channels, k, L = c.case
    arms = tcn_arms(c.case)
    tags = set()
    tags |= {"slot r=1", "LDS full"} if any(a[2] for a in arms) else set()
    tags |= {"ncol=129"} if any(a[0] == 129 for a in arms) else set()
    tags |= {"groups=2"} if any(a[1] == 2 for a in arms) else set()
    tags |= {"tile tail"} if (c.N * L) % 32 else set()
    tags |= {"first level cin > 1"} if c0 > 1 else set()
    tags |= {"identity residual in the row dtype"} if c0 == channels[0] else set()
    tags |= {"downsample over rin > 1"} if c0 > 1 and c0 != channels[0] else set()
    tags |= {"c0=MAXC"} if c0 == TCN_MAXC else set()
    tags |= {"levels=8"} if len(channels) == TCN_MAXLV else set()
    tags |= {"dilation > L"} if (1 << (len(channels) - 1)) > L else set()
    tags |= {"L=%d" % L} & {"L=1", "L=%d" % TCN_MAXL}
    tags |= {"one live channel in the last chunk"} if any(a[4] == 1 for a in arms) else set()
    tags |= {"cout=%d" % ch for ch in channels} & {"cout=8", "cout=9", "cout=16", "cout=17"}
    tags |= {"a level without downsample"} if any(a == b for a, b in zip([c0] + list(channels), channels)) else set()
    tags |= {"no downsample anywhere"} if all(a == b for a, b in zip([c0] + list(channels), channels)) else set()
    if c.dropout:
        tags |= {"drop conv=15"} if len(channels) == 8 else set()
        tags |= {"drop channel=31"} if max(channels) == 32 else set()
        tags |= {"drop t=4095"} if L == 4096 else set()
    return tags


TCN_REQUIRED = {"slot r=1", "LDS full", "ncol=129", "groups=2", "tile tail", "first level cin > 1",
                "identity residual in the row dtype", "downsample over rin > 1", "c0=MAXC", "levels=8", "dilation > L",
                "L=1", "L=4096", "one live channel in the last chunk", "cout=8", "cout=9", "cout=16", "cout=17",
                "a level without downsample", "no downsample anywhere", "drop conv=15", "drop channel=31", "drop t=4095"}


# ------------------------------------------------------------------------------------- problems and float64 references
Problem = collections.namedtuple("Problem", "net x dy ref r32 hidden h32 pre extra")


def _named(y, x, named):
    return [("y", y.detach()), ("dx", x.grad)] + [(n, g) for n, g in named]


def _rnn_masked(rnn, x, dy, masks, dtype):
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    pre, hid = [], []
    y, leaves = elman(rnn, xr, masks, dtype, pre, hid)
    y.backward(dy.to(dtype))
    return _named(y, xr, [(n, q.grad) for (n, _), q in zip(rnn.named_parameters(), leaves)]), torch.stack(hid), pre


@functools.lru_cache(maxsize=None)
def rnn_problem(i, kind):
    """Case RNN_CASES[i] in row dtype `kind`: the nn.RNN holding the parameters, x and dy rounded to the row dtype, the
    float64 reference [(name, tensor)] of y, dx and every parameter gradient, torch's fp32 run of the same, the last
    hidden states in both, and the float64 pre-activations.  Computed once; nothing in it may be written."""
    c = RNN_CASES[i]
    T, _I, H, layers, dirs, _nl, _b = c.case
    seed = seed_of(c, kind)
    rnn = make_rnn(c.case, dropout=DROP_P if c.dropout else 0.0, seed=seed)
    x, dy = make_inputs(c.case, c.N, KINDS[kind], seed=seed)
    masks = [None] * layers
    if c.dropout:
        masks = [rnn_hash_masks(DROP_SEED, DROP_P, c.N, dirs * H, T, l) for l in range(layers - 1)] + [None]
        ref, href, pre = _rnn_masked(rnn, x, dy, masks, torch.float64)
        r32, h32, _p = _rnn_masked(rnn, x, dy, masks, torch.float32)
    else:
        ref, r32 = run_torch(rnn, x, dy, torch.float64), run_torch(rnn, x, dy, torch.float32)
        with torch.no_grad():
            pre, hid = [], []
            ye, _leaves = elman(rnn, x.double(), masks, torch.float64, pre, hid)
            href = torch.stack(hid)
            _y, h32 = rnn(x.float())
        # the written-out recurrence is nn.RNN: its pre-activations are the ones the ReLU margin is taken on
        assert float((ye - ref[0][1]).abs().max()) <= 1e-12 * float(ref[0][1].abs().max())
    return Problem(rnn, x, dy, ref, r32, href, h32, pre, masks)


def _tcn_run(net, x, dy, masks, dtype, pre=None, weights=None):
    m = tcn_twin(net, dtype).train()
    def keep(mod, _inputs, _output):              # d loss / d effective taps: weight norm recomputes .weight per call
        if mod.weight.requires_grad:
            mod.weight.retain_grad()
            weights.append(mod.weight)

    if weights is not None:
        for blk in m.network:
            for conv in blk.convs:
                conv.register_forward_hook(keep)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y = tcn_masked_reference(m, xr, masks, pre)
    y.backward(dy.to(dtype))
    return m, _named(y, xr, [(n, p.grad) for n, p in m.named_parameters()])


@functools.lru_cache(maxsize=None)
def tcn_problem(i, kind):
    """Case TCN_CASES[i] in row dtype `kind`, as rnn_problem: `hidden` / `h32` are unused, `extra` = (masks, the float64
    gradients of the EFFECTIVE taps of conv1 and conv2 of every level: what k_tcnc_dw's partial sums add up to)."""
    c = TCN_CASES[i]
    c0, channels, k, L = c.case
    seed = seed_of(c, kind)
    net, _ref = make_tcn(c0, channels, k, dropout=DROP_P if c.dropout else 0.0, seed=seed)
    g = torch.Generator().manual_seed(3000 + seed)
    # the rounded inputs both sides see; several input channels at half the spread: the residuals' positive downsample
    # weights add them up level by level, and max|Y| of the four-level case leaves the live range (1e3) otherwise
    x = (torch.randn(c.N, c0, L, generator=g) * (0.5 if c0 > 1 else 1.0)).to(KINDS[kind])
    dy = torch.randn(c.N, channels[-1], L, generator=g).to(KINDS[kind])
    masks = [None] * (2 * len(channels))
    if c.dropout:
        masks = [tcn_hash_masks(DROP_SEED, DROP_P, c.N, channels[ci // 2], L, ci) for ci in range(2 * len(channels))]
    pre, weights = [], []
    m64, ref = _tcn_run(net, x, dy, masks, torch.float64, pre, weights)
    _m, r32 = _tcn_run(net, x, dy, masks, torch.float32)
    if not c.dropout:                            # the written-out composition is the module's own forward
        with torch.no_grad():
            ym = m64(x.double())
        assert float((ym - ref[0][1]).abs().max()) <= 1e-12 * float(ref[0][1].abs().max())
    return Problem(net, x, dy, ref, r32, None, None, pre, (masks, [w.grad for w in weights]))


def relu_margin(pre):
    """Over the ReLUs of a net (`pre`: their pre-activations, one tensor per layer), the smallest
    min|pre-activation| / max|pre-activation| of a layer; inf for a net without ReLU.  Taken over the pre-activations
    that are not exactly zero in float64: an exact zero is a sum of exact zeros (every input dropped or dead, no bias
    or a dropped branch plus a dead residual), it is zero in any precision and order, and ReLU and its derivative are
    zero there on both sides."""
    out = float("inf")
    for z in pre:
        a = z.abs()
        out = min(out, float(a[a > 0].min()) / float(a.max()))
    return out


def e32_of(p):
    """torch's fp32 CPU run against float64, |error| over the float64 tensor's max: {name: e32}; a tensor that is
    identically zero in float64 must be so in fp32."""
    out = {}
    for (n, a), (_n, b) in zip(p.r32, p.ref):
        err, scale = wc.max_err(a, b)
        out[n] = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
    return out
