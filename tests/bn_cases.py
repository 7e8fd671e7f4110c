"""Float64 reference, a plain fp32 restatement, inputs and the case table for the sparse-row BatchNorm (+ ReLU) entry
points of csrc/bn.hip: wfs_bn_relu_fwd / wfs_bn_relu_bwd, called through the C ABI.

NumPy only; the product is not imported.  tests/test_bn_cases_host.py pins the reference against torch in float64,
proves every case well-posed on the CPU and checks the table's claims about the dispatch against wfs_bn_plan;
tests/test_gpu_bn_edges.py runs the table through the kernels.

The arithmetic (header comment of csrc/bn.hip), over the first ``valid`` rows of a [cap, C] array:
  training  mean_c, var_c (biased) over the rows; invstd = 1 / sqrt(var + eps); xhat = (x - mean) invstd
            running = (1 - momentum) running + momentum (mean | var n / (n - 1));  n = 1: factor 1 (the kernels' rule)
  eval      mean = running_mean, invstd = 1 / sqrt(running_var + eps); the running statistics stay
  pre = gamma xhat + beta;  y = pre, or max(0, pre) with ReLU;  g = dy [pre > 0] with ReLU, else dy
  dbeta = sum g;  dgamma = sum g xhat;  dX = gamma invstd (g - dbeta / n - xhat dgamma / n), eval: gamma invstd g

restate32() is the same in fp32, in the order a kernel of this shape sums: d = x - x[row 0] (shifted sums),
var = E[d^2] - E[d]^2, mean = x[row 0] + E[d]; every column sum is taken over blocks of 64 consecutive rows, one row
after the other, and the block sums are then added pairwise (neighbours first, a binary tree).  Its distance from the
float64 reference, e32, is what fp32 arithmetic of this shape costs on this input: a property of the input alone.  A
case must keep e32 <= E32_MAX for every tensor, a third of the fp32 bar the kernels are held to.

Inputs.  x = offset_c + scale_c * normal with scale 0.5 .. 3 and offset within +-4, dy normal, gamma 0.5 .. 1.5, beta
within +-0.5 and not closer to 0 than 0.02 (with one row xhat is 0 and beta alone decides the ReLU); x and dy rounded
to the row type first.  Then the inputs are conditioned, in this order, until nothing changes:
  * a column whose standard deviation over the valid rows is below half its scale (few rows drawn close together: the
    rounding of an fp32 mean near 4 then costs more than E32_MAX of xhat), or which has no element on one side of the
    ReLU, is replaced by offset + scale * (a permutation of n evenly spaced values in -1.7 .. 1.7);
  * ReLU margin: every element with |pre| < MARGIN max|pre| is moved away from the zero crossing by
    MOVE max|pre| / (gamma invstd), rounded to the row type, and stepped one unit in the last place if the rounding gave
    the old value back.  At most MOVED_MAX of a case's elements may be moved.
A draw whose margin moved more than MOVED_MAX of the elements is drawn again from the next seed (make_problem): in a
case of a few hundred elements a single moved element is already above that share.
Two rows are a case of their own: dX = +-(g0 - g1) / 2 * gamma invstd eps / (var + eps) is a difference of terms
1 + var / eps times its size, so no fp32 evaluation holds it where var is of order one.  The two-row case has its rows
a few sqrt(eps) apart around a mean of that size (var = 1 .. 9 eps), which is also the one case where eps weighs in.
The running statistics start near the data's (mean + 0.1 sigma U(-1, 1), var U(0.8, 1.25)) so that eval mode keeps both
sides of the ReLU populated.

Long serial sums.  At C = 516 the loop kernels have one row slot, so a thread adds ceil(N / 32) = 510 rows one after
the other.  A serial fp32 sum of d^2 over 16-bit rows loses about 1e-8 of itself per row, 6e-6 at 510 rows against 7e-7
in blocks of 64: d^2 of quantised values leaves few distinct residues below the sum's unit in the last place, and the
roundings do not average out.  var = E[d^2] - E[d]^2 multiplies that by 1 + (x[row 0] - mean)^2 / var; with row 0 two
sigma out, plain fp32 in THAT order misses invstd by 1.3e-5 (bf16 rows; fp32 rows: 7e-7), and so did the kernel.  e32
is therefore taken in the kernels' longest run of rows as well (chain_rows), and a case with such a run draws its
row 0 within 0.3 sigma of the channel means.

Two cases stand for the header's claim "shifted sums: no cancellation":
  offset2000  fp32 rows at scale 0.5 around 2000: naive sums of x^2 = 4e6 carry 0.25 .. 0.5 per unit in the last place
              and lose a variance of 0.25 entirely.  save_mean is an fp32 number by the ABI; half a unit in the last
              place of 2000 (6e-5) against sigma = 0.5 alone costs 3e-5 of max|y| in ANY fp32 implementation.  So the
              rows are nudged, by one unit in the last place each, until every column sum is a multiple of n units: the
              exact mean is then an fp32 number and the case measures the sums, not the format of save_mean.
  row0far     row 0, the shift, lies 4 sigma from its channel means.

Garbage: with a device-side count, X and dY rows at and beyond it hold NaN; every index stays in range.

Dispatch constants of csrc/bn.hip, from which expected_plan() derives family, rows per thread and partial count:
TB 256, MAXC 1024, FOLD_PER 32, RR_BLOCKS 256, BW_COLS 64, BW_SLOTS 4, BW_MAX_CHUNKS 256.
  C = 124  31 channel groups, 8 row slots (248 live threads), Cp = 128 -> 64 blocks, 512 rows per unit of PER:
           PER 2 to 1024 rows, 4 to 2048, 8 to 4096, 16 to 8192; 8193 rows leave the registers.  31 is no power of
           two: the serial block sum.  The fp32 backward stops at PER 8 (4097 rows and up run the loop kernels).
  C = 64   16 groups, 16 slots, 128 blocks, 2048 rows per unit: PER 2 / 4 / 8 / 16 at 4096 / 4097 / 8193 / 16385, the
           lane-exchange block sum; 32769 rows: loop kernels, VEC 4, 128 partials (the cap at Cp = 64).
  C = 4    1 group, 256 slots.  C = 20: 5 groups, 51 slots, 255 live threads, 256 x 51 = 13056 rows per unit.
  C = 516  129 groups, 1 slot, Cp = 256: three column passes of the fold; N C > 2^23 needs 16257 rows or more.
  VEC 1    C not a multiple of 4 and below 128; C = 7: Cp = 8, up to 1024 partials (65537 rows reach the cap).
  column-block: C >= 128 and (C > 1024 or C % 4 != 0 or N C <= 2^23); chunks = ceil(N / 32), at most 256
           (8160 rows: 255, 8161: 256, 8193: the cap, chunks of 36 rows of which the last 28 are empty).
"""
import functools
from types import SimpleNamespace

import numpy as np

from tail_cases import round_to

KINDS = ("f32", "bf16", "f16")
U_ROUND = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}          # one round to nearest of the stored value
BAR32 = 1e-5                         # the project's fp32 bar, of a tensor's largest magnitude
E32_MAX = 3e-6                       # what the fp32 restatement may lose on a case's inputs
MARGIN, MOVE, MOVED_MAX = 1e-4, 2e-4, 2e-3
EPS, MOMENTUM = 1e-5, 0.1
TRACKED0 = 41                        # num_batches_tracked before the call

TB, MAXC, FOLD_PER, RR_BLOCKS, BW_COLS, BW_SLOTS, BW_MAX_CHUNKS = 256, 1024, 32, 256, 64, 4, 256
COLUMN, RR, LOOP4, LOOP1, SLICES = 0, 1, 2, 3, 4
FAMILY_NAMES = {COLUMN: "column-block", RR: "register-resident", LOOP4: "loop VEC4", LOOP1: "loop VEC1", SLICES: "slices"}
F32_TENSORS = ("save_mean", "save_invstd", "running_mean", "running_var", "dgamma", "dbeta")
ROW_TENSORS = ("y", "dX")


# ------------------------------------------------------------------------------------------------------- dispatch
def _cdiv(a, b):
    return -(-a // b)


def fold_cp(C):
    Cp = 1
    while Cp < C and Cp < TB:
        Cp *= 2
    return Cp


def block_sum_path(C):
    """Which block sum the register-resident kernels take: lane exchanges when the channel groups divide the wave."""
    groups = C // 4
    return "lane-exchange" if groups <= 64 and groups & (groups - 1) == 0 else "serial"


def expected_plan(N, C, kind, training, backward):
    """(family, rows per thread, partials folded) as derived from the constants above; N > 0."""
    sums = bool(training or backward)
    if C >= 128 and (C > MAXC or C % 4 != 0 or N * C <= 1 << 23):
        return COLUMN, 0, (min(max(_cdiv(N, 32), 1), BW_MAX_CHUNKS) if sums else 0)
    assert 1 <= C <= (MAXC if C % 4 == 0 else TB)
    cap = FOLD_PER * (TB // fold_cp(C))
    if C % 4 == 0 and sums:
        blocks, slots = min(cap, RR_BLOCKS), TB // (C // 4)
        need = _cdiv(N, blocks * slots)
        for per in (2, 4, 8, 16):
            if need <= per <= (8 if backward and kind == "f32" else 16):
                return RR, per, blocks
    return (LOOP4 if C % 4 == 0 else LOOP1), 0, (min(max(_cdiv(N, 64), 1), cap) if sums else 0)


# ------------------------------------------------------------------------------------------------------ references
def _stats64(x64, rm, rv, training):
    if training:
        mean = x64.mean(axis=0)
        var = np.square(x64 - mean).mean(axis=0)
    else:
        mean, var = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
    return mean, var, 1.0 / np.sqrt(var + EPS)


def reference(x, g, gamma, beta, rm, rv, valid, relu, training):
    """Float64 BatchNorm (+ ReLU) forward and backward over x[:valid], g[:valid] of [cap, C] arrays.  gamma / beta /
    rm / rv may be None (rm and rv only in training).  y and dX come back [cap, C] with NaN = "untouched" in the rows
    at and beyond ``valid``."""
    cap, C = x.shape
    n = int(valid)
    assert 1 <= n <= cap and (training or (rm is not None and rv is not None))
    x64, g64 = np.asarray(x[:n], np.float64), np.asarray(g[:n], np.float64)
    ga = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    be = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    mean, var, invstd = _stats64(x64, rm, rv, training)
    r = SimpleNamespace(valid=n, mean=mean, var=var, invstd=invstd, save_mean=mean, save_invstd=invstd,
                        running_mean=None, running_var=None)
    if rm is not None:
        rm64, rv64 = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
        if training:
            unbiased = var * (n / (n - 1.0) if n > 1 else 1.0)
            r.running_mean = (1 - MOMENTUM) * rm64 + MOMENTUM * mean
            r.running_var = (1 - MOMENTUM) * rv64 + MOMENTUM * unbiased
        else:
            r.running_mean, r.running_var = rm64, rv64
    xhat = (x64 - mean) * invstd
    pre = ga * xhat + be
    live = pre > 0 if relu else np.ones_like(pre, bool)
    gm = np.where(live, g64, 0.0)
    r.pre = pre
    r.dbeta = gm.sum(axis=0)
    r.dgamma = (gm * xhat).sum(axis=0)
    dX = ga * invstd * (gm - r.dbeta / n - xhat * r.dgamma / n) if training else ga * invstd * gm
    r.y = np.full((cap, C), np.nan)
    r.dX = np.full((cap, C), np.nan)
    r.y[:n] = np.where(live, pre, 0.0)
    r.dX[:n] = dX
    return r


def _bsum32(a, block=64):
    """Column sums of an fp32 [n, C] array: blocks of ``block`` consecutive rows, row after row; then the block sums
    pairwise."""
    n, C = a.shape
    nb = _cdiv(n, block)
    p = np.zeros((nb * block, C), np.float32)
    p[:n] = a
    p = p.reshape(nb, block, C)
    acc = p[:, 0, :].copy()
    for i in range(1, block):
        acc += p[:, i, :]
    while acc.shape[0] > 1:
        if acc.shape[0] & 1:
            acc = np.concatenate([acc, np.zeros((1, C), np.float32)])
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def restate32(x, g, gamma, beta, rm, rv, valid, relu, training, block=64):
    """The same formulas in fp32 and in the summation order of the module docstring; {tensor: fp32 array} over the
    valid rows."""
    f = np.float32
    n = int(valid)
    X, G = np.asarray(x[:n], f), np.asarray(g[:n], f)
    C = X.shape[1]
    ga = np.ones(C, f) if gamma is None else np.asarray(gamma, f)
    be = np.zeros(C, f) if beta is None else np.asarray(beta, f)
    nf, one, mom, eps = f(n), f(1), f(MOMENTUM), f(EPS)
    out = {}
    if training:
        shift = X[0]
        d = X - shift
        md = _bsum32(d, block) / nf
        var = np.maximum(_bsum32(d * d, block) / nf - md * md, f(0))
        mean, inv = shift + md, one / np.sqrt(var + eps)
        if rm is not None:
            unbiased = var * (nf / (nf - one)) if n > 1 else var
            out["running_mean"] = (one - mom) * np.asarray(rm, f) + mom * mean
            out["running_var"] = (one - mom) * np.asarray(rv, f) + mom * unbiased
    else:
        mean, inv = np.asarray(rm, f), one / np.sqrt(np.asarray(rv, f) + eps)
        out["running_mean"], out["running_var"] = np.asarray(rm, f), np.asarray(rv, f)
    xhat = (X - mean) * inv
    pre = ga * xhat + be
    live = pre > 0 if relu else np.ones_like(pre, bool)
    gm = np.where(live, G, f(0))
    dbeta, dgamma = _bsum32(gm, block), _bsum32(gm * xhat, block)
    k1, k2 = (dbeta / nf, dgamma / nf) if training else (np.zeros(C, f), np.zeros(C, f))
    out.update(save_mean=mean, save_invstd=inv, dbeta=dbeta, dgamma=dgamma, y=np.where(live, pre, f(0)),
               dX=ga * inv * (gm - k1 - xhat * k2))
    assert all(v.dtype == f for v in out.values())
    return out


def wanted(ref):
    """{tensor: float64 array} of the tensors a case compares (running statistics only when it has them)."""
    out = {t: getattr(ref, t) for t in F32_TENSORS if getattr(ref, t) is not None}
    out["y"], out["dX"] = ref.y, ref.dX
    return out


def chain_rows(case):
    """The longest run of rows ONE thread of the case's arms adds one after the other (from the dispatch constants):
    the loop kernels give a block ceil(N / partials) rows on TB / groups row slots; the register-resident kernels hold
    at most 16 rows per thread and the column blocks at most 9 per slot."""
    longest = 0
    for backward in (False, True):
        fam, _per, partials = expected_plan(case.N, case.C, "f32", case.training, backward)
        if fam in (LOOP4, LOOP1) and partials:
            slots = TB // (case.C // 4 if fam == LOOP4 else case.C)
            longest = max(longest, _cdiv(_cdiv(case.N, partials), slots))
    return longest


def e32_of(problem, ref):
    """{tensor: max |restate32 - float64| / max |float64|}; 0 where both are identically zero.  The restatement sums
    in blocks of 64 rows and, where a thread of the case's kernels walks more rows than that, in blocks of that length
    as well: the larger distance counts."""
    p = problem
    out = {}
    for block in sorted({64, max(64, chain_rows(p.case))}):
        got = restate32(p.x, p.g, p.gamma, p.beta, p.rm, p.rv, p.valid, p.case.relu, p.case.training, block)
        for t, want in wanted(ref).items():
            w = want[:p.valid] if t in ROW_TENSORS else want
            err = float(np.abs(got[t].astype(np.float64) - w).max())
            top = float(np.abs(w).max())
            out[t] = max(out.get(t, 0.0), err / top if top > 0 else (0.0 if err == 0 else float("inf")))
    return out


def ratio_f32(got, want):
    """max |got - want| / (BAR32 max|want|); a reference that is identically zero must be met exactly."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    if top == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / (BAR32 * top)


def ratio_rows(got, want, u):
    """max over the elements of |got - want| / (BAR32 max|want| + u |want|), over valid rows; as ratio_f32 for zero."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err, top = np.abs(got - want), float(np.abs(want).max())
    if top == 0.0:
        return 0.0 if not err.any() else float("inf")
    return float((err / (BAR32 * top + u * np.abs(want))).max())


# ---------------------------------------------------------------------------------------------------------- inputs
def step_ulp(v, direction, kind):
    """v (fp32 array of values of the row type) moved one unit in the last place of that type towards direction * inf."""
    v = np.ascontiguousarray(v, np.float32)
    direction = np.asarray(direction, np.float32)
    if kind == "f32":
        return np.nextafter(v, direction * np.float32(np.inf))
    if kind == "f16":
        return np.nextafter(v.astype(np.float16), (direction * np.float32(np.inf)).astype(np.float16)).astype(np.float32)
    bits = v.view(np.int32).astype(np.int64)
    away = np.where(v > 0, direction > 0, direction < 0)              # away from zero = larger magnitude bits
    out = np.where(away, bits + 0x10000, bits - 0x10000).astype(np.int32).view(np.float32)
    return np.where(v == 0, direction * np.float32(2.0 ** -100), out).astype(np.float32)


def _spread(rng, n, offset, scale):
    return offset + scale * rng.permutation(np.linspace(-1.7, 1.7, n) if n > 1 else np.zeros(1))


def _make_sums_exact(x, n):
    """offset2000: one more unit in the last place on as many rows (after row 0) as make every column sum of x[:n] a
    multiple of n units, so that the exact mean is an fp32 number.  All values lie in [1024, 2048): unit 2^-13."""
    unit = 2.0 ** -13
    assert n >= 2 and float(x[:n].min()) >= 1024 and float(x[:n].max()) < 2047
    k = np.rint(x[:n].astype(np.float64).sum(axis=0) / unit).astype(np.int64)
    add = (-k) % n                                                     # 0 .. n - 1 rows per column
    rows = np.arange(1, n)[:, None]
    x[1:n] += np.where(rows <= add[None, :], np.float32(unit), np.float32(0))
    s = x[:n].astype(np.float64).sum(axis=0) / unit
    assert np.array_equal(s, np.rint(s)) and not (np.rint(s).astype(np.int64) % n).any()


CASES = []


def _case(tag, C, N, fwd, bwd, bwd_f32=None, valid=None, kinds=KINDS, relu=True, training=True, affine=True, running=True,
          special=None, why=""):
    name = "%s-C%d-N%d" % (tag, C, N) + ("" if valid is None else "-v%d" % valid)
    CASES.append(SimpleNamespace(name=name, tag=tag, C=C, N=N, valid=valid, kinds=tuple(kinds), relu=relu, training=training,
                                 affine=affine, running=running or not training, special=special, fwd=fwd, bwd=bwd,
                                 bwd_f32=bwd_f32 or bwd, why=why, seed=len(CASES)))


def claimed(case, kind, backward):
    """(family, rows per thread) the table claims for one direction and row type."""
    return (case.bwd_f32 if kind == "f32" else case.bwd) if backward else case.fwd


_L4 = (LOOP4, 0)
# register-resident, serial block sum (31 groups): PER 2 / 4 / 8 / 16 and each boundary.  From 4097 rows the fp32
# backward has left the registers (max_per 8) while its forward stays at PER 16; 16-bit rows keep PER 16 both ways.
for _N, _per in ((1, 2), (2, 2), (7, 2), (8, 2), (9, 2), (1024, 2), (1025, 4), (2048, 4), (2049, 8), (4096, 8), (4097, 16),
                 (8192, 16)):
    _case("rr_serial", 124, _N, (RR, _per), (RR, _per), bwd_f32=_L4 if _per == 16 else None, why="PER and its boundaries")
# register-resident, lane-exchange block sum (16 groups)
for _N, _per in ((4096, 2), (4097, 4), (8193, 8), (16385, 16)):
    _case("rr_lanes", 64, _N, (RR, _per), (RR, _per), bwd_f32=_L4 if _per == 16 else None, why="PER on the other sum")
# other widths: 1 group of 256 slots; 5 groups, 51 slots, 255 live threads (one row past a unit of 13056); the PSD width
for _C, _N in ((4, 300), (20, 33), (20, 13057), (32, 257)):
    _case("rr_width", _C, _N, (RR, 2), (RR, 2), why="group / slot layouts")
# loop kernels, VEC 4, training: the smallest batch that does not fit (64 partials: the cap at Cp = 128); 128 partials
_case("loop4", 124, 8193, _L4, _L4, why="first batch beyond the registers")
_case("loop4", 64, 32769, _L4, _L4, why="first batch beyond the registers, 16 groups")
# loop kernels, VEC 4, C >= 128: 129 groups, 1 slot, the fold's second and third column pass
_case("loop4_wide", 516, 16300, _L4, _L4, kinds=("f32", "bf16"), why="N C > 2^23; fold with C > 256")
# loop kernels, VEC 4, eval forward (k_bn_apply without partials); the eval backward of these is register-resident
_case("loop4_eval", 32, 257, _L4, (RR, 2), training=False, why="eval forward")
_case("loop4_eval", 124, 65, _L4, (RR, 2), training=False, why="eval forward, 31 groups")
# loop kernels, VEC 1: 1 channel; Cp = 2 .. 128; 2 slots of 127; 1 -> 2 blocks; 1024 partials
for _C, _N in ((1, 65), (2, 64), (5, 63), (7, 1), (7, 65537), (31, 200), (33, 64), (46, 65), (127, 129)):
    _case("loop1", _C, _N, (LOOP1, 0), (LOOP1, 0), why="scalar layouts and partial counts")
# column-block: 2 full column blocks; last block with 1 and 2 live lanes; C > MAXC; fewer rows than row slots; 1 -> 2
# chunks; 255 -> 256 chunks and beyond the cap
for _C, _N in ((128, 5), (129, 1), (130, 3), (130, 4), (130, 32), (130, 33), (130, 8160), (130, 8161), (130, 8193), (1025, 40),
               (2050, 33)):
    _case("column", _C, _N, (COLUMN, 0), (COLUMN, 0), why="column blocks and chunk counts")
# device-side counts: 1, a count that ends inside a block / chunk, the capacity
for _C, _cap, _mid, _f in ((124, 1100, 700, (RR, 4)), (124, 8193, 5000, _L4), (7, 300, 130, (LOOP1, 0)), (130, 200, 75, (COLUMN, 0))):
    for _v in (1, _mid, _cap):
        _case("count", _C, _cap, _f, _f, valid=_v, why="device-side row count")
# one small shape per family: no ReLU, eval (forward and backward), no affine parameters, no running statistics
SMALL = ((32, 257, (RR, 2)), (124, 8193, _L4), (31, 200, (LOOP1, 0)), (130, 33, (COLUMN, 0)))
for _C, _N, _f in SMALL:
    _case("norelu", _C, _N, _f, _f, relu=False)
    if _f[0] != RR:                                      # (32, 257) in eval mode is loop4_eval-C32-N257
        _case("eval", _C, _N, _f, _f, training=False)
    _case("noaffine", _C, _N, _f, _f, affine=False)
    _case("norunning", _C, _N, _f, _f, running=False)
# "shifted sums: no cancellation"
for _C, _N, _f in ((124, 1025, (RR, 4)), (124, 8193, _L4), (7, 300, (LOOP1, 0)), (130, 33, (COLUMN, 0))):
    _case("offset2000", _C, _N, _f, _f, kinds=("f32",), special="offset2000")
# A shift 4 sigma away makes var = E[d^2] - E[d]^2 a difference of terms 17 and 16 times its size, so the fp32
# restatement's invstd is 2e-6 .. 7e-6 away on the worst of 124 channels and reaches E32_MAX only at fewer channels or
# rows; at 124 x 8193 (the smallest batch of the VEC 4 loop kernels) it does for fp32 rows and for no 16-bit draw.
for _C, _N, _f, _k in ((32, 257, (RR, 2), KINDS), (124, 8193, _L4, ("f32",)), (7, 300, (LOOP1, 0), KINDS),
                       (130, 33, (COLUMN, 0), KINDS)):
    _case("row0far", _C, _N, _f, _f, kinds=_k, special="row0far")

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases_for(kind):
    return [c for c in CASES if kind in c.kinds]


ATTEMPTS = 12


@functools.lru_cache(maxsize=6)
def make_problem(name, kind):
    """One case in one row type: x, g [cap, C] as fp32 arrays of values of the row type (NaN rows beyond the count),
    gamma, beta, rm, rv fp32 or None.  Read-only: shared between tests.  A draw in which the margin moved more than
    MOVED_MAX of the elements is drawn again from the next seed (a case of a few hundred elements may not have a single
    one moved); so is a row0far draw whose e32 is above E32_MAX.  Both are conditions on the inputs and the float64
    reference alone."""
    case = BY_NAME[name]
    assert kind in case.kinds
    for attempt in range(ATTEMPTS):
        p = _draw(case, kind, attempt)
        if p.moved_share > MOVED_MAX:
            continue
        if case.special == "row0far":
            ref = reference(p.x, p.g, p.gamma, p.beta, p.rm, p.rv, p.valid, case.relu, case.training)
            if max(e32_of(p, ref).values()) > E32_MAX:
                continue
        return p
    raise AssertionError("%s %s: no draw out of %d is well-posed" % (name, kind, ATTEMPTS))


def _far_row(n, r=4.0):
    """t such that a row at mean + t sigma of the OTHER n - 1 rows lies r sigma from the mean of all n rows."""
    assert n - 1 > r * r
    return np.sqrt(r * r * n / (n - 1 - r * r))


def _draw(case, kind, attempt):
    name = case.name
    rng = np.random.default_rng(91000 + case.seed + 977 * attempt)
    C, cap = case.C, case.N
    n = cap if case.valid is None else case.valid
    scale, offset = rng.uniform(0.5, 3.0, C), rng.uniform(-4.0, 4.0, C)
    if case.special == "offset2000":
        scale, offset = np.full(C, 0.5), np.full(C, 2000.0)
    x64 = offset + scale * rng.standard_normal((n, C))
    if case.special == "row0far":
        x64[0] = x64[1:].mean(axis=0) + _far_row(n) * x64[1:].std(axis=0) * rng.choice([-1.0, 1.0], C)
    if chain_rows(case) > 64:
        x64[0] = offset + 0.3 * scale * rng.uniform(-1.0, 1.0, C)      # long serial sums: see the module docstring
    if n == 2 and case.training:
        # two rows: dX = +-(g0 - g1) / 2 * gamma invstd eps / (var + eps), a difference of terms 1 + var / eps times its
        # size.  It is well-posed only where the variance is a few eps: rows a few sqrt(eps) apart, around a mean of
        # that size (the rounding of an fp32 mean near 4 would cost more than the rows are apart).
        h = np.sqrt(EPS) * rng.uniform(1.0, 3.0, C)
        x64 = h * rng.uniform(-1.0, 1.0, C) + h * np.array([[-1.0], [1.0]]) * rng.choice([-1.0, 1.0], C)
    x = round_to(x64, kind).copy()
    g = round_to(rng.standard_normal((n, C)), kind).copy()
    gamma = beta = None
    if case.affine:
        gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
        beta = (rng.choice([-1.0, 1.0], C) * rng.uniform(0.02, 0.5, C)).astype(np.float32)
    ga64 = np.ones(C) if gamma is None else gamma.astype(np.float64)
    be64 = np.zeros(C) if beta is None else beta.astype(np.float64)
    u_run, v_run = rng.uniform(-1.0, 1.0, C), rng.uniform(0.8, 1.25, C)
    moved = np.zeros((n, C), bool)
    replaced = np.zeros(C, bool)
    rm = rv = None
    for _pass in range(40):
        if case.special == "offset2000":
            _make_sums_exact(x, n)
        xd = x.astype(np.float64)
        mean, var, _i = _stats64(xd, None, None, True)
        if rm is None and case.running:                    # fixed once: the eval-mode passes normalise with them
            rm = (mean + 0.1 * np.sqrt(var) * u_run).astype(np.float32)
            rv = np.maximum(var * v_run, 0.01).astype(np.float32)
        mean, var, invstd = _stats64(xd, rm, rv, case.training)
        pre = ga64 * ((xd - mean) * invstd) + be64
        bad = np.zeros(C, bool)
        if n > 2 and case.special is None:
            bad |= xd.std(axis=0) < 0.5 * scale
            if case.relu and n >= 8:
                bad |= ~((pre > 0).any(axis=0) & (pre <= 0).any(axis=0))
            bad &= ~replaced
        if bad.any():
            for c in np.flatnonzero(bad):
                x[:, c] = round_to(_spread(rng, n, offset[c], scale[c]), kind)
            replaced |= bad
            moved[:, bad] = False
            rm = rv = None                                 # drawn again from the new columns
            continue
        top = float(np.abs(pre).max())
        inside = np.abs(pre) < MARGIN * top
        if not inside.any():
            break
        sign = np.where(pre >= 0, 1.0, -1.0)
        delta = (MOVE * top / (ga64 * invstd))[None, :] * sign
        old = x[inside]
        new = round_to(old.astype(np.float64) + delta[inside], kind)
        same = new == old
        new[same] = step_ulp(old[same], sign[inside][same], kind)
        x[inside] = new
        moved |= inside
    else:
        raise AssertionError("%s %s: the inputs did not settle" % (name, kind))
    X = np.full((cap, C), np.nan, np.float32)
    G = np.full((cap, C), np.nan, np.float32)
    X[:n], G[:n] = x, g
    p = SimpleNamespace(case=case, kind=kind, x=X, g=G, gamma=gamma, beta=beta, rm=rm, rv=rv, valid=n, cap=cap,
                        padded=case.valid is not None, moved_share=float(moved.mean()), replaced=int(replaced.sum()),
                        scale=scale, offset=offset)
    for a in (X, G, gamma, beta, rm, rv):
        if a is not None:
            a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=6)
def reference_of(name, kind):
    p = make_problem(name, kind)
    return reference(p.x, p.g, p.gamma, p.beta, p.rm, p.rv, p.valid, p.case.relu, p.case.training)
