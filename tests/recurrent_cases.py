"""Shared by tests/test_recurrent_host.py and tests/test_gpu_recurrent.py: the RNN cases, the parameter recipe that keeps
them alive, and the float64 oracle.  (Not a test module: nothing here is collected.)

Why a recipe: with N(0, 0.5^2) weights the committed shape (ReLU, no bias, 4 hidden units, 4 layers) is DEAD -- every
output and gradient exactly zero -- for one seed in three, and positive weights with only W_hh normalised grow to 1e15
through eight layers.  So: every W_hh is scaled to spectral radius 0.9; every W_ih is row-normalised (L1: a row maps
inputs of size s to a pre-activation of size <= s); biases are positive (0.1 .. 0.4); W_ih is positive for ReLU nets and
wherever there is no bias (a positive mean in place of the positive bias), and the inputs are positive-mean pulses.  `assert_live` states what the
recipe must achieve; the tests assert it on the float64 run before they compare anything.
"""
import torch

# (T, I, H, layers, directions, nonlinearity, bias)
CASES = [
    (59, 1, 4, 4, 1, "relu", False),      # the committed config (config/waveform_rnn_z.json)
    (62, 1, 4, 4, 2, "relu", True),       # ... with use_detector_number, bidirectional
    (59, 1, 7, 8, 1, "relu", True),       # H not a padded size, the deepest stack
    (1024, 1, 32, 2, 1, "tanh", True),    # long rows, the widest state
    (1024, 1, 16, 3, 2, "relu", True),
    (12, 3, 5, 2, 2, "tanh", False),      # I > 1
]


def case_id(c):
    return "-".join(str(v) for v in c)


def make_rnn(case, dropout=0.0, seed=0):
    """torch.nn.RNN (fp32, CPU) of the case with the live-parameter recipe applied."""
    T, I, H, layers, dirs, nonlin, bias = case
    torch.manual_seed(seed)
    rnn = torch.nn.RNN(I, H, layers, nonlinearity=nonlin, bias=bias, dropout=dropout, bidirectional=dirs == 2,
                       batch_first=True)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in rnn.named_parameters():
            if name.startswith("weight_hh"):
                w = torch.randn(p.shape, generator=g, dtype=torch.float64)
                rho = float(torch.linalg.eigvals(w).abs().max())
                p.copy_((w * (0.9 / rho)).float())
            elif name.startswith("weight_ih"):
                w = torch.randn(p.shape, generator=g, dtype=torch.float64)
                if nonlin == "relu" or not bias:
                    w = w.abs() + 0.1
                p.copy_((w / w.abs().sum(1, keepdim=True)).float())
            else:
                p.copy_(torch.rand(p.shape, generator=g) * 0.3 + 0.1)
    return rnn


def make_inputs(case, N, dtype, seed=0):
    """x [N, T, I] and dy [N, T, dirs H], already rounded to the row dtype: positive-mean pulses, mixed-sign dy."""
    T, I, H, _layers, dirs, _n, _b = case
    g = torch.Generator().manual_seed(2000 + seed)
    x = (torch.randn(N, T, I, generator=g) * 0.5 + 0.6).to(dtype)
    dy = torch.randn(N, T, dirs * H, generator=g).to(dtype)
    return x, dy


def run_torch(rnn, x, dy, dtype):
    """nn.RNN in `dtype` (float64: the oracle; float32: torch's own error) on the CPU: [(name, tensor)] of y, dx and
    every parameter gradient, in named_parameters order."""
    import copy
    m = copy.deepcopy(rnn).to(dtype)
    m.zero_grad(set_to_none=True)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y, _h = m(xr)
    y.backward(dy.to(dtype))
    return [("y", y.detach()), ("dx", xr.grad)] + [(n, p.grad) for n, p in m.named_parameters()]


def assert_live(ref):
    """The three conditions on the float64 run: every compared tensor has a non-zero maximum, at most half of Y's
    elements are exactly zero, max|Y| in [1e-2, 1e3]."""
    for name, t in ref:
        assert float(t.abs().max()) > 0, "dead tensor %s" % name
    y = ref[0][1]
    zeros = float((y == 0).double().mean())
    ymax = float(y.abs().max())
    assert zeros <= 0.5, "%.3f of Y is exactly zero" % zeros
    assert 1e-2 <= ymax <= 1e3, "max|Y| = %g" % ymax
    return zeros, ymax
