"""GPU checks of GraphNet (psd/graphnet.py on csrc/graphconv.hip) against the float64 restatement of tests/graph_cases.py
on the same rounded inputs, at the project's bars (waveform_cases.TOL: 1e-5 / 2e-2 / 3e-3 of each tensor's largest
magnitude).  Every case is first held to the margin of graph_cases.margin_ok on the float64 run: no non-zero ReLU
argument within 1e-5 of its tensor's largest magnitude.

16-bit gradients of the whole net are not held to the bars (a 16-bit rounding flips ReLUs that float64 keeps): they were
measured against float64 on an MI355X, per tensor, and are asserted at 1.5 x the recorded maxima (GRAD16).
The net widens bf16 rows at its input, so its bf16 column holds what is left of that: the rounding of dX."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import graph_cases as gc
from waveform_cases import TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"classifier": os.path.join(ROOT, "config", "segment_classifier_graph.json"),
           "quantifier": os.path.join(ROOT, "config", "segment_quantifier_graph.json")}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
# largest |gradient - float64| / largest |float64 gradient| of the small plan's case per tensor, measured on an MI355X
# (DESIGN.md 4 has the table); the test asserts 1.5 x these
GRAD16 = {
    "bf16": {
        "dX": 0.00266,
        "graph_layers.0.batchnorm.module.bias": 0.00146,
        "graph_layers.0.batchnorm.module.weight": 0.00191,
        "graph_layers.0.graph_net.film_skip.weight": 0.00128,
        "graph_layers.0.graph_net.films.0.bias": 0.00173,
        "graph_layers.0.graph_net.films.0.weight": 0.00171,
        "graph_layers.0.graph_net.lin_skip.weight": 0.00222,
        "graph_layers.0.graph_net.lins.0.weight": 0.00189,
        "graph_layers.1.batchnorm.module.bias": 0.00117,
        "graph_layers.1.batchnorm.module.weight": 0.0016,
        "graph_layers.1.graph_net.film_skip.weight": 0.00146,
        "graph_layers.1.graph_net.films.0.bias": 0.0012,
        "graph_layers.1.graph_net.films.0.weight": 0.00152,
        "graph_layers.1.graph_net.lin_skip.weight": 0.00197,
        "graph_layers.1.graph_net.lins.0.weight": 0.00242,
        "graph_layers.2.batchnorm.module.bias": 0.0015,
        "graph_layers.2.batchnorm.module.weight": 0.00127,
        "graph_layers.2.graph_net.film_skip.weight": 0.00169,
        "graph_layers.2.graph_net.films.0.bias": 0.00154,
        "graph_layers.2.graph_net.films.0.weight": 0.00193,
        "graph_layers.2.graph_net.lin_skip.weight": 0.00202,
        "graph_layers.2.graph_net.lins.0.weight": 0.00209,
        "graph_layers.3.batchnorm.module.bias": 0.00192,
        "graph_layers.3.batchnorm.module.weight": 0.00274,
        "graph_layers.3.graph_net.film_skip.weight": 0.00194,
        "graph_layers.3.graph_net.films.0.bias": 0.00208,
        "graph_layers.3.graph_net.films.0.weight": 0.0014,
        "graph_layers.3.graph_net.lin_skip.weight": 0.00227,
        "graph_layers.3.graph_net.lins.0.weight": 0.00196,
        "graph_layers.4.batchnorm.module.bias": 0.000877,
        "graph_layers.4.batchnorm.module.weight": 0.00127,
        "graph_layers.4.graph_net.film_skip.weight": 0.00191,
        "graph_layers.4.graph_net.films.0.bias": 0.00324,
        "graph_layers.4.graph_net.films.0.weight": 0.00191,
        "graph_layers.4.graph_net.lin_skip.weight": 0.00141,
        "graph_layers.4.graph_net.lins.0.weight": 0.00211,
    },
    "f16": {
        "dX": 0.018,
        "graph_layers.0.batchnorm.module.bias": 0.00911,
        "graph_layers.0.batchnorm.module.weight": 0.0107,
        "graph_layers.0.graph_net.film_skip.weight": 0.00585,
        "graph_layers.0.graph_net.films.0.bias": 0.122,
        "graph_layers.0.graph_net.films.0.weight": 0.058,
        "graph_layers.0.graph_net.lin_skip.weight": 0.00781,
        "graph_layers.0.graph_net.lins.0.weight": 0.093,
        "graph_layers.1.batchnorm.module.bias": 0.0101,
        "graph_layers.1.batchnorm.module.weight": 0.00869,
        "graph_layers.1.graph_net.film_skip.weight": 0.0133,
        "graph_layers.1.graph_net.films.0.bias": 0.0094,
        "graph_layers.1.graph_net.films.0.weight": 0.00767,
        "graph_layers.1.graph_net.lin_skip.weight": 0.0185,
        "graph_layers.1.graph_net.lins.0.weight": 0.0148,
        "graph_layers.2.batchnorm.module.bias": 0.0136,
        "graph_layers.2.batchnorm.module.weight": 0.0115,
        "graph_layers.2.graph_net.film_skip.weight": 0.00653,
        "graph_layers.2.graph_net.films.0.bias": 0.00933,
        "graph_layers.2.graph_net.films.0.weight": 0.0162,
        "graph_layers.2.graph_net.lin_skip.weight": 0.00804,
        "graph_layers.2.graph_net.lins.0.weight": 0.00882,
        "graph_layers.3.batchnorm.module.bias": 0.0128,
        "graph_layers.3.batchnorm.module.weight": 0.00706,
        "graph_layers.3.graph_net.film_skip.weight": 0.0147,
        "graph_layers.3.graph_net.films.0.bias": 0.00702,
        "graph_layers.3.graph_net.films.0.weight": 0.00739,
        "graph_layers.3.graph_net.lin_skip.weight": 0.0151,
        "graph_layers.3.graph_net.lins.0.weight": 0.00693,
        "graph_layers.4.batchnorm.module.bias": 0.000118,
        "graph_layers.4.batchnorm.module.weight": 0.000798,
        "graph_layers.4.graph_net.film_skip.weight": 0.00429,
        "graph_layers.4.graph_net.films.0.bias": 0.0506,
        "graph_layers.4.graph_net.films.0.weight": 0.0158,
        "graph_layers.4.graph_net.lin_skip.weight": 0.0071,
        "graph_layers.4.graph_net.lins.0.weight": 0.00475,
    },
}


# largest |captured - eager| of a parameter after one step at the configs' widths over the tensor's largest magnitude,
# measured on an MI355X; test_captured_step_on_a_padded_batch_equals_the_eager_step asserts 1.5 x these
WIDE_STEP = {"classifier": 2.81e-4, "quantifier": 1.01e-6}


def dev_tables(c, k, self_loop=False, n_valid=None):
    from waveformml_amd.psd.graphnet import NeighbourTables
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int64, device=DEV)
    return NeighbourTables(torch.from_numpy(np.ascontiguousarray(c)).to(DEV), k, self_loop, nv)


def check_tables(t, c, k, self_loop=False, n_valid=None):
    nbr, deg = gc.restated_knn(c, k, self_loop, n_valid)
    got_nbr, got_deg = t.nbr.cpu().numpy(), t.deg.cpu().numpy()
    assert np.array_equal(got_nbr, nbr) and np.array_equal(got_deg, deg), (k, self_loop, n_valid)
    pos, rows = t.rev_pos.cpu().numpy(), t.rev_rows.cpu().numpy()
    used = np.zeros(len(rows), bool)
    for j in range(len(c)):
        want = [i for i in range(len(c)) for q in range(deg[i]) if nbr[i, q] == j]          # ascending rows
        start, count = int(pos[j, 0]), int(pos[j, 1])
        assert count == len(want) and list(rows[start:start + count]) == want, j
        assert not used[start:start + count].any()                                           # no two lists overlap
        used[start:start + count] = True
    return nbr, deg


def test_neighbour_tables_equal_the_restatement_on_the_crafted_events():
    c = gc.crafted_events()
    for k, loop in [(3, False), (1, False), (8, False), (3, True), (8, True)]:
        check_tables(dev_tables(c, k, loop), c, k, loop)
    from waveformml_amd.psd.graphnet import NeighbourTables
    with pytest.raises(RuntimeError, match="k = 9"):
        NeighbourTables(torch.from_numpy(c).to(DEV), 9, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        NeighbourTables(torch.from_numpy(c), 3, False)


def test_neighbour_tables_ignore_the_rows_beyond_the_valid_count():
    """A capacity-padded batch: the rows beyond n_valid hold an earlier batch (events that reuse the numbers of the valid
    ones, the last valid event's included) -- they get deg = 0 and appear in no list."""
    rng = np.random.default_rng(5)
    c = gc.crafted_events()
    nv = len(c)
    stale = gc.event_rows(rng, (4, 6, 3, 7, 5), first_event=int(c[-1, 2]))       # first stale event = last valid number
    full = np.concatenate([c, stale])
    t = dev_tables(full, 3, n_valid=nv)
    nbr, deg = check_tables(t, full, 3, n_valid=nv)
    assert (deg[nv:] == 0).all() and (nbr[nv:] == -1).all() and nbr.max() < nv
    assert (t.rev_pos.cpu().numpy()[nv:, 1] == 0).all()
    cut = 16 + 70                                                                # the count ends inside the grid event
    check_tables(dev_tables(full, 3, n_valid=cut), full, 3, n_valid=cut)
    check_tables(dev_tables(full, 3, n_valid=0), full, 3, n_valid=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("D", [1, 5, 37, 251, 374])
def test_message_kernels_alone(D, k, dtype):
    from waveformml_amd.psd.graphnet import LAUNCHES, film_message
    P, c, nbr, deg, dout = gc.message_case(D, k, dtype, seed=D + k)
    P64 = P.double().requires_grad_(True)
    want = gc.film_messages64(P64, nbr, deg)
    want.backward(dout.double())
    before = dict(LAUNCHES)
    Pg = P.to(DEV).requires_grad_(True)
    got = film_message(Pg, dev_tables(c, k))
    got.backward(dout.to(DEV))
    assert got.dtype == dtype and Pg.grad.dtype == dtype
    assert LAUNCHES["message_fwd"] == before["message_fwd"] + 1 and LAUNCHES["message_bwd"] == before["message_bwd"] + 1
    gc.close(got.detach().float().cpu().numpy(), want.detach().numpy(), TOL[dtype], "out")
    for i, name in enumerate(("ds", "dbs", "dgs", "dh", "db", "dg")):
        gc.close(Pg.grad[:, i * D:(i + 1) * D].float().cpu().numpy(), P64.grad[:, i * D:(i + 1) * D].numpy(), TOL[dtype], name)
    # exact zeros stay masked out on both sides: row 3's skip term, row 7's edges
    assert float(P64.grad[3, :D].abs().max()) == 0.0 and float(Pg.grad[3, :3 * D].abs().max()) == 0.0
    assert float(P64.grad[7, 4 * D:].abs().max()) == 0.0 and float(Pg.grad[7, 4 * D:].abs().max()) == 0.0


def run_small(net, c, x, dtype, w, n_valid=None):
    """(out, dX, {parameter gradient}) of sum(out * w) through the HIP path."""
    net = copy.deepcopy(net).to(DEV).train()
    xg = x.to(dtype).to(DEV).requires_grad_(True)
    data = [torch.from_numpy(c).to(DEV), xg]
    if n_valid is not None:
        data.append(torch.tensor([n_valid], dtype=torch.int64, device=DEV))
    out = net(data)
    loss = (out.float() * w.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), xg.grad, {n: p.grad for n, p in net.named_parameters()}, loss.detach()


@pytest.fixture(scope="module")
def small():
    net, c, x, ref, out, seed, worst = gc.small_net_case()
    return net, c, x, seed, worst


def small_reference(net, c, x, dtype):
    """The float64 run on the inputs rounded to ``dtype``: (out, dX, parameter gradients, loss, w)."""
    ref = gc.RefNet(net.state_dict(), 5, 3)
    x64 = x.to(dtype).double().requires_grad_(True)
    out = ref.forward(c, x64)
    # non-negative weights: the loss is then a sum of non-negative terms (the outputs follow a ReLU), nothing cancels, and
    # it is held to the bar relative to itself
    w = torch.from_numpy(np.abs(np.random.default_rng(77).standard_normal(tuple(out.shape))).astype(np.float32))
    loss = (out * w.double()).sum()
    loss.backward()
    return out.detach(), x64.grad, {n: p.grad for n, p in ref.params.items()}, loss.detach(), w, gc.margin_ok(ref.args)


def test_whole_net_small_plan_fp32_output_and_every_gradient(small):
    net, c, x, seed, worst = small
    out64, dx64, grads64, loss64, w, (ok, margin) = small_reference(net, c, x, torch.float32)
    print("small plan: seed %d, smallest non-zero ReLU argument %.2e of its tensor's scale" % (seed, margin))
    assert ok and 6 <= len(set(c[:, 2])) <= 8 and net.graph_planes == gc.SMALL_PLANES
    out, dx, grads, loss = run_small(net, c, x, torch.float32, w)
    gc.close(out.cpu().numpy(), out64.numpy(), 1e-5, "out")
    assert abs(float(loss) - float(loss64)) <= 1e-5 * abs(float(loss64))
    gc.close(dx.cpu().numpy(), dx64.numpy(), 1e-5, "dX")
    assert sorted(grads) == sorted(grads64) and len(grads) == 5 * 7
    for name in grads64:
        gc.close(grads[name].cpu().numpy(), grads64[name].numpy(), 1e-5, name)
    assert ((out == 0).cpu().numpy() == (out64 == 0).numpy()).all()


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=IDS[1:])
def test_whole_net_small_plan_16_bit_output_and_loss(small, dtype):
    """Outputs and loss of the small plan at the project's 16-bit bars.  fp16 rows run through the layers in fp16; bf16
    rows are widened at the net's input (psd/graphnet.py: bf16 storage between the layers left this output 3.33e-2 away on
    an MI355X, as a float64 model of the format alone does, 3.54e-2) and the result is rounded back to bf16."""
    net, c, x, _seed, _worst = small
    out64, _dx64, _grads64, loss64, w, _margin = small_reference(net, c, x, dtype)
    out, _dx, _grads, loss = run_small(net, c, x, dtype, w)
    assert out.dtype == dtype
    rel = float((out.float().cpu().double() - out64).abs().max() / out64.abs().max())
    print("small plan %s: output error %.3e of the largest magnitude (bar %.1e)" % (dtype, rel, TOL[dtype]))
    gc.close(out.float().cpu().numpy(), out64.numpy(), TOL[dtype], "out")
    assert abs(float(loss) - float(loss64)) <= TOL[dtype] * abs(float(loss64)), (float(loss), float(loss64))


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=IDS[1:])
def test_whole_net_small_plan_16_bit_gradients(small, dtype):
    net, c, x, _seed, _worst = small
    key = IDS[DTYPES.index(dtype)]
    _out64, dx64, grads64, _loss64, w, _margin = small_reference(net, c, x, dtype)
    _out, dx, grads, _loss = run_small(net, c, x, dtype, w)
    worst = {}
    for name, g64 in list(grads64.items()) + [("dX", dx64)]:
        g = dx if name == "dX" else grads[name]
        scale = float(g64.abs().max())
        rel = float((g.double().cpu() - g64).abs().max()) / scale if scale > 0 else 0.0
        worst[name] = rel
    print("16-bit gradient errors (%s): %s" % (key, json.dumps(worst, sort_keys=True)))
    assert sorted(worst) == sorted(GRAD16[key]), "GRAD16 holds no record for this case"
    for name, rel in worst.items():
        assert rel <= 1.5 * GRAD16[key][name], (name, rel, GRAD16[key][name])


def test_padding_rows_change_nothing_and_come_back_as_zeros(small):
    """The small plan behind a device-side count: stale rows of an earlier batch beyond it.  Outputs and gradients equal
    the exact-size run's (the same kernels on the same rows), the padding rows are zeros."""
    net, c, x, _seed, _worst = small
    rng = np.random.default_rng(3)
    stale = gc.event_rows(rng, (5, 4), first_event=int(c[-1, 2]))
    cc = np.concatenate([c, stale])
    xx = torch.cat([x, torch.from_numpy(rng.standard_normal((len(stale), 16)).astype(np.float32)) * 50])
    w = torch.from_numpy(rng.standard_normal((len(cc), 5)).astype(np.float32))
    out, dx, grads, _loss = run_small(net, c, x, torch.float32, w[:len(c)])
    outp, dxp, gradsp, _lossp = run_small(net, cc, xx, torch.float32, w, n_valid=len(c))
    assert float(outp[len(c):].abs().max()) == 0.0
    gc.close(outp[:len(c)].cpu().numpy(), out.cpu().numpy(), 1e-5, "out")
    gc.close(dxp[:len(c)].cpu().numpy(), dx.cpu().numpy(), 1e-5, "dX")
    for name in grads:
        gc.close(gradsp[name].cpu().numpy(), grads[name].cpu().numpy(), 1e-5, name)


def config_module(which, n_samples=None, seed=11):
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litseg import LitSegClassifier
    from waveformml_amd.psd.litsegq import LitSegQuantifier
    cfg = json.load(open(CONFIGS[which]))
    if n_samples is not None:
        cfg["system_config"]["n_samples"] = n_samples
    torch.manual_seed(seed)
    return (LitSegClassifier if which == "classifier" else LitSegQuantifier)(load_config(cfg)), cfg


def reference_loss(which, module, out64, c, target):
    """The module's loss in float64 from the restatement's output: the mean cross-entropy over all rows, or the mean
    |prediction - target[:, 4]| over the rows of single-ended segments."""
    if which == "classifier":
        return torch.nn.functional.cross_entropy(out64, target)
    se = module.SE_mask[0, 0, torch.from_numpy(c[:, 0]).long(), torch.from_numpy(c[:, 1]).long()].cpu() == 1.0
    assert 0 < int(se.sum()) < len(c)
    return (out64.squeeze(1) - target[:, 4].double()).abs()[se].mean()


def module_batch(which, rng, n_rows_sizes, width):
    c = gc.event_rows(rng, n_rows_sizes)
    f = torch.from_numpy(rng.standard_normal((len(c), width)).astype(np.float32))
    if which == "classifier":
        y = torch.from_numpy(rng.integers(0, 5, len(c)))
    else:
        y = torch.from_numpy(rng.random((len(c), 8)).astype(np.float32))
    return c, f, y


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["classifier", "quantifier"])
def test_whole_net_at_the_config_widths(which, dtype):
    """Both configs' plans at about 40 rows: output and loss against float64; the output is live; the HIP path ran."""
    from waveformml_amd.psd import graphnet
    module, _cfg = config_module(which)
    rng = np.random.default_rng(31)
    c, f, y = module_batch(which, rng, (1, 6, 4, 7, 2, 5, 6, 3, 6), 130)
    assert len(c) == 40
    ref = gc.RefNet(module.model.state_dict(), 5, 3)
    out64 = ref.forward(c, f.to(dtype).double()).detach()
    loss64 = reference_loss(which, module, out64, c, y)
    before = dict(graphnet.LAUNCHES)
    module = module.to(DEV).train()
    out = module.model([torch.from_numpy(c).to(DEV), f.to(dtype).to(DEV)])
    assert out.dtype == dtype and tuple(out.shape) == (40, 5 if which == "classifier" else 1)
    gc.close(out.detach().float().cpu().numpy(), out64.numpy(), TOL[dtype], "out")
    loss = module.training_step(([torch.from_numpy(c).to(DEV), f.to(dtype).to(DEV)], y.to(DEV)), 0)
    print("%s %s: loss %.8g, float64 %.8g" % (which, dtype, loss.item(), float(loss64)))
    assert abs(loss.item() - float(loss64)) <= TOL[dtype] * abs(float(loss64)), (loss.item(), float(loss64))
    # live: the final ReLU leaves zeros and non-zeros, on both sides in the same places (up to the bar)
    zero64 = (out64 == 0).numpy()
    assert 0.5 < zero64.mean() < 0.8, zero64.mean()          # default initialisation: 60-70 % (40 or 200 outputs)
    assert (out64 != 0).any()
    got = out.detach().float().cpu().numpy()
    scale = float(out64.abs().max())
    assert (np.abs(got[zero64]) <= TOL[dtype] * scale).all()
    assert (got[np.abs(out64.numpy()) > TOL[dtype] * scale] != 0).all()
    # the HIP path: one table build, one message launch per layer and call, and nothing else to fall back to
    assert graphnet.LAUNCHES["knn"] == before["knn"] + 2 and graphnet.LAUNCHES["message_fwd"] == before["message_fwd"] + 10


def test_event_max_head_under_one_label_per_event():
    """n_lin = 2: per-event max over the rows, then the LinearBlock; one label per event as LitPSD hands them.  An event
    number without rows in the middle (2) and one at the end give zero rows and pass no gradient; two rows of event 1 are
    alike, so every maximum they reach is tied and the first row takes the gradient."""
    from waveformml_amd.psd.graphnet import LAUNCHES, event_max
    net, c, x, ref, out64, seed, _worst = gc.small_net_case(n_lin=2, skip={2}, tie=True)
    B = int(c[-1, 2]) + 2
    assert tuple(out64.shape) == (B, 3)
    y = torch.from_numpy(np.random.default_rng(9).integers(0, 3, B))
    x64 = x.double().requires_grad_(True)
    ref = gc.RefNet(net.state_dict(), 5, 3, n_lin=2)
    loss64 = torch.nn.functional.cross_entropy(ref.forward(c, x64, batch_size=B), y)
    loss64.backward()
    assert gc.margin_ok(ref.args)[0]
    gnet = copy.deepcopy(net).to(DEV).train()
    gnet.batch_size_hint = B
    xg = x.to(DEV).requires_grad_(True)
    before = dict(LAUNCHES)
    out = gnet([torch.from_numpy(c).to(DEV), xg])
    loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
    loss.backward()
    assert LAUNCHES["event_max_fwd"] == before["event_max_fwd"] + 1 and LAUNCHES["event_max_bwd"] == before["event_max_bwd"] + 1
    gc.close(out.detach().cpu().numpy(), out64.detach().numpy(), 1e-5, "logits")
    assert abs(loss.item() - float(loss64)) <= 1e-5 * abs(float(loss64))
    gc.close(xg.grad.cpu().numpy(), x64.grad.numpy(), 1e-5, "dX")
    for name, p in gnet.named_parameters():
        gc.close(p.grad.cpu().numpy(), ref.params[name].grad.numpy(), 1e-5, name)
    # the pooling alone: ties, an empty event, rows beyond a device-side count
    rows = torch.tensor([[1., 5.], [1., 7.], [0., 7.], [9., 9.]], device=DEV, requires_grad=True)
    cc = torch.tensor([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 1]], dtype=torch.int32, device=DEV)
    nv = torch.tensor([3], dtype=torch.int64, device=DEV)
    ymax, arg = event_max(rows, cc, 3, nv)
    assert ymax.tolist() == [[1., 7.], [0., 0.], [0., 0.]] and arg.tolist() == [[0, 1], [-1, -1], [-1, -1]]
    ymax.sum().backward()
    assert rows.grad.tolist() == [[1., 0.], [0., 1.], [0., 0.], [0., 0.]]
    with pytest.raises(RuntimeError, match="batch_size_hint"):
        gnet.batch_size_hint = None
        gnet([torch.from_numpy(c).to(DEV), xg, torch.tensor([len(c)], dtype=torch.int64, device=DEV)])


def test_two_runs_are_bit_identical(small):
    net, c, x, _seed, _worst = small
    w = torch.from_numpy(np.random.default_rng(1).standard_normal((len(c), 5)).astype(np.float32))
    for dtype in DTYPES:
        a = run_small(net, c, x, dtype, w)
        b = run_small(net, c, x, dtype, w)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
        for name in a[2]:
            assert torch.equal(a[2][name], b[2][name]), name


@pytest.mark.parametrize("which", ["classifier", "quantifier"])
def test_lightning_module_eager_step_against_the_restatement(which):
    """One training step of the module built from the new config: at the config's widths the loss, on the small plan
    (n_samples = 8, a seed whose float64 run keeps the ReLU margin) the loss and every parameter gradient."""
    graph_out = 5 if which == "classifier" else 1
    net, c, x, _ref, _out, seed, _worst = gc.small_net_case(graph_out=graph_out, first_seed=100)
    module, _cfg = config_module(which, n_samples=8)
    module.model.load_state_dict(net.state_dict())
    rng = np.random.default_rng(41)
    y = torch.from_numpy(rng.integers(0, 5, len(c))) if which == "classifier" else \
        torch.from_numpy(rng.random((len(c), 8)).astype(np.float32))
    ref = gc.RefNet(net.state_dict(), 5, 3)
    loss64 = reference_loss(which, module, ref.forward(c, x.double()), c, y)
    loss64.backward()
    module = module.to(DEV).train()
    loss = module.training_step(([torch.from_numpy(c).to(DEV), x.to(DEV)], y.to(DEV)), 0)
    loss.backward()
    assert abs(float(loss) - float(loss64)) <= 1e-5 * abs(float(loss64)), (float(loss), float(loss64))
    for name, p in module.model.named_parameters():
        gc.close(p.grad.cpu().numpy(), ref.params[name].grad.numpy(), 1e-5, name)
    # the config's own widths: the loss
    module, _cfg = config_module(which)
    c, f, y = module_batch(which, np.random.default_rng(43), (3, 6, 1, 7, 5, 6, 4, 6, 2), 130)
    ref = gc.RefNet(module.model.state_dict(), 5, 3)
    loss64 = reference_loss(which, module, ref.forward(c, f.double()).detach(), c, y)
    module = module.to(DEV).train()
    loss = module.training_step(([torch.from_numpy(c).to(DEV), f.to(DEV)], y.to(DEV)), 0)
    assert abs(float(loss) - float(loss64)) <= 1e-5 * abs(float(loss64)), (float(loss), float(loss64))


def one_step(which, capture, c, f, y, n_samples=None, state=None):
    """(loss, every parameter after the step, eager fallbacks) of one Trainer step on one batch."""
    from waveformml_amd.psd.trainer import Trainer
    module, _cfg = config_module(which, n_samples=n_samples, seed=13)
    if state is not None:
        module.model.load_state_dict(state)
    tr = Trainer(max_epochs=1, device=DEV, capture=capture, check_every=1)
    hist = tr.fit(module, [([torch.from_numpy(c).clone(), f.clone()], y.clone())])
    torch.cuda.synchronize()
    return hist[0]["train_loss"], {n: p.detach().cpu() for n, p in module.model.named_parameters()}, tr.eager_fallbacks


@pytest.mark.parametrize("which", ["classifier", "quantifier"])
def test_captured_step_on_a_padded_batch_equals_the_eager_step(which):
    """GraphedTrainStep pads rows and targets to its capacity.  One captured step on the padded batch against one eager
    step on the batch as it is, no eager fallback: at the config's widths the loss at the fp32 bar; the parameters after
    the step on the small plan, with a seed whose float64 run keeps every ReLU argument outside the margin -- the two
    steps sum in different orders, and at the config's widths some argument always lies inside it (what they differ by
    there was measured on an MI355X and is asserted at 1.5 x the record, WIDE_STEP)."""
    rng = np.random.default_rng(51)
    c, f, y = module_batch(which, rng, (6, 3, 7, 1, 5, 6, 4, 2, 6), 130)
    loss0, p0, _ = one_step(which, False, c, f, y)
    loss1, p1, fallbacks = one_step(which, True, c, f, y)
    assert fallbacks == 0 and abs(loss0 - loss1) <= 1e-5 * abs(loss0), (loss0, loss1)
    wide = max(float((p1[n] - p0[n]).abs().max() / p0[n].abs().max()) for n in p0)
    print("%s at the config's widths: parameters after one step differ by at most %.3e of a tensor's largest" % (which, wide))
    assert wide <= 1.5 * WIDE_STEP[which], (wide, WIDE_STEP[which])
    net, c, x, _ref, _out, _seed, _worst = gc.small_net_case(graph_out=5 if which == "classifier" else 1, first_seed=100)
    y = torch.from_numpy(rng.integers(0, 5, len(c))) if which == "classifier" else \
        torch.from_numpy(rng.random((len(c), 8)).astype(np.float32))
    loss0, p0, _ = one_step(which, False, c, x, y, n_samples=8, state=net.state_dict())
    loss1, p1, fallbacks = one_step(which, True, c, x, y, n_samples=8, state=net.state_dict())
    assert fallbacks == 0 and abs(loss0 - loss1) <= 1e-5 * abs(loss0), (loss0, loss1)
    for name in p0:
        gc.close(p1[name].numpy(), p0[name].numpy(), 1e-5, name)


@pytest.mark.parametrize("which", ["classifier", "quantifier"])
def test_trainer_captures_both_configs_from_files_with_a_falling_loss(which):
    """Trainer(capture=True) over the ioni130 fixture: per-row PID classes for the classifier, the per-row physics rows
    (scored on column 4 over the single-ended segments) for the quantifier."""
    from torch.utils.data import DataLoader
    from waveformml_amd.psd import data as psd_data, h5data
    from waveformml_amd.psd.trainer import Trainer
    root = os.path.join(ROOT, "tests", "golden", "h5", "r3", "ioni130")
    labels = dict(label_name="PID", label_map={"1": 0, "4": 1, "6": 2, "256": 3, "258": 2, "512": 4}) \
        if which == "classifier" else dict(label_name="phys")
    ds = h5data.HDF5Dataset([root], "*WaveformPairSim.h5", "WaveformPairs", "coord", "waveform", 39, normalize=True, **labels)
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=psd_data.collate_fn)
    batches = sorted(list(loader), key=lambda b: -b[0][0].shape[0])          # the capture sizes itself on its first batch
    module, _cfg = config_module(which, seed=7)
    module.lr = 0.01
    tr = Trainer(max_epochs=4, device=DEV, capture=True, check_every=2)
    hist = tr.fit(module, [([c.clone(), f.clone()], y.clone()) for (c, f), y in batches])
    torch.cuda.synchronize()
    losses = [h["train_loss"] for h in hist]
    print("captured %s losses per epoch:" % which, losses)
    assert tr.eager_fallbacks == 0 and all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_segment_test_loops_run_with_both_evaluators():
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.pid_evaluator import PIDEvaluator
    from waveformml_amd.psd.quantifier_evaluator import SegEvaluator
    rng = np.random.default_rng(61)
    for which, cls, field in (("classifier", PIDEvaluator, "phys"), ("quantifier", SegEvaluator, "PID")):
        module, _cfg = config_module(which)
        module = module.to(DEV)
        loader = []
        for sizes in ((5, 6, 3, 6, 4), (6, 2, 7)):
            c, f, y = module_batch(which, rng, sizes, 130)
            extra = torch.from_numpy(rng.random((len(c), 8)).astype(np.float32)) if field == "phys" else \
                torch.from_numpy(np.array([1, 4, 6, 258, 256, 512, 3])[rng.integers(0, 7, len(c))])
            loader.append(([torch.from_numpy(c), [f, extra]], y))
        ev = module.evaluator
        assert isinstance(ev, cls) and ev.additional_field_names == [field]
        out = segment_test_loop(module, copy.deepcopy(loader), DEV, evaluator=ev)
        assert out["rows"] == sum(len(b[0][0]) for b in loader) and np.isfinite(out["test_loss"])
        assert "evaluation" in out and len(out["evaluation"]) > 0
