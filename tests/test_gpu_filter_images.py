"""Filter images (include/wfsparse.h "filter images"): the 16-bit LDS image of a 32 -> 32 layer's fp32 filter, made once
per step and handed to the conv launches, whose blocks copy it into LDS instead of converting the filter.

The image holds the bits the kernels compute themselves and neither the products nor their order change, so every
comparison here is for bit identity:
  1. the images against the layout formula in NumPy;
  2. forward, dX and the one-launch backward with the image against the same call without one;
  3. the hand-over launch with image jobs against wfs_load_batch plus the stand-alone image entry;
  4. three replays of a captured training step with the images on and off.

Row counts of (2), from gconv32_grid (csrc/conv_mfma.hip) with a device-side count: a capacity of 3200 rows is 100 tiles
of 32 rows, sized for 7/8 of them = 88 -> 4 waves per block, 24 blocks, 3 blocks and 12 wave slots per XCD.  The VALID
tiles are cut into 8 XCD ranges of ceil(tiles / 8):
    3190 valid rows   100 tiles, 13 per range: the first slot of a range takes a second tile; the last range holds 9, so
                      wave 3 of its blocks has none
     300 valid rows   10 tiles, 2 per range: the third block of every range and every block of ranges 5 .. 7 have no tile
       0              no block has a tile
Capacities 1 and 33 are one tile and one row past a tile (8 blocks, seven or six of them without a tile).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import conv32_cases as cc          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}
SENT = -768.0                      # exactly representable in bf16 and fp16
COUNTS = {1: (1, 0), 33: (33, 20, 0), 3200: (3190, 300, 0)}


def _L():
    from waveformml_amd import _lib
    return _lib


def _images(W, kind, fwd=True, t=True):
    """(forward image, dX image) of W [K, 32, 32] from the stand-alone entry, as uint8 tensors; None where not asked."""
    L = _L()
    lib = L.load()
    K = int(W.shape[0])
    n = int(lib.wfs_filter_image_bytes(K))
    assert n == K * 2048
    imgs = [torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV) if want else None for want in (fwd, t)]
    code = L.WFS_BF16 if kind == "bf16" else L.WFS_F16
    L.check(lib.wfs_conv_filter_images(L.ptr(W), K, code, L.ptr(imgs[0]), L.ptr(imgs[1]), L.stream_ptr()))
    return imgs


def _image_formula(W, kind):
    """img[k][s][h][col][j] = H(B[16h + 8s + j][col]), B = W[k] / W[k]^T, as int16 arrays [K * 128 * 8]."""
    K = W.shape[0]
    H = torch.from_numpy(W).to(TORCH[kind]).view(torch.int16).numpy()              # torch's round to nearest even
    fwd = H.reshape(K, 2, 2, 8, 32).transpose(0, 2, 1, 4, 3)                        # [k, h, s, j, col] -> [k, s, h, col, j]
    t = H.reshape(K, 32, 2, 2, 8).transpose(0, 3, 2, 1, 4)                          # [k, col, h, s, j] -> [k, s, h, col, j]
    return np.ascontiguousarray(fwd).reshape(-1), np.ascontiguousarray(t).reshape(-1)


# ---------------------------------------------------------------------------------------------------- 1. image contents
@pytest.mark.parametrize("K", [27, 9])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_images_hold_the_layout_formula(kind, K):
    rng = np.random.default_rng(100 + K)
    W = (rng.standard_normal((K, 32, 32)) * 0.25).astype(np.float32)
    W[0, 0, :4] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9]                 # ties and signed zero
    # the filter as a captured step holds it: a view into a flat parameter buffer, 4-byte aligned only
    flat = torch.zeros((W.size + 1,), dtype=torch.float32, device=DEV)
    Wd = flat[1:].view(K, 32, 32)
    Wd.copy_(torch.from_numpy(W))
    assert Wd.data_ptr() % 16 == 4
    want = _image_formula(W, kind)
    both = _images(Wd, kind)
    for got, ref in zip(both, want):
        assert np.array_equal(got.view(torch.int16).cpu().numpy(), ref)
    # either image may be NULL: the other one is the same, the NULL one is simply not written
    only_f, none_t = _images(Wd, kind, t=False)
    none_f, only_t = _images(Wd, kind, fwd=False)
    assert none_t is None and none_f is None
    assert torch.equal(only_f, both[0]) and torch.equal(only_t, both[1])


# ------------------------------------------------------------------------------------------------ 2. with image vs NULL
def _problem(kind, R, valid, arm, seed):
    """Tables, rows and filters of one call on the device.  arm: (op, table form, identity_k)."""
    op, form, ik = arm
    rng = np.random.default_rng(seed)
    K = 27
    src = R if ik >= 0 else R + 29
    table, _facts = cc.build_table(rng, "subm" if ik >= 0 else "random", K, R, valid, min(src, max(valid, 1)) if ik >= 0 else src,
                                   ik, form == "packed")
    d = dict(K=K, R=R, ik=ik, pk=cc.PACKED_KL if form == "packed" else 0)
    d["table"] = torch.from_numpy(cc.encode_packed(table) if form == "packed" else table).to(DEV)
    d["kmap"] = _L().i32_array([K - 1 - k for k in range(K)]) if form == "mirror" else None
    d["G"] = torch.from_numpy(rng.standard_normal((src, 32)).astype(np.float32)).to(DEV).to(TORCH[kind])    # gathered rows
    d["S"] = torch.from_numpy(rng.standard_normal((R, 32)).astype(np.float32)).to(DEV).to(TORCH[kind])      # stationary rows
    d["W"] = torch.from_numpy((rng.standard_normal((K, 32, 32)) * 0.25).astype(np.float32)).to(DEV)
    d["bias"] = torch.from_numpy(rng.standard_normal(32).astype(np.float32)).to(DEV) if op == "fwd" else None
    d["r_dev"] = torch.tensor([valid], dtype=torch.int64, device=DEV)
    return d


def _call(op, d, kind, image):
    """One call through the C ABI into sentinel-filled outputs; ``image`` None = the plain entry's route (NULL)."""
    L = _L()
    lib = L.load()
    out = torch.full((d["R"], 32), SENT, dtype=TORCH[kind], device=DEV)
    if op in ("fwd", "dx"):
        L.check(lib.wfs_gather_conv_image(L.ptr(d["table"]), d["kmap"], d["K"], d["ik"], d["R"], L.ptr(d["G"]),
                                          d["G"].shape[0], 32, L.ptr(d["W"]), 32, 32, 1 if op == "dx" else 0,
                                          L.ptr(d["bias"]), L.ptr(out), L.dtype_code(d["G"]), L.ptr(d["r_dev"]), d["pk"],
                                          L.ptr(image), L.stream_ptr()))
        return (out,)
    dW = torch.full((d["K"], 32, 32), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty((max(int(lib.wfs_gather_dw_workspace_bytes(d["K"], d["R"], 32, 32)), 1),), dtype=torch.uint8, device=DEV)
    L.check(lib.wfs_conv_backward_image(L.ptr(d["table"]), d["K"], d["ik"], d["R"], L.ptr(d["S"]), L.ptr(d["G"]),
                                        d["G"].shape[0], 32, 32, L.ptr(d["W"]), L.ptr(out), L.ptr(dW), L.dtype_code(d["S"]),
                                        L.ptr(ws), ws.numel(), L.ptr(d["r_dev"]), None, d["pk"], L.ptr(image),
                                        L.stream_ptr()))
    return out, dW


ARMS = [("fwd", "dense", -1), ("fwd", "mirror", 13), ("dx", "dense", -1), ("dx", "packed", -1), ("dx", "dense", 13),
        ("bwd", "dense", -1), ("bwd", "packed", -1), ("bwd", "dense", 13)]


@pytest.mark.parametrize("R", sorted(COUNTS))
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_calls_with_an_image_equal_the_calls_without(kind, R):
    for valid in COUNTS[R]:
        for n, arm in enumerate(ARMS):
            op = arm[0]
            d = _problem(kind, R, valid, arm, seed=1000 * R + 10 * valid + n)
            img_f, img_t = _images(d["W"], kind)
            image = img_f if op == "fwd" else img_t
            plain = _call(op, d, kind, None)
            what = "%s %s R %d valid %d" % (kind, arm, R, valid)
            rows = plain[0].float()
            assert bool((rows[valid:] == SENT).all()), what + ": a row at or beyond the valid count was written"
            assert valid == 0 or bool(torch.isfinite(rows[:valid]).all() and (rows[:valid] != SENT).any()), what
            for rerun in range(2):              # run-to-run: a fragment read before its copy landed would differ
                got = _call(op, d, kind, image)
                for a, b in zip(got, plain):
                    assert torch.equal(a.view(torch.int16) if a.dtype != torch.float32 else a.view(torch.int32),
                                       b.view(torch.int16) if b.dtype != torch.float32 else b.view(torch.int32)), \
                        "%s (run %d)" % (what, rerun)


# ------------------------------------------------------------------------------------------------------ 3. hand-over form
def test_hand_over_with_jobs_equals_the_plain_hand_over_and_the_stand_alone_images():
    L = _L()
    lib = L.load()
    rng = np.random.default_rng(7)
    n, B, ncap = 1500, 8, 2000
    ev = np.sort(rng.integers(0, B, n)).astype(np.int32)
    coords = np.stack([rng.integers(0, 14, n), rng.integers(0, 11, n), rng.integers(0, 64, n), ev], axis=1).astype(np.int32)
    feats = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    labels = torch.from_numpy(rng.integers(0, 3, B).astype(np.int64)).to(DEV)
    cd = torch.from_numpy(coords).to(DEV)
    perm = L.i32_array([3, 0, 1, 2])
    Ws = [torch.from_numpy((rng.standard_normal((K, 32, 32)) * 0.25).astype(np.float32)).to(DEV) for K in (27, 9, 27)]
    kinds = ["bf16", "f16", "bf16"]

    def run(jobs):
        dst = dict(coords=torch.full((ncap, 4), -7, dtype=torch.int32, device=DEV),
                   indices=torch.full((ncap, 4), -7, dtype=torch.int32, device=DEV),
                   feats=torch.full((ncap, 2), SENT, dtype=torch.bfloat16, device=DEV),
                   labels=torch.full((B,), -7, dtype=torch.int64, device=DEV),
                   n_valid=torch.full((1,), -7, dtype=torch.int64, device=DEV),
                   events=torch.full((int(lib.wfs_event_offsets_ints(B)),), -7, dtype=torch.int32, device=DEV))
        args = (L.ptr(cd), n, 4, perm, L.ptr(dst["coords"]), L.ptr(dst["indices"]), L.ptr(feats), L.ptr(dst["feats"]),
                feats.numel() * 2, L.ptr(labels), L.ptr(dst["labels"]), B, L.ptr(dst["n_valid"]), L.ptr(dst["events"]), B)
        if jobs == "plain":
            L.check(lib.wfs_load_batch(*args, L.stream_ptr()))
        else:
            L.check(lib.wfs_load_batch_images(*args, jobs, 0 if jobs is None else len(jobs), L.stream_ptr()))
        return dst

    imgs = [[torch.full((W.shape[0] * 2048,), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(2)] for W in Ws]
    imgs[2][0] = None                                   # a job may leave either image out
    jobs = (L.FilterImageJob * len(Ws))()
    for job, W, kind, (f, t) in zip(jobs, Ws, kinds, imgs):
        job.W, job.img_fwd, job.img_t, job.K = W.data_ptr(), L.ptr(f), L.ptr(t), int(W.shape[0])
        job.dtype = L.WFS_BF16 if kind == "bf16" else L.WFS_F16
    plain, with_jobs, zero_jobs = run("plain"), run(jobs), run(None)
    assert int(plain["n_valid"].item()) == n and bool((plain["coords"][:n] == cd).all())
    for k in plain:
        assert torch.equal(plain[k], with_jobs[k]), k
        assert torch.equal(plain[k], zero_jobs[k]), k
    for W, kind, (f, t) in zip(Ws, kinds, imgs):
        want_f, want_t = _images(W, kind)
        assert f is None or torch.equal(f, want_f)
        assert torch.equal(t, want_t)
    # more jobs than the launch takes, or a filter that is not 32 x 32 x K <= 32: refused, nothing launched
    assert lib.wfs_load_batch_images(*([None, 0, 4, None] + [None] * 4 + [0, None, None, 0, None, None, 0]),
                                     (L.FilterImageJob * 17)(), 17, L.stream_ptr()) != 0
    assert lib.wfs_conv_filter_images(L.ptr(Ws[0]), 33, L.WFS_BF16, L.ptr(imgs[0][0]), None, L.stream_ptr()) != 0
    assert lib.wfs_conv_filter_images(L.ptr(Ws[0]), 27, L.WFS_F32, L.ptr(imgs[0][0]), None, L.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------ 4. captured step
def _c2_module(T, seed=11):
    import copy
    import json
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    cfg = json.load(open(os.path.join(os.path.dirname(HERE), "config", "psd_c2_3d.json")))
    cfg["system_config"]["n_samples"] = T
    cfg["net_config"]["algorithm"][-1] = [32 * 10 * 7 * (T // 16), 3]
    torch.manual_seed(seed)
    return LitPSD(DictionaryUtility.to_object(copy.deepcopy(cfg)))


def _state(mod, loss):
    out = {"loss": loss.detach().clone()}
    out.update({"p." + k: v.detach().clone() for k, v in mod.model.named_parameters()})
    out.update({"b." + k: v.detach().clone() for k, v in mod.model.named_buffers()})
    return out


def test_captured_step_is_bit_identical_with_and_without_images(monkeypatch):
    from waveformml_amd.psd import synthetic
    from waveformml_amd.psd.ddp import FlatGradAllReducer
    from waveformml_amd.psd.graph import GraphedTrainStep
    from waveformml_amd.spconv import ops
    from waveformml_amd.spconv.conv import SparseConvolution
    T, B = 64, 4
    batches = []
    for seed in (5, 6, 7):
        c, f, y = synthetic.generate(B, T, 3, seed=seed)
        batches.append(([torch.from_numpy(c).to(DEV), torch.from_numpy(f).to(DEV).to(torch.bfloat16)],
                        torch.from_numpy(y).to(DEV)))
    example = max(batches, key=lambda b: b[0][0].shape[0])
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "FILTER_IMAGES", on)
        mod = _c2_module(T).to(DEV)
        mod.train()
        red = FlatGradAllReducer(mod.model.parameters(), world_size=1)
        mod.optimizer_parameters = red.optimizer_parameters()
        opt = mod.configure_optimizers()[0][0]
        step = GraphedTrainStep(mod, opt, red, example, warmup=2)
        convs = [m for m in mod.modules() if isinstance(m, SparseConvolution) and m.in_channels == 32]
        assert len(step._images) == (len(convs) if on else 0) and len(convs) >= 2
        assert all(m.filter_images is None for m in convs), "the images are live only inside the runner's own step"
        assert not any("filter_images" in k for k in mod.state_dict())
        states = []
        for i, batch in enumerate(batches):
            if i == 2:
                # a weight changed from outside between two replays (a checkpoint, another optimizer): the next
                # hand-over makes the images from it
                with torch.no_grad():
                    convs[1].weight.mul_(-0.5)
            loss = step(batch)
            step.check()
            torch.cuda.synchronize()
            states.append(_state(mod, loss))
        step.close()
        runs[on] = states
    for i, (a, b) in enumerate(zip(runs[True], runs[False])):
        assert bool(torch.isfinite(a["loss"]).all())
        for k in a:
            assert torch.equal(a[k], b[k]), "replay %d: %s" % (i, k)
    assert not torch.equal(runs[True][1]["loss"], runs[True][2]["loss"])
