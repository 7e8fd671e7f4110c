"""Cost of the calibrated z / E baseline inside the LitZ test loop (psd/evaluate.segment_test_loop, a SingleEndedZConv on
150-sample waveform pairs; fp32 rows, synthetic batches of 256 events / about 765 rows), of the reconstruction kernel
alone, and the split of a calibrated ``add`` over its launches; no kernel trace:

  none        the loop without an evaluator
  plain       the loop + psd/segment_evaluator.ZEvaluator without a calibration (two launches per batch)
  calibrated  the loop + ZEvaluator(calibration=...) (wfs_calib_z_E, then the two launches of wfs_seg_z_accumulate_cal)
  host        the loop + the path the reference takes: predictions, targets, coordinates and waveform rows to the host, the
              reconstruction and the tables there.  The CPU side is a row-by-row PYTHON restatement of calc_calib_z_E
              (NumPy inside a row: argrelmax-style peak search, np.interp curves) and np.add.at tables.  The reference
              compiles its row walks with numba, so this arm PENALISES the host: read it as the cost of the reference's
              algorithm without its compiler, not as the reference's own time.
  kernel      wfs_calib_z_E alone (HIP events around back-to-back calls) at about 765 and 86 k rows, with the bytes per
              second it achieves against the row bytes it must read (rows x 2 L x 4); k_align_pulses, which reads the same
              rows once, is at 509 GB/s at 86.5 k rows (profiles/z_real_evaluator_ab.txt)
  split       a calibrated add at about 765 rows: the whole add, the reconstruction alone, the accumulate call alone

The loop arms run in ONE process, alternating, `rounds` times; the figure per arm is the median over rounds and the
spread is (max - min) over rounds.  The kernel figures are the median and spread of `rounds` windows of 100 calls (20 at
86 k rows).  Every timed window ends in a device synchronise.

usage: python tools/bench_calibrated_z.py [--batches 8] [--loops 4] [--rounds 7] [--out FILE] [--profile FILE]
prints one JSON line; --out appends it to FILE; --profile writes profiles/calibrated_z_ab.txt's text to FILE"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 150


def z_config():
    return {"system_config": {"model_name": "SingleEndedZConv", "n_samples": L, "gpu_enabled": True, "half_precision": 0},
            "net_config": {"criterion_class": "L1Loss", "criterion_params": [],
                           "imports": ["torch.nn", "waveformml_amd.spconv"], "net_type": "2DConvolution",
                           "algorithm": "conv", "hparams": {"conv": {"kernel_size": 3, "n_layers": 3},
                                                            "point": {"pointwise_layers": 2}}},
            "optimize_config": {"imports": ["torch.optim"], "lr": 0.01, "optimizer_class": "optim.SGD",
                                "optimizer_params": {"momentum": 0.9}},
            "dataset_config": {"imports": []}}


def synthetic_curves(np, seed=3):
    """Curves shaped like real ones (the recipe of tests/golden/make_calibrated_z_goldens.py, vectorised)."""
    from waveformml_amd.psd.calibration import CalibrationCurves
    rng = np.random.default_rng(seed)
    has = rng.random((14, 11, 2)) < 0.6
    xs = np.linspace(0., 4., 50)
    tint = np.zeros((14, 11, 2, 50, 2))
    tint[..., 0] = np.where(has[..., None], xs, 0.)
    tint[..., 1] = np.where(has[..., None], xs + rng.uniform(0.1, 0.4, (14, 11, 2, 1)) * np.sin(np.pi * xs / 4.), 0.)
    dts, R, zs = np.linspace(-14., 14., 50), np.linspace(-4., 4., 51), np.linspace(-600., 600., 50)
    tpos = np.stack(np.broadcast_arrays(dts, rng.uniform(55., 65., (14, 11, 1)) * dts), axis=-1)
    lpos = np.stack(np.broadcast_arrays(R, rng.uniform(380., 420., (14, 11, 1)) * R), axis=-1)
    lsum = np.stack(np.broadcast_arrays(zs, rng.uniform(250., 350., (14, 11, 1)) * (1. + 0.25 * (zs / 600.) ** 2)), axis=-1)
    return CalibrationCurves(gains=rng.uniform(300., 600., (14, 11, 2)), eres=rng.uniform(80., 120., (14, 11, 2)),
                             rel_times=rng.uniform(-2., 2., (14, 11)), sampletime=np.where(has, 4., 0.), t_interp_curves=tint,
                             time_pos_curves=tpos, light_pos_curves=lpos, light_sum_curves=lsum)


class HostCalibratedZ:
    """add() as the reference's: four tensors to the host, calc_calib_z_E row by row in Python, np.add.at tables."""

    def __init__(self, ev):
        import numpy as np
        self.np, self.ev, self.cal = np, ev, ev.calibration
        self.gf = self.cal.gain_factor
        self.seg = ev.seg_status.cpu().numpy()
        self.tab = [np.zeros((14, 11, ev.nmult + 1)) for _ in range(2)]

    def _peaks(self, v):
        np = self.np
        d = np.sign(np.diff(v))
        nz = np.flatnonzero(d)
        if len(nz) < 2:
            return []
        turn = np.flatnonzero((d[nz][:-1] > 0) & (d[nz][1:] < 0))
        loc = ((nz[turn] + 1 + nz[turn + 1]) // 2)[:50]
        loc = loc[np.argsort(-v[loc], kind="stable")]
        kept = []
        for p in loc:
            if all(abs(int(p) - q) > 20 for q in kept):
                kept.append(int(p))
            if len(kept) == 5:
                break
        kept = [p for p in kept if v[p] * 16383. > 30.]
        return [] if len(kept) == 5 else sorted(kept, reverse=True)

    def _arrival(self, v, p):
        th = 0.5 * v[p]
        below = self.np.flatnonzero(v[:p] < th)
        if not len(below):
            return th / v[0] if p else 0.5
        s = below[-1]
        return s + 1 + (th - v[s]) / (v[s + 1] - v[s])

    def _pair(self, wf, m0, m1, x, y):
        np, c, t, Ls = self.np, self.cal, [], []
        for i, (m, v) in enumerate(((m0, wf[:L]), (m1, wf[L:]))):
            ti = self._arrival(v, m) * 4.
            if c.t_interp_curves[x, y, i, 10, 0] != 0:
                st = c.sampletime[x, y, i]
                t0 = st * np.floor(ti / st)
                ti = t0 + np.interp(ti - t0, c.t_interp_curves[x, y, i, :, 0], c.t_interp_curves[x, y, i, :, 1])
            t.append(ti)
            Ls.append(v[max(m - 3, 0):m + 26].sum() * self.gf[x, y, i])
        return t[1] - t[0] - c.rel_times[x, y], Ls

    def _light(self, L0, L1, x, y):
        np, c = self.np, self.cal
        PE = [L0 * c.eres[x, y, 0], L1 * c.eres[x, y, 1]]
        with np.errstate(all="ignore"):
            R = np.log(L1 / L0)
        lp = c.light_pos_curves[x, y]
        if R != R:
            return 0., 0., PE
        dR = np.sqrt(1. / max(PE[0], 1.) + 1. / max(PE[1], 1.))
        d = abs(np.interp(R + 0.5 * dR, lp[:, 0], lp[:, 1]) - np.interp(R - 0.5 * dR, lp[:, 0], lp[:, 1]))
        return np.interp(R, lp[:, 0], lp[:, 1]), (1. / (d * d) if d > 0 else 0.), PE

    def _row(self, wf, x, y):
        np, c = self.np, self.cal
        p0, p1 = self._peaks(wf[:L]), self._peaks(wf[L:])
        ls = c.light_sum_curves[x, y]
        if not p0 and not p1:
            return 0.
        if not p0 or not p1:
            return 0.5
        tw = 1. / 3600.
        if len(p0) == len(p1):
            zw = area = 0.
            for m0, m1 in zip(p0, p1):
                dt, (L0, L1) = self._pair(wf, m0, m1, x, y)
                tpos = np.interp(dt, c.time_pos_curves[x, y, :, 0], c.time_pos_curves[x, y, :, 1])
                if L0 == 0 or L1 == 0:
                    z, E = 0., (L0 + L1) / np.interp(0., ls[:, 0], ls[:, 1])
                else:
                    Rpos, Rw, PE = self._light(L0, L1, x, y)
                    z = float(np.clip((Rw * Rpos + tw * tpos) / (Rw + tw), -650., 650.))
                    E = (PE[0] + PE[1]) / np.interp(z, ls[:, 0], ls[:, 1])
                zw, area = zw + z * E, area + E
            return zw / area / 1200. + 0.5
        small, large, swap = (p0, p1, False) if len(p0) < len(p1) else (p1, p0, True)
        zw = tot = 0.
        for m in small:
            o = large[int(np.argmin([abs(m - q) for q in large]))]
            dt, (L0, L1) = self._pair(wf, o if swap else m, m if swap else o, x, y)
            zw, tot = zw + dt * (L0 + L1), tot + L0 + L1
        L0, L1 = wf[:L].sum() * self.gf[x, y, 0], wf[L:].sum() * self.gf[x, y, 1]
        if L0 == 0 or L1 == 0:
            z, w = 0., 1e-5
        else:
            z, w, _PE = self._light(L0, L1, x, y)
            z = float(np.clip(z, -650., 650.))
        return (tw * zw / tot + z * w) / (w + tw) / 1200. + 0.5

    def add(self, predictions, target, c, f, E=None, **_kw):
        np = self.np
        pred, targ, co = predictions.detach().cpu().numpy(), target.detach().cpu().numpy(), c.detach().cpu().numpy()
        wf = f.detach().cpu().numpy().astype(np.float64)
        e, x, y = co[:, 2], co[:, 0], co[:, 1]
        zc = np.array([self._row(wf[i], x[i], y[i]) for i in range(len(co))])
        t = targ[e, 0, x, y].astype(np.float64)
        col = np.minimum(np.bincount(e)[e], self.ev.nmult + 1) - 1
        for tab, p in zip(self.tab, (pred[e, 0, x, y].astype(np.float64), zc)):
            np.add.at(tab, (x, y, col), np.abs(p - t))

    def state_tensors(self):
        return []

    def results(self):
        return {"seg_mult_mae": self.tab[0], "seg_mult_mae_cal": self.tab[1]}


def time_calls(torch, fn, rounds, warm=10, n=100):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / n)
    return us


def summary(us):
    return {"us_per_call": round(statistics.median(us), 2), "spread_us": round(max(us) - min(us), 2)}


def wave_batch(torch, g, events, per_event, dev):
    """About ``events * per_event * 0.98`` distinct active segments, grouped by event; one to three pulses a side."""
    rows = sorted({(int(x), int(y), e) for e in range(events)
                   for x, y in zip(torch.randint(0, 14, (per_event,), generator=g).tolist(),
                                   torch.randint(0, 11, (per_event,), generator=g).tolist())}, key=lambda r: r[2])
    n = len(rows)
    c = torch.tensor(rows, dtype=torch.int32)
    t = torch.arange(L, dtype=torch.float32)[None, :]
    sides = []
    for _s in range(2):
        v = torch.zeros(n, L)
        for k in range(3):
            pk = (10 + 45 * k + torch.randint(0, 20, (n, 1), generator=g)).float()
            amp = torch.rand(n, 1, generator=g) * 0.06 * (torch.rand(n, 1, generator=g) < (1.0 if k == 0 else 0.3))
            v += amp * torch.where(t <= pk, torch.exp(-0.5 * ((t - pk) / 1.6) ** 2), torch.exp(-(t - pk) / 5.0))
        sides.append(v)
    return ([c.to(dev), torch.cat(sides, dim=1).to(dev)], (0.05 + 0.9 * torch.rand(n, generator=g)).to(dev))


def render_profile(d, line):
    rows = ["Calibrated z / E baseline: GPU ZEvaluator(calibration=...) against the plain evaluator and a host path",
            "(tools/bench_calibrated_z.py --profile; MI355X, no kernel trace).  Written by the tool; method: its docstring.",
            "",
            "evaluate.segment_test_loop of LitZ (SingleEndedZConv, 150-sample waveform pairs); synthetic batches of %d events /"
            % d["events_per_batch"],
            "%s rows on average, %d batches per timed window; the four arms alternate in one process, %d rounds; median over"
            % (d["rows_per_batch"], d["batches_per_window"], d["rounds"]),
            "rounds, spread = max - min over rounds.",
            "",
            "arm                                                                  ms per batch   spread"]
    for key, label in (("none", "loop, no evaluator"), ("plain", "loop + GPU ZEvaluator (two launches per batch)"),
                       ("calibrated", "loop + GPU ZEvaluator(calibration=...) (three launches per batch)"),
                       ("host", "loop + host path (4 D2H copies + Python row walk)")):
        rows.append("%-68s %-14s %s" % (label, d[key]["ms_per_batch"], d[key]["spread_ms"]))
    rows += ["added per batch: plain %+.4f ms, calibrated %+.4f ms, host %+.4f ms"
             % (d["plain_added_ms"], d["calibrated_added_ms"], d["host_added_ms"]),
             "(the host arm walks the rows in plain Python where the reference runs numba-compiled walks: it PENALISES the",
             "host; it is the reference's algorithm without its compiler, not the reference's time)",
             "",
             "entry points alone (HIP events around back-to-back calls, 10 warm-up calls; median of %d windows)" % d["rounds"],
             "                                                                     us per call  spread"]
    for tag in ("765", "86000"):
        k = d["kernel_" + tag]
        rows.append("%-68s %-12s %s" % ("wfs_calib_z_E alone, %d rows (%.1f GB/s of %d row bytes)"
                                        % (k["rows"], k["gbytes_per_s"], k["row_bytes"]), k["us_per_call"], k["spread_us"]))
    rows += ["k_align_pulses, which reads the same kind of rows once, runs at 509 GB/s at 86.5 k rows",
             "(profiles/z_real_evaluator_ab.txt); at 765 rows the grid is one wave per row on a fraction of the CUs, and the",
             "time is the latency of a row's serial chain (sort, pairing, fp64 divisions, ordered sums), not memory.",
             "",
             "split of a calibrated add at %d rows (each alone, back to back):" % d["split"]["rows"]]
    for key, label in (("add", "ZEvaluator.add with a calibration (three launches)"),
                       ("reconstruction", "wfs_calib_z_E (one launch)"),
                       ("accumulate", "wfs_seg_z_accumulate_cal (event offsets + rows)"),
                       ("plain_add", "ZEvaluator.add without a calibration (two launches)")):
        rows.append("%-68s %-12s %s" % (label, d["split"][key]["us_per_call"], d["split"][key]["spread_us"]))
    rows += ["", "raw line of the tool:", line, ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--loops", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--events", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None, help="write the profile text (profiles/calibrated_z_ab.txt) there")
    args = ap.parse_args()
    import numpy as np
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd.calibration import CalibratedReconstruction
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.litz import LitZ
    from waveformml_amd.psd.segment_evaluator import ZEvaluator
    if not torch.cuda.is_available():
        raise SystemExit("bench_calibrated_z: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    curves = synthetic_curves(np)
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "events_per_batch": args.events, "rounds": args.rounds}

    mod = LitZ(DictionaryUtility.to_object(z_config())).to(dev)
    batches = [wave_batch(torch, g, args.events, 3, dev) for _ in range(args.batches)]
    out["rows_per_batch"] = round(sum(b[1].shape[0] for b in batches) / len(batches), 1)
    out["batches_per_window"] = args.batches * args.loops
    cal_ev = ZEvaluator(dev, calibration=curves, n_samples=L)
    arms = {"none": None, "plain": ZEvaluator(dev), "calibrated": cal_ev, "host": HostCalibratedZ(cal_ev)}
    with torch.no_grad():
        for ev in arms.values():                                                      # warm every arm
            segment_test_loop(mod, batches, dev, evaluator=ev)
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for name, ev in arms.items():
                if name in ("plain", "calibrated"):
                    ev.reset()
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = segment_test_loop(mod, batches * args.loops, dev, evaluator=ev)    # ends in a read-back
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t) / (args.loops * len(batches)) * 1e3)
                out.setdefault("test_loss", res["test_loss"])
    for name, v in times.items():
        out[name] = {"ms_per_batch": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
    for name in ("plain", "calibrated", "host"):
        out[name + "_added_ms"] = round(out[name]["ms_per_batch"] - out["none"]["ms_per_batch"], 4)

    for tag, events in (("765", 256), ("86000", 28800)):
        (c, f), target = wave_batch(torch, g, events, 3, dev)
        rows = int(c.shape[0])
        n = 100 if rows < 10000 else 20
        rec = CalibratedReconstruction(dev, curves, n_samples=L)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        k = summary(time_calls(torch, lambda: rec.run(f, c, flags), args.rounds, n=n))
        k["rows"], k["row_bytes"] = rows, rows * 2 * L * 4
        k["gbytes_per_s"] = round(k["row_bytes"] / k["us_per_call"] / 1e3, 2)
        k["states"] = torch.bincount(rec.state[:rows], minlength=4).tolist()
        k["flags"] = int(flags.item())
        out["kernel_" + tag] = k
        if tag == "765":
            tdense = torch.zeros((events, 1, 14, 11), device=dev)
            tdense[c[:, 2].long(), 0, c[:, 0].long(), c[:, 1].long()] = target
            pdense = (tdense + 0.05 * (torch.rand(events, 1, 14, 11, generator=g).to(dev) - 0.5)).contiguous()
            ev, plain = ZEvaluator(dev, calibration=curves, n_samples=L), ZEvaluator(dev)
            cal = rec.run(f, c, flags)
            out["split"] = {
                "rows": rows,
                "add": summary(time_calls(torch, lambda: ev.add(pdense, tdense, c, f), args.rounds)),
                "reconstruction": {kk: k[kk] for kk in ("us_per_call", "spread_us")},
                "accumulate": summary(time_calls(torch, lambda: ev.add_planes(pdense, 0, tdense, 0, c, cal=cal), args.rounds)),
                "plain_add": summary(time_calls(torch, lambda: plain.add(pdense, tdense, c, f), args.rounds))}
    line = json.dumps(out)
    print(line)
    if args.profile:
        with open(args.profile, "w") as fh:
            fh.write(render_profile(out, line))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
