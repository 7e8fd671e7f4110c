"""Cost of the LitZ / LitEZ training step with and without ``net_config.fused_segment_loss`` (psd/litz.py, the fused segment
loss of csrc/segloss.hip), and of the loss alone against the torch composition it replaces
(LitSegmentBase._calc_segment_loss); configs: config/segment_z.json and config/segment_ez.json (20 samples, 40 channels),
fp32 rows, synthetic batches of 256 events / about 765 rows and of 28 800 events / about 86.5 k rows:

  off       the eager step without the key: the torch composition, torch's SGD on ``model.parameters()``
  on        the eager step with the key: the fused loss, FlatSGD on the flat parameter
  on_hint   the same with the net's ``batch_size_hint`` at the batch's own event count: B as in ``on``, but without the
            host read-back of the last coordinate row that ``on`` pays to learn it
  on_cap_b  the same with the hint at the row capacity a captured step would have, i.e. the dense map and ToDense over
            B = capacity events instead of the batch's own.  on_cap_b - on_hint is what the captured step's B costs,
            eagerly: the two arms differ in B alone (on_cap_b - on would also count the read-back that the hint removes)
  captured  the step with the key replayed from its graph (psd/graph.GraphedTrainStep through Trainer._captured_step)
  loss      forward + backward of the loss alone on a [B, planes, 14, 11] leaf map: spconv.functional.segment_map_loss
            (one launch each way) against the composition, LitZ (1 plane) and LitEZ (2 planes, the composition twice)

A step is module.training_step + backward + optimizer step (Trainer.training_step / Trainer._captured_step).  The arms of a
module and size run in ONE process, alternating window by window, ``rounds`` windows each; the figure per arm is the median
over the windows and the spread is (max - min).  A window is ``calls`` back-to-back steps between two HIP events and ends in
a device synchronise.

Launch counts of the two loss routes come from a run of their own under ``rocprofv3 --kernel-trace --stats``:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_segment_train.py --trace-loss fused
runs exactly ``--trace-calls`` forward + backward calls of one route (LitEZ, 256 events) and nothing else on the device;
``--count-kernels DIR`` then prints the kernel launches per call from the kernel_stats.csv under DIR, and the main run takes
the two figures with ``--launches FUSED TORCH``.

``--previous FILE`` takes the last line of an earlier ``--out`` file of the same command and prints its B-cost figures
beside this run's: a difference of two medians is only worth what it repeats to.

``--row-handover`` runs another arm pair INSTEAD of the above (its own result line and profile text,
profiles/row_handover_ab.txt): the captured step of LitZ (config/segment_z.json, key on) and of LitSegClassifier
(config/segment_classifier_graph.json, 130 channels, 6 rows per event) with the hand-over of the per-row batch as the
torch copies, fills and gather (psd/graph.ROW_HANDOVER = 0, WFS_ROW_HANDOVER=0) and as the one launch of
wfs_load_rows_batch (1), at about 765 and about 86 k rows; and the hand-over alone (GraphedTrainStep._load) in both forms.
The switch is read by every hand-over, so ONE captured step serves both arms: the same graph, the same buffers, windows
alternating.

usage: python tools/bench_segment_train.py [--rounds 7] [--calls 30] [--out FILE] [--profile FILE] [--launches F T]
                                           [--previous FILE]
prints one JSON line; --out appends it to FILE; --profile writes profiles/segment_loss_ab.txt's text to FILE"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (("765", 256), ("86500", 28800))
CONFIGS = {"LitZ": "segment_z.json", "LitEZ": "segment_ez.json"}


def summary(us):
    return {"us_per_call": round(statistics.median(us), 2), "spread_us": round(max(us) - min(us), 2)}


def window(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def alternate(torch, arms, rounds, calls, warm=3):
    """{name: summary} of the callables in ``arms``, one window each per round, in turn."""
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            us[name].append(window(torch, fn, calls))
    return {k: summary(v) for k, v in us.items()}


def segment_batch(torch, g, events, per_event, channels, planes):
    """About ``events * per_event * 0.99`` distinct active segments grouped by event, features and per-row targets (CPU)."""
    rows = sorted({(int(x), int(y), e) for e in range(events)
                   for x, y in zip(torch.randint(0, 14, (per_event,), generator=g).tolist(),
                                   torch.randint(0, 11, (per_event,), generator=g).tolist())}, key=lambda r: r[2])
    n = len(rows)
    c = torch.tensor(rows, dtype=torch.int32)
    y = torch.rand((n, 2), generator=g) if planes == 2 else torch.rand(n, generator=g)
    return [c, torch.rand(n, channels, generator=g)], y


def load_cfg(name, key):
    with open(os.path.join(ROOT, "config", CONFIGS[name])) as f:
        cfg = json.load(f)
    cfg["net_config"]["fused_segment_loss"] = bool(key)
    cfg["optimize_config"].update(lr=1e-4)
    cfg["optimize_config"].pop("scheduler_class", None)
    return cfg


def module_class(name):
    from waveformml_amd.psd import litz
    return getattr(litz, name)


class Stepper:
    """One module with its reducer, optimizer and trainer, as Trainer.fit wires them."""

    def __init__(self, torch, name, key, capture, dev):
        from waveformml_amd.psd.config import load_config
        from waveformml_amd.psd.ddp import FlatGradAllReducer
        from waveformml_amd.psd.trainer import Trainer
        torch.manual_seed(0)
        self.module = module_class(name)(load_config(load_cfg(name, key))).to(dev)
        self.module.train()
        self.reducer = FlatGradAllReducer(self.module.model.parameters())
        self.module.optimizer_parameters = self.reducer.optimizer_parameters()
        self.optimizer = self.module.configure_optimizers()
        self.trainer = Trainer(max_epochs=1, device=dev, capture=capture, check_every=0)
        self.capture = capture

    def step(self, batch):
        (c, f), y = batch
        batch = ([c, f], y)
        if self.capture:
            return self.trainer._captured_step(self.module, self.reducer, self.optimizer, batch, 0)
        return self.trainer.training_step(self.module, self.reducer, self.optimizer, batch, 0)

    def close(self):
        if self.trainer._graph is not None:
            self.trainer._graph.close()
            self.trainer._graph = None
        self.reducer.remove()


def loss_routes(torch, name, events, dev, g):
    """(fused, composed, sizes): forward + backward of the two loss routes on the same leaf map."""
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.spconv import functional as Fsp
    planes = 2 if name == "LitEZ" else 1
    (c, _f), y = segment_batch(torch, g, events, 3, 1, planes)
    c, y = c.to(dev), y.to(dev)
    pred = torch.rand((events, planes, 14, 11), generator=g).to(dev).requires_grad_(True)
    mod = module_class(name)(load_config(load_cfg(name, False))).to(dev)
    kind = Fsp.segment_loss_kind(mod.criterion)
    cols = (0, 1) if planes == 2 else (0,)

    def fused():
        pred.grad = None
        total, _per = Fsp.segment_map_loss(pred, c, y, cols, kind)
        total.backward()
        return total

    def composed():
        pred.grad = None
        if planes == 1:
            loss = mod._calc_segment_loss(c, pred, y)[0]
        else:                                                     # LitEZ._process_batch: the second call reuses the mask
            zl, _t, _p, sparse_mask = mod._calc_segment_loss(c, pred[:, 0].unsqueeze(1), y[:, 0])
            el = mod._calc_segment_loss(c, pred[:, 1].unsqueeze(1), y[:, 1], sparse_mask=sparse_mask)[0]
            loss = zl + el
        loss.backward()
        return loss

    return fused, composed, {"rows": int(c.shape[0]), "events": events, "planes": planes}, pred


HANDOVER_MODULES = (("LitZ", "segment_z.json", 3, 40), ("LitSegClassifier", "segment_classifier_graph.json", 6, 130))


class RowStepper(Stepper):
    """A captured Stepper of one of HANDOVER_MODULES."""

    def __init__(self, torch, name, config, dev):
        from waveformml_amd.psd import litseg, litz
        from waveformml_amd.psd.config import load_config
        from waveformml_amd.psd.ddp import FlatGradAllReducer
        from waveformml_amd.psd.trainer import Trainer
        with open(os.path.join(ROOT, "config", config)) as f:
            cfg = json.load(f)
        if name == "LitZ":
            cfg["net_config"]["fused_segment_loss"] = True
        cfg["optimize_config"].update(lr=1e-4)
        cfg["optimize_config"].pop("scheduler_class", None)
        torch.manual_seed(0)
        self.module = (litz.LitZ if name == "LitZ" else litseg.LitSegClassifier)(load_config(cfg)).to(dev)
        self.module.train()
        self.reducer = FlatGradAllReducer(self.module.model.parameters())
        self.module.optimizer_parameters = self.reducer.optimizer_parameters()
        opt = self.module.configure_optimizers()
        self.optimizer = opt[0][0] if isinstance(opt, tuple) else opt
        self.trainer = Trainer(max_epochs=1, device=dev, capture=True, check_every=0)
        self.capture = True


def row_handover_ab(torch, args, dev, g):
    """The result of --row-handover (see the module docstring)."""
    from waveformml_amd import _lib
    from waveformml_amd.psd import graph
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "rounds": args.rounds, "calls": args.calls}
    for name, config, per_event, channels in HANDOVER_MODULES:
        for tag, events in SIZES:
            events = events * 3 // per_event
            (c, f), y = segment_batch(torch, g, events, per_event, channels, 1)
            if name == "LitSegClassifier":
                y = torch.randint(0, 5, (c.shape[0],), generator=g)
            batch = ((c.to(dev), f.to(dev)), y.to(dev))
            stepper = RowStepper(torch, name, config, dev)
            stepper.step(batch)                                   # captures
            runner = stepper.trainer._graph

            def arm(on, fn):
                def call():
                    graph.ROW_HANDOVER = on
                    fn()
                return call
            calls = args.calls if events <= 1024 else max(5, args.calls // 3)
            was = graph.ROW_HANDOVER
            try:
                res = alternate(torch, {"step_torch": arm(False, lambda: stepper.step(batch)),
                                        "step_one_launch": arm(True, lambda: stepper.step(batch))}, args.rounds, calls)
                res.update(alternate(torch, {"handover_torch": arm(False, lambda: runner._load(batch)),
                                             "handover_one_launch": arm(True, lambda: runner._load(batch))},
                                     args.rounds, calls * 3))
            finally:
                graph.ROW_HANDOVER = was
            res.update(events=events, rows=int(c.shape[0]), n_cap=int(runner.n_cap), calls=calls,
                       eager_fallbacks=stepper.trainer.eager_fallbacks, event_offsets_in_launch=runner.events is not None)
            out["%s_%s" % (name, tag)] = res
            stepper.close()
            del stepper, runner
            torch.cuda.empty_cache()
    return out


def render_row_handover(d, line):
    """The text of profiles/row_handover_ab.txt from one --row-handover result."""
    rows = ["Hand-over of a per-row batch into a captured training step: the torch copies, fills and gather of",
            "psd/graph._CapturedRunner._load (WFS_ROW_HANDOVER=0) against the one launch of wfs_load_rows_batch (1).",
            "tools/bench_segment_train.py --row-handover --profile; MI355X.  Written by the tool; method: its docstring.  fp32 rows,",
            "device-resident synthetic batches, ONE captured step per module and size serving both arms (the switch is read by",
            "every hand-over), the arms alternating window by window, %d windows; median over windows, spread = max - min."
            % d["rounds"],
            "",
            "module            rows    capacity  what                          arm          us per call   spread"]
    for name, _config, _pe, _ch in HANDOVER_MODULES:
        for tag, _events in SIZES:
            s = d["%s_%s" % (name, tag)]
            for what, key in (("captured step", "step"), ("hand-over alone (host-bound)", "handover")):
                for arm_key, label in (("torch", "torch"), ("one_launch", "one launch")):
                    r = s["%s_%s" % (key, arm_key)]
                    rows.append("%-17s %-7d %-9d %-29s %-12s %-13s %s" % (name, s["rows"], s["n_cap"], what, label,
                                                                           r["us_per_call"], r["spread_us"]))
            gain = s["step_torch"]["us_per_call"] - s["step_one_launch"]["us_per_call"]
            spread = max(s["step_torch"]["spread_us"], s["step_one_launch"]["spread_us"])
            rows.append("                  step: torch - one launch = %+.1f us (larger spread of the two arms %.1f us)%s"
                        % (gain, spread, "; eager fallbacks %d" % s["eager_fallbacks"] if s["eager_fallbacks"] else ""))
    rows += ["", "A window of steps is %d (about 765 rows) or %d (about 86 k rows) back-to-back calls between two HIP events and"
             % (d["calls"], max(5, d["calls"] // 3)),
             "ends in a device synchronise; a window of hand-overs alone is three times as many calls, and is bound by the host's",
             "enqueue time (several eager launches against one), not by the device.", "", "raw line of the tool:", line, ""]
    return "\n".join(rows)


def count_kernels(directory):
    """Kernel launches in the kernel_stats.csv files of a rocprofv3 --kernel-trace --stats run under ``directory``."""
    total, names = 0, 0
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                total += int(row["Calls"])
                names += 1
    return total, names


def b_cost(step):
    return round(step["on_cap_b"]["us_per_call"] - step["on_hint"]["us_per_call"], 1)


def render_profile(d, line):
    """The text of profiles/segment_loss_ab.txt from one result of this tool."""
    rows = ["LitZ / LitEZ training step with and without net_config.fused_segment_loss, and the fused segment loss against the",
            "torch composition it replaces (tools/bench_segment_train.py --profile; MI355X).  Written by the tool; method: its",
            "docstring.  fp32 rows, 40 channels, synthetic batches; the arms of a module and size alternate window by window in",
            "one process, %d windows of %d steps each; median over windows, spread = max - min over windows." % (d["rounds"], d["calls"]),
            "",
            "Training step (training_step + backward + optimizer step), us per step:",
            "module  events  rows    arm                                                      us per step   spread"]
    labels = (("off", "eager, key off (composition, torch SGD)"), ("on", "eager, key on (fused loss, FlatSGD)"),
              ("on_hint", "eager, key on, hint = the batch's own events"),
              ("on_cap_b", "eager, key on, hint = the captured step's row capacity"), ("captured", "captured, key on"))
    for name in ("LitZ", "LitEZ"):
        for tag, _events in SIZES:
            s = d["step_%s_%s" % (name, tag)]
            for key, label in labels:
                rows.append("%-7s %-7d %-7d %-56s %-13s %s" % (name, s["events"], s["rows"], label, s[key]["us_per_call"],
                                                               s[key]["spread_us"]))
            rows.append("        row capacity of the captured step %d (B of its dense map; %.2f x the batch's events)"
                        % (s["n_cap"], s["n_cap"] / s["events"]))
    rows += ["",
             "The captured step's B.  Its targets are per row, so the only bound the runner has on the events is the row capacity:",
             "the dense map and ToDense cover B = capacity events, about %.1f x the batch's own at 3 rows per event.  The two hint"
             % (d["step_LitEZ_86500"]["n_cap"] / d["step_LitEZ_86500"]["events"]),
             "arms run the eager keyed step on the exact-size batch and differ in B alone (neither reads the event count back from",
             "the device, which the plain keyed arm does: at 765 rows that read-back is most of what separates it from them).",
             "hint = row capacity minus hint = own events, us per step (spreads of the two arms in brackets):"]
    for tag in ("765", "86500"):
        for name in ("LitZ", "LitEZ"):
            st = d["step_%s_%s" % (name, tag)]
            line_b = "  %-6s %6d rows  %+9.1f  (%s, %s)" % (name, st["rows"], b_cost(st), st["on_hint"]["spread_us"],
                                                             st["on_cap_b"]["spread_us"])
            prev = (d.get("previous_b_cost") or {}).get("%s_%s" % (name, tag))
            rows.append(line_b + ("   an earlier run of the same command: %+.1f" % prev if prev is not None else ""))
    rows += [
             "",
             "Loss alone: forward + backward on a [events, planes, 14, 11] leaf map, eager calls, the two routes alternating.",
             "module  events  rows    route               us per forward + backward   spread"]
    for name in ("LitZ", "LitEZ"):
        for tag, _events in SIZES:
            s = d["loss_%s_%s" % (name, tag)]
            for key, label in (("fused", "fused"), ("torch", "torch composition")):
                rows.append("%-7s %-7d %-7d %-19s %-27s %s" % (name, s["events"], s["rows"], label, s[key]["us_per_call"],
                                                               s[key]["spread_us"]))
    rows += ["Eager calls at 765 rows are bound by the host's enqueue time, not by the device: read them with their spreads.", ""]
    if d.get("launches"):
        rows += ["Kernel launches per forward + backward of the loss (LitEZ, 256 events; rocprofv3 --kernel-trace --stats, a run of",
                 "its own per route, %d calls each, every kernel of the process counted): fused %.1f, torch composition %.1f."
                 % (d["launches"]["calls"], d["launches"]["fused"], d["launches"]["torch"]), ""]
    else:
        rows += ["Kernel launches per call of the two loss routes: not measured in this run.", ""]
    rows += ["Losses of the arms at the end of their windows (same seed, same batch; they trained for different numbers of steps",
             "only where the window counts differ): %s" % json.dumps(d["final_losses"]),
             "",
             "raw line of the tool:", line, ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None, help="write the profile text (profiles/segment_loss_ab.txt) there")
    ap.add_argument("--trace-loss", choices=("fused", "torch"), default=None,
                    help="run only --trace-calls calls of one loss route (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--trace-calls", type=int, default=20)
    ap.add_argument("--count-kernels", default=None, metavar="DIR",
                    help="print the kernel launches per call from the kernel_stats.csv files under DIR (no GPU needed)")
    ap.add_argument("--previous", default=None, metavar="FILE",
                    help="an earlier --out file of the same command: its B-cost figures are printed beside this run's")
    ap.add_argument("--row-handover", action="store_true",
                    help="the WFS_ROW_HANDOVER arm pair instead of the arms above (profiles/row_handover_ab.txt)")
    ap.add_argument("--launches", type=float, nargs=2, default=None, metavar=("FUSED", "TORCH"),
                    help="kernel launches per call of the two loss routes, from --count-kernels")
    args = ap.parse_args()
    if args.count_kernels:
        total, names = count_kernels(args.count_kernels)
        print(json.dumps({"kernel_launches": total, "kernels": names, "per_call": round(total / args.trace_calls, 2)}))
        return
    import torch
    from waveformml_amd import _lib
    from waveformml_amd.psd.graph import GraphedTrainStep
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment_train: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    if args.trace_loss:
        fused, composed, _sizes, _pred = loss_routes(torch, "LitEZ", 256, dev, g)
        torch.cuda.synchronize()
        for _ in range(args.trace_calls):
            (fused if args.trace_loss == "fused" else composed)()
        torch.cuda.synchronize()
        return
    if args.row_handover:
        out = row_handover_ab(torch, args, dev, g)
        line = json.dumps(out)
        print(line)
        if args.profile:
            with open(args.profile, "w") as f:
                f.write(render_row_handover(out, line))
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return
    out = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "rounds": args.rounds, "calls": args.calls, "final_losses": {}}
    if args.launches:
        out["launches"] = {"fused": args.launches[0], "torch": args.launches[1], "calls": args.trace_calls}

    for name in ("LitZ", "LitEZ"):
        planes = 2 if name == "LitEZ" else 1
        for tag, events in SIZES:
            (c, f), y = segment_batch(torch, g, events, 3, 40, planes)
            batch = ((c.to(dev), f.to(dev)), y.to(dev))
            n = int(c.shape[0])
            n_cap = int(GraphedTrainStep.capacity_for(n, n))
            steppers = {"off": Stepper(torch, name, False, False, dev), "on": Stepper(torch, name, True, False, dev),
                        "on_hint": Stepper(torch, name, True, False, dev),
                        "on_cap_b": Stepper(torch, name, True, False, dev), "captured": Stepper(torch, name, True, True, dev)}
            steppers["on_hint"].module.model.batch_size_hint = events
            steppers["on_cap_b"].module.model.batch_size_hint = n_cap
            last = {}

            def arm(key):
                def fn():
                    last[key] = steppers[key].step(batch)
                return fn
            calls = args.calls if events <= 1024 else max(5, args.calls // 3)
            res = alternate(torch, {k: arm(k) for k in steppers}, args.rounds, calls)
            res.update(events=events, rows=n, n_cap=n_cap, calls=calls,
                       eager_fallbacks=steppers["captured"].trainer.eager_fallbacks)
            out["step_%s_%s" % (name, tag)] = res
            out["final_losses"]["%s_%s" % (name, tag)] = {k: round(float(v.detach()), 6) for k, v in last.items()}
            for s in steppers.values():
                s.close()
            del steppers, last
            torch.cuda.empty_cache()

            fused, composed, sizes, _pred = loss_routes(torch, name, events, dev, g)
            a, b = float(fused().detach()), float(composed().detach())
            res = alternate(torch, {"fused": fused, "torch": composed}, args.rounds, calls * 3)
            res.update(sizes, loss_fused=round(a, 6), loss_torch=round(b, 6))
            out["loss_%s_%s" % (name, tag)] = res
    if args.previous:
        with open(args.previous) as f:
            prev = json.loads(f.read().strip().splitlines()[-1])
        out["previous_b_cost"] = {k[len("step_"):]: b_cost(v) for k, v in prev.items() if k.startswith("step_")}
    line = json.dumps(out)
    print(line)
    if args.profile:
        with open(args.profile, "w") as f:
            f.write(render_profile(out, line))
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
