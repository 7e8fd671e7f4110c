"""Rows per second of ``ZPredictionWriter.write_predictions()`` (psd/PredictionWriter.py) on a synthetic
``WaveformPairCal`` file at the bench's event density (psd/synthetic: 1 + Poisson(2) rows per event, 65 samples per PMT,
int16 ADC values), with a small LitZ net (3 conv layers + 2 pointwise), fp32 rows:

  gpu       one raw read into a page-locked buffer, one upload, wfs_predict_prepare, the eager forward,
            wfs_predict_scatter, one download, one append
  captured  the same with the forward as a psd/graph.GraphedEvalStep replay
  host      the reference's route restated in this tool on the same file library and the same chunks: records to numpy,
            normalisation and event renumbering on the host, two uploads, the forward, read-back, the swap on the host.
            The host side is VECTORISED numpy, which is more favourable to it than the reference's row-by-row walks
            (numba there, unavailable here); its output table is compared with the gpu arm's byte for byte.

at ``n_rows_per_read`` 2048 (the reference's default) and 65536.  The arms of one chunk size run in ONE process,
alternating, ``rounds`` times; the figure per arm is the median over rounds, the spread (max - min) over rounds.  Every
timed window is a whole ``write_predictions()`` / host loop and ends with the file closed (device idle).

``shares``: a separate, untimed-for-rate pass of the gpu arms with a device synchronise after every stage
(``profile=True``): seconds per stage over the file, as shares of their sum.  The append is libhdf5's gzip level 9.

usage: python tools/bench_predict.py [--rows 131072] [--rounds 5] [--out FILE] [--profile FILE]
prints one JSON line; --out appends it to FILE; --profile writes profiles/prediction_writer_ab.txt's text to FILE"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = {
    "system_config": {"model_name": "SingleEndedZConv", "n_samples": 65, "gpu_enabled": True, "half_precision": 0},
    "net_config": {"criterion_class": "L1Loss", "criterion_params": [], "imports": ["torch.nn", "waveformml_amd.spconv"],
                   "net_type": "2DConvolution", "algorithm": "conv",
                   "hparams": {"conv": {"kernel_size": 3, "n_layers": 3}, "point": {"pointwise_layers": 2}}},
    "optimize_config": {"imports": ["torch.optim"], "lr": 0.01, "optimizer_class": "optim.SGD",
                        "optimizer_params": {"momentum": 0.9}},
    "dataset_config": {"imports": []},
}


def make_file(path, rows):
    """A WaveformPairCal file of about ``rows`` rows (whole events), with a Chanmap and the table attributes."""
    import numpy as np
    import prediction_cases as pc
    from waveformml_amd.psd import h5records, synthetic
    coords, feats, _y = synthetic.generate(int(rows / 3.0) + 1, 65, 3, seed=4321, layout="2d")
    n = len(coords)
    rec = np.zeros(n, dtype=pc.dtype_of(pc.CAL_MEMBERS, pc.CAL_ITEM))
    rec["coord"] = coords
    rec["coord"][:, 2] += 1000
    rec["evt"] = rec["coord"][:, 2]
    rec["waveform"] = np.rint(feats * synthetic.ADC_MAX).astype(np.int16)
    rng = np.random.default_rng(1)
    rec["EZ"] = rng.random((n, 2), dtype=np.float32)
    rec["t"] = np.cumsum(rng.random(n))
    with h5records.RecordOutput(path) as out:
        out.create_table("Chanmap", pc.CHANMAP, 20)
        out.append(pc.chanmap_rows().view(np.uint8), 28)
        out.create_table("WaveformPairCal", pc.CAL_MEMBERS, pc.CAL_ITEM)
        for a in range(0, n, 1 << 16):
            b = min(n, a + (1 << 16))
            out.append(np.ascontiguousarray(rec[a:b]).view(np.uint8), b - a)
        out.set_attr("CLASS", "TABLE")
        out.set_attr("TITLE", "bench")
        out.set_attr("VERSION", "3.0")
        out.set_attr("nevents", float(coords[-1, 2] + 1))
    return n, int(coords[-1, 2] + 1)


def table_bytes(path):
    import numpy as np
    from waveformml_amd.psd import h5records
    with h5records.RecordInput(path, "WaveformPairCal") as t:
        buf = np.zeros((t.n_rows, t.item_size), np.uint8)
        t.read_records(0, t.n_rows, buf)
    return buf.tobytes()


def host_route(path, input_path, module, gains, nrows, dev):
    """The reference's swap_values loop (ZPredictionWriter) with numpy in place of its numba row walks."""
    import numpy as np
    import torch
    import prediction_cases as pc
    from waveformml_amd.psd import h5records
    from waveformml_amd.psd.PredictionWriter import chunk_bounds, gain_factors
    factors = gain_factors(gains)
    with h5records.RecordInput(input_path, "WaveformPairCal") as t, h5records.RecordOutput(path) as out:
        out.copy_dataset(t, "Chanmap")
        out.create_table_like(t)
        out.copy_table_attrs(t)
        dtype = t.numpy_dtype()
        # the reference reads the event column row by row while cutting; one column read is kinder to it
        from waveformml_amd.psd.h5data import H5Table
        with H5Table(input_path, "WaveformPairCal", "coord", "waveform") as ht:
            events = ht.read_member("coord", 0, t.n_rows).numpy()[:, 2]
        with torch.no_grad():
            for a, b in chunk_bounds(events, nrows):
                buf = np.zeros((b - a, t.item_size), np.uint8)
                t.read_records(a, b, buf)
                data = buf.view(dtype).reshape(-1)
                coords = np.array(data["coord"])
                vals = pc.host_normalize(coords, data["waveform"], factors)
                coords[:, 2] = pc.host_renumber(coords[:, 2])
                v = torch.tensor(vals, dtype=torch.float32, device=dev)
                c = torch.tensor(coords, dtype=torch.int32, device=dev)
                output = (module([c, v]).detach().cpu().numpy() - np.float32(0.5)) * np.float32(1200.0)
                ez = np.array(data["EZ"])
                pc.host_swap("dense", ez[:, 1:2], output, np.array(data["coord"]))
                data["EZ"] = ez
                out.append(buf, b - a)
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--profile")
    args = ap.parse_args()
    import numpy as np
    import torch
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litz import LitZ
    from waveformml_amd.psd.PredictionWriter import ZPredictionWriter
    from waveformml_amd.psd.trainer import Trainer, load_from_checkpoint
    assert torch.cuda.is_available(), "bench_predict needs the GPU: there is no CPU path to time"
    dev = "cuda:0"
    work = tempfile.mkdtemp(prefix="bench_predict_")
    src = os.path.join(work, "bench_WFCal.h5")
    n_rows, n_events = make_file(src, args.rows)
    torch.manual_seed(3)
    module = LitZ(load_config(CONFIG))
    ckpt = Trainer().save_checkpoint(module, module.configure_optimizers(), None, 0, os.path.join(work, "z.ckpt"))
    gains = 0.6 + 0.8 * np.random.default_rng(5).random((14, 11, 2))
    host_module = load_from_checkpoint(ckpt, load_config(CONFIG), LitZ).eval().to(dev)
    result = {"rows": n_rows, "events": n_events, "file_bytes": os.path.getsize(src), "rounds": args.rounds, "sizes": {}}

    def gpu_arm(nrows, capture, profile=False):
        w = ZPredictionWriter(os.path.join(work, "out_gpu.h5"), src, CONFIG, ckpt, gains=gains, n_rows_per_read=nrows,
                              capture=capture, profile=profile)
        t0 = time.perf_counter()
        w.write_predictions()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, w

    def host_arm(nrows):
        t0 = time.perf_counter()
        host_route(os.path.join(work, "out_host.h5"), src, host_module, gains, nrows, dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for nrows in (2048, 65536):
        arms = {"gpu": [], "captured": [], "host": []}
        gpu_arm(nrows, False), gpu_arm(nrows, True), host_arm(nrows)          # warm every shape the windows use
        for _ in range(args.rounds):
            arms["gpu"].append(gpu_arm(nrows, False)[0])
            arms["captured"].append(gpu_arm(nrows, True)[0])
            arms["host"].append(host_arm(nrows))
        # same bytes out of the gpu (eager) arm and the host route
        gpu_arm(nrows, False)
        same = table_bytes(os.path.join(work, "out_gpu.h5")) == table_bytes(os.path.join(work, "out_host.h5"))
        entry = {"host_file_equals_gpu_file": bool(same)}
        for k, secs in arms.items():
            entry[k] = {"rows_per_s": round(n_rows / statistics.median(secs)), "seconds": round(statistics.median(secs), 4),
                        "spread_s": round(max(secs) - min(secs), 4)}
        for capture in (False, True):
            _s, w = gpu_arm(nrows, capture, profile=True)
            tot = sum(w.timings.values())
            entry["shares_" + ("captured" if capture else "gpu")] = {
                "chunks": w.chunks_written, "seconds": {k: round(v, 4) for k, v in w.timings.items()},
                "share": {k: round(v / tot, 3) for k, v in w.timings.items()}}
        result["sizes"][str(nrows)] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.profile:
        with open(args.profile, "w") as f:
            f.write("tools/bench_predict.py on one MI355X: ZPredictionWriter on a synthetic WaveformPairCal file, %d rows in %d "
                    "events (%d bytes, gzip 9),\nsmall LitZ net, fp32 rows; median over %d alternating rounds, spread = max - min\n\n"
                    % (n_rows, n_events, result["file_bytes"], args.rounds))
            for nrows, e in result["sizes"].items():
                f.write("n_rows_per_read %s   (host route's table equals the gpu arm's byte for byte: %s)\n"
                        % (nrows, e["host_file_equals_gpu_file"]))
                for k in ("gpu", "captured", "host"):
                    f.write("  %-9s %9d rows/s   %.4f s per file   spread %.4f s\n"
                            % (k, e[k]["rows_per_s"], e[k]["seconds"], e[k]["spread_s"]))
                for k in ("shares_gpu", "shares_captured"):
                    f.write("  %-15s %d chunks; " % (k, e[k]["chunks"]) +
                            "  ".join("%s %.1f%%" % (s, 100 * v) for s, v in e[k]["share"].items()) + "\n")
                f.write("\n")
            f.write(line + "\n")
    import shutil
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
