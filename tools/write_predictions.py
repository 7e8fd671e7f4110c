#!/usr/bin/env python
"""Apply a trained model to a data file and write a copy whose prediction columns hold its output
(waveformml_amd/psd/PredictionWriter.py).  The command line is the one users of the reference's WritePredictions.py
know -- positional input file, config, checkpoint; -w z|irn|irnim; -o; -s; -d; -cpu; -nt; -b; -r -- and the output is
named the same way: ``<input without ".h5">ModelOut.h5`` next to the input, or ``-o`` as a ``.h5`` path or a directory.
Differences:

  -g / --gains FILE.npy   gains [14, 11, 2] for WaveformPairCal input, in place of the calibration-database lookup
                          (-c / --calgroup is still parsed, and refused by the writers: there is no database here)
  --capture               run the forward as replays of one captured HIP graph

No XML sidecar is written.

    python tools/write_predictions.py run_WFNorm.h5 config.json model.ckpt -w irn
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WRITERS = {"z": "ZPredictionWriter", "irn": "IRNPredictionWriter", "irnim": "IRNIMPredictionWriter"}


def existing(path):
    path = os.path.abspath(os.path.expanduser(path))
    if not os.path.exists(path):
        raise IOError("no such file: %s" % path)
    return path


def output_path(input_path, output=None, datatype=None):
    stem = input_path[:-3]
    default = input_path[:input_path.rfind("_")] + "_Phys.h5" if datatype == "PhysPulse" else stem + "ModelOut.h5"
    if output is None:
        return default
    output = os.path.expanduser(output)
    if output.endswith(".h5"):
        return output
    if os.path.isdir(output):
        return os.path.join(output, os.path.basename(stem) + "ModelOut.h5")
    raise IOError("--output %s is neither a directory nor a .h5 path" % output)


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("input_path", help="HDF5 file to predict on (*WFNorm.h5: WaveformPairNorm, otherwise WaveformPairCal)")
    p.add_argument("config", help="JSON config the model was trained with")
    p.add_argument("checkpoint", help="checkpoint of the trained model")
    p.add_argument("--writer", "-w", choices=sorted(WRITERS), default="z", help="which columns to fill (default z)")
    p.add_argument("--output", "-o", help="output .h5 path, or a directory for the default name")
    p.add_argument("--calgroup", "-c", help="not available: use --gains")
    p.add_argument("--gains", "-g", help=".npy file with gains [14, 11, 2]")
    p.add_argument("--scale_factor", "-s", type=float, help="extra factor on the normalisation (float32 gain table)")
    p.add_argument("--datatype", "-d", help="WaveformPairCal (PhysPulse is not available)")
    p.add_argument("--cpu", "-cpu", action="store_true", help="load the checkpoint through host memory")
    p.add_argument("--num_threads", "-nt", type=int, help="host threads for torch")
    p.add_argument("--buffer_size", "-b", type=int, default=1024 * 16, help="rows between flushes of the output")
    p.add_argument("--read_size", "-r", type=int, default=2048, help="rows per chunk (extended to the end of an event)")
    p.add_argument("--capture", action="store_true", help="replay the forward from a captured HIP graph")
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import numpy as np
    import torch
    from waveformml_amd.psd import PredictionWriter as pw
    input_path = existing(args.input_path)
    output = output_path(input_path, args.output, args.datatype)
    kwargs = {"n_buffer_rows": args.buffer_size, "n_rows_per_read": args.read_size, "capture": args.capture}
    if args.cpu:
        kwargs["map_location"] = "cpu"
    for name in ("calgroup", "scale_factor", "datatype"):
        if getattr(args, name) is not None:
            kwargs[name] = getattr(args, name)
    if args.gains:
        kwargs["gains"] = np.load(existing(args.gains))
    if args.num_threads:
        torch.set_num_threads(args.num_threads)
    t0 = time.time()
    writer = getattr(pw, WRITERS[args.writer])(output, input_path, existing(args.config), existing(args.checkpoint), **kwargs)
    print("writing %s with %s" % (output, type(writer).__name__))
    writer.write_predictions()
    print("done: %d chunks in %.2f s" % (writer.chunks_written, time.time() - t0))
    return output


if __name__ == "__main__":
    main()
