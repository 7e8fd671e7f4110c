"""Writes the extracted-feature fixtures under tests/golden/h5/det/ THROUGH libwfh5w (include/wfh5w.h; h5py is not
available): two class directories, ``gamma`` and ``neutron``, of five ``*DetCoordSim.h5`` files each, ten events a file, in
the reference's ``DetPulseCoord`` compound layout (src/datasets/H5CompoundTypes.py: coord int32 [3] = (x, y, event), pulse
float32 [7] = E / 12, dt / 30 + 0.5, PE0 / 5000, PE1 / 5000, z / 1200 + 0.5, PSD, t offset / 30; 40 bytes) with an
``nevents`` attribute.  libwfh5w writes every table in gzip-compressed chunks.  The two classes differ in PSD and in
multiplicity so that a small net can learn them; the cells of an event are distinct; expected_det.npz keeps the rows for
tests/test_h5data_det.py.

Run (after `make -C waveformml_amd/csrc`):  python tests/golden/make_h5_fixtures_det.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from waveformml_amd.psd import h5records  # noqa: E402

MEMBERS = [("coord", 0, h5records.I32, 3), ("pulse", 12, h5records.F32, 7)]
ITEM = 40
CLASSES = ("gamma", "neutron")
FILES, EVENTS = 5, 10


def records(rng, cls):
    rows = []
    for e in range(EVENTS):
        n = int(rng.integers(1, 4)) if cls == 0 else int(rng.integers(2, 7))
        cells = rng.choice(14 * 11, size=n, replace=False)
        for k in cells:
            pulse = [rng.uniform(0.01, 0.2), rng.uniform(0.3, 0.7), rng.uniform(0.02, 0.6), rng.uniform(0.02, 0.6),
                     rng.uniform(0.1, 0.9), rng.uniform(0.10, 0.20) if cls == 0 else rng.uniform(0.22, 0.36),
                     rng.uniform(0.05, 0.9)]
            rows.append(((k // 11, k % 11, e), pulse))
    rec = np.zeros(len(rows), h5records.members_dtype(MEMBERS, ITEM))
    rec["coord"] = np.array([r[0] for r in rows], np.int32)
    rec["pulse"] = np.array([r[1] for r in rows], np.float32)
    return rec


def main():
    rng = np.random.default_rng(679)
    keep = {}
    for ci, cls in enumerate(CLASSES):
        out_dir = os.path.join(HERE, "h5", "det", cls)
        os.makedirs(out_dir, exist_ok=True)
        for i in range(FILES):
            rec = records(rng, ci)
            path = os.path.join(out_dir, "%s_%d_DetCoordSim.h5" % (cls, i))
            with h5records.RecordOutput(path) as out:
                out.create_table("DetPulseCoord", MEMBERS, ITEM)
                out.append(np.ascontiguousarray(rec).view(np.uint8), len(rec))
                out.set_attr("CLASS", "TABLE")
                for k, m in enumerate(MEMBERS):
                    out.set_attr("FIELD_%d_NAME" % k, m[0])
                out.set_attr("TITLE", "Detpulse coord pair data")
                out.set_attr("VERSION", "3.0")
                out.set_attr("nevents", float(EVENTS))
                out.flush()
            keep["%s_%d_coord" % (cls, i)], keep["%s_%d_pulse" % (cls, i)] = rec["coord"].copy(), rec["pulse"].copy()
            print("wrote %s: %d rows, %d bytes" % (path, len(rec), os.path.getsize(path)))
    np.savez_compressed(os.path.join(HERE, "expected_det.npz"), **keep)


if __name__ == "__main__":
    main()
