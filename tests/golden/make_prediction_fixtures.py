"""Writes the prediction-writer fixtures under tests/golden/h5/pred/ THROUGH libwfh5w (include/wfh5w.h; h5py is not
available): one ``WaveformPairCal`` file and one ``WaveformPairNorm`` file in the reference's compound layouts
(src/datasets/H5CompoundTypes.py: 324 / 584 bytes), each with a ``Chanmap`` table and the P2X table attributes
(src/datasets/HDF5IO.py copy_p2x_attrs).  130 rows in about 40 events; event numbers start above 0, leave gaps and go
back now and then; the cells of an event are distinct; the last event is six rows long.

Run (after `make -C waveformml_amd/csrc`):  python tests/golden/make_prediction_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import prediction_cases as pc  # noqa: E402
from waveformml_amd.psd import h5records  # noqa: E402


def main():
    out_dir = os.path.join(HERE, "h5", "pred")
    os.makedirs(out_dir, exist_ok=True)
    chan = pc.chanmap_rows()
    for kind in ("cal", "norm"):
        rec, n_events = pc.fixture_records(kind)
        members, item = pc.layout(kind)
        path = os.path.join(out_dir, pc.FIXTURE_FILES[kind])
        with h5records.RecordOutput(path) as out:
            out.create_table("Chanmap", pc.CHANMAP, 20)
            out.append(chan.view(np.uint8), len(chan))
            for k, v in (("CLASS", "TABLE"), ("TITLE", "channel map"), ("VERSION", "3.0")):
                out.set_attr(k, v)
            out.create_table(pc.FIXTURE_TABLES[kind], members, item)
            out.append(np.ascontiguousarray(rec).view(np.uint8), len(rec))
            out.set_attr("CLASS", "TABLE")
            for i, m in enumerate(members):
                out.set_attr("FIELD_%d_NAME" % i, m[0])
            out.set_attr("TITLE", "%s fixture" % pc.FIXTURE_TABLES[kind])
            out.set_attr("VERSION", "3.0")
            out.set_attr("abstime", 1520304327.0)
            out.set_attr("runtime", 3599.5)
            out.set_attr("calgrp", "fixture_cal")
            out.set_attr("nevents", float(n_events))
            if kind == "cal":
                out.set_attr("rname", "series015/s015_f00003")       # the norm file lacks rname and scalingfactor
                out.set_attr("scalingfactor", 1.0)
            out.flush()
        print("wrote %s: %d rows, %d events, %d bytes" % (path, len(rec), n_events, os.path.getsize(path)))


if __name__ == "__main__":
    main()
