"""Generates tests/golden/prediction_writer_cases.npz from the REFERENCE's own row walks (the reference tree, this
container only): what its functions make of the seeded inputs of tests/prediction_cases.py.  No reference text is written
anywhere; the npz holds arrays only.

How the reference is run
  * numba is not installed here, so src/utils/SparseUtils.py cannot be imported.  normalize_waveforms,
    swap_sparse_from_dense and swap_sparse_from_event are taken from the file's syntax tree IN MEMORY, their ``@nb.jit``
    decorators dropped, and executed unmodified.  Plain numpy scalars type ``int16 * float32`` as float32 where numba
    uses float64; the product of an int16 and a float32 is exact in float64, so both round the exact product once to
    float32 and agree.  ``int16 * float64`` is float64 on both sides, rounded on assignment to the float32 output.
  * H5Input.next_chunk / get_event_number (src/datasets/HDF5IO.py) come from the syntax tree the same way and run over a
    stub table backed by a numpy structured array (``len()`` and slicing are all they use).
  * ``z_scale`` is the literal ``Z_NORMALIZATION_FACTOR`` the evaluator constructor assigns (src/evaluation/AD1Evaluator.py);
    ``(output - 0.5) * z_scale`` is formed as ZPredictionWriter.swap_values forms it, in float32 numpy.
  * swap_sparse_from_dense indexes ``dense[b, x, y]``: for L > 1 it is called once per plane on ``dense[:, l]``.
  * ``pulse`` inputs: the reference hands the file's event numbers to the model; the goldens renumber them by the rule of
    normalize_waveforms (run on a two-column dummy waveform), which is what this project does for every input kind.

Run:  python tests/golden/make_prediction_goldens.py
"""
import ast
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import prediction_cases as pc  # noqa: E402

WANTED = ["normalize_waveforms", "swap_sparse_from_dense", "swap_sparse_from_event"]


def tree_of(*path):
    return ast.parse(open(os.path.join(REF, *path)).read())


def run_nodes(nodes, ns, label):
    mod = ast.Module(body=nodes, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "<reference %s, in memory>" % label, "exec"), ns)
    return ns


def reference_functions():
    keep = []
    for node in tree_of("src", "utils", "SparseUtils.py").body:
        if isinstance(node, ast.FunctionDef) and node.name in WANTED:
            node.decorator_list = []
            keep.append(node)
    assert sorted(n.name for n in keep) == sorted(WANTED)
    return run_nodes(keep, {}, "SparseUtils")


def reference_chunker():
    cls = [n for n in tree_of("src", "datasets", "HDF5IO.py").body if isinstance(n, ast.ClassDef) and n.name == "H5Input"][0]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("next_chunk", "get_event_number")]
    assert len(methods) == 2
    ns = run_nodes(methods, {"append": np.append}, "HDF5IO")
    return type("Chunker", (), {m.name: ns[m.name] for m in methods})


def reference_z_scale():
    for node in tree_of("src", "evaluation", "AD1Evaluator.py").body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "Z_NORMALIZATION_FACTOR":
            return float(ast.literal_eval(node.value))
    raise AssertionError("Z_NORMALIZATION_FACTOR not found")


class StubTable:
    def __init__(self, rows):
        self.rows = rows

    def len(self):
        return len(self.rows)

    def __getitem__(self, key):
        return self.rows[key]

    def close(self):
        pass


def chunks_of(chunker, events, nrows):
    rows = np.zeros(len(events), dtype=[("coord", np.int32, (3,))])
    rows["coord"][:, 2] = events
    o = chunker()
    o.table, o.table_length = StubTable(rows), len(rows)
    o.event_index_name, o.event_index_coord, o.current_index = "coord", 2, -1
    out, at = [], 0
    while True:
        data = o.next_chunk(nrows)
        if data is None:
            break
        out.append((at, at + data.shape[0]))
        at += data.shape[0]
    assert at == len(rows)
    return np.array(out, np.int64).reshape(-1, 2)


def main():
    fn = reference_functions()
    chunker = reference_chunker()
    z_scale = reference_z_scale()
    out = {"z_scale": np.float64(z_scale)}
    # the rule itself, as the issue states it
    coo = np.array([[0, 0, e] for e in (5, 5, 9, 9, 5)], np.int32)
    fn["normalize_waveforms"](coo, np.zeros((5, 2), np.int16), np.ones((pc.NX, pc.NY, 2)), np.zeros((5, 2), np.float32))
    assert coo[:, 2].tolist() == [0, 0, 1, 1, 2]

    for name, lay, width, n, pattern, gkind, seed in pc.PREPARE_CASES:
        rec = pc.make_records(lay, width, n, pattern, seed)
        coords = np.array(rec["coord"], np.int32).reshape(n, 3).copy()
        assert coords[0, 2] != -1
        if "waveform" in rec.dtype.names:
            wf = np.ascontiguousarray(rec["waveform"]).reshape(n, width)
            vals = np.zeros((n, width), np.float32)
            fn["normalize_waveforms"](coords, wf, pc.gains_table(gkind), vals)
            out["prep_%s_feats" % name] = vals
        else:
            fn["normalize_waveforms"](coords, np.zeros((n, 2), np.int16), np.ones((pc.NX, pc.NY, 2)),
                                      np.zeros((n, 2), np.float32))
        out["prep_%s_coords" % name] = coords

    for case in pc.SCATTER_CASES:
        name, lay, width, n, pattern, seed, mode, L, member, col0, affine = case
        if mode == "rows":
            continue                                       # the reference assigns the output: nothing to record
        rec = pc.make_records(lay, width, n, pattern, seed)
        coords = np.array(rec["coord"], np.int32).reshape(n, 3)
        assert coords[0, 2] != -1
        B = pc.n_events(coords[:, 2])
        for dt in pc.scatter_dtypes(case):
            src = pc.scatter_source(mode, L, n, B, seed, dt).float().numpy()
            target = np.array(rec[member], np.float32).reshape(n, -1).copy()
            if mode == "dense" and L == 1:
                output = src
                if affine:
                    output = (src.squeeze(1) - 0.5) * z_scale          # ZPredictionWriter.swap_values, float32 numpy
                    assert output.dtype == np.float32
                else:
                    output = src.squeeze(1)
                fn["swap_sparse_from_dense"](target[:, col0], output, coords)
            elif mode == "dense":
                for l in range(L):
                    fn["swap_sparse_from_dense"](target[:, col0 + l], np.ascontiguousarray(src[:, l]), coords)
            else:
                fn["swap_sparse_from_event"](target[:, col0:col0 + L], src, coords)
            out["scat_%s_%s" % (name, dt)] = target[:, col0:col0 + L].copy()

    for cname, events in pc.chunk_columns().items():
        out["chunkcol_%s" % cname] = events
        for nrows in pc.chunk_sizes(len(events)):
            out["chunks_%s_%d" % (cname, nrows)] = chunks_of(chunker, events, nrows)
    tail = out["chunkcol_tail"]
    last = out["chunks_tail_16"][-1]
    assert last[1] == len(tail) and last[0] < len(tail) - 9 < last[0] + 16 < len(tail)   # the final cut falls inside the last event

    path = os.path.join(HERE, "prediction_writer_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote prediction_writer_cases.npz: %d arrays, %d bytes, z_scale %g" % (len(out), os.path.getsize(path), z_scale))


if __name__ == "__main__":
    main()
