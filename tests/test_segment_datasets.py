"""The per-segment dataset classes of psd/PulseDataset.py (reference src/datasets/PulseDataset.py:628-1232) on small files
written by the test itself: what an item holds is the reference's rule restated over the numpy records that went into the
files -- rows of the item's event range, ``_convert_label``'s conversion, the chained ``label_map``, ``label_index``,
``waveform_subset`` on both halves, the real-data z scaling, the PMT factor vector.  Host only."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import prediction_cases as pc
from waveformml_amd.psd import PulseDataset, h5records
from waveformml_amd.psd.config import DictionaryUtility, ModuleUtility
from waveformml_amd.psd.data import _PackedCollate, collate_fn
from waveformml_amd.psd.PSDDataModule import PSDDataModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CLASSES = ["PulseDatasetPMT", "PulseDataset2DWithZ", "PulseDataset2DWithEZ", "PulseDatasetDetWithZ",
               "PulseDatasetDetWithEZ", "PulseDatasetWFPair", "PulseDatasetWFPairEZ", "PulseDatasetRealWFPair",
               "PulseDatasetWFPairNorm", "PulseDatasetNormFeatures"]
MAX_INV = np.float32(1.0 / (2 ** 14 - 1))
PID_VALUES = np.array([1, 4, 6, 258, 256, 512], dtype=np.int32)       # the particle codes the configs' label_map names

# (x, y, evt) int32, waveform int16 [2 * 8], z float32: a WaveformPairsWithZ layout, 52 bytes
WITHZ_MEMBERS = [("coord", 0, pc.I32, 3), ("waveform", 12, pc.I16, 16), ("z", 44, pc.F32, 1), ("PID", 48, pc.I32, 1)]
WITHZ_ITEM = 52
# DetPulseCoord of the PMT files: coord, pulse float32 [8]
PMT_MEMBERS = [("coord", 0, pc.I32, 3), ("pulse", 12, pc.F32, 8)]
PMT_ITEM = 44


def _records(members, item, n_events, seed):
    """Events of 1 to 4 rows each: a structured array in the layout, every member drawn."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 5, size=n_events)
    n = int(counts.sum())
    rec = np.zeros(n, dtype=pc.dtype_of(members, item))
    for name, _off, kind, count in members:
        shape = (n, count) if count > 1 else (n,)
        if name == "coord":
            cells = np.concatenate([rng.choice(154, size=k, replace=False) for k in counts])    # distinct per event
            rec[name][:, 0] = cells % 14
            rec[name][:, 1] = cells // 14
            rec[name][:, 2] = np.repeat(np.arange(n_events), counts)
        elif name == "PID":
            rec[name] = PID_VALUES[rng.integers(0, len(PID_VALUES), size=n)]
        elif kind in (pc.F32, pc.F64):
            rec[name] = rng.uniform(-600.0, 600.0, size=shape)
        else:
            rec[name] = rng.integers(0, 2 ** 14 - 1, size=shape)
    return rec


def _write(path, table, members, item, rec, n_events):
    with h5records.RecordOutput(str(path)) as out:
        out.create_table(table, members, item)
        out.append(rec, len(rec))
        out.set_attr("nevents", n_events)


def make_files(root, subdir, mask_tail, table, members, item, n_files=3, n_events=5, seed=0):
    """``n_files`` files ``f_<i><mask_tail>`` under root/subdir; returns {resolved path: records}."""
    d = os.path.join(str(root), subdir)
    os.makedirs(d, exist_ok=True)
    made = {}
    for i in range(n_files):
        rec = _records(members, item, n_events + i, seed + 101 * i)
        path = os.path.join(d, "f_%d%s" % (i, mask_tail))
        _write(path, table, members, item, rec, n_events + i)
        made[os.path.realpath(path)] = rec
    return made


def _config(root, subdir, cls, params=None, test_params=None, n=5):
    dc = {"imports": ["waveformml_amd.psd.PulseDataset"], "base_path": str(root), "paths": [subdir],
          "dataset_class": cls, "dataset_params": params or {},
          "dataloader_params": {"num_workers": 0, "batch_size": 2, "pin_memory": False},
          "n_train": n, "n_validate": n, "n_test": n}
    if test_params is not None:
        dc["test_dataset_params"] = test_params
    return DictionaryUtility.to_object({"system_config": {"half_precision": 0}, "dataset_config": dc})


def _rec_of(ds, made, index=0):
    di = ds.info["data_info"][index]
    rec = made[os.path.realpath(di["file_path"])]
    e0, e1 = di["event_range"]
    if not ds.info["event_based"]:
        return rec[e0:e1 + 1]
    keep = (rec["coord"][:, 2] >= e0) & (rec["coord"][:, 2] <= e1)
    return rec[keep]


@pytest.mark.parametrize("name", NEW_CLASSES)
def test_class_resolves_by_bare_and_qualified_name(name):
    util = ModuleUtility(["waveformml_amd.psd.PulseDataset"])
    cls = util.retrieve_class(name)
    assert cls is getattr(PulseDataset, name)
    assert util.retrieve_class("PulseDataset." + name) is cls
    with pytest.raises(NotImplementedError):
        cls.retrieve_config("x.json", None)


def test_wfpair_norm_labels_index_map_and_subset(tmp_path):
    made = make_files(tmp_path, "a", "_WFNorm.h5", "WaveformPairNorm", pc.NORM_MEMBERS, pc.NORM_ITEM)
    # EZ (float32 [2]) sliced by label_index; pulse kept as stored (normalize=False)
    ds = PulseDataset.PulseDatasetWFPairNorm(_config(tmp_path, "a", "PulseDatasetWFPairNorm"), "train", 5, None,
                                             label_index=1)
    (c, f), y = ds[0]
    rec = _rec_of(ds, made)
    assert c.dtype == torch.int32 and np.array_equal(c.numpy(), rec["coord"])
    assert f.dtype == torch.float32 and np.array_equal(f.numpy(), rec["pulse"])
    assert y.dtype == torch.float32 and np.array_equal(y.numpy(), rec["EZ"][:, 1])
    # an int32 member with a chained label_map: 1 -> 6, then 6 -> 0 remaps the fresh 6s too; int64 class indices
    ds = PulseDataset.PulseDatasetWFPairNorm(_config(tmp_path, "a", "PulseDatasetWFPairNorm"), "train", 5, None,
                                             label_name="PID", label_map={"1": 6, "6": 0}, additional_fields=["phys"],
                                             waveform_subset=[3, 10])
    (c, f), y = ds[0]
    want = rec["PID"].astype(np.int64)
    want[want == 1] = 6
    want[want == 6] = 0
    assert (rec["PID"] == 1).any() and (rec["PID"] == 6).any() and not (want == 6).any()
    assert y.dtype == torch.int64 and np.array_equal(y.numpy(), want)
    assert isinstance(f, list) and len(f) == 2
    keep = np.r_[3:11, 65 + 3:65 + 11]                       # samples 3 .. 10 inclusive of BOTH halves
    assert f[0].shape[1] == 16 and np.array_equal(f[0].numpy(), rec["pulse"][:, keep])
    assert np.array_equal(f[1].numpy(), rec["phys"])
    # without fields the subset is taken of the tensor itself
    ds = PulseDataset.PulseDatasetWFPairNorm(_config(tmp_path, "a", "PulseDatasetWFPairNorm"), "train", 5, None,
                                             waveform_subset=[0, 0])
    (c, f), y = ds[0]
    assert np.array_equal(f.numpy(), rec["pulse"][:, [0, 65]]) and np.array_equal(y.numpy(), rec["EZ"])


def test_wfpair_cal_classes(tmp_path):
    made = make_files(tmp_path, "sim", "_WFPairSim.h5", "WaveformPairCal", pc.CAL_MEMBERS, pc.CAL_ITEM)
    cfg = _config(tmp_path, "sim", "PulseDatasetWFPair")
    ds = PulseDataset.PulseDatasetWFPair(cfg, "train", 5, None)
    (c, f), y = ds[0]
    rec = _rec_of(ds, made)
    # label_name=None: the directory index per EVENT; int16 waveforms normalised by one float32 multiply
    assert y.dtype == torch.int64 and y.tolist() == [0] * 5
    assert np.array_equal(f.numpy(), rec["waveform"].astype(np.float32) * MAX_INV)
    ds = PulseDataset.PulseDatasetWFPairEZ(cfg, "train", 5, None, label_index=0, additional_fields=["PID"])
    (c, f), y = ds[0]
    assert np.array_equal(y.numpy(), rec["EZ"][:, 0]) and f[1].dtype == torch.int32
    assert np.array_equal(f[1].numpy(), rec["PID"])
    assert np.array_equal(f[0].numpy(), rec["waveform"].astype(np.float32) * MAX_INV)
    # real data: its own file mask; z -> z / 1200 + 0.5, E -> E / 12, anything else untouched
    real = make_files(tmp_path, "real", "_WFCalFilteredSE.h5", "WaveformPairCal", pc.CAL_MEMBERS, pc.CAL_ITEM, seed=7)
    rcfg = _config(tmp_path, "real", "PulseDatasetRealWFPair")
    ds = PulseDataset.PulseDatasetRealWFPair(rcfg, "train", 5, None)
    rec = _rec_of(ds, real)
    assert np.array_equal(ds[0][1].numpy(), rec["z"] * np.float32(1.0 / 1200.0) + np.float32(0.5))
    ds = PulseDataset.PulseDatasetRealWFPair(rcfg, "train", 5, None, label_name="E")
    assert np.array_equal(ds[0][1].numpy(), rec["E"] * np.float32(1.0 / 12.0))
    ds = PulseDataset.PulseDatasetRealWFPair(rcfg, "train", 5, None, label_name="PSD")
    assert np.array_equal(ds[0][1].numpy(), rec["PSD"])
    other = make_files(tmp_path, "real", "_Other.h5", "WaveformPairCal", pc.CAL_MEMBERS, pc.CAL_ITEM, n_files=1, seed=9)
    ds = PulseDataset.PulseDatasetRealWFPair(rcfg, "train", 5, None, file_pattern="*_Other.h5", label_name=None)
    assert [os.path.realpath(p) for p in ds.get_file_list()] == list(other)


def test_with_z_pmt_and_row_counted_classes(tmp_path):
    made = make_files(tmp_path, "z", "_WaveformPairZSim.h5", "WaveformPairsWithZ", WITHZ_MEMBERS, WITHZ_ITEM)
    ds = PulseDataset.PulseDataset2DWithZ(_config(tmp_path, "z", "PulseDataset2DWithZ"), "train", 3, None)
    (c, f), y = ds[0]
    rec = _rec_of(ds, made)                                   # 3 of the first file's 5 events: a partial range
    assert len(rec) < len(made[os.path.realpath(ds.info["data_info"][0]["file_path"])])
    assert np.array_equal(c.numpy(), rec["coord"]) and np.array_equal(y.numpy(), rec["z"])
    assert np.array_equal(f.numpy(), rec["waveform"].astype(np.float32) * MAX_INV)
    # the same layout under the other event-based bindings (table, mask and members are all the class fixes)
    for cls, tail, table, feat in (("PulseDataset2DWithEZ", "_WaveformPairEZSim.h5", "WaveformPairsWithEZ", "waveform"),
                                   ("PulseDatasetDetWithEZ", "_DetCoordEZSim.h5", "DetPulseCoordWithEZ", "pulse"),
                                   ("PulseDatasetDetWithZ", "_DetCoordZSim.h5", "DetPulseCoordWithZ", "pulse")):
        members = [("coord", 0, pc.I32, 3), (feat, 12, pc.F32, 7), ("EZ", 40, pc.F32, 2), ("z", 48, pc.F32, 1)]
        made = make_files(tmp_path, cls, tail, table, members, 52, seed=3)
        kw = {"label_index": 1} if cls.endswith("EZ") else {}
        ds = getattr(PulseDataset, cls)(_config(tmp_path, cls, cls), "train", 5, None, **kw)
        (c, f), y = ds[0]
        rec = _rec_of(ds, made)
        scale = MAX_INV if feat == "waveform" else np.float32(1.0)
        assert np.array_equal(f.numpy(), rec[feat] * scale), cls
        assert np.array_equal(y.numpy(), rec["EZ"][:, 1] if cls.endswith("EZ") else rec["z"]), cls
    made = make_files(tmp_path, "pmt", "_PMTCoordSim.h5", "DetPulseCoord", PMT_MEMBERS, PMT_ITEM)
    ds = PulseDataset.PulseDatasetPMT(_config(tmp_path, "pmt", "PulseDatasetPMT"), "train", 5, None)
    (c, f), y = ds[0]
    m = float(2 ** 14 - 1)
    factors = np.array([1. / m, 1. / (m * 10), 0.001, 1.0, 1. / m, 1. / (m * 10), 0.001, 1.0], dtype=np.float32)
    assert f.dtype == torch.float32 and np.array_equal(f.numpy(), _rec_of(ds, made)["pulse"] * factors)
    # NormFeatures: ranges count ROWS (no nevents needed); 4 rows out of the first file
    members = [("coord", 0, pc.I32, 3), ("features", 12, pc.F32, 5), ("EZ", 32, pc.F32, 2), ("PID", 40, pc.I32, 1)]
    made = make_files(tmp_path, "nf", "_WFFeatures.h5", "NormFeatures", members, 44)
    ds = PulseDataset.PulseDatasetNormFeatures(_config(tmp_path, "nf", "PulseDatasetNormFeatures"), "train", 4, None,
                                               label_index=0, additional_fields=["PID"])
    (c, f), y = ds[0]
    rec = _rec_of(ds, made)
    assert len(rec) == 4 and np.array_equal(f[0].numpy(), rec["features"]) and np.array_equal(y.numpy(), rec["EZ"][:, 0])


def _quantifier_module(tmp_path, n=5):
    """PSDDataModule from config/segment_quantifier_z.json pointed at three temporary WFNorm files."""
    with open(os.path.join(ROOT, "config", "segment_quantifier_z.json")) as fh:
        cfg = json.load(fh)
    made = make_files(tmp_path, "ioni_nonioni", "_WFNorm.h5", "WaveformPairNorm", pc.NORM_MEMBERS, pc.NORM_ITEM)
    dc = cfg["dataset_config"]
    dc["base_path"] = str(tmp_path)
    dc["n_train"] = dc["n_validate"] = dc["n_test"] = n
    dc["dataloader_params"]["num_workers"] = 0
    return PSDDataModule(DictionaryUtility.to_object(copy.deepcopy(cfg)), None), made


def test_quantifier_config_builds_its_three_datasets(tmp_path):
    dm, made = _quantifier_module(tmp_path)
    dm.setup()
    sets = [set(d.get_file_list()) for d in (dm.train_dataset, dm.val_dataset, dm.test_dataset)]
    assert all(len(s) == 1 for s in sets) and len(sets[0] | sets[1] | sets[2]) == 3
    (c, f), y = dm.train_dataset[0]
    rec = _rec_of(dm.train_dataset, made)
    assert y.dtype == torch.float32 and y.dim() == 1 and np.array_equal(y.numpy(), rec["phys"][:, 4])
    assert torch.is_tensor(f) and np.array_equal(f.numpy(), rec["pulse"])
    (c, f), y = dm.test_dataset[0]
    rec = _rec_of(dm.test_dataset, made)
    assert isinstance(f, list) and len(f) == 2 and f[1].dtype == torch.int32
    assert np.array_equal(f[1].numpy(), rec["PID"]) and np.array_equal(y.numpy(), rec["phys"])


@pytest.mark.parametrize("name", ["segment_quantifier_z", "segment_quantifier_graph", "segment_classifier_graph"])
def test_the_configs_naming_wfpair_norm_build(tmp_path, name):
    with open(os.path.join(ROOT, "config", name + ".json")) as fh:
        cfg = json.load(fh)
    dc = cfg["dataset_config"]
    for p in dc["paths"]:
        make_files(tmp_path, p, "_WFNorm.h5", "WaveformPairNorm", pc.NORM_MEMBERS, pc.NORM_ITEM)
    dc["base_path"] = str(tmp_path)
    dc["n_train"] = dc["n_validate"] = dc["n_test"] = 5
    dm = PSDDataModule(DictionaryUtility.to_object(cfg), None)
    dm.setup()
    files = [f for d in (dm.train_dataset, dm.val_dataset, dm.test_dataset) for f in d.get_file_list()]
    assert len(files) == len(set(files)) == 3 * len(dc["paths"])
    for d in (dm.train_dataset, dm.val_dataset, dm.test_dataset):
        (c, f), y = d[0]
        assert c.shape[0] == y.shape[0] == (f[0] if isinstance(f, list) else f).shape[0]


def test_collate_and_packed_collate_carry_the_fields(tmp_path):
    made = make_files(tmp_path, "a", "_WFNorm.h5", "WaveformPairNorm", pc.NORM_MEMBERS, pc.NORM_ITEM)
    ds = PulseDataset.PulseDatasetWFPairNorm(_config(tmp_path, "a", "PulseDatasetWFPairNorm"), "test", 11, None,
                                             label_name="phys", additional_fields=["PID"])
    assert len(ds) == 2                                       # 5 + 6 events: two items
    recs = [_rec_of(ds, made, i) for i in range(2)]
    n0_events = int(recs[0]["coord"][:, 2].max()) + 1
    (c, f), y = collate_fn([ds[0], ds[1]])
    want_c = np.concatenate([recs[0]["coord"], recs[1]["coord"]])
    want_c[len(recs[0]):, 2] += len(recs[0])                  # the reference's offset: the ROWS of the items before
    assert n0_events <= len(recs[0])
    assert np.array_equal(c.numpy(), want_c)
    assert np.array_equal(f[0].numpy(), np.concatenate([r["pulse"] for r in recs]))
    assert np.array_equal(f[1].numpy(), np.concatenate([r["PID"] for r in recs])) and f[1].dtype == torch.int32
    assert np.array_equal(y.numpy(), np.concatenate([r["phys"] for r in recs]))
    packed = _PackedCollate(collate_fn)([ds[0], ds[1]])
    (((pc_, pf), py),) = _PackedCollate.unpack(packed)
    assert isinstance(pf, list) and len(pf) == 2 and pf[1].dtype == torch.int32
    assert torch.equal(pc_, c) and torch.equal(pf[0], f[0]) and torch.equal(pf[1], f[1]) and torch.equal(py, y)


def test_batches_iterate_on_the_host_without_a_prefetcher(tmp_path):
    dm, made = _quantifier_module(tmp_path)
    rows = 0
    for (c, f), y in dm.test_dataloader():
        assert not c.is_cuda and isinstance(f, list) and f[0].shape[0] == f[1].shape[0] == y.shape[0] == c.shape[0]
        rows += c.shape[0]
    assert rows == sum(len(_rec_of(dm.test_dataset, made, i)) for i in range(len(dm.test_dataset)))
    for (c, f), y in dm.train_dataloader():
        assert torch.is_tensor(f) and y.dim() == 1
