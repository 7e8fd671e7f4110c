"""``PulseDatasetDet`` (psd/h5data.py, psd/PulseDataset.py) on the fixture files under tests/golden/h5/det/ (written by
tests/golden/make_h5_fixtures_det.py through libwfh5w): shapes, dtypes, values as stored (no normalisation), labels by
directory, and the data module's three splits."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DET = os.path.join(HERE, "golden", "h5", "det")
EXPECTED = np.load(os.path.join(HERE, "golden", "expected_det.npz"))


def test_items_are_the_stored_rows():
    from waveformml_amd.psd import h5data
    ds = h5data.PulseDatasetDet([os.path.join(DET, "gamma"), os.path.join(DET, "neutron")], 50)
    assert len(ds) == 10 and ds.normalize is False and ds.batch_index == 2
    assert ds.info["file_pattern"] == "*DetCoordSim.h5" and ds.info["data_name"] == "DetPulseCoord"
    assert ds.info["coord_name"] == "coord" and ds.info["feat_name"] == "pulse"
    seen = set()
    for i in range(len(ds)):
        (c, f), y = ds[i]
        name = os.path.basename(ds.info["data_info"][i]["file_path"])
        cls, k = name.split("_")[0], int(name.split("_")[1])
        seen.add((cls, k))
        assert c.dtype == torch.int32 and f.dtype == torch.float32 and y.dtype == torch.int64
        assert c.shape[1] == 3 and f.shape == (c.shape[0], 7) and y.shape == (10,)
        assert np.array_equal(c.numpy(), EXPECTED["%s_%d_coord" % (cls, k)])
        assert np.array_equal(f.numpy(), EXPECTED["%s_%d_pulse" % (cls, k)])               # as stored: not normalised
        assert y.tolist() == [0 if cls == "gamma" else 1] * 10                             # the directory's index
        assert c[:, 2].tolist() == sorted(c[:, 2].tolist()) and int(c[-1, 2]) == 9
    assert seen == {(cls, k) for cls in ("gamma", "neutron") for k in range(5)}
    # a budget below a file's events cuts the item at an event boundary
    part = h5data.PulseDatasetDet([os.path.join(DET, "gamma")], 4)
    (c, f), y = part[0]
    assert len(part) == 1 and y.shape == (4,) and int(c[-1, 2]) == 3
    assert np.array_equal(f.numpy(), EXPECTED["gamma_0_pulse"][:c.shape[0]])


def test_config_class_and_data_module_splits():
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    from waveformml_amd.psd.PulseDataset import PulseDatasetDet
    with open(os.path.join(ROOT, "config", "psd_features_det.json")) as fh:
        cfg = json.load(fh)
    cfg["dataset_config"]["base_path"] = DET
    cfg["dataset_config"]["dataloader_params"]["pin_memory"] = False
    config = load_config(cfg)
    dm = PSDDataModule(config, "cpu")
    dm.setup()
    assert isinstance(dm.train_dataset, PulseDatasetDet) and dm.train_dataset.normalize is False
    assert dm.train_dataset.use_half is False and dm.train_dataset.n_categories == 2
    files = [set(d.get_file_list()) for d in (dm.train_dataset, dm.val_dataset, dm.test_dataset)]
    assert [len(f) for f in files] == [4, 2, 4] and not (files[0] & files[1]) and not (files[2] & (files[0] | files[1]))
    batches = list(dm.test_dataloader())
    assert len(batches) == 2
    for (c, f), y in batches:
        assert f.shape[1] == 7 and y.tolist() == [0] * 10 + [1] * 10
        assert int(c[-1, 2]) == 19 and c[:, 2].tolist() == sorted(c[:, 2].tolist())       # events renumbered by the collate
    half = PulseDatasetDet(config, "train", 10, "cpu", use_half=True)
    assert half[0][0][1].dtype == torch.float16
