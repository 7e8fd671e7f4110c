"""The per-segment modules trained and tested FROM FILES through PSDDataModule: small ``*WFNorm.h5`` files written by the
test (tests/test_segment_datasets.py), ``Trainer(capture=True)`` over the data module's own train loader with the
one-launch row hand-over (graph.ROW_HANDOVER) on and off -- the same bytes in front of the same graph, so losses and
parameters are EQUAL -- and against the eager trainer within the 1e-4 relative bar of tests/test_gpu_segment_capture.py;
a train dataset that carries ``additional_fields``; the quantifier's test loader (fields ``["PID"]``) through
``segment_test_loop`` with the module's evaluator."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import prediction_cases as pc
from test_host_mirror import _z_config
from test_segment_callers import IONI
from test_segment_datasets import ROOT, make_files

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PID_MAP = {"1": 0, "4": 1, "6": 2, "256": 3, "258": 2, "512": 4}


def _dataset_config(tmp_path, params, test_params=None):
    """Five files of 20 .. 24 events: three train (63 events), one validate, one test."""
    make_files(tmp_path, "ioni_nonioni", "_WFNorm.h5", "WaveformPairNorm", pc.NORM_MEMBERS, pc.NORM_ITEM, n_files=5,
               n_events=20, seed=40)
    dc = {"imports": ["waveformml_amd.psd.PulseDataset"], "base_path": str(tmp_path), "paths": ["ioni_nonioni"],
          "dataset_class": "PulseDatasetWFPairNorm", "dataset_params": params,
          "dataloader_params": {"pin_memory": False, "num_workers": 0, "batch_size": 1},
          "n_train": 63, "n_validate": 23, "n_test": 24}
    if test_params is not None:
        dc["test_dataset_params"] = test_params
    return dc


def _config(which, tmp_path, fields=False):
    extra = {"additional_fields": ["PID"]} if fields else {}
    if which == "LitSegClassifier":
        cfg = copy.deepcopy(IONI)
        cfg["net_config"]["imports"] = ["waveformml_amd.spconv" if m == "oracle.spconv" else m
                                        for m in cfg["net_config"]["imports"]]
        cfg["dataset_config"] = _dataset_config(tmp_path, dict(label_name="PID", label_map=PID_MAP, **extra))
    elif which == "LitZ":
        cfg = _z_config(["waveformml_amd.spconv"])               # 20 samples: the first 20 of both halves of a row
        cfg["net_config"]["fused_segment_loss"] = True
        cfg["dataset_config"] = _dataset_config(tmp_path, dict(label_name="phys", label_index=4, waveform_subset=[0, 19],
                                                               **extra))
    else:
        with open(os.path.join(ROOT, "config", "segment_quantifier_z.json")) as fh:
            cfg = json.load(fh)
        dc = _dataset_config(tmp_path, dict(cfg["dataset_config"]["dataset_params"], **extra),
                             cfg["dataset_config"]["test_dataset_params"])
        cfg["dataset_config"] = dc
    cfg["optimize_config"].update(lr=0.01, optimizer_params={"momentum": 0.9})
    return cfg


def _module(which, cfg):
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.litseg import LitSegClassifier
    from waveformml_amd.psd.litsegq import LitSegQuantifier
    from waveformml_amd.psd.litz import LitZ
    torch.manual_seed(7)
    config = load_config(copy.deepcopy(cfg))
    return {"LitSegClassifier": LitSegClassifier, "LitZ": LitZ, "LitSegQuantifier": LitSegQuantifier}[which](config), config


def _fit(which, cfg, capture, monkeypatch, handover=True):
    """Two epochs over the data module's train loader; (epoch losses, flat parameters, eager fallbacks, one-launch calls)."""
    from waveformml_amd import _lib
    from waveformml_amd.psd import graph
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    from waveformml_amd.psd.trainer import Trainer
    monkeypatch.setattr(graph, "ROW_HANDOVER", bool(handover))
    lib, calls = _lib.load(), []
    entry = lib.wfs_load_rows_batch
    monkeypatch.setattr(lib, "wfs_load_rows_batch", lambda *a: (calls.append(1), entry(*a))[1])
    mod, config = _module(which, cfg)
    dm = PSDDataModule(config, DEV)
    loader = dm.train_dataloader()
    assert len(loader) == 3
    tr = Trainer(max_epochs=2, device=DEV, capture=capture, check_every=2)
    hist = tr.fit(mod, loader)
    torch.cuda.synchronize()
    monkeypatch.setattr(lib, "wfs_load_rows_batch", entry)
    flat = torch.cat([p.detach().reshape(-1) for p in mod.model.parameters()]).cpu()
    return [h["train_loss"] for h in hist], flat, tr.eager_fallbacks, len(calls)


@pytest.mark.parametrize("which", ["LitSegClassifier", "LitZ", "LitSegQuantifier"])
def test_captured_training_from_files_with_and_without_the_one_launch(which, tmp_path, monkeypatch):
    cfg = _config(which, tmp_path)
    on, p_on, fb_on, calls_on = _fit(which, cfg, True, monkeypatch, handover=True)
    off, p_off, fb_off, calls_off = _fit(which, cfg, True, monkeypatch, handover=False)
    eager, p_eager, _, calls_eager = _fit(which, cfg, False, monkeypatch)
    print(which, "epoch losses: one launch", on, "torch hand-over", off, "eager", eager, "fallbacks", fb_on, fb_off)
    assert calls_on >= 6 - fb_on and calls_off == 0 and calls_eager == 0      # every replayed step took the launch
    assert fb_on == fb_off and fb_on < 6
    assert len(on) == 2 and on == off and torch.equal(p_on, p_off)            # bit for bit
    for a, b in zip(eager, on):
        assert np.isfinite(a) and abs(a - b) <= 1e-4 * abs(a), (eager, on)


def test_training_ignores_additional_fields_bit_for_bit(tmp_path, monkeypatch):
    """``Trainer.fit`` over a train dataset with ``additional_fields``: the prefetcher stages the [feats, *fields] list,
    the step trains on the features -- the losses of the same files read without the fields, exactly."""
    plain = _fit("LitSegQuantifier", _config("LitSegQuantifier", tmp_path), True, monkeypatch)
    fields = _fit("LitSegQuantifier", _config("LitSegQuantifier", tmp_path, fields=True), True, monkeypatch)
    eager = _fit("LitSegQuantifier", _config("LitSegQuantifier", tmp_path, fields=True), False, monkeypatch)
    assert fields[0] == plain[0] and torch.equal(fields[1], plain[1]) and fields[3] == plain[3] > 0
    for a, b in zip(eager[0], fields[0]):
        assert np.isfinite(a) and abs(a - b) <= 1e-4 * abs(a), (eager[0], fields[0])


def test_prefetcher_yields_the_field_list_on_the_device(tmp_path):
    from waveformml_amd.psd.config import load_config
    from waveformml_amd.psd.data import DevicePrefetcher, to_device
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    dm = PSDDataModule(load_config(_config("LitSegQuantifier", tmp_path)), DEV)
    loader = dm.test_dataloader()
    staged = list(DevicePrefetcher(loader, DEV, feature_dtype=torch.bfloat16))
    direct = [to_device(b, DEV, torch.bfloat16) for b in loader]
    torch.cuda.synchronize()
    assert len(staged) == len(direct) == 1
    for ((c, f), y), ((c2, f2), y2) in zip(staged, direct):
        assert isinstance(f, list) and len(f) == 2 and all(t.is_cuda for t in [c, y] + f)
        assert f[0].dtype == torch.bfloat16 and f[1].dtype == torch.int32          # the fields keep their dtype
        assert torch.equal(c, c2) and torch.equal(y, y2) and torch.equal(f[0], f2[0]) and torch.equal(f[1], f2[1])


def _equal_tables(a, b, name):
    """Every array of two results dictionaries equal, element for element; the number of elements compared."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), name
        return sum(_equal_tables(a[k], b[k], "%s.%s" % (name, k)) for k in a)
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), name
        return sum(_equal_tables(x, y, name) for x, y in zip(a, b))
    x, y = np.asarray(a), np.asarray(b)
    assert x.shape == y.shape and np.array_equal(x, y), name
    return int(x.size)


def test_quantifier_test_loader_fills_the_evaluator(tmp_path):
    """``segment_test_loop(..., evaluator=module.evaluator)`` over the test loader of config/segment_quantifier_z.json:
    the tables equal those of the same batch built by hand from the records that went into the file."""
    from waveformml_amd.psd.evaluate import segment_test_loop
    from waveformml_amd.psd.PSDDataModule import PSDDataModule
    cfg = _config("LitSegQuantifier", tmp_path)
    cfg["evaluation_config"] = {"bin_overrides": {"4": [-600.0, 600.0, 20]}}
    results = []
    for by_hand in (False, True):
        mod, config = _module("LitSegQuantifier", cfg)
        mod.to(DEV)
        dm = PSDDataModule(config, DEV)
        loader = dm.test_dataloader()
        if by_hand:
            made = make_files(tmp_path, "ioni_nonioni", "_WFNorm.h5", "WaveformPairNorm", pc.NORM_MEMBERS, pc.NORM_ITEM,
                              n_files=5, n_events=20, seed=40)
            (path,) = dm.test_dataset.get_file_list()
            rec = made[os.path.realpath(path)]
            loader = [([torch.from_numpy(rec["coord"].copy()), [torch.from_numpy(rec["pulse"].copy()),
                                                                 torch.from_numpy(rec["PID"].copy())]],
                       torch.from_numpy(rec["phys"].copy()))]
        out = segment_test_loop(mod, loader, DEV, evaluator=mod.evaluator)
        assert sorted(out) == ["evaluation", "rows", "test_loss", "test_mse"] and out["rows"] >= 24
        results.append(out)
    a, b = results
    assert a["rows"] == b["rows"] and a["test_loss"] == b["test_loss"]
    counted = _equal_tables(a["evaluation"], b["evaluation"], "evaluation")
    assert counted > 0 and a["evaluation"]["error_hist"].sum() > 0
