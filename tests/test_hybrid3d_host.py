"""CPU checks of the hybrid 3-D net (BASELINE configs[4], config/psd_c5_hybrid3d.json): the config resolves the class
with the 8 x 5 x 16 x 32 dense tail, the voxeliser's C entry points are declared, bound and exported, and there is no CPU
path."""
import ctypes
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wfs_voxelize_offsets_ints", "wfs_voxelize_plan", "wfs_voxelize_emit", "wfs_voxelize_bwd"]


def _config():
    with open(os.path.join(ROOT, "config", "psd_c5_hybrid3d.json")) as f:
        return json.load(f)


def test_config_resolves_the_hybrid_3d_net():
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.net import SPConvHybrid3DNet
    from waveformml_amd.psd.tcn import TemporalConvNet
    from waveformml_amd.psd.voxel import Voxelizer
    cfg = _config()
    assert cfg["net_config"]["net_class"] == "SPConvNet.SPConvHybrid3DNet"
    m = LitPSD(DictionaryUtility.to_object(cfg)).model
    assert type(m) is SPConvHybrid3DNet
    assert m.n_linear == 20480 == 8 * 5 * 16 * 32
    assert m.spatial_size == [14, 11, 1024]
    assert isinstance(m.waveformLayer, TemporalConvNet) and len(m.waveformLayer.network) == 3
    assert m.waveformLayer.kernel_size == 3
    assert isinstance(m.voxelizer, Voxelizer) and m.voxelizer.threshold == 0.0 and m.voxelizer.out_capacity is None
    assert m.sparseModel[0].in_channels == 2
    assert m.linear[0].in_features == 20480 and m.linear[0].out_features == 3
    assert not hasattr(m, "permute_tensor")          # the captured step hands over the rows, not batch-first voxels


def test_voxelize_abi_is_declared_bound_and_exported():
    from waveformml_amd import _lib
    text = open(os.path.join(ROOT, "include", "wfsparse.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text, n
        assert n in _lib.SIGNATURES, n
        assert hasattr(lib, n), n
    assert _lib.WFS_ABI_VERSION == 6


def test_cpu_tensors_raise():
    from waveformml_amd.psd.config import DictionaryUtility
    from waveformml_amd.psd.lit import LitPSD
    from waveformml_amd.psd.voxel import voxelize
    rows = torch.rand(4, 32)
    coords = torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        voxelize(rows, rows, coords)
    cfg = _config()
    cfg["system_config"]["n_samples"] = 16
    m = LitPSD(DictionaryUtility.to_object(cfg)).model
    with pytest.raises(RuntimeError, match="GPU"):
        m([coords, rows])
