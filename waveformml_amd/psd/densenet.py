"""``DenseConvNet``: host-side mirror of the reference's dense PSD net (src/models/DenseConvNet.py; BASELINE configs[0],
"C1"): COO rows ``[coords (x, y, event), feats [n, 2T]]`` -> the dense map [B, 2T, 14, 11] -> ``Conv2DBlock`` ->
``view(-1, n_linear)`` (channels first: C, H, W) -> ``LinearBlock``.  Built from ``net_config.hparams`` = {n_conv, n_lin,
out_planes[, conv_params, lin_params]}; same attribute names (``model``, ``linear``, ``n_linear``) and module tree as the
reference, so state dicts and checkpoints are the reference's.

On the GPU the map is built by ONE launch (convnet2d.densify_rows, wfs_densify_rows) straight in the layout the
conv-stack kernels read, the block runs as one fused call per direction (csrc/conv2d.hip), and the linears run as
SPConvNet's tail does (spconv/functional.head_forward).  On the CPU, and wherever the kernels do not take the call, the
forward is the reference's torch composition.

``batch_size_hint`` (set by LitPSD._predict: one label per event) spares the device -> host read of the last coordinate
row; without it the batch size is read as the reference reads it.  The optional third list element ``n_valid`` is the
device int64 row count of a capacity-padded captured batch (psd/graph.py): only the densify launch can honour it
without a host read-back, so a call that carries one and cannot run on the kernels raises.
"""
import logging

import torch
from torch import nn

from .blocks import LinearBlock
from .config import DictionaryUtility, ModuleUtility
from .convnet2d import Conv2DBlock, densify_rows


class DenseConvNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.log = logging.getLogger(__name__)
        self.system_config = config.system_config
        self.net_config = config.net_config
        self.nsamples = self.system_config.n_samples
        self.ntype = self.system_config.n_type
        self.modules_util = ModuleUtility(self.net_config.imports)
        self.x = 14
        self.y = 11
        self.batch_size_hint = None            # the number of events of the batch, when the caller knows it
        self.get_algorithm()
        self.dense_permute = [0, 3, 1, 2]

    def get_algorithm(self):
        if hasattr(self.net_config, "hparams"):
            try:
                self.create_algorithm(self.net_config.hparams, self.ntype)
            except AssertionError as e:
                raise AssertionError("Parameters {0} \nlead to error : {1}".format(
                    DictionaryUtility.to_dict(self.net_config.hparams), e))
        else:
            raise IOError("net_config must contain one of either 'algorithm' or 'hparams'")

    def create_algorithm(self, hparams, n_classes):
        requirements = ["n_conv", "n_lin", "out_planes"]
        size = [14, 11, int(self.nsamples * 2)]
        if not hasattr(hparams, "n_conv"):
            raise IOError("hparams must be a dictionary containing the following minimal settings:\n"
                          "  n_dil: int, number of dilation waveform layers\n"
                          "  n_conv: int, number of n-d sparse convolutional layers\n"
                          "  n_lin: int, number of linear layers")
        for rq in requirements:
            if not hasattr(hparams, rq):
                raise IOError(rq + " is required to create the conv algorithm.")
        params = DictionaryUtility.to_dict(hparams.conv_params) if hasattr(hparams, "conv_params") else {}
        # fused=True: the stack runs on the conv-stack kernels (wfs_conv2d_*) where they take it
        self.model = Conv2DBlock(size[2], hparams.out_planes, hparams.n_conv, size, fused=True, **params)
        size = self.model.out_size
        flat_size = 1
        for s in size:
            flat_size = flat_size * s
        self.n_linear = flat_size
        head = LinearBlock(flat_size, n_classes, hparams.n_lin)
        self.linear_widths = head.widths
        self.linear = head.func

    def forward(self, x):
        coords, feats = x[0], x[1]
        n_valid = x[2] if len(x) > 2 else None
        batch_size = self.batch_size_hint
        if batch_size is None:
            if n_valid is not None:
                raise RuntimeError("DenseConvNet: a capacity-padded batch needs batch_size_hint (its last coordinate row "
                                   "is padding)")
            batch_size = int(coords[-1, -1]) + 1          # one device->host read, as the reference's
        C = self.nsamples * 2
        if feats.is_cuda and feats.dtype in (torch.float32, torch.bfloat16, torch.float16):
            dense = densify_rows(feats, coords, int(batch_size), self.x, self.y, n_valid)
            if self.model.can_fuse(dense) is None and n_valid is not None:
                raise RuntimeError("DenseConvNet: a valid-row count needs the conv-stack kernels, and they do not take "
                                   "this call")
            out = self.model(dense)
        else:
            if n_valid is not None:
                raise RuntimeError("DenseConvNet: a valid-row count needs the GPU kernels (the dense map is built from "
                                   "the valid rows only)")
            index = torch.transpose(coords[:, [2, 0, 1]].long(), 0, 1)
            sparse = torch.sparse_coo_tensor(index, feats, size=[batch_size, self.x, self.y, C], device=coords.device)
            out = self.model(torch.permute(sparse.to_dense(), self.dense_permute))
        out = out.reshape(-1, self.n_linear) if not out.is_contiguous() else out.view(-1, self.n_linear)
        if out.is_cuda:
            from ..spconv import functional as fsp
            return fsp.head_forward(out, self.linear)     # per layer: streaming / matrix-core HIP kernels or torch
        head_dtype = next(self.linear.parameters()).dtype
        if out.dtype != head_dtype:
            out = out.to(head_dtype)
        return self.linear(out)
