"""``GraphNet``: mirror of the reference's graph net (src/models/GraphNet.py:83-243) for the slice its example configs
use -- ``graph_class_index`` 11, torch_geometric's ``FiLMConv``, on the ``k`` nearest neighbours of every segment inside
its event (config/examples/IoniClassifierGraph.json under LitSegClassifier, SegQuantifier.json under LitSegQuantifier).

Constructor, plane arithmetic, ``IOError``s, module tree and parameter names are the reference's, so a reference
checkpoint's ``state_dict`` loads: ``graph_layers.{i}.graph_net.{lins.0, films.0, lin_skip, film_skip}``,
``graph_layers.{i}.batchnorm.module`` (torch_geometric's ``BatchNorm`` holds a ``BatchNorm1d`` as ``.module``) and
``linear.*`` (``LinearBlock``) when ``n_lin > 0``.  Every other ``graph_class_index`` raises ``NotImplementedError`` naming
the torch_geometric class it stands for; PointNet, Graph3DNet, SingleEndedEZGraph, GraphZ, the ``Data`` batch form and
GraphDataModule are out of scope.

torch_geometric and torch_cluster are not available to compare with: the layer and the neighbour rule are RESTATED
(parity unpinned).  Per layer, with nbr(i) the neighbours of row i and deg_i their number:

    s = x . lin_skip^T        (bs, gs) = split(x . film_skip^T)            first half beta, second half gamma; no bias
    h = x . lins.0^T          (b, g)   = split(x . films.0^T + bias)
    out_i = relu(gs_i * s_i + bs_i) + (1 / deg_i) sum_{j in nbr(i)} relu(g_i * h_j + b_i)
    x' = relu(BatchNorm1d(out))        batch statistics over the valid rows; also after the LAST layer (final_norm)

On the GPU a layer is: ONE dense product onto the six column blocks s | bs | gs | h | b | g (spconv.functional
.pointwise_conv: csrc/wide.hip from 128 channels, the generic MFMA kernel below) of the four weights laid side by side,
the message kernel (csrc/graphconv.hip) and the BatchNorm1d + ReLU kernels (csrc/bn.hip).  Without ``final_norm`` the
reference still applies a ReLU; ``out`` is a sum of ReLU outputs, so that ReLU changes nothing and is not launched.
The neighbour tables are built once per forward (two launches) and have a fixed size, so the net sits in a captured
step: ``forward([c, f, n_valid])`` takes the device-side count of valid rows; rows at and beyond it have no edges, are
nobody's neighbour, stay out of the BatchNorm statistics and come back as zeros.  There is no CPU path.

Row types.  fp32 and fp16 rows run through the layers as they are.  bf16 rows are widened to fp32 once at the net's
input, the layers run on fp32 rows and the result is rounded back to bf16: with bf16 STORAGE between the layers
(weights, product rows, message rows and layer outputs each rounded to 8 bits of mantissa) five FiLM + BatchNorm layers
leave the output 2e-2 .. 7e-2 of its largest magnitude away from float64 and the parameter gradients up to 0.7 of theirs
-- measured on the kernels and reproduced by a float64 model of the format alone -- which is of no use for
training.  The message kernels themselves take all three row types.
"""
import logging

import torch
from torch import nn
from torch.autograd import Function

from .. import _lib
from .blocks import LinearBlock
from .config import DictionaryUtility

# the table of reference GraphNet.retrieve_class (GraphNet.py:279-315)
GRAPH_CLASSES = ["GCNConv", "SAGEConv", "GraphConv", "GATConv", "GATv2Conv", "TransformerConv", "TAGConv", "GINConv",
                 "ARMAConv", "SGConv", "GMMConv", "FiLMConv", "EdgeConv", "FeaStConv", "LEConv", "ClusterGCNConv",
                 "GENConv", "SuperGATConv"]
FILM_INDEX = 11
KMAX = 8                  # neighbours per row the tables hold (csrc/wfs_graphknn.h; checked against the library on first use)

# launches of the HIP path since import, by kind (tests: the HIP path ran; there is no other)
LAUNCHES = {"knn": 0, "message_fwd": 0, "message_bwd": 0, "event_max_fwd": 0, "event_max_bwd": 0, "zero_tail": 0}


def graph_planes(feat_size, n_graph, n_expansion, expansion_factor, graph_out, reduction_type="linear"):
    """The reference's channel plan, its integer arithmetic included (GraphNet.py:162-192)."""
    planes = [feat_size]
    n_contract = n_graph - n_expansion
    if reduction_type == "linear":
        if n_expansion > 0:
            exp = int((planes[0] * expansion_factor - planes[0]) / n_expansion)
            for _ in range(n_expansion):
                planes.append(planes[-1] + exp)
            if n_contract > 0:
                red = int((planes[-1] - graph_out) / n_contract)
                for _ in range(n_contract):
                    planes.append(planes[-1] - red)
        else:
            red = int((planes[0] - graph_out) / n_graph)
            for _ in range(n_graph):
                planes.append(planes[-1] - red)
    elif reduction_type == "geometric":
        if n_expansion > 0:
            exp = float(expansion_factor) ** (1. / n_expansion)
            for _ in range(n_expansion):
                planes.append(int(planes[-1] * exp))
            if n_contract > 0:
                red = float(graph_out / planes[-1]) ** (1. / n_contract)
                for _ in range(n_contract):
                    planes.append(int(planes[-1] * red))
        else:
            red = float(graph_out / planes[0]) ** (1. / n_graph)
            for _ in range(n_graph):
                planes.append(int(planes[-1] * red))
    else:
        raise IOError("net_config.hparams.reduction_type must be either linear or geometric")
    planes[-1] = int(graph_out)
    return planes


# ---- the HIP calls --------------------------------------------------------------------------------------------------
class NeighbourTables(object):
    """nbr [N, KMAX] / deg [N] and the reverse lists of one batch (include/wfsparse.h wfs_graph_knn)."""

    def __init__(self, coords, k, self_loop, n_dev=None):
        lib = _lib.load()
        assert int(lib.wfs_graph_kmax()) == KMAX
        if not coords.is_cuda:
            raise RuntimeError("waveformml_amd.psd.graphnet: coordinates must be on the GPU (there is no CPU path)")
        if coords.dim() != 2 or coords.shape[1] != 3:
            raise RuntimeError("GraphNet takes coordinates [N, 3] = (x, y, event), got %s" % (tuple(coords.shape),))
        if coords.dtype != torch.int32 or not coords.is_contiguous():
            coords = coords.to(torch.int32).contiguous()
        N, dev = int(coords.shape[0]), coords.device
        self.coords, self.n_dev, self.N = coords, n_dev, N
        self.nbr = torch.empty((N, KMAX), dtype=torch.int32, device=dev)
        self.deg = torch.empty((N,), dtype=torch.int32, device=dev)
        self.rev_pos = torch.empty((N, 2), dtype=torch.int32, device=dev)
        self.rev_rows = torch.empty((max(N * KMAX, 1),), dtype=torch.int32, device=dev)
        _lib.check(lib.wfs_graph_knn(_lib.ptr(coords), N, _lib.ptr(n_dev), int(k), 1 if self_loop else 0,
                                     _lib.ptr(self.nbr), _lib.ptr(self.deg), _lib.ptr(self.rev_pos),
                                     _lib.ptr(self.rev_rows), _lib.stream_ptr()))
        LAUNCHES["knn"] += 1


def knn_host(coords, k, self_loop=False, n_valid=None):
    """(nbr [N, KMAX], deg [N]) of HOST coordinates by the library's selection rule (wfs_graph_knn_host): the same
    function the device kernel calls, for checks without a GPU."""
    lib = _lib.load()
    coords = coords.to(torch.int32).contiguous().cpu()
    N = int(coords.shape[0])
    nbr = torch.empty((N, KMAX), dtype=torch.int32)
    deg = torch.empty((N,), dtype=torch.int32)
    _lib.check(lib.wfs_graph_knn_host(coords.data_ptr(), N, N if n_valid is None else int(n_valid), int(k),
                                      1 if self_loop else 0, nbr.data_ptr(), deg.data_ptr()))
    return nbr, deg


class FiLMMessageFunction(Function):
    """out [N, D] from the product rows P [N, 6 D] (s | bs | gs | h | b | g) over the tables of the batch."""

    @staticmethod
    def forward(ctx, P, tables):
        lib = _lib.load()
        if not P.is_cuda:
            raise RuntimeError("waveformml_amd.psd.graphnet: rows must be on the GPU (there is no CPU path)")
        P = P.contiguous()
        N, D = int(P.shape[0]), int(P.shape[1]) // 6
        assert P.shape[1] == 6 * D and N == tables.N
        out = torch.empty((N, D), dtype=P.dtype, device=P.device)
        _lib.check(lib.wfs_film_message_fwd(_lib.ptr(P), _lib.ptr(tables.nbr), _lib.ptr(tables.deg), N, D, _lib.ptr(out),
                                            _lib.dtype_code(P), _lib.ptr(tables.n_dev), _lib.stream_ptr()))
        LAUNCHES["message_fwd"] += 1
        ctx.save_for_backward(P)
        ctx.tables = tables
        return out

    @staticmethod
    def backward(ctx, grad_output):
        from ..spconv.functional import as_grad
        lib = _lib.load()
        (P,), t = ctx.saved_tensors, ctx.tables
        N, D = int(P.shape[0]), int(P.shape[1]) // 6
        dout = as_grad(grad_output, P.dtype)
        # rows beyond a device-side count are not written, and nothing downstream (the product's backward takes the same
        # count) reads them
        dP = torch.empty_like(P)
        _lib.check(lib.wfs_film_message_bwd(_lib.ptr(P), _lib.ptr(dout), _lib.ptr(t.nbr), _lib.ptr(t.deg),
                                            _lib.ptr(t.rev_pos), _lib.ptr(t.rev_rows), N, D, _lib.ptr(dP),
                                            _lib.dtype_code(P), _lib.ptr(t.n_dev), _lib.stream_ptr()))
        LAUNCHES["message_bwd"] += 1
        return dP, None


def film_message(P, tables):
    return FiLMMessageFunction.apply(P, tables)


class ZeroTailFunction(Function):
    """Rows at and beyond the device-side count := 0, in place (what the net hands back for a captured batch's padding);
    their gradient is nobody's business: the layers' backward passes take the same count."""

    @staticmethod
    def forward(ctx, x, n_dev):
        _lib.check(_lib.load().wfs_rows_zero_tail(_lib.ptr(x), int(x.shape[0]), int(x.shape[1]), _lib.dtype_code(x),
                                                  _lib.ptr(n_dev), _lib.stream_ptr()))
        LAUNCHES["zero_tail"] += 1
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output, None


class EventMaxFunction(Function):
    """torch_geometric's ``global_max_pool`` over the event column: [N, D] -> [B, D]; the first row wins a tie, an event
    without rows gives a zero row and passes no gradient."""

    @staticmethod
    def forward(ctx, x, coords, batch_size, n_dev):
        lib = _lib.load()
        if not x.is_cuda:
            raise RuntimeError("waveformml_amd.psd.graphnet: rows must be on the GPU (there is no CPU path)")
        x = x.contiguous()
        N, D, B = int(x.shape[0]), int(x.shape[1]), int(batch_size)
        y = torch.empty((B, D), dtype=x.dtype, device=x.device)
        arg = torch.empty((B, D), dtype=torch.int32, device=x.device)
        _lib.check(lib.wfs_event_max_fwd(_lib.ptr(coords), _lib.ptr(x), N, D, B, _lib.ptr(y), _lib.ptr(arg),
                                         _lib.dtype_code(x), _lib.ptr(n_dev), _lib.stream_ptr()))
        LAUNCHES["event_max_fwd"] += 1
        ctx.save_for_backward(arg, coords)
        ctx.shape, ctx.n_dev = (N, D, B), n_dev
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, grad_y, _grad_arg):
        from ..spconv.functional import as_grad
        lib = _lib.load()
        arg, coords = ctx.saved_tensors
        N, D, B = ctx.shape
        dy = as_grad(grad_y, grad_y.dtype)
        dx = torch.empty((N, D), dtype=dy.dtype, device=dy.device)
        _lib.check(lib.wfs_event_max_bwd(_lib.ptr(coords), _lib.ptr(dy), _lib.ptr(arg), N, D, B, _lib.ptr(dx),
                                         _lib.dtype_code(dy), _lib.ptr(ctx.n_dev), _lib.stream_ptr()))
        LAUNCHES["event_max_bwd"] += 1
        return dx, None, None, None


def event_max(x, coords, batch_size, n_dev=None):
    """(max [B, D], winning row int32 [B, D]) per event and channel."""
    return EventMaxFunction.apply(x, coords, batch_size, n_dev)


# ---- the modules, named as the reference's ----------------------------------------------------------------------------
class FiLMConv(nn.Module):
    """torch_geometric.nn.FiLMConv(in_channels, out_channels) with its defaults (one relation, ReLU, mean aggregation),
    restated: parameters ``lins.0.weight [D, C]``, ``films.0.{weight [2 D, C], bias [2 D]}``, ``lin_skip.weight [D, C]``,
    ``film_skip.weight [2 D, C]``, each initialised as a ``torch.nn.Linear``."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False)])
        self.films = nn.ModuleList([nn.Linear(in_channels, 2 * out_channels)])
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False)
        self.film_skip = nn.Linear(in_channels, 2 * out_channels, bias=False)

    def jittable(self):
        return self

    def filters(self):
        """([C, 6 D] filter, [6 D] bias) of the layer's one product: the four weights side by side, in the column order
        the message kernel reads (s | bs | gs | h | b | g).  One concatenation writes the filter as the product reads
        it (contiguous [C, 6 D]: no transposed copy follows), one padding launch the bias."""
        D = self.out_channels
        w = torch.cat([self.lin_skip.weight.t(), self.film_skip.weight.t(), self.lins[0].weight.t(),
                       self.films[0].weight.t()], dim=1)
        return w, torch.nn.functional.pad(self.films[0].bias, (4 * D, 0))

    def forward(self, x, tables):
        from ..spconv.functional import pointwise_conv
        w, bias = self.filters()
        return film_message(pointwise_conv(x, w, bias, tables.n_dev), tables)


class BatchNorm(nn.Module):
    """torch_geometric.nn.BatchNorm: a ``torch.nn.BatchNorm1d`` held as ``.module``."""

    def __init__(self, in_channels):
        super().__init__()
        self.module = nn.BatchNorm1d(in_channels)


class GraphLayer(nn.Module):
    """Reference GraphLayer (GraphNet.py:43-79) for a layer without edge attributes: graph_net, [batchnorm], ReLU."""

    def __init__(self, net, batchnorm=None):
        super().__init__()
        self.graph_net = net
        self.batchnorm = batchnorm

    def forward(self, x, tables):
        from ..spconv.functional import batch_norm_relu
        x = self.graph_net(x, tables)
        if self.batchnorm is not None:
            return batch_norm_relu(x, self.batchnorm.module, True, tables.n_dev)
        return x              # the reference's ReLU of a sum of ReLU outputs: the identity


class GraphNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.log = logging.getLogger(__name__)
        self.config = config
        self.lin_outputs = 0
        self.feat_size = self.config.system_config.n_samples * 2
        self.n_lin = 0
        self.n_graph = 0
        self.n_expansion = 0
        self.expansion_factor = 1.0
        hp = config.net_config.hparams
        if hasattr(hp, "n_graph"):
            self.n_graph = hp.n_graph
        elif hasattr(hp, "n_contract"):
            if not hasattr(hp, "n_expand"):
                raise IOError("if net_config.hparams.n_graph not specified, must specify n_expand and n_contract")
            self.n_graph = hp.n_contract + hp.n_expand
        else:
            raise IOError("if net_config.hparams.n_graph not specified, must specify n_expand and n_contract")
        if hasattr(hp, "expansion_factor"):
            self.expansion_factor = hp.expansion_factor
        if hasattr(hp, "n_expand"):
            self.n_expansion = hp.n_expand
        self.graph_index = hp.graph_class_index
        self.graph_class = self.retrieve_class(self.graph_index)
        if hasattr(hp, "n_lin"):
            self.n_lin = hp.n_lin
            if hasattr(config.system_config, "n_type"):
                self.lin_outputs = config.system_config.n_type
            elif hasattr(config.net_config, "n_out"):
                self.lin_outputs = config.net_config.n_out
            else:
                raise IOError("Need to specify system_config.n_type for classifier or net_config.n_out to determine "
                              "number of outputs of linear layer")
        self.k = hp.k if hasattr(hp, "k") else 6
        self.final_norm = hp.final_norm if hasattr(hp, "final_norm") else True
        self.graph_out = 10
        self.graph_params = {}
        if hasattr(hp, "graph_params"):
            self.graph_params = DictionaryUtility.to_dict(hp.graph_params)
        if self.graph_params:
            raise NotImplementedError("GraphNet: net_config.hparams.graph_params %r (FiLMConv is built with its defaults)"
                                      % (sorted(self.graph_params),))
        if hasattr(hp, "graph_out"):
            self.graph_out = hp.graph_out
        else:
            self.log.debug("no net_config.hparams.graph_out set, setting graph outputs default to {}".format(self.graph_out))
        self.pool_ratio = hp.pool_ratio if hasattr(hp, "pool_ratio") else 0.8
        self.use_self_loops = hp.self_loop if hasattr(hp, "self_loop") else False
        if self.n_lin > 0:
            self.linear = LinearBlock(self.graph_out, self.lin_outputs, self.n_lin).func
        else:
            self.linear = None
        self.edge_attr_dim = 2
        if hasattr(hp, "edge_transform"):
            # validated as the reference does; FiLMConv takes no edge attributes, so no transform is ever applied
            if hp.edge_transform not in ("cartesian", "localcartesian"):
                raise IOError("net_config.hparams.edge_transform must be one of 'cartesian', 'localcartesian'")
        self.reduction_type = hp.reduction_type if hasattr(hp, "reduction_type") else "linear"
        self.graph_planes = graph_planes(self.feat_size, self.n_graph, self.n_expansion, self.expansion_factor,
                                         self.graph_out, self.reduction_type)
        self.n_contract = self.n_graph - self.n_expansion
        self.uses_edge_attr = False
        if not 1 <= int(self.k) <= KMAX:
            raise NotImplementedError("GraphNet: k = %r; the neighbour tables hold 1 .. %d neighbours" % (self.k, KMAX))
        self.graph_layers = nn.ModuleList()
        for i in range(self.n_graph):
            nin, nout = self.graph_planes[i], self.graph_planes[i + 1]
            self.graph_layers.append(GraphLayer(self.graph_class(nin, nout).jittable(),
                                                batchnorm=BatchNorm(nout) if self.final_norm else None))
        self.batch_size_hint = None       # the number of events, when the caller knows it (LitPSD: one label per event)

    @staticmethod
    def retrieve_class(index):
        if index == FILM_INDEX:
            return FiLMConv
        if isinstance(index, int) and 0 <= index < len(GRAPH_CLASSES):
            raise NotImplementedError("GraphNet: graph_class_index %d is torch_geometric's %s; only index %d (FiLMConv) "
                                      "is built here" % (index, GRAPH_CLASSES[index], FILM_INDEX))
        raise NotImplementedError("GraphNet: graph_class_index %r names no class (0 .. %d)"
                                  % (index, len(GRAPH_CLASSES) - 1))

    def forward(self, data):
        if not isinstance(data, (list, tuple)):
            raise NotImplementedError("GraphNet: the torch_geometric Data batch form is out of scope; pass [c, f]")
        coords, x = data[0], data[1]
        n_valid = data[2] if len(data) > 2 else None
        if not (coords.is_cuda and x.is_cuda):
            raise RuntimeError("waveformml_amd.psd.graphnet: tensors must be on the GPU (there is no CPU path)")
        # bf16 rows are widened once here and the layers run on fp32 rows (module docstring); fp16 rows stay fp16
        rows_dtype = x.dtype
        if rows_dtype == torch.bfloat16:
            x = x.float()
        tables = NeighbourTables(coords, self.k, self.use_self_loops, n_valid)
        for layer in self.graph_layers:
            x = layer(x, tables)
        if self.n_lin > 0:
            from ..spconv.functional import head_forward
            batch_size = self.batch_size_hint
            if batch_size is None:
                if n_valid is not None:
                    raise RuntimeError("GraphNet: a capacity-padded batch needs batch_size_hint (its last coordinate row "
                                       "is padding)")
                batch_size = int(coords[-1, -1]) + 1          # one device->host read, as the reference's
            x = event_max(x, tables.coords, batch_size, n_valid)[0]
            x = head_forward(x, self.linear)
        elif n_valid is not None:
            x = ZeroTailFunction.apply(x, n_valid)
        return x if x.dtype == rows_dtype else x.to(rows_dtype)
