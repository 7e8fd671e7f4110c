"""``spconv.pool`` counterpart: SparseMaxPool and its thin subclasses (spconv 1.2.1).  The reference constructs no
pool; a config's ``algorithm`` list can name one ("spconv.SparseMaxPool3d", [[1, 1, 4], [1, 1, 4]])."""
from . import functional as Fsp
from . import ops
from .modules import SparseModule
from .tensor import SparseConvTensor


class SparseMaxPool(SparseModule, ops.StickyFlags):
    """Max pool over the active sites: the output set, its order and its shape are those of a ``SparseConv`` of the same
    geometry (``subm=True``: of a ``SubMConv``).  No parameters, no ``indice_key``: the pool builds its own rulebook.
    As in spconv the output row starts at ZERO: ``y = max(0, active neighbours)``, the plain maximum only for non-negative rows."""

    def __init__(self, ndim, kernel_size, stride=1, padding=0, dilation=1, subm=False):
        super(SparseMaxPool, self).__init__()
        self.ndim = ndim
        self.kernel_size = ops._listify(kernel_size, ndim)
        self.stride = ops._listify(stride, ndim)
        self.padding = ops._listify(padding, ndim)
        self.dilation = ops._listify(dilation, ndim)
        self.subm = subm
        for d, s in zip(self.dilation, self.stride):
            assert any([s == 1, d == 1]), "don't support this."

    def calibration_count(self):
        """A strided pool's output rows in its last build (its capacity in a captured step follows them)."""
        if self.subm:
            return None
        return self.last_rulebook.M

    def forward(self, input):
        assert isinstance(input, SparseConvTensor)
        features = input.features
        indices = input.indices
        spatial_shape = input.spatial_shape
        batch_size = input.batch_size
        if not self.subm:
            out_spatial_shape = ops.get_conv_output_size(spatial_shape, self.kernel_size, self.stride, self.padding,
                                                         self.dilation)
        else:
            out_spatial_shape = spatial_shape
        pre = getattr(input, "prefetched", None)
        if pre is not None and id(self) in pre:
            rb = pre[id(self)]                  # built on the side stream by SparseSequential's prefetch
            if rb.ready is not None:
                rb.ready.wait()
        else:
            rb = ops.build_rulebook(indices, batch_size, spatial_shape, self.kernel_size, self.stride, self.padding,
                                    self.dilation, self.subm, known_unique=input.unique, n_dev=input.n_valid,
                                    out_capacity=getattr(self, "out_capacity", None),
                                    events=getattr(input, "events", None), flags=self._sticky_flags(),
                                    want_cell_map=getattr(input, "dense_follows", True))
            if getattr(rb, "events_in", None) is not None:
                input.events = rb.events_in          # the offsets of this row set, for the layers that follow
        self.last_rulebook = rb          # capacity calibration / overflow checks of graph-captured steps
        input.unique = not rb.has_dup
        out_features = Fsp.indice_maxpool(features, rb)
        out_tensor = SparseConvTensor(out_features, rb.out_indices, out_spatial_shape, batch_size)
        out_tensor.indice_dict = input.indice_dict
        out_tensor.grid = input.grid
        out_tensor.unique = input.unique if self.subm else True      # a regular rulebook numbers DISTINCT output sites
        out_tensor.n_valid = rb.m_dev
        out_tensor.prefetched = pre
        if self.subm:
            out_tensor.events = getattr(input, "events", None)          # same row set, same event offsets
        else:
            if getattr(rb, "events_out", None) is not None:
                out_tensor.events = rb.events_out                       # the event-local build numbered them by event
            out_tensor.cell_map = getattr(rb, "cell_map", None)         # dense() of THIS row set can use the build's map
        return out_tensor


class SparseMaxPool2d(SparseMaxPool):
    def __init__(self, kernel_size, stride=1, padding=0, dilation=1):
        super(SparseMaxPool2d, self).__init__(2, kernel_size, stride, padding, dilation)


class SparseMaxPool3d(SparseMaxPool):
    def __init__(self, kernel_size, stride=1, padding=0, dilation=1):
        super(SparseMaxPool3d, self).__init__(3, kernel_size, stride, padding, dilation)
