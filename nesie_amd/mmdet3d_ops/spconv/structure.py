"""``SparseConvTensor`` and ``scatter_nd`` (the role of ``mmdet3d/ops/spconv/structure.py``).
Pure torch: both work on CPU tensors."""
import numpy as np
import torch


def scatter_nd(indices, updates, shape):
    """zeros(shape) with ``updates`` written at ``indices`` (..., ndim): the leading ``ndim``
    dimensions of the result are addressed, the rest is copied.  Repeated rows are not summed."""
    ret = torch.zeros(*shape, dtype=updates.dtype, device=updates.device)
    ndim = indices.shape[-1]
    flat = indices.reshape(-1, ndim)
    tail = list(shape[ndim:])
    ret[tuple(flat[:, d] for d in range(ndim))] = updates.reshape([flat.shape[0]] + tail)
    return ret


class SparseConvTensor:
    """features (N, C), indices (N, 1 + ndim) int32 rows (batch, z, y, x), the grid
    ``spatial_shape`` and ``batch_size``.  ``indice_dict`` carries the rulebooks of the layers
    that named an ``indice_key``; ``grid`` is kept for interface parity only (the rulebook here
    never uses a dense grid, and a layer refuses a tensor that brings one)."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.features = features
        self.indices = indices if indices.dtype == torch.int32 else indices.int()
        self.spatial_shape = spatial_shape
        self.batch_size = batch_size
        self.indice_dict = {}
        self.grid = grid

    @property
    def spatial_size(self):
        return np.prod(self.spatial_shape)

    def find_indice_pair(self, key):
        if key is None:
            return None
        return self.indice_dict.get(key)

    def dense(self, channels_first=True):
        shape = [self.batch_size] + list(self.spatial_shape) + [self.features.shape[1]]
        res = scatter_nd(self.indices.long(), self.features, shape)
        if not channels_first:
            return res
        ndim = len(self.spatial_shape)
        order = [0, ndim + 1] + list(range(1, ndim + 1))
        return res.permute(*order).contiguous()

    @property
    def sparity(self):
        return self.indices.shape[0] / np.prod(self.spatial_shape) / self.batch_size
