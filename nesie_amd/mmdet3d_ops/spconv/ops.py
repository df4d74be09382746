"""Output sizes and the rulebook builder (the role of ``mmdet3d/ops/spconv/ops.py``).
``include/nesie_ops.h`` ("mmdet3d/ops/spconv") states the pinned semantics: the rulebook is two
gather tables built from sorted keys, not the reference's pair lists."""
import torch

from ..roiaware_pool3d import _hip_backend


def _ntuple(v, ndim):
    return [int(e) for e in v] if isinstance(v, (list, tuple)) else [int(v)] * ndim


def get_conv_output_size(input_size, kernel_size, stride, padding, dilation):
    ndim = len(input_size)
    output_size = []
    for i in range(ndim):
        size = (input_size[i] + 2 * padding[i] - dilation[i] * (kernel_size[i] - 1) - 1) \
            // stride[i] + 1
        if kernel_size[i] == -1:
            output_size.append(1)
        else:
            output_size.append(size)
    return output_size


def get_deconv_output_size(input_size, kernel_size, stride, padding, dilation, output_padding):
    ndim = len(input_size)
    output_size = []
    for i in range(ndim):
        if kernel_size[i] == -1:
            raise ValueError("deconv don't support kernel_size < 0")
        size = (input_size[i] - 1) * stride[i] - 2 * padding[i] + kernel_size[i] \
            + output_padding[i]
        output_size.append(size)
    return output_size


class Rules:
    """The rulebook of one geometry: ``nbr`` (M, K) int32, the input row output row o reads at
    tap k or -1, and ``nbr_t`` (N, K), the output row input row i feeds at tap k or -1."""

    __slots__ = ('nbr', 'nbr_t')

    def __init__(self, nbr, nbr_t):
        self.nbr, self.nbr_t = nbr, nbr_t

    @property
    def kvol(self):
        return int(self.nbr.shape[1])

    def to(self, device):
        if self.nbr.device == torch.device(device):
            return self
        return Rules(self.nbr.to(device), self.nbr_t.to(device))


def get_indice_pairs(indices, batch_size, spatial_shape, ksize=3, stride=1, padding=0, dilation=1,
                     out_padding=0, subm=False, transpose=False, grid=None):
    """indices (N, 4) int32 rows (b, z, y, x) -> (outids (M, 4), rules, pair_num (K)).  The one
    place that reads from the device: M and the count of offending rows (outside the grid, or a
    repeated site) in one copy; offending rows raise ValueError before any feature kernel runs."""
    backend = _hip_backend('get_indice_pairs', indices)
    if indices.dim() != 2 or indices.shape[1] != 4 or indices.dtype != torch.int32:
        raise TypeError(f'get_indice_pairs: indices must be int32 (N, 4) rows (b, z, y, x), got '
                        f'{indices.dtype} {tuple(indices.shape)} (3 spatial dimensions only)')
    ndim = 3
    ksize, stride, padding = _ntuple(ksize, ndim), _ntuple(stride, ndim), _ntuple(padding, ndim)
    if any(d != 1 for d in _ntuple(dilation, ndim)):
        raise NotImplementedError('get_indice_pairs: dilation other than 1 is not built')
    if transpose:
        raise NotImplementedError('get_indice_pairs: transposed convolution is not built')
    if grid is not None:
        raise NotImplementedError('get_indice_pairs: the rulebook uses no dense grid; pass grid=None')
    spatial_shape = [int(s) for s in spatial_shape]
    indices = indices.contiguous()
    n, kvol = int(indices.shape[0]), ksize[0] * ksize[1] * ksize[2]
    # refuses a grid of 2^31 cells or more before anything is allocated
    _, out_cells = backend.spconv_out_shape(spatial_shape, ksize, stride, padding, subm, batch_size)
    backend.spconv_rules_workspace_bytes(n, kvol, subm)
    new = indices.new_empty
    if n == 0:
        return (indices if subm else new((0, 4))), Rules(new((0, kvol)), new((0, kvol))), \
            indices.new_zeros((kvol,))
    sorted_keys, sorted_rows, counts = new((n,)), new((n,)), new((2,))
    nbr_t = new((n, kvol))                                               # written in full
    worst = None if subm else new((min(n * kvol, out_cells), 4))
    backend.spconv_out_sites(indices, batch_size, spatial_shape, ksize, stride, padding, subm,
                             sorted_keys, sorted_rows, nbr_t, worst, counts)
    m, bad = counts.tolist()
    if bad:
        raise ValueError(f'get_indice_pairs: {bad} of {n} rows of indices lie outside the '
                         f'{batch_size} x {tuple(spatial_shape)} grid or repeat an earlier site')
    outids = indices if subm else worst[:m].clone()                    # frees the worst case
    nbr, pair_num = new((m, kvol)), new((kvol,))
    if m:
        backend.spconv_gather_table(outids, sorted_keys, sorted_rows, batch_size, spatial_shape,
                                    ksize, stride, padding, subm, nbr, pair_num)
    else:
        pair_num.zero_()
    return outids, Rules(nbr, nbr_t), pair_num
