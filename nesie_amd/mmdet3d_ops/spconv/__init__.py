"""Mirror of ``mmdet3d.ops.spconv`` (same ``__all__``): sparse 3-D convolution on a sort-based
rulebook and a gather-GEMM in HIP (``csrc/sparse_conv.hip``; ``include/nesie_ops.h`` states the
semantics).  ``SubMConv3d``, ``SparseConv3d`` and ``SparseInverseConv3d`` are real; the 2-D,
transposed and pooling layers import and refuse construction.  Nothing here is launched by the
default training step."""
from .conv import (SparseConv2d, SparseConv3d, SparseConvTranspose2d, SparseConvTranspose3d,
                   SparseInverseConv2d, SparseInverseConv3d, SparseMaxPool2d, SparseMaxPool3d,
                   SubMConv2d, SubMConv3d)
from .modules import SparseModule, SparseSequential
from .structure import SparseConvTensor, scatter_nd

__all__ = [
    'SparseConv2d',
    'SparseConv3d',
    'SubMConv2d',
    'SubMConv3d',
    'SparseConvTranspose2d',
    'SparseConvTranspose3d',
    'SparseInverseConv2d',
    'SparseInverseConv3d',
    'SparseModule',
    'SparseSequential',
    'SparseMaxPool2d',
    'SparseMaxPool3d',
    'SparseConvTensor',
    'scatter_nd',
]
