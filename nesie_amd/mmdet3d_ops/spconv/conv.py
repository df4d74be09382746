"""The sparse convolution layers (the role of ``mmdet3d/ops/spconv/conv.py``): ``SubMConv3d``,
``SparseConv3d`` and ``SparseInverseConv3d`` are real; the other names of the reference's package
import and refuse construction."""
import math

import numpy as np
import torch
from torch.nn import init
from torch.nn.parameter import Parameter

from . import functional as Fsp
from . import ops
from ..roiaware_pool3d import _hip_backend
from .modules import SparseModule
from .structure import SparseConvTensor


def _calculate_fan_in_and_fan_out_hwio(tensor):
    """Fans of a weight stored (*kernel, in, out)."""
    if tensor.dim() < 2:
        raise ValueError('fan in and fan out can not be computed for tensor with fewer than 2 '
                         'dimensions')
    receptive_field = tensor[..., 0, 0].numel() if tensor.dim() > 2 else 1
    return tensor.size(-2) * receptive_field, tensor.size(-1) * receptive_field


def _as_list(v, ndim):
    return list(v) if isinstance(v, (list, tuple)) else [v] * ndim


class SparseConvolution(SparseModule):

    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0,
                 dilation=1, groups=1, bias=True, subm=False, output_padding=0, transposed=False,
                 inverse=False, indice_key=None, fused_bn=False):
        super().__init__()
        name = type(self).__name__
        if ndim != 3:
            raise NotImplementedError(f'{name}: only 3 spatial dimensions are built')
        if groups != 1:
            raise NotImplementedError(f'{name}: groups other than 1 are not built')
        if transposed:
            raise NotImplementedError(f'{name}: transposed sparse convolution is not built')
        if fused_bn:
            raise NotImplementedError(f'{name}: fused_bn is not built')
        kernel_size, stride = _as_list(kernel_size, ndim), _as_list(stride, ndim)
        padding, dilation = _as_list(padding, ndim), _as_list(dilation, ndim)
        output_padding = _as_list(output_padding, ndim)
        if any(d != 1 for d in dilation):
            raise NotImplementedError(f'{name}: dilation other than 1 is not built')
        if inverse and indice_key is None:
            raise ValueError(f'{name}: an inverse conv needs the indice_key of its partner')

        self.ndim = ndim
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.conv1x1 = np.prod(kernel_size) == 1
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.transposed = transposed
        self.inverse = inverse
        self.output_padding = output_padding
        self.groups = groups
        self.subm = subm
        self.indice_key = indice_key
        self.fused_bn = fused_bn

        self.weight = Parameter(torch.empty(*kernel_size, in_channels, out_channels))
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in, _ = _calculate_fan_in_and_fan_out_hwio(self.weight)
            bound = 1 / math.sqrt(fan_in)
            init.uniform_(self.bias, -bound, bound)

    def forward(self, input):
        assert isinstance(input, SparseConvTensor)
        name = type(self).__name__
        features, indices = input.features, input.indices
        datas = input.find_indice_pair(self.indice_key)
        if self.inverse and not self.conv1x1:
            if datas is None:
                raise ValueError(f'{name}: no conv with indice_key={self.indice_key!r} ran before '
                                 'this inverse conv')
            if datas[2].kvol != np.prod(self.kernel_size):
                raise ValueError(f'{name}: an inverse conv must have the kernel size of its '
                                 'partner')
        _hip_backend(name, features)
        if input.grid is not None:
            raise NotImplementedError(f'{name}: the rulebook uses no dense grid; drop it with '
                                      'RemoveGrid or build the tensor with grid=None')
        if features.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {features.dtype} (fp16 is not '
                                      'built)')
        spatial_shape, batch_size = input.spatial_shape, input.batch_size
        if self.subm:
            out_spatial_shape = spatial_shape
        else:
            out_spatial_shape = ops.get_conv_output_size(spatial_shape, self.kernel_size,
                                                         self.stride, self.padding, self.dilation)
        if self.conv1x1:
            features = torch.mm(features, self.weight.view(self.in_channels, self.out_channels))
            if self.bias is not None:
                features = features + self.bias
            out_tensor = SparseConvTensor(features, indices, spatial_shape, batch_size)
            out_tensor.indice_dict = input.indice_dict
            out_tensor.grid = input.grid
            return out_tensor
        if self.inverse:
            _, outids, rules, pair_num, out_spatial_shape = datas
        elif self.indice_key is not None and datas is not None:
            outids, _, rules, pair_num, _ = datas
        else:
            outids, rules, pair_num = ops.get_indice_pairs(
                indices, batch_size, spatial_shape, self.kernel_size, self.stride, self.padding,
                self.dilation, self.output_padding, self.subm, self.transposed, grid=input.grid)
            input.indice_dict[self.indice_key] = (outids, indices, rules, pair_num, spatial_shape)
        rules = rules.to(features.device)
        if self.subm:
            out_features = Fsp.indice_subm_conv(features, self.weight, rules, pair_num,
                                                outids.shape[0])
        elif self.inverse:
            out_features = Fsp.indice_inverse_conv(features, self.weight, rules, pair_num,
                                                   outids.shape[0])
        else:
            out_features = Fsp.indice_conv(features, self.weight, rules, pair_num, outids.shape[0])
        if self.bias is not None:
            out_features = out_features + self.bias
        out_tensor = SparseConvTensor(out_features, outids, out_spatial_shape, batch_size)
        out_tensor.indice_dict = input.indice_dict
        out_tensor.grid = input.grid
        return out_tensor


class SparseConv3d(SparseConvolution):

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation,
                         groups, bias, indice_key=indice_key)


class SubMConv3d(SparseConvolution):

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias=True, indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation,
                         groups, bias, True, indice_key=indice_key)


class SparseInverseConv3d(SparseConvolution):

    def __init__(self, in_channels, out_channels, kernel_size, indice_key, bias=True):
        super().__init__(3, in_channels, out_channels, kernel_size, bias=bias, inverse=True,
                         indice_key=indice_key)


def _not_built(name, what):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f'mmdet3d.ops.spconv.{name}: {what} is not built; the real '
                                  'layers are SubMConv3d, SparseConv3d and SparseInverseConv3d')
    return type(name, (SparseModule,), {'__init__': __init__, '__doc__': f'{what}: not built.'})


SparseConv2d = _not_built('SparseConv2d', '2-D sparse convolution')
SubMConv2d = _not_built('SubMConv2d', '2-D submanifold convolution')
SparseConvTranspose2d = _not_built('SparseConvTranspose2d', 'transposed sparse convolution')
SparseConvTranspose3d = _not_built('SparseConvTranspose3d', 'transposed sparse convolution')
SparseInverseConv2d = _not_built('SparseInverseConv2d', '2-D inverse sparse convolution')
SparseMaxPool2d = _not_built('SparseMaxPool2d', 'sparse max pooling')
SparseMaxPool3d = _not_built('SparseMaxPool3d', 'sparse max pooling')
