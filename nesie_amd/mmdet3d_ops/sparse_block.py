"""``make_sparse_convmodule`` and ``SparseBasicBlock`` (the role of
``mmdet3d/ops/sparse_block.py:67-185``), self-contained: no registry, the three real sparse layers
by name and ``BN1d`` as the norm."""
from torch import nn

from . import spconv

_CONV_TYPES = {'SubMConv3d': spconv.SubMConv3d, 'SparseConv3d': spconv.SparseConv3d,
               'SparseInverseConv3d': spconv.SparseInverseConv3d}


def _build_conv(cfg, in_channels, out_channels, kernel_size, **kwargs):
    cfg = dict(type='SubMConv3d') if cfg is None else dict(cfg)
    conv_type = cfg.pop('type')
    if conv_type not in _CONV_TYPES:
        raise NotImplementedError(f'sparse conv type {conv_type!r} is not built; choose among '
                                  f'{sorted(_CONV_TYPES)}')
    return _CONV_TYPES[conv_type](in_channels, out_channels, kernel_size, **cfg, **kwargs)


def _build_norm(cfg, num_features):
    cfg = dict(type='BN1d') if cfg is None else dict(cfg)
    norm_type = cfg.pop('type')
    if norm_type != 'BN1d':
        raise NotImplementedError(f'norm type {norm_type!r} is not built for sparse modules; '
                                  "use dict(type='BN1d', ...)")
    requires_grad = cfg.pop('requires_grad', True)
    cfg.setdefault('eps', 1e-5)
    layer = nn.BatchNorm1d(num_features, **cfg)
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return layer


class SparseBasicBlock(spconv.SparseModule):
    """The residual block of Part-A^2's sparse encoder: two 3 x 3 x 3 submanifold convs with
    BatchNorm1d, ReLU after the first and after the residual sum.  State-dict keys are those of
    mmdet's ``BasicBlock``: conv1.weight, bn1.*, conv2.weight, bn2.*, downsample.*."""

    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, conv_cfg=None, norm_cfg=None):
        super().__init__()
        self.bn1 = _build_norm(norm_cfg, planes)
        self.bn2 = _build_norm(norm_cfg, planes)
        self.conv1 = _build_conv(conv_cfg, inplanes, planes, 3, stride=stride, padding=1,
                                 bias=False)
        self.conv2 = _build_conv(conv_cfg, planes, planes, 3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    @property
    def norm1(self):
        return self.bn1

    @property
    def norm2(self):
        return self.bn2

    def forward(self, x):
        identity = x.features
        assert x.features.dim() == 2, f'x.features.dim()={x.features.dim()}'
        out = self.conv1(x)
        out.features = self.relu(self.norm1(out.features))
        out = self.conv2(out)
        out.features = self.norm2(out.features)
        if self.downsample is not None:
            identity = self.downsample(x)
        out.features = self.relu(out.features + identity)
        return out


def make_sparse_convmodule(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0,
                           conv_type='SubMConv3d', norm_cfg=None, order=('conv', 'norm', 'act')):
    """-> ``spconv.SparseSequential`` of a sparse conv (no bias), its norm and a ReLU in ``order``
    (a sequence drawn from 'conv', 'norm', 'act')."""
    assert isinstance(order, tuple) and len(order) <= 3
    assert set(order) | {'conv', 'norm', 'act'} == {'conv', 'norm', 'act'}
    conv_cfg = dict(type=conv_type, indice_key=indice_key)
    layers = []
    for layer in order:
        if layer == 'conv':
            if conv_type == 'SparseInverseConv3d':
                layers.append(_build_conv(conv_cfg, in_channels, out_channels, kernel_size,
                                          bias=False))
            else:
                layers.append(_build_conv(conv_cfg, in_channels, out_channels, kernel_size,
                                          stride=stride, padding=padding, bias=False))
        elif layer == 'norm':
            layers.append(_build_norm(norm_cfg, out_channels))
        elif layer == 'act':
            layers.append(nn.ReLU(inplace=True))
    return spconv.SparseSequential(*layers)
