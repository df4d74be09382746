"""Mirror of ``mmdet3d/ops/pointnet_modules/paconv_sa_module.py``: the set-abstraction modules of
PAConv networks -- ``PointSAModule*`` with the shared MLP of every scale replaced by PAConv
layers.  ``PAConvSAModule{MSG,}`` (:10-149) run the torch-op ``PAConv`` on grouped features;
``PAConvCUDASAModule{MSG,}`` (:153-340) run ``PAConvCUDA`` on ungrouped features plus the
neighbour indices, pooling after every layer.  Constructor keywords and defaults are the
reference's; a caller's ``scorenet_cfg`` is copied, never modified."""
from collections import OrderedDict

import torch
from torch import nn

from .paconv import PAConv, PAConvCUDA
from .pointnet_modules import SA_MODULES, BasePointSAModule

_SCORENET = dict(mlp_channels=[16, 16, 16], score_norm='softmax', temp_factor=1.0, last_bn=False)
_SCORENET_CUDA = dict(mlp_channels=[8, 16, 16], score_norm='softmax', temp_factor=1.0,
                      last_bn=False)


def _paconv_layers(layer_cls, module, paconv_num_kernels, use_xyz, bias, norm_cfg,
                   paconv_kernel_input, scorenet_input, scorenet_cfg):
    """-> per scale, the list of ``layer_cls`` layers over ``module.mlp_channels`` (whose first
    width grows by 3 with ``use_xyz``).  In PAConv a bias exists in the ScoreNet only."""
    assert len(paconv_num_kernels) == len(module.mlp_channels)
    for kernels, widths in zip(paconv_num_kernels, module.mlp_channels):
        assert len(kernels) == len(widths) - 1, 'PAConv number of weight kernels wrong'
    scorenet_cfg = dict(scorenet_cfg, bias=bias)
    scales = []
    for widths, kernels in zip(module.mlp_channels, paconv_num_kernels):
        if use_xyz:
            widths[0] += 3
        scales.append([layer_cls(cin, cout, m, norm_cfg=norm_cfg, kernel_input=paconv_kernel_input,
                                 scorenet_input=scorenet_input, scorenet_cfg=scorenet_cfg)
                       for cin, cout, m in zip(widths, widths[1:], kernels)])
    return scales


class PAConvSAModuleMSG(BasePointSAModule):
    """Multi-scale grouping with ``PAConv`` layers: ``mlps.{scale}.layer{j}``;
    ``paconv_num_kernels[scale][j]`` is the bank size of layer j."""

    def __init__(self, num_point, radii, sample_nums, mlp_channels, paconv_num_kernels,
                 fps_mod=['D-FPS'], fps_sample_range_list=[-1], dilated_group=False,
                 norm_cfg=dict(type='BN2d', momentum=0.1), use_xyz=True, pool_mod='max',
                 normalize_xyz=False, bias='auto', paconv_kernel_input='w_neighbor',
                 scorenet_input='w_neighbor_dist', scorenet_cfg=_SCORENET):
        super().__init__(num_point=num_point, radii=radii, sample_nums=sample_nums,
                         mlp_channels=mlp_channels, fps_mod=fps_mod,
                         fps_sample_range_list=fps_sample_range_list, dilated_group=dilated_group,
                         use_xyz=use_xyz, pool_mod=pool_mod, normalize_xyz=normalize_xyz,
                         grouper_return_grouped_xyz=True)
        for layers in _paconv_layers(PAConv, self, paconv_num_kernels, use_xyz, bias, norm_cfg,
                                     paconv_kernel_input, scorenet_input, scorenet_cfg):
            self.mlps.append(nn.Sequential(OrderedDict(
                (f'layer{j}', layer) for j, layer in enumerate(layers))))

    def _forward(self, points_xyz, features, indices, target_xyz, precomputed):
        """The literal sequence of point_sa_module.py:182-211 (none of the base class's fused
        paths applies): every grouper returns (features, grouped xyz), the PAConv chain returns
        such a pair, and its first element is pooled."""
        assert precomputed is None, 'PAConv modules take no precomputed grouping'
        new_xyz, indices = self._sample_points(points_xyz, features, indices, target_xyz)
        pooled = [self._pool_features(mlp(grouper(points_xyz, new_xyz, features))[0])
                  for grouper, mlp in zip(self.groupers, self.mlps)]
        return new_xyz, torch.cat(pooled, dim=1), indices


class PAConvSAModule(PAConvSAModuleMSG):
    """The single-scale case (:108-149)."""

    def __init__(self, mlp_channels, paconv_num_kernels, num_point=None, radius=None,
                 num_sample=None, norm_cfg=dict(type='BN2d', momentum=0.1), use_xyz=True,
                 pool_mod='max', fps_mod=['D-FPS'], fps_sample_range_list=[-1],
                 normalize_xyz=False, paconv_kernel_input='w_neighbor',
                 scorenet_input='w_neighbor_dist', scorenet_cfg=_SCORENET):
        super().__init__(mlp_channels=[mlp_channels], paconv_num_kernels=[paconv_num_kernels],
                         num_point=num_point, radii=[radius], sample_nums=[num_sample],
                         norm_cfg=norm_cfg, use_xyz=use_xyz, pool_mod=pool_mod, fps_mod=fps_mod,
                         fps_sample_range_list=fps_sample_range_list, normalize_xyz=normalize_xyz,
                         paconv_kernel_input=paconv_kernel_input, scorenet_input=scorenet_input,
                         scorenet_cfg=scorenet_cfg)


class PAConvCUDASAModuleMSG(BasePointSAModule):
    """Multi-scale grouping with ``PAConvCUDA`` layers: ``mlps.{scale}.{j}``.  The layers take
    ungrouped features and the neighbour indices, so every layer is followed by the pooling
    over its K neighbours and the next layer groups the pooled centres around themselves."""

    def __init__(self, num_point, radii, sample_nums, mlp_channels, paconv_num_kernels,
                 fps_mod=['D-FPS'], fps_sample_range_list=[-1], dilated_group=False,
                 norm_cfg=dict(type='BN2d', momentum=0.1), use_xyz=True, pool_mod='max',
                 normalize_xyz=False, bias='auto', paconv_kernel_input='w_neighbor',
                 scorenet_input='w_neighbor_dist', scorenet_cfg=_SCORENET_CUDA):
        super().__init__(num_point=num_point, radii=radii, sample_nums=sample_nums,
                         mlp_channels=mlp_channels, fps_mod=fps_mod,
                         fps_sample_range_list=fps_sample_range_list, dilated_group=dilated_group,
                         use_xyz=use_xyz, pool_mod=pool_mod, normalize_xyz=normalize_xyz,
                         grouper_return_grouped_xyz=True, grouper_return_grouped_idx=True)
        self.use_xyz = use_xyz   # the coordinates join the features here, not in the grouper
        for layers in _paconv_layers(PAConvCUDA, self, paconv_num_kernels, use_xyz, bias, norm_cfg,
                                     paconv_kernel_input, scorenet_input, scorenet_cfg):
            self.mlps.append(nn.ModuleList(layers))

    def forward(self, points_xyz, features=None, indices=None, target_xyz=None):
        """points_xyz (B, N, 3), features (B, C, N) -> (new_xyz (B, M, 3), features
        (B, sum of the scales' last widths, M), indices (B, M))."""
        new_xyz, indices = self._sample_points(points_xyz, features, indices, target_xyz)
        pooled = []
        for grouper, layers in zip(self.groupers, self.mlps):
            xyz, new_features = points_xyz, features
            for j, layer in enumerate(layers):
                # only the coordinates and the indices are used: with use_xyz the grouper need not
                # gather the features at all
                _, grouped_xyz, grouped_idx = grouper(xyz, new_xyz,
                                                      None if grouper.use_xyz else new_features)
                if self.use_xyz and j == 0:
                    lead = points_xyz.permute(0, 2, 1)
                    new_features = lead if new_features is None else \
                        torch.cat((lead, new_features), dim=1)
                grouped = layer((new_features, grouped_xyz, grouped_idx.long()))[0]
                new_features = self._pool_features(grouped)   # (B, out, M)
                xyz = new_xyz   # the features now belong to the sampled centres
            pooled.append(new_features)
        return new_xyz, torch.cat(pooled, dim=1), indices


class PAConvCUDASAModule(PAConvCUDASAModuleMSG):
    """The single-scale case (:298-340)."""

    def __init__(self, mlp_channels, paconv_num_kernels, num_point=None, radius=None,
                 num_sample=None, norm_cfg=dict(type='BN2d', momentum=0.1), use_xyz=True,
                 pool_mod='max', fps_mod=['D-FPS'], fps_sample_range_list=[-1],
                 normalize_xyz=False, paconv_kernel_input='w_neighbor',
                 scorenet_input='w_neighbor_dist', scorenet_cfg=_SCORENET_CUDA):
        super().__init__(mlp_channels=[mlp_channels], paconv_num_kernels=[paconv_num_kernels],
                         num_point=num_point, radii=[radius], sample_nums=[num_sample],
                         norm_cfg=norm_cfg, use_xyz=use_xyz, pool_mod=pool_mod, fps_mod=fps_mod,
                         fps_sample_range_list=fps_sample_range_list, normalize_xyz=normalize_xyz,
                         paconv_kernel_input=paconv_kernel_input, scorenet_input=scorenet_input,
                         scorenet_cfg=scorenet_cfg)


SA_MODULES.update(PAConvSAModuleMSG=PAConvSAModuleMSG, PAConvSAModule=PAConvSAModule,
                  PAConvCUDASAModuleMSG=PAConvCUDASAModuleMSG,
                  PAConvCUDASAModule=PAConvCUDASAModule)
