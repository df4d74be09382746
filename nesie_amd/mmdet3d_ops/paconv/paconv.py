"""Mirror of ``mmdet3d/ops/paconv/paconv.py``: ``ScoreNet`` (:12-103), ``PAConv`` (:106-297) and
``PAConvCUDA`` (:300-385).  A PAConv layer keeps a bank of ``m`` weight matrices; a small MLP over
the relative position of every (centre, neighbour) pair predicts ``m`` scores, and the layer's
output for the pair is the score-weighted blend of the bank applied to the pair's features.
Module and parameter names are the reference's, so its checkpoints' keys line up."""
import copy
from collections import OrderedDict

import torch
from torch import nn
from torch.nn import functional as F

from ..norm import FusedBNReLU2d
from ..pointnet_modules import ConvModule
from .assign_score import assign_score_withk
from .utils import assign_kernel_withoutk, assign_score, calc_euclidian_dist

_DEFAULT_SCORENET = dict(mlp_channels=[8, 16, 16], score_norm='softmax', temp_factor=1.0,
                         last_bn=False)


class ScoreNet(nn.Module):
    """Shared MLP over per-pair position features (B, C, N, K) -> scores (B, N, K, M).  The last
    layer has no activation and a norm only with ``last_bn``; ``score_norm`` ('softmax' |
    'sigmoid' | 'identity') is taken over the M scores of a pair after division by
    ``temp_factor``."""

    def __init__(self, mlp_channels, last_bn=False, score_norm='softmax', temp_factor=1.0,
                 norm_cfg=dict(type='BN2d'), bias='auto'):
        super().__init__()
        assert score_norm in ['softmax', 'sigmoid', 'identity'], \
            f'unsupported score_norm function {score_norm}'
        self.score_norm = score_norm
        self.temp_factor = temp_factor
        last = len(mlp_channels) - 2
        layers = OrderedDict()
        for i, (cin, cout) in enumerate(zip(mlp_channels, mlp_channels[1:])):
            kw = dict(norm_cfg=norm_cfg) if i < last else \
                dict(norm_cfg=norm_cfg if last_bn else None, act_cfg=None)
            layers[f'layer{i}'] = ConvModule(cin, cout, kernel_size=(1, 1), stride=(1, 1),
                                             conv_cfg=dict(type='Conv2d'), bias=bias, **kw)
        self.mlps = nn.Sequential(layers)

    def init_weights(self):
        """Xavier-normal convolutions with zero biases (mmcv's ``xavier_init`` defaults)."""
        for module in self.mlps.modules():
            if isinstance(module, nn.Conv2d):
                nn.init.xavier_normal_(module.weight, gain=1)
                if module.bias is not None:
                    nn.init.constant_(module.bias, 0)

    def forward(self, xyz_features):
        scores = self.mlps(xyz_features)   # (B, M, N, K)
        if self.score_norm == 'softmax':
            scores = F.softmax(scores / self.temp_factor, dim=1)
        elif self.score_norm == 'sigmoid':
            scores = torch.sigmoid(scores / self.temp_factor)
        return scores.permute(0, 2, 3, 1)  # (B, N, K, M)


class PAConv(nn.Module):
    """The torch-op form: inputs ``(features (B, C, npoint, K), points_xyz (B, 3, npoint, K))``
    already grouped, output ``(new_features (B, out, npoint, K), points_xyz)`` so that layers
    chain in an ``nn.Sequential``.  The first neighbour of every row is its centre.

    ``kernel_input``: 'identity' feeds the grouped features to the bank, 'w_neighbor' feeds
    cat(features - centre features, features).  ``scorenet_input``: 'identity' = xyz - centre
    (3 channels), 'w_neighbor' = cat(xyz - centre, xyz) (6), 'w_neighbor_dist' = cat(centre,
    xyz - centre, distance) (7).  ``weight_bank`` is (kernel_mul * in, m * out), initialised
    ('kaiming' | 'xavier') as (m, kernel_mul * in, out).  ``scorenet_cfg`` is never modified."""

    def __init__(self, in_channels, out_channels, num_kernels,
                 norm_cfg=dict(type='BN2d', momentum=0.1), act_cfg=dict(type='ReLU', inplace=True),
                 scorenet_input='w_neighbor_dist', weight_bank_init='kaiming',
                 kernel_input='w_neighbor', scorenet_cfg=_DEFAULT_SCORENET):
        super().__init__()
        if kernel_input not in ('identity', 'w_neighbor'):
            raise NotImplementedError(f'unsupported kernel_input {kernel_input}')
        self.kernel_input = kernel_input
        self.kernel_mul = 1 if kernel_input == 'identity' else 2
        widths = dict(identity=3, w_neighbor=6, w_neighbor_dist=7)
        if scorenet_input not in widths:
            raise NotImplementedError(f'unsupported scorenet_input {scorenet_input}')
        self.scorenet_input = scorenet_input
        self.scorenet_in_channels = widths[scorenet_input]
        inits = dict(kaiming=nn.init.kaiming_normal_, xavier=nn.init.xavier_normal_)
        if weight_bank_init not in inits:
            raise NotImplementedError(f'unsupported weight bank init method {weight_bank_init}')

        self.m = num_kernels
        rows = in_channels * self.kernel_mul
        bank = inits[weight_bank_init](torch.empty(self.m, rows, out_channels))
        bank = bank.permute(1, 0, 2).reshape(rows, self.m * out_channels).contiguous()
        self.weight_bank = nn.Parameter(bank, requires_grad=True)

        cfg = copy.deepcopy(dict(scorenet_cfg))
        cfg['mlp_channels'] = [self.scorenet_in_channels, *cfg['mlp_channels'], self.m]
        self.scorenet = ScoreNet(**cfg)

        if act_cfg is not None:
            assert act_cfg['type'] == 'ReLU'
        # as in ConvModule: the norm layer applies a ReLU that follows it (its backward reads the
        # output it saved, which an in-place activation would overwrite)
        self.act_fused = norm_cfg is not None and act_cfg is not None
        self.bn = None
        if norm_cfg is not None:
            options = {k: v for k, v in norm_cfg.items() if k not in ('type', 'requires_grad')}
            if norm_cfg['type'] != 'BN2d':
                raise KeyError(f"unsupported norm type {norm_cfg['type']}")
            self.bn = FusedBNReLU2d(out_channels, relu=self.act_fused, **options)
        self.activate = None
        if act_cfg is not None:
            self.activate = nn.ReLU(inplace=act_cfg.get('inplace', False))
        self.init_weights()

    def init_weights(self):
        self.scorenet.init_weights()
        if self.bn is not None:
            nn.init.constant_(self.bn.weight, 1)
            nn.init.constant_(self.bn.bias, 0)

    def _prepare_scorenet_input(self, points_xyz):
        """points_xyz (B, 3, npoint, K) -> the per-pair position features (B, 3 | 6 | 7, npoint, K)."""
        B, _, npoint, K = points_xyz.size()
        center_xyz = points_xyz[..., :1].repeat(1, 1, 1, K)
        xyz_diff = points_xyz - center_xyz
        if self.scorenet_input == 'identity':
            return xyz_diff
        if self.scorenet_input == 'w_neighbor':
            return torch.cat((xyz_diff, points_xyz), dim=1)
        dist = calc_euclidian_dist(
            center_xyz.permute(0, 2, 3, 1).reshape(B * npoint * K, 3),
            points_xyz.permute(0, 2, 3, 1).reshape(B * npoint * K, 3)).reshape(B, 1, npoint, K)
        return torch.cat((center_xyz, xyz_diff, dist), dim=1)

    def _norm_act(self, x):
        if self.bn is not None:
            x = self.bn(x)
        if self.activate is not None and not self.act_fused:
            x = self.activate(x)
        return x

    def forward(self, inputs):
        features, points_xyz = inputs
        B, _, npoint, K = features.size()
        if self.kernel_input == 'w_neighbor':
            center_features = features[..., :1].repeat(1, 1, 1, K)
            features = torch.cat((features - center_features, features), dim=1)
        scores = self.scorenet(self._prepare_scorenet_input(points_xyz))   # (B, npoint, K, m)
        # the bank applied to every pair: (B, npoint, K, m, out) -- the operand PAConvCUDA avoids
        per_kernel = torch.matmul(features.permute(0, 2, 3, 1), self.weight_bank).view(
            B, npoint, K, self.m, -1)
        blended = assign_score(scores, per_kernel).permute(0, 3, 1, 2).contiguous()
        return (self._norm_act(blended), points_xyz)


class PAConvCUDA(PAConv):
    """The kernel form ('w_neighbor' only): inputs ``(features (B, C, N) of ALL points, points_xyz
    (B, 3, npoint, K), points_idx (B, npoint, K))``.  The bank is applied to every point once
    (``assign_kernel_withoutk``) and ``assign_score_withk`` gathers and blends on the fly, so
    nothing of size (B, npoint, K, m, out) exists.  Returns ``(new_features (B, out, npoint, K),
    points_xyz, points_idx)``."""

    def __init__(self, in_channels, out_channels, num_kernels,
                 norm_cfg=dict(type='BN2d', momentum=0.1), act_cfg=dict(type='ReLU', inplace=True),
                 scorenet_input='w_neighbor_dist', weight_bank_init='kaiming',
                 kernel_input='w_neighbor', scorenet_cfg=_DEFAULT_SCORENET):
        super().__init__(in_channels, out_channels, num_kernels, norm_cfg=norm_cfg, act_cfg=act_cfg,
                         scorenet_input=scorenet_input, weight_bank_init=weight_bank_init,
                         kernel_input=kernel_input, scorenet_cfg=scorenet_cfg)
        assert self.kernel_input == 'w_neighbor', \
            'CUDA implemented PAConv only supports w_neighbor kernel_input'

    def forward(self, inputs):
        features, points_xyz, points_idx = inputs
        scores = self.scorenet(self._prepare_scorenet_input(points_xyz))   # (B, npoint, K, m)
        point_feat, center_feat = assign_kernel_withoutk(features, self.weight_bank, self.m)
        blended = assign_score_withk(scores, point_feat, center_feat, points_idx, 'sum').contiguous()
        return (self._norm_act(blended), points_xyz, points_idx)
