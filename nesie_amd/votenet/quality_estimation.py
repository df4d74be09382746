"""SAQE quality head (``mmdet3d/models/dense_heads/quelity_estimation_module.py``): the
SidePooling variant with a 3x3x3 grid, every face sampled on three planes (the face and
the face shifted by -/+10 % of its offset: 27 points), 128-wide MiniPointNets, and ONE
global head over the six concatenated face features that emits per-class IoU scores,
per-class rotation scores and a 2-way objectness (``:54-76, 142-167, 323-344``)."""
import torch
from torch import nn

from ..mmdet3d_ops.norm import FusedBNReLU1d
from ..mmdet3d_ops.pointnet_modules import PointwiseConv1d
from .side_pooling import SidePooling


class QualityEstimation(SidePooling):
    grid_size = 3
    hide_dim = 128
    # faces are (front, back, top, down, left, right): the +-10 % plane offset acts on x for
    # front/back, z for top/down, y for the sides
    plane_axes = (0, 0, 2, 2, 1, 1)

    def _side_head(self, in_ch):
        return nn.Sequential(PointwiseConv1d(in_ch, 128, 1), FusedBNReLU1d(128), nn.Identity(),
                             PointwiseConv1d(128, self.iou_size, 1))

    def _add_final(self, before, head):
        """No box grid: one global head over the six concatenated face inputs."""
        head.append(nn.Sequential(
            PointwiseConv1d((128 + 33 + 4 + 1) * 6, 512, 1), FusedBNReLU1d(512), nn.Identity(),
            PointwiseConv1d(512, 256, 1), FusedBNReLU1d(256), nn.Identity(),
            PointwiseConv1d(256, self.iou_size * 2 + 2, 1)))

    def grid_for_side(self, whole_grid, center, heading):
        B, K = center.shape[:2]
        g2 = self.grid_size * self.grid_size
        faces = torch.index_select(whole_grid, 2, self._face_idx).view(B, K, 6, g2, 3)
        zero = faces * self._plane_axis.view(1, 1, 6, 1, 3)   # face * 0.1 on its own axis only
        planes = torch.cat([faces - zero, faces, faces + zero], dim=3)  # (B,K,6,3*g2,3)
        return self._to_scene(planes.reshape(B, K, -1, 3), center, heading)

    def forward(self, center, size, heading, end_points, prefix=''):
        x, _ = self._side_input(center, size, heading, end_points, prefix)
        end_points[f'{prefix}side_scores'] = self._side_scores(x)
        # x.flatten(1, 2) == cat of the six (B,166,2K) head inputs
        global_scores = self.mlps_head[6](x.flatten(1, 2)).transpose(2, 1)
        n = self.iou_size
        end_points[f'{prefix}iou_scores'] = global_scores[..., :n]
        end_points[f'{prefix}rotate_scores'] = global_scores[..., n:n * 2]
        end_points[f'{prefix}R_obj_scores'] = global_scores[..., n * 2:]
        return end_points
