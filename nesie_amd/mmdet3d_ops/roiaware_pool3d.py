"""Mirror of ``mmdet3d/ops/roiaware_pool3d``: ``points_in_boxes.py:6-123`` and
``roiaware_pool3d.py:9-111``.  ``include/nesie_ops.h`` (``nesie_roiaware_pool3d_forward``) states
the pinned semantics."""
import math

import torch
from torch import nn
from torch.autograd import Function

from ..kernels import backend_for


def _hip_backend(name, tensor):
    """The HIP back end for ``tensor``; an injected one has none of these ops."""
    backend = backend_for(tensor)
    if getattr(backend, 'name', '') != 'hip':
        raise RuntimeError(f'{name} runs on the HIP back end only; there is no CPU fallback')
    return backend


def points_in_boxes_batch(points, boxes):
    """points (B,M,3) LiDAR frame, boxes (B,T,7) bottom-centre -> (B,M,T) int32."""
    assert boxes.shape[0] == points.shape[0], \
        f'Points and boxes should have the same batch size, got {boxes.shape[0]} and {points.shape[0]}'
    assert boxes.shape[2] == 7, f'boxes dimension should be 7, got unexpected shape {boxes.shape[2]}'
    assert points.shape[2] == 3, f'points dimension should be 3, got unexpected shape {points.shape[2]}'
    batch_size, num_points, _ = points.shape
    num_boxes = boxes.shape[1]
    box_idxs_of_pts = points.new_zeros((batch_size, num_points, num_boxes), dtype=torch.int)
    assert points.device == boxes.device, 'Points and boxes should be put on the same device'
    backend_for(points).points_in_boxes_batch(boxes.contiguous(), points.contiguous(),
                                              box_idxs_of_pts)
    return box_idxs_of_pts


def points_in_boxes_count(points, boxes):
    """points (B,M,3) LiDAR frame, boxes (B,T,7) -> (B,T) int32: how many of the scene's points
    lie in each box -- ``points_in_boxes_batch(points, boxes).sum(1)`` without the table (the
    non-empty test of NesieHead.multiclass_nms_single, nesie_head.py:744-750)."""
    assert boxes.shape[0] == points.shape[0] and boxes.shape[2] == 7 and points.shape[2] == 3
    counts = points.new_empty((boxes.shape[0], boxes.shape[1]), dtype=torch.int)
    backend_for(points).points_in_boxes_count(boxes.contiguous(), points.contiguous(), counts)
    return counts


def points_in_boxes_gpu(points, boxes):
    """points (B,M,3) LiDAR frame, boxes (B,T,7) bottom-centre -> (B,M) int32: the index of the
    first box that holds the point, -1 for background (points_in_boxes.py:6-50)."""
    assert boxes.shape[0] == points.shape[0], \
        f'Points and boxes should have the same batch size, got {boxes.shape[0]} and {points.shape[0]}'
    assert boxes.shape[2] == 7, f'boxes dimension should be 7, got unexpected shape {boxes.shape[2]}'
    assert points.shape[2] == 3, f'points dimension should be 3, got unexpected shape {points.shape[2]}'
    backend = _hip_backend('points_in_boxes_gpu', points)
    assert points.device == boxes.device, 'Points and boxes should be put on the same device'
    batch_size, num_points, _ = points.shape
    # (the reference fills -1 first; the kernel writes every element)
    box_idxs_of_pts = points.new_empty((batch_size, num_points), dtype=torch.int)
    backend.points_in_boxes_gpu(boxes.contiguous(), points.contiguous(), box_idxs_of_pts)
    return box_idxs_of_pts


def points_in_boxes_cpu(points, boxes):
    """points (P,3) LiDAR frame, boxes (N,7) bottom-centre -> (N,P) int32, 1 where the box holds
    the point (points_in_boxes.py:53-82).  The one op of the family that runs on the CPU: torch
    ops in the kernels' canonical arithmetic (cos / sin of the fp32 angle in double, rounded to
    fp32; fp32 products and sums; z window and half extents compared in double; x / y strict,
    z inclusive), so the table equals the device ops' bit for bit."""
    assert boxes.shape[1] == 7, f'boxes dimension should be 7, got unexpected shape {boxes.shape[1]}'
    assert points.shape[1] == 3, f'points dimension should be 3, got unexpected shape {points.shape[1]}'
    points, boxes = points.detach().float().cpu(), boxes.detach().float().cpu()
    f64 = torch.float64
    cx, cy, cz, w, l, h, rz = (boxes[:, i:i + 1] for i in range(7))
    x, y, z = (points[:, i].unsqueeze(0) for i in range(3))
    czm = (cz.to(f64) + h.to(f64) / 2.0).float()
    rot = (rz.to(f64) + math.pi / 2).float().to(f64)
    # libm per box, the function the referee and the C oracle call
    cosa = torch.tensor([math.cos(a) for a in rot.flatten().tolist()], dtype=f64).float().view(-1, 1)
    sina = torch.tensor([math.sin(a) for a in rot.flatten().tolist()], dtype=f64).float().view(-1, 1)
    z_in = ~((z - czm).abs().to(f64) > h.to(f64) / 2.0)
    sx, sy = x - cx, y - cy
    lx = (sx * cosa + sy * (-sina)).to(f64)
    ly = (sx * sina + sy * cosa).to(f64)
    hl, hw = l.to(f64) / 2.0, w.to(f64) / 2.0
    inside = z_in & (lx > -hl) & (lx < hl) & (ly > -hw) & (ly < hw)
    return inside.to(torch.int)


class RoIAwarePool3dFunction(Function):

    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_per_voxel, mode):
        """rois (N,7) LiDAR frame bottom-centre, pts (P,3), pts_feature (P,C), out_size an int or
        three, mode 0 (max) / 1 (avg) -> pooled_features (N, out_x, out_y, out_z, C)."""
        if isinstance(out_size, int):
            out_x = out_y = out_z = out_size
        else:
            assert len(out_size) == 3
            assert all(isinstance(s, int) for s in out_size)
            out_x, out_y, out_z = out_size
        backend = _hip_backend('RoIAwarePool3d', pts_feature)
        assert rois.device == pts.device == pts_feature.device, \
            'rois, pts and pts_feature should be put on the same device'
        num_rois = rois.shape[0]
        num_channels = pts_feature.shape[-1]
        num_pts = pts.shape[0]
        backend.roiaware_pool3d_sizes(num_rois, num_pts, num_channels, (out_x, out_y, out_z),
                                      max_pts_per_voxel)
        # (the reference zero-fills all three; the kernels write every element)
        pooled_features = pts_feature.new_empty((num_rois, out_x, out_y, out_z, num_channels))
        argmax = pts_feature.new_empty((num_rois, out_x, out_y, out_z, num_channels),
                                       dtype=torch.int)
        pts_idx_of_voxels = pts_feature.new_empty(
            (num_rois, out_x, out_y, out_z, max_pts_per_voxel), dtype=torch.int)
        # the voxel each box keeps each point in: what the backward gathers through (no backward,
        # no table)
        pts_voxel = pts_feature.new_empty((num_rois, num_pts), dtype=torch.int) \
            if ctx.needs_input_grad[2] else None
        backend.roiaware_pool3d_forward(rois.contiguous(), pts.contiguous(),
                                        pts_feature.contiguous(), argmax, pts_idx_of_voxels,
                                        pooled_features, mode, pts_voxel)
        ctx.roiaware_pool3d_for_backward = (pts_idx_of_voxels, argmax, pts_voxel, mode, num_pts,
                                            num_channels)
        return pooled_features

    @staticmethod
    def backward(ctx, grad_out):
        """grad_out (N, out_x, out_y, out_z, C) -> grad of pts_feature (P, C)."""
        pts_idx_of_voxels, argmax, pts_voxel, mode, num_pts, num_channels = \
            ctx.roiaware_pool3d_for_backward
        grad_in = grad_out.new_empty((num_pts, num_channels))   # written in full
        backend_for(grad_out).roiaware_pool3d_backward(pts_idx_of_voxels, argmax, pts_voxel,
                                                       grad_out.contiguous(), grad_in, mode)
        return None, None, grad_in, None, None, None


class RoIAwarePool3d(nn.Module):
    """Per box: the points inside voxelised into an out_x x out_y x out_z grid, their features
    max- or average-pooled per voxel (at most ``max_pts_per_voxel - 1`` points per voxel, the
    first in point order)."""

    def __init__(self, out_size, max_pts_per_voxel=128, mode='max'):
        super().__init__()
        self.out_size = out_size
        self.max_pts_per_voxel = max_pts_per_voxel
        assert mode in ['max', 'avg']
        pool_method_map = {'max': 0, 'avg': 1}
        self.mode = pool_method_map[mode]

    def forward(self, rois, pts, pts_feature):
        """rois (N,7) LiDAR frame, (x, y, z) the bottom centre; pts (P,3); pts_feature (P,C)
        -> pooled_features (N, out_x, out_y, out_z, C)."""
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size,
                                            self.max_pts_per_voxel, self.mode)
