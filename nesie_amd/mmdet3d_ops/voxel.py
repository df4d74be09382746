"""Mirror of ``mmdet3d/ops/voxel``: ``voxelize.py:10-122`` and ``scatter_points.py:9-107``.
``include/nesie_ops.h`` (``nesie_hard_voxelize``, ``nesie_dynamic_scatter_forward``) states the
pinned semantics and the two departures from the reference.  Nothing here is launched by the
default training step."""
import torch
from torch import nn
from torch.autograd import Function
from torch.nn.modules.utils import _pair

from .roiaware_pool3d import _hip_backend

_REDUCE = {'sum': 0, 'mean': 1, 'max': 2}


def _points_2d(name, points):
    if points.dim() != 2 or points.dtype != torch.float32:
        raise TypeError(f'{name}: expected a float32 (N, C) tensor, got {points.dtype} '
                        f'{tuple(points.shape)}')


class _Voxelization(Function):

    @staticmethod
    def forward(ctx, points, voxel_size, coors_range, max_points=35, max_voxels=20000):
        """points (N, C>=3) fp32, voxel_size 3 floats (x, y, z), coors_range 6 floats (min xyz,
        max xyz).  ``max_points == -1`` or ``max_voxels == -1``: dynamic voxelization -> coors
        (N, 3) int32, the (z, y, x) cell of every point, (-1, -1, -1) out of range.  Otherwise
        hard voxelization -> voxels (M, max_points, C), coors (M, 3), num_points_per_voxel (M):
        voxels in order of first appearance, M = min(distinct cells, max_voxels) read from the
        device once."""
        backend = _hip_backend('voxelization', points)
        _points_2d('voxelization', points)
        if points.shape[1] < 3:
            raise ValueError(f'voxelization: points need at least 3 columns, got {points.shape[1]}')
        points = points.contiguous()
        voxel_size = [float(v) for v in voxel_size]
        coors_range = [float(v) for v in coors_range]
        if len(voxel_size) != 3 or len(coors_range) != 6:
            raise ValueError('voxelization: voxel_size takes 3 values and coors_range 6 '
                             '(3 spatial dimensions only)')
        n, c = points.shape
        _, cells = backend.voxel_grid_size(voxel_size, coors_range)   # refuses before allocation
        if max_points == -1 or max_voxels == -1:
            coors = points.new_empty((n, 3), dtype=torch.int)          # written in full
            backend.dynamic_voxelize(points, voxel_size, coors_range, coors)
            return coors
        backend.voxel_workspace_bytes(n, cells)
        # (the reference zero-fills; the rows that are returned are written in full)
        voxels = points.new_empty((max_voxels, max_points, c))
        coors = points.new_empty((max_voxels, 3), dtype=torch.int)
        num_points_per_voxel = points.new_empty((max_voxels,), dtype=torch.int)
        voxel_num = points.new_empty((1,), dtype=torch.int)
        backend.hard_voxelize(points, voxel_size, coors_range, voxels, coors,
                              num_points_per_voxel, voxel_num)
        voxel_num = int(voxel_num.item())
        return voxels[:voxel_num], coors[:voxel_num], num_points_per_voxel[:voxel_num]


voxelization = _Voxelization.apply


class Voxelization(nn.Module):
    """voxel_size [x, y, z], point_cloud_range [x_min, y_min, z_min, x_max, y_max, z_max],
    max_num_points per voxel (-1: dynamic), max_voxels an int or a (training, testing) pair."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000):
        super().__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.max_num_points = max_num_points
        if isinstance(max_voxels, tuple):
            self.max_voxels = max_voxels
        else:
            self.max_voxels = _pair(max_voxels)

        point_cloud_range = torch.tensor(point_cloud_range, dtype=torch.float32)
        voxel_size = torch.tensor(voxel_size, dtype=torch.float32)
        grid_size = (point_cloud_range[3:] - point_cloud_range[:3]) / voxel_size
        grid_size = torch.round(grid_size).long()
        input_feat_shape = grid_size[:2]
        self.grid_size = grid_size
        # [w, h, d] -> [d, h, w]
        self.pcd_shape = [*input_feat_shape, 1][::-1]

    def forward(self, input):
        max_voxels = self.max_voxels[0] if self.training else self.max_voxels[1]
        return voxelization(input, self.voxel_size, self.point_cloud_range, self.max_num_points,
                            max_voxels)

    def __repr__(self):
        tmpstr = self.__class__.__name__ + '('
        tmpstr += 'voxel_size=' + str(self.voxel_size)
        tmpstr += ', point_cloud_range=' + str(self.point_cloud_range)
        tmpstr += ', max_num_points=' + str(self.max_num_points)
        tmpstr += ', max_voxels=' + str(self.max_voxels)
        tmpstr += ')'
        return tmpstr


class _dynamic_scatter(Function):

    @staticmethod
    def forward(ctx, feats, coors, reduce_type='max', dims=None):
        """feats (N, C) fp32, coors (N, 3) int32, reduce_type 'max' / 'sum' / 'mean' ->
        voxel_feats (M, C), voxel_coors (M, 3): one row per distinct valid row of ``coors`` in
        lexicographic order.  ``dims`` (3 exclusive upper bounds; a row with an entry outside
        0 .. dims - 1 is invalid) defaults to one device reduction of ``coors``."""
        backend = _hip_backend('dynamic_scatter', feats)
        _points_2d('dynamic_scatter', feats)
        if reduce_type not in _REDUCE:
            raise ValueError(f"dynamic_scatter: reduce_type must be 'max', 'sum' or 'mean', "
                             f'got {reduce_type!r}')
        if coors.dtype != torch.int32 or coors.dim() != 2 or coors.shape[1] != 3 \
                or coors.shape[0] != feats.shape[0]:
            raise TypeError(f'dynamic_scatter: coors must be int32 (N, 3), got {coors.dtype} '
                            f'{tuple(coors.shape)} (3 spatial dimensions only)')
        assert feats.device == coors.device, 'feats and coors should be put on the same device'
        feats, coors = feats.contiguous(), coors.contiguous()
        n, c = feats.shape
        if dims is None:
            # the one host read the data-dependent M costs anyway comes a little earlier
            dims = [max(int(d) + 1, 1) for d in coors.amax(0).tolist()] if n else [1, 1, 1]
        dims = [int(d) for d in dims]
        cells = dims[0] * dims[1] * dims[2] if min(dims) >= 1 else 0
        backend.voxel_workspace_bytes(n, cells)                       # refuses before allocation
        mode = _REDUCE[reduce_type]
        voxel_feats = feats.new_empty((n, c))
        voxel_coors = coors.new_empty((n, 3))
        coors_map, reduce_count, order, voxel_start = (coors.new_empty((n,)) for _ in range(4))
        num_voxels = coors.new_empty((1,))
        backend.dynamic_scatter_forward(feats, coors, dims, mode, voxel_feats, voxel_coors,
                                        coors_map, reduce_count, num_voxels, order, voxel_start)
        m = int(num_voxels.item())
        voxel_feats, voxel_coors = voxel_feats[:m], voxel_coors[:m]
        ctx.reduce_type, ctx.num_voxels = mode, m
        ctx.save_for_backward(feats, voxel_feats, coors_map, reduce_count, order, voxel_start,
                              num_voxels)
        ctx.mark_non_differentiable(voxel_coors)
        return voxel_feats, voxel_coors

    @staticmethod
    def backward(ctx, grad_voxel_feats, grad_voxel_coors=None):
        feats, voxel_feats, coors_map, reduce_count, order, voxel_start, num_voxels = \
            ctx.saved_tensors
        if ctx.num_voxels == 0 or feats.numel() == 0:
            return torch.zeros_like(feats), None, None, None
        grad_feats = torch.empty_like(feats)                           # written in full
        _hip_backend('dynamic_scatter', feats).dynamic_scatter_backward(
            grad_voxel_feats.contiguous(), feats, voxel_feats, coors_map, reduce_count, order,
            voxel_start, num_voxels, ctx.reduce_type, grad_feats)
        return grad_feats, None, None, None


dynamic_scatter = _dynamic_scatter.apply


class DynamicScatter(nn.Module):
    """Scatters points into voxels (the voxel encoders' pooling with dynamic voxelization):
    mean when ``average_points`` else max.  The bounds of ``coors`` come from the configured grid:
    (grid_z, grid_y, grid_x)."""

    def __init__(self, voxel_size, point_cloud_range, average_points: bool):
        super().__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.average_points = average_points

    def forward_single(self, points, coors):
        reduce = 'mean' if self.average_points else 'max'
        backend = _hip_backend('DynamicScatter', points)
        (gx, gy, gz), _ = backend.voxel_grid_size(self.voxel_size, self.point_cloud_range)
        return dynamic_scatter(points.contiguous(), coors.contiguous(), reduce, (gz, gy, gx))

    def forward(self, points, coors):
        """points (N, C); coors (N, 3), or (N, 4) with the batch index first."""
        if coors.size(-1) == 3:
            return self.forward_single(points, coors)
        batch_size = int(coors[-1, 0]) + 1
        voxels, voxel_coors = [], []
        for i in range(batch_size):
            inds = torch.where(coors[:, 0] == i)
            voxel, voxel_coor = self.forward_single(points[inds], coors[inds][:, 1:])
            coor_pad = nn.functional.pad(voxel_coor, (1, 0), mode='constant', value=i)
            voxel_coors.append(coor_pad)
            voxels.append(voxel)
        features = torch.cat(voxels, dim=0)
        feature_coors = torch.cat(voxel_coors, dim=0)
        return features, feature_coors

    def __repr__(self):
        tmpstr = self.__class__.__name__ + '('
        tmpstr += 'voxel_size=' + str(self.voxel_size)
        tmpstr += ', point_cloud_range=' + str(self.point_cloud_range)
        tmpstr += ', average_points=' + str(self.average_points)
        tmpstr += ')'
        return tmpstr
