"""Host-side mirror of ``mmdet3d.ops`` (reference mmdet3d/ops/__init__.py:1-41).  The reference's
own operator families are real, and so is the one mmcv re-export that sits on a training path:
``sigmoid_focal_loss`` / ``SigmoidFocalLoss`` (``focal_loss.py``, the kernel behind mmdet's
``FocalLoss``).  ``NaiveSyncBatchNorm1d`` / ``NaiveSyncBatchNorm2d`` (``norm.py``; the norm types
``naiveSyncBN1d`` / ``naiveSyncBN2d`` of ``ConvModule``) are real too: batch statistics over every
rank of a process group, on the ``nesie_syncbn_*`` kernels.  The rest of the reference's ``__all__``
(the other mmcv re-exports: nms, RoIAlign ..., and SparseBottleneck) resolves to stubs that raise on use, so
``from mmdet3d.ops import X`` style code keeps importing ("import-time
requirement").

PAConv is real, with one wrinkle in its spelling.  The top-level names ``assign_score_withk``,
``PAConv`` and ``SparseBottleneck`` were published as raising stubs and the suite pins them as
such, so they stay in ``_OUT_OF_SCOPE`` and keep raising ``NotImplementedError`` (the message
points here); the real ``assign_score_withk``, ``PAConv`` and ``PAConvCUDA`` live in the
subpackage ``nesie_amd.mmdet3d_ops.paconv``, which mirrors ``mmdet3d.ops.paconv``:
``from nesie_amd.mmdet3d_ops.paconv import PAConv, assign_score_withk``.  ``PAConvCUDA`` and the
four set-abstraction modules ``PAConv{,CUDA}SAModule{,MSG}`` were pinned by nothing and are real
at the top level (``_HOT``); ``build_sa_module`` builds them.
"""
from .axis_aligned_iou import AxisAlignedBboxOverlaps3D, axis_aligned_bbox_overlaps_3d
from .ball_query import ball_query
from .furthest_point_sample import (Points_Sampler, furthest_point_sample,
                                    furthest_point_sample_with_dist)
from .gather_points import gather_points
from .group_points import GroupAll, QueryAndGroup, group_points, grouping_operation
from .interpolate import blend_conv, three_interpolate, three_interpolate_segmented, three_nn
from .pointnet_modules import (ConvModule, PointFPModule, PointSAModule, PointSAModuleMSG,
                               PointwiseConv1d, PointwiseConv2d, build_sa_module,
                               pointwise_conv)
from .knn import knn
from .iou3d import batched_nms_bev, boxes_iou_bev, boxes_overlap_bev, nms_gpu, nms_normal_gpu
from .roiaware_pool3d import (RoIAwarePool3d, points_in_boxes_batch, points_in_boxes_count,
                              points_in_boxes_cpu, points_in_boxes_gpu)
from .rotated_iou import cal_giou_3d, cal_iou_3d, sort_v
from .sparse_block import SparseBasicBlock, make_sparse_convmodule
from .voxel import DynamicScatter, Voxelization, dynamic_scatter, voxelization
from .paconv import PAConvCUDA
from .focal_loss import SigmoidFocalLoss, sigmoid_focal_loss
from .norm import NaiveSyncBatchNorm1d, NaiveSyncBatchNorm2d
from .paconv_sa_module import (PAConvCUDASAModule, PAConvCUDASAModuleMSG, PAConvSAModule,
                               PAConvSAModuleMSG)

_HOT = [
    'ball_query', 'furthest_point_sample', 'furthest_point_sample_with_dist',
    'three_interpolate', 'three_nn', 'gather_points', 'grouping_operation', 'group_points',
    'GroupAll', 'QueryAndGroup', 'PointSAModule', 'PointSAModuleMSG', 'PointFPModule',
    'points_in_boxes_batch', 'Points_Sampler', 'build_sa_module', 'cal_iou_3d', 'sort_v',
    'ConvModule', 'boxes_overlap_bev', 'points_in_boxes_count',
    'boxes_iou_bev', 'nms_gpu', 'nms_normal_gpu', 'knn', 'cal_giou_3d',
    'AxisAlignedBboxOverlaps3D', 'axis_aligned_bbox_overlaps_3d',
    'RoIAwarePool3d', 'points_in_boxes_gpu', 'points_in_boxes_cpu',
    'Voxelization', 'voxelization', 'dynamic_scatter', 'DynamicScatter',
    'SparseBasicBlock', 'make_sparse_convmodule',
    'PAConvCUDA', 'PAConvSAModuleMSG', 'PAConvSAModule', 'PAConvCUDASAModule',
    'PAConvCUDASAModuleMSG', 'sigmoid_focal_loss', 'SigmoidFocalLoss',
    'NaiveSyncBatchNorm1d', 'NaiveSyncBatchNorm2d',
]
_OUT_OF_SCOPE = [
    'nms', 'soft_nms', 'RoIAlign', 'roi_align', 'get_compiler_version',
    'get_compiling_cuda_version', 'batched_nms',
    'SparseBottleneck', 'assign_score_withk', 'PAConv',
]
_IN_SUBPACKAGE = {'assign_score_withk': 'paconv', 'PAConv': 'paconv'}
__all__ = _HOT + _OUT_OF_SCOPE


def __getattr__(name):
    if name in _OUT_OF_SCOPE:
        def _stub(*args, **kwargs):
            if name in _IN_SUBPACKAGE:
                raise NotImplementedError(
                    f'the top-level name mmdet3d.ops.{name} stays a stub; import the real one '
                    f'from nesie_amd.mmdet3d_ops.{_IN_SUBPACKAGE[name]}')
            raise NotImplementedError(
                f'mmdet3d.ops.{name} is outside the VoteNet/Nesie hot path this build '
                'covers (SURVEY.md section 2a/2b)')
        _stub.__name__ = name
        return _stub
    raise AttributeError(name)
