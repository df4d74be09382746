"""Mirror of ``mmdet3d/ops/knn/knn.py:7-72``."""
import torch
from torch.autograd import Function

from ..kernels import backend_for


class KNN(Function):
    """The ``k`` nearest points of every centre, in ascending order of (squared distance, point
    index); ``include/nesie_ops.h`` ``nesie_knn_wrapper`` states the rule and how it relates to
    the reference's heap."""

    @staticmethod
    def forward(ctx, k: int, xyz: torch.Tensor, center_xyz: torch.Tensor = None,
                transposed: bool = False, return_dist2: bool = False):
        """xyz (B, N, 3), center_xyz (B, npoint, 3) or None = the points themselves; with
        ``transposed`` both are (B, 3, N) / (B, 3, npoint).  -> idx (B, k, npoint) int32.
        ``return_dist2`` (not in the reference): -> (idx, dist2), dist2 (B, k, npoint) float32 =
        the squared distances of those neighbours.  ``knn`` is ``KNN.apply``, which takes no
        keywords: pass the arguments by position, as the reference asks for ``transposed``."""
        assert k > 0

        if center_xyz is None:
            center_xyz = xyz

        if transposed:
            xyz = xyz.transpose(2, 1).contiguous()
            center_xyz = center_xyz.transpose(2, 1).contiguous()

        assert xyz.is_contiguous()  # [B, N, 3]
        assert center_xyz.is_contiguous()  # [B, npoint, 3]
        assert center_xyz.device == xyz.device, \
            'center_xyz and xyz should be put on the same device'

        B, npoint, _ = center_xyz.shape
        N = xyz.shape[1]
        backend = backend_for(xyz)

        # (the reference zero-fills both; the kernel writes every slot, padding included)
        idx = center_xyz.new_empty((B, npoint, k), dtype=torch.int32)
        dist2 = center_xyz.new_empty((B, npoint, k), dtype=torch.float32)
        backend.knn_wrapper(B, N, npoint, k, xyz, center_xyz, idx, dist2)
        idx = idx.transpose(2, 1).contiguous()  # [B, k, npoint]
        ctx.mark_non_differentiable(idx)
        if not return_dist2:
            return idx
        dist2 = dist2.transpose(2, 1).contiguous()
        ctx.mark_non_differentiable(dist2)
        return idx, dist2

    @staticmethod
    def backward(ctx, *grads):
        return None, None, None, None, None


knn = KNN.apply
