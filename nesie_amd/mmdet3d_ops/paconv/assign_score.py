"""Mirror of ``mmdet3d/ops/paconv/assign_score.py:7-101`` on the HIP kernels of
``csrc/paconv.hip`` (semantics and departures: ``include/nesie_ops.h``)."""
import torch
from torch.autograd import Function

from ...kernels import backend_for

_AGGREGATE = {'sum': 0, 'avg': 1, 'max': 2}


def _hip_backend(tensor):
    backend = backend_for(tensor)
    if getattr(backend, 'name', '') != 'hip':
        raise RuntimeError('assign_score_withk runs on the HIP back end only; there is no CPU '
                           'fallback')
    return backend


class AssignScoreWithK(Function):
    """out[b, :, n, k] = sum_m scores[b, n, k, m] * (point_features[b, knn_idx[b, n, k], m] -
    center_features[b, knn_idx[b, n, 0], m]): PAConv's blend of the weight bank's outputs over a
    neighbourhood without the (B, npoint, K, M, out_dim) operand.  A neighbour index outside
    [0, N) gives a zero column.  Every sum has a fixed order: two runs give the same bits."""

    @staticmethod
    def forward(ctx, scores, point_features, center_features, knn_idx, aggregate='sum'):
        """scores (B, npoint, K, M), point_features / center_features (B, N, M, out_dim),
        knn_idx (B, npoint, K) int64 or int32 whose first column names the centre ->
        (B, out_dim, npoint, K).  ``aggregate`` ('sum' | 'avg' | 'max') is checked and, as in
        the reference's kernels, has no effect on the arithmetic."""
        _AGGREGATE[aggregate]
        B, N, M, out_dim = point_features.size()
        _, npoint, K, _ = scores.size()
        assert tuple(center_features.shape) == (B, N, M, out_dim)
        assert tuple(scores.shape) == (B, npoint, K, M) and tuple(knn_idx.shape) == (B, npoint, K)
        backend = _hip_backend(point_features)
        points, centers = point_features.contiguous(), center_features.contiguous()
        scores, knn_idx = scores.contiguous(), knn_idx.long().contiguous()
        if min(B, N, npoint, K, M, out_dim) == 0:
            output = point_features.new_zeros((B, out_dim, npoint, K))
        else:
            output = point_features.new_empty((B, out_dim, npoint, K))   # written in full
            backend.assign_score_withk_forward(B, N, npoint, M, K, out_dim, points, centers, scores,
                                               knn_idx, output)
        ctx.save_for_backward(points, centers, scores, knn_idx)
        return output

    @staticmethod
    def backward(ctx, grad_out):
        """grad_out (B, out_dim, npoint, K) -> (grad_scores, grad_point_features,
        grad_center_features, None, None); what ``needs_input_grad`` does not ask for is None."""
        points, centers, scores, knn_idx = ctx.saved_tensors
        B, N, M, out_dim = points.size()
        _, npoint, K, _ = scores.size()
        want_s, want_p, want_c = ctx.needs_input_grad[:3]
        if min(B, N, npoint, K, M, out_dim) == 0:
            return (torch.zeros_like(scores) if want_s else None,
                    torch.zeros_like(points) if want_p else None,
                    torch.zeros_like(centers) if want_c else None, None, None)
        grad_s = torch.empty_like(scores) if want_s else None
        grad_p = torch.empty_like(points) if want_p else None
        grad_c = torch.empty_like(centers) if want_c else None
        if want_s or want_p or want_c:
            _hip_backend(points).assign_score_withk_backward(
                B, N, npoint, M, K, out_dim, grad_out.contiguous(), points, centers, scores,
                knn_idx, grad_p, grad_c, grad_s)
        return grad_s, grad_p, grad_c, None, None


assign_score_withk = AssignScoreWithK.apply
