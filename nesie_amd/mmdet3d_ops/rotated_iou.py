"""``mmdet3d/ops/rotated_iou`` on the native kernels: ``sort_v`` (cuda_op/cuda_ext.py:6-17 ->
``nesie_sort_vertices_forward``) and ``cal_iou_3d`` (oriented_iou_loss.py:86-109), which the
reference evaluates as ~100 torch kernels around ``sort_v`` and this library as ONE kernel
(``nesie_iou3d_forward``: value + Jacobian w.r.t. the first box).  ``cal_giou_3d`` / ``cal_diou_3d``
(oriented_iou_loss.py:112-152) with the "smallest" and "aligned" enclosing boxes are one kernel too
(``nesie_giou3d_forward``: loss, IoU and the loss's Jacobian); the "pca" enclosing box is not built.

There is no torch chain in the product: an injected test back end supplies its own
``rotated_iou_3d`` (the CPU oracle restates the reference chain in oracle/rotated_iou.py); the
enclosing-box losses exist on the HIP back end only.
"""
import torch
from torch.autograd import Function

from ..kernels import backend_for


class SortVertices(Function):
    """vertices (B,N,24,2) f32, mask (B,N,24) bool, num_valid (B,N) i32 -> (B,N,9) i32."""

    @staticmethod
    def forward(ctx, vertices, mask, num_valid):
        if vertices.dtype != torch.float32 or mask.dtype != torch.bool \
                or num_valid.dtype != torch.int32:
            raise RuntimeError('sort_vertices: vertices f32, mask bool, num_valid int32')
        vertices, mask, num_valid = vertices.contiguous(), mask.contiguous(), num_valid.contiguous()
        B, N = vertices.shape[:2]
        idx = vertices.new_empty((B, N, 9), dtype=torch.int32)
        backend_for(vertices).sort_vertices_forward(vertices, mask, num_valid, idx)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, gradout):
        return None, None, None


sort_v = SortVertices.apply


class RotatedIoU3D(Function):
    """cal_iou_3d as one native kernel: the IoU and its Jacobian w.r.t. the first box."""

    @staticmethod
    def forward(ctx, box3d1, box3d2):
        shape = box3d1.shape[:-1]
        b1 = box3d1.reshape(-1, 7).contiguous().float()
        b2 = box3d2.reshape(-1, 7).contiguous().float()
        iou = b1.new_empty(b1.shape[0])
        jac = b1.new_empty(b1.shape[0], 7) if box3d1.requires_grad else None
        backend_for(b1).iou3d_forward(b1, b2, iou, jac)
        ctx.save_for_backward(jac)
        ctx.in_shape = box3d1.shape
        return iou.view(shape)

    @staticmethod
    def backward(ctx, grad):
        (jac,) = ctx.saved_tensors
        if jac is None:
            return None, None
        return (grad.reshape(-1, 1) * jac).view(ctx.in_shape), None


def cal_iou_3d(box3d1, box3d2):
    """3-D IoU of (B,N,7) boxes rotated about z only; differentiable in ``box3d1`` (the second
    box is a target and never requires grad on this path)."""
    backend = backend_for(box3d1)
    if getattr(backend, 'name', '') == 'hip':
        if box3d2.requires_grad:
            raise RuntimeError('cal_iou_3d: the second box must not require grad')
        return RotatedIoU3D.apply(box3d1, box3d2)
    return backend.rotated_iou_3d(box3d1, box3d2)


class EnclosingIoU3DLoss(Function):
    """cal_giou_3d (kind 0) / cal_diou_3d (kind 1) as one native kernel: the loss, the IoU and the
    loss's Jacobian w.r.t. the first box."""

    @staticmethod
    def forward(ctx, box3d1, box3d2, kind, enclosing):
        shape = box3d1.shape[:-1]
        b1 = box3d1.reshape(-1, 7).contiguous().float()
        b2 = box3d2.reshape(-1, 7).contiguous().float()
        loss = b1.new_empty(b1.shape[0])
        iou = b1.new_empty(b1.shape[0])
        jac = b1.new_empty(b1.shape[0], 7) if box3d1.requires_grad else None
        backend_for(b1).giou3d_forward(b1, b2, kind, enclosing, loss, iou, jac)
        ctx.save_for_backward(jac)
        ctx.in_shape = box3d1.shape
        iou = iou.view(shape)
        ctx.mark_non_differentiable(iou)
        return loss.view(shape), iou

    @staticmethod
    def backward(ctx, grad, _grad_iou):
        (jac,) = ctx.saved_tensors
        if jac is None:
            return None, None, None, None
        return (grad.reshape(-1, 1) * jac).view(ctx.in_shape), None, None, None


_ENCLOSING = {'smallest': 0, 'aligned': 1}


def _enclosing_loss(name, kind, box3d1, box3d2, enclosing_type):
    if enclosing_type == 'pca':
        raise NotImplementedError(
            f"{name}: enclosing_type 'pca' is not built: the reference's eigenvector_22 "
            '(oriented_iou_loss.py:228-255) divides by the off-diagonal covariance, which is '
            'exactly 0 for two axis-aligned boxes, so it returns NaN on every yaw-0 target')
    if enclosing_type not in _ENCLOSING:
        raise ValueError(f"{name}: unknown enclosing_type {enclosing_type!r}; supported: "
                         "'smallest', 'aligned'")
    if getattr(backend_for(box3d1), 'name', '') != 'hip':
        raise RuntimeError(f'{name} runs on the HIP back end only; there is no CPU fallback')
    if box3d2.requires_grad:
        raise RuntimeError(f'{name}: the second box must not require grad')
    return EnclosingIoU3DLoss.apply(box3d1, box3d2, kind, _ENCLOSING[enclosing_type])


def cal_giou_3d(box3d1, box3d2, enclosing_type='smallest'):
    """3-D GIoU loss of (..., 7) boxes rotated about z only: 1 - IoU + (v_c - u) / v_c with v_c the
    volume of the enclosing box -> (loss, iou3d), both of shape ``box3d1.shape[:-1]``.  The loss
    is differentiable in ``box3d1``; the returned IoU is not (no reference caller differentiates
    it, and it would take a second Jacobian): use ``cal_iou_3d`` for a differentiable IoU."""
    return _enclosing_loss('cal_giou_3d', 0, box3d1, box3d2, enclosing_type)


def cal_diou_3d(box3d1, box3d2, enclosing_type='smallest'):
    """3-D DIoU loss: 1 - IoU + |centre1 - centre2|^2 / c2 with c2 the squared diagonal of the
    enclosing box -> (loss, iou3d) as ``cal_giou_3d``; the returned IoU is not differentiable."""
    return _enclosing_loss('cal_diou_3d', 1, box3d1, box3d2, enclosing_type)
