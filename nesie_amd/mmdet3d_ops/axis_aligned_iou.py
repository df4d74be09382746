"""``AxisAlignedBboxOverlaps3D`` / ``axis_aligned_bbox_overlaps_3d`` of
``mmdet3d/core/bbox/iou_calculators/iou3d_calculator.py:170-320``: IoU or GIoU of upright boxes in
corner form (x1, y1, z1, x2, y2, z2), pair by pair (``is_aligned=True``) or every box of the first
set against every box of the second.

The tensor-op form below (``_overlaps_torch``) is the definition and autograd supplies its gradient;
it serves CPU tensors and every dtype but float32.  Float32 tensors on the device go through
``csrc/aa_iou3d.hip``: one launch for the values (plus both Jacobians in the paired form), one
fixed-order launch pair for the matrix form's gradients.  Both inputs are differentiable.
"""
import torch
from torch.autograd import Function

from ..kernels import backend_for

_MODES = {'iou': 0, 'giou': 1}


def _overlaps_torch(bboxes1, bboxes2, mode, is_aligned, eps):
    """The reference's chain, operation by operation and in its order (its float32 rounding, and the
    order in which autograd adds up the branches, are the yardstick)."""
    area1 = (bboxes1[..., 3] - bboxes1[..., 0]) * (bboxes1[..., 4] - bboxes1[..., 1]) \
        * (bboxes1[..., 5] - bboxes1[..., 2])
    area2 = (bboxes2[..., 3] - bboxes2[..., 0]) * (bboxes2[..., 4] - bboxes2[..., 1]) \
        * (bboxes2[..., 5] - bboxes2[..., 2])
    if is_aligned:
        def lo(b, _second):
            return b[..., :3]

        def hi(b, _second):
            return b[..., 3:]
    else:                      # (..., m, 1, 3) against (..., 1, n, 3)
        def lo(b, second):
            return b[..., None, :, :3] if second else b[..., :, None, :3]

        def hi(b, second):
            return b[..., None, :, 3:] if second else b[..., :, None, 3:]
        area1, area2 = area1[..., None], area2[..., None, :]
    lt = torch.max(lo(bboxes1, False), lo(bboxes2, True))
    rb = torch.min(hi(bboxes1, False), hi(bboxes2, True))
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1] * wh[..., 2]
    union = area1 + area2 - overlap
    if mode == 'giou':
        enclosed_lt = torch.min(lo(bboxes1, False), lo(bboxes2, True))
        enclosed_rb = torch.max(hi(bboxes1, False), hi(bboxes2, True))
    eps = union.new_tensor([eps])
    union = torch.max(union, eps)
    ious = overlap / union
    if mode == 'iou':
        return ious
    enclose_wh = (enclosed_rb - enclosed_lt).clamp(min=0)
    enclose = torch.max(enclose_wh[..., 0] * enclose_wh[..., 1] * enclose_wh[..., 2], eps)
    return ious - (enclose - union) / enclose


def _rows(t):
    """(…, rows, 6) -> contiguous (…, rows, 6) whose rows the kernels can read as 8-byte pairs."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 8 else t


class AxisAlignedIoU3DPaired(Function):
    """(…, 6) x (…, 6) -> (…): value and the Jacobians of the inputs that need one, one launch."""

    @staticmethod
    def forward(ctx, bboxes1, bboxes2, mode, eps):
        b1, b2 = _rows(bboxes1.reshape(-1, 6)), _rows(bboxes2.reshape(-1, 6))
        n = b1.shape[0]
        out = b1.new_empty(n)
        jac1 = b1.new_empty(n, 6) if ctx.needs_input_grad[0] else None
        jac2 = b1.new_empty(n, 6) if ctx.needs_input_grad[1] else None
        backend_for(b1).aa_iou3d_paired_forward(b1, b2, mode, eps, out, jac1, jac2)
        ctx.save_for_backward(jac1, jac2)
        ctx.shapes = (bboxes1.shape, bboxes2.shape)
        return out.view(bboxes1.shape[:-1])

    @staticmethod
    def backward(ctx, grad):
        g = grad.reshape(-1, 1)
        return tuple(None if jac is None else (g * jac).view(shape)
                     for jac, shape in zip(ctx.saved_tensors, ctx.shapes)) + (None, None)


class AxisAlignedIoU3DMatrix(Function):
    """(b, m, 6) x (b, n, 6) -> (b, m, n); the backward recomputes the Jacobian and reduces over
    n (first input) and m (second input) in a fixed order."""

    @staticmethod
    def forward(ctx, bboxes1, bboxes2, mode, eps):
        b1, b2 = _rows(bboxes1), _rows(bboxes2)
        out = b1.new_empty(b1.shape[0], b1.shape[1], b2.shape[1])
        backend_for(b1).aa_iou3d_matrix_forward(b1, b2, mode, eps, out)
        ctx.save_for_backward(b1, b2)
        ctx.mode, ctx.eps = mode, eps
        return out

    @staticmethod
    def backward(ctx, grad):
        b1, b2 = ctx.saved_tensors
        grad1 = torch.empty_like(b1) if ctx.needs_input_grad[0] else None
        grad2 = torch.empty_like(b2) if ctx.needs_input_grad[1] else None
        if grad1 is not None or grad2 is not None:
            backend_for(b1).aa_iou3d_matrix_backward(b1, b2, ctx.mode, ctx.eps, grad.contiguous(),
                                                     grad1, grad2)
        return grad1, grad2, None, None


def _native(bboxes1, bboxes2):
    if not (bboxes1.is_cuda and bboxes2.is_cuda and bboxes1.device == bboxes2.device
            and bboxes1.dtype == torch.float32 == bboxes2.dtype):
        return False
    return getattr(backend_for(bboxes1), 'name', '') == 'hip'


def axis_aligned_bbox_overlaps_3d(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=1e-6):
    """bboxes1 (B…, m, 6), bboxes2 (B…, n, 6) or empty -> (B…, m, n), or (B…, m) with
    ``is_aligned`` (then m == n).  mode 'iou' or 'giou'; ``eps`` is the floor of the union and of
    the enclosing volume."""
    assert mode in _MODES, f'Unsupported mode {mode}'
    # either the boxes are empty or their last dimension is 6
    assert bboxes1.size(-1) == 6 or bboxes1.size(0) == 0
    assert bboxes2.size(-1) == 6 or bboxes2.size(0) == 0
    assert bboxes1.shape[:-2] == bboxes2.shape[:-2]
    batch_shape = tuple(bboxes1.shape[:-2])
    rows, cols = bboxes1.size(-2), bboxes2.size(-2)
    if is_aligned:
        assert rows == cols
    if rows * cols == 0:
        return bboxes1.new_empty(batch_shape + ((rows,) if is_aligned else (rows, cols)))
    if not _native(bboxes1, bboxes2):
        return _overlaps_torch(bboxes1, bboxes2, mode, is_aligned, eps)
    if bboxes1.numel() == 0:          # a zero among the batch dimensions: nothing to launch
        return bboxes1.new_empty(batch_shape + ((rows,) if is_aligned else (rows, cols)))
    if is_aligned:
        return AxisAlignedIoU3DPaired.apply(bboxes1, bboxes2, _MODES[mode], float(eps))
    out = AxisAlignedIoU3DMatrix.apply(bboxes1.reshape(-1, rows, 6), bboxes2.reshape(-1, cols, 6),
                                       _MODES[mode], float(eps))
    return out.view(batch_shape + (rows, cols))


class AxisAlignedBboxOverlaps3D(object):
    """Axis-aligned 3-D overlaps (IoU / GIoU) calculator (iou3d_calculator.py:170-198)."""

    def __call__(self, bboxes1, bboxes2, mode='iou', is_aligned=False):
        assert bboxes1.size(-1) == bboxes2.size(-1) == 6
        return axis_aligned_bbox_overlaps_3d(bboxes1, bboxes2, mode, is_aligned)

    def __repr__(self):
        return self.__class__.__name__ + '()'
