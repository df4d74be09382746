"""``sigmoid_focal_loss`` / ``SigmoidFocalLoss`` as ``mmcv.ops`` exports them and ``mmdet3d.ops``
re-exports them (reference mmdet3d/ops/__init__.py:1-3; the mmcv source is not in the reference tree,
semantics from SURVEY.md appendix C), on ``csrc/focal_loss.hip``.

HIP only, as mmcv's op is CUDA only.  The value is the softplus form of include/nesie_ops.h: it
agrees with mmcv's to rounding for |x| below about 87 and, unlike it, stays accurate and finite
beyond; a label outside [0, C) gives an all-negative row and takes class weight 1.0 (mmcv indexes the
weight with it).  ``'sum'`` and ``'mean'`` never store the (N, C) loss: the forward is the fused
fixed-order reduction, the backward one launch that reads the upstream scalar on the device.  An
empty input launches nothing: ``'none'`` gives an empty tensor, ``'sum'`` 0 and ``'mean'`` (N == 0)
NaN, the same as ``FocalLoss``.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ..kernels import backend_for

_REDUCTIONS = {'none': 0, 'mean': 1, 'sum': 2}      # mmcv's reduction_dict


def focal_forward(input, target, weight, sample_weight, gamma, alpha, reduce, scale=1.0,
                  scale_dev=None):
    """-> the (N, C) weighted loss times ``scale`` (``reduce`` false) or the 0-d sum of it times
    ``scale * scale_dev`` (``reduce`` true): one back-end call.  An empty input launches nothing."""
    n, c = input.shape
    if not reduce:
        out = input.new_empty(n, c)
        if out.numel():
            backend_for(input).sigmoid_focal_loss_forward(
                input, target, weight, out, gamma, alpha, sample_weight, scale)
        return out
    if input.numel() == 0:
        return input.new_zeros(())
    out = input.new_empty(1)
    backend_for(input).sigmoid_focal_loss_forward_sum(
        input, target, weight, out, gamma, alpha, sample_weight, scale, scale_dev)
    return out.view(())


def focal_backward(grad, input, target, weight, sample_weight, gamma, alpha, reduce, scale=1.0,
                   scale_dev=None):
    """-> d loss / d input for the forward of the same arguments, ``grad`` being the gradient of its
    result ((N, C) or 0-d, left on the device): one back-end call."""
    grad_input = torch.empty_like(input)
    if input.numel():
        grad = grad.contiguous()
        backend_for(input).sigmoid_focal_loss_backward(
            input, target, weight, grad_input, gamma, alpha, sample_weight,
            None if reduce else grad, grad.view(1) if reduce else None, scale,
            scale_dev if reduce else None)
    return grad_input


class SigmoidFocalLossFunction(Function):

    @staticmethod
    def forward(ctx, input, target, gamma=2.0, alpha=0.25, weight=None, reduction='mean'):
        assert isinstance(target, torch.Tensor) and target.dtype == torch.int64
        assert input.dim() == 2
        assert target.dim() == 1
        assert input.size(0) == target.size(0)
        if weight is not None:
            assert weight.dim() == 1
            assert input.size(1) == weight.size(0)
            weight = weight.contiguous()
        ctx.reduce = _REDUCTIONS[reduction] != 0            # an unknown reduction: KeyError
        ctx.gamma, ctx.alpha = float(gamma), float(alpha)
        # 'mean' is over the N rows, not the N * C elements
        ctx.scale = 1.0 / input.size(0) if reduction == 'mean' and input.size(0) else 1.0
        input, target = input.contiguous(), target.contiguous()
        backend_for(input)                                  # a CPU tensor: "no CPU fallback"
        ctx.save_for_backward(input, target, weight)
        if reduction == 'mean' and input.size(0) == 0:
            # sum / N with N == 0: NaN, as mmcv's division and FocalLoss's mean of nothing give
            return input.new_full((), float('nan'))
        return focal_forward(input, target, weight, None, ctx.gamma, ctx.alpha, ctx.reduce,
                             ctx.scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, target, weight = ctx.saved_tensors
        grad_input = focal_backward(grad_output, input, target, weight, None, ctx.gamma, ctx.alpha,
                                    ctx.reduce, ctx.scale)
        return grad_input, None, None, None, None, None


sigmoid_focal_loss = SigmoidFocalLossFunction.apply


class SigmoidFocalLoss(nn.Module):

    def __init__(self, gamma, alpha, weight=None, reduction='mean'):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha
        self.register_buffer('weight', weight)
        self.reduction = reduction

    def forward(self, input, target):
        return sigmoid_focal_loss(input, target, self.gamma, self.alpha, self.weight,
                                  self.reduction)

    def __repr__(self):
        return (f'{self.__class__.__name__}(gamma={self.gamma}, alpha={self.alpha}, '
                f'reduction={self.reduction})')
