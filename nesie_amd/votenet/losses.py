"""Losses of the Nesie head.

Restates ``mmdet3d/models/losses/{chamfer_distance,surface_loss,side_pred_loss,
iou3d_loss,axis_aligned_iou_loss,gfocal_loss,lovasz_loss}.py`` and the mmdet 2.19 losses and loss plumbing they
stand beside (``weighted_loss`` / ``weight_reduce_loss`` / MSE / L1 / SmoothL1 / CrossEntropy /
FocalLoss; source not in the reference tree, semantics from SURVEY.md appendix C).
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ..kernels import backend_for, injected_backend
from ..mmdet3d_ops.axis_aligned_iou import axis_aligned_bbox_overlaps_3d
from ..mmdet3d_ops.focal_loss import focal_backward, focal_forward
from ..mmdet3d_ops.lovasz import lovasz_softmax_op
from ..mmdet3d_ops.rotated_iou import cal_diou_3d, cal_giou_3d, cal_iou_3d


# ---- mmdet loss plumbing (appendix C) ------------------------------------------
def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        if reduction == 'mean':
            return loss.mean()
        if reduction == 'sum':
            return loss.sum()
        return loss
    if reduction == 'mean':
        return loss.sum() / avg_factor
    if reduction == 'none':
        return loss
    raise ValueError('avg_factor can not be used with reduction="sum"')


class _ElementwiseLoss(nn.Module):
    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def elementwise(self, pred, target):
        raise NotImplementedError

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        loss = self.elementwise(pred, target)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


class MSELoss(_ElementwiseLoss):
    def elementwise(self, pred, target):
        return F.mse_loss(pred, target, reduction='none')


class L1Loss(_ElementwiseLoss):
    def elementwise(self, pred, target):
        return torch.abs(pred - target)


class SmoothL1Loss(_ElementwiseLoss):
    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0):
        super().__init__(reduction, loss_weight)
        self.beta = beta

    def elementwise(self, pred, target):
        diff = torch.abs(pred - target)
        return torch.where(diff < self.beta, 0.5 * diff * diff / self.beta,
                           diff - 0.5 * self.beta)


class CrossEntropyLoss(nn.Module):
    """Softmax CE with optional class weights; per-sample weight then reduce."""

    def __init__(self, class_weight=None, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.class_weight = class_weight
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.register_buffer('_cw', None if class_weight is None else
                             torch.tensor(class_weight, dtype=torch.float32), persistent=False)

    def forward(self, cls_score, label, weight=None, avg_factor=None,
                reduction_override=None):
        reduction = reduction_override if reduction_override else self.reduction
        cw = self._cw.to(cls_score.dtype) if self._cw is not None else None
        loss = F.cross_entropy(cls_score, label, weight=cw, reduction='none')
        if weight is not None:
            weight = weight.float()
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


# ---- chamfer (behaviour of chamfer_distance.py:8-146) ----------------------------
def _huber_unit(d):
    a = d.abs()
    return torch.where(a < 1.0, 0.5 * a * a, a - 0.5)


_COORD_PENALTY = {'l1': torch.abs, 'l2': torch.square, 'smooth_l1': _huber_unit}
_FOLD = {'none': lambda t: t, 'sum': torch.sum, 'mean': torch.mean}


def chamfer_distance(src, dst, src_weight=1.0, dst_weight=1.0, criterion_mode='l2',
                     reduction='mean'):
    """src (B, N, C), dst (B, M, C).  The cost of a pair is the per-coordinate penalty summed
    over C; every source point is charged its cheapest destination and vice versa.
    -> (source term, destination term, cheapest dst per src (B, N), cheapest src per dst (B, M))."""
    if criterion_mode not in _COORD_PENALTY or reduction not in _FOLD:
        raise NotImplementedError((criterion_mode, reduction))
    pair = _COORD_PENALTY[criterion_mode](src[:, :, None] - dst[:, None]).sum(-1)   # (B, N, M)
    to_dst, to_src = pair.min(dim=2), pair.min(dim=1)
    fold = _FOLD[reduction]
    return (fold(to_dst.values * src_weight), fold(to_src.values * dst_weight),
            to_dst.indices, to_src.indices)


class ChamferDistance(nn.Module):
    """Configured Chamfer term: the two directions scaled by ``loss_src_weight`` /
    ``loss_dst_weight`` (the vote loss uses mode 'l1', reduction 'none', dst weight 10)."""

    def __init__(self, mode='l2', reduction='mean', loss_src_weight=1.0, loss_dst_weight=1.0):
        super().__init__()
        if mode not in _COORD_PENALTY or reduction not in _FOLD:
            raise AssertionError((mode, reduction))
        self.mode, self.reduction = mode, reduction
        self.loss_src_weight, self.loss_dst_weight = loss_src_weight, loss_dst_weight

    def forward(self, source, target, src_weight=1.0, dst_weight=1.0,
                reduction_override=None, return_indices=False, **kwargs):
        if reduction_override is not None and reduction_override not in _FOLD:
            raise AssertionError(reduction_override)
        src_term, dst_term, src_pick, dst_pick = chamfer_distance(
            source, target, src_weight, dst_weight, self.mode, reduction_override or self.reduction)
        out = (src_term * self.loss_src_weight, dst_term * self.loss_dst_weight)
        return out + (src_pick, dst_pick) if return_indices else out


# ---- side surfaces (surface_loss.py:90-100) -------------------------------------
def Bbox2Surface(bbox2):
    """(…,>=6) centre+size -> (…,6) planes (x-,y-,z-,x+,y+,z+)."""
    center = bbox2[..., :3]
    half = 0.5 * bbox2[..., 3:6]
    return torch.cat([center - half, center + half], dim=-1)


class SurfaceLoss(nn.Module):
    """Per-side regression loss against the GT box planes (surface_loss.py:10-88).
    Only the MSE / SmoothL1 forms are used by the shipped configs."""

    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0, func_type='MSELoss'):
        super().__init__()
        self.func_type = func_type
        if func_type == 'MSELoss':
            self.loss_func = MSELoss(reduction, loss_weight)
        elif func_type == 'SmoothL1Loss':
            self.loss_func = SmoothL1Loss(beta, reduction, loss_weight)
        else:
            raise NotImplementedError(f'SurfaceLoss func_type {func_type} is not used by '
                                      'any shipped Nesie/SAQE config')

    def forward(self, pred, target, scale, center, prob, weight=None, avg_factor=None,
                reduction_override=None, **kwargs):
        target = Bbox2Surface(target)
        return self.loss_func(pred, target, weight, avg_factor, reduction_override)


class SidePredLoss(nn.Module):
    """Side-quality loss: label = min(1, 4*|pred side - GT side|) (an L1 with weight 4,
    clamped), loss = MSE(side score, label)  (side_pred_loss.py:10-83)."""

    def __init__(self, beta=1.0, reduction='mean', loss_weight=1.0,
                 label_func_type='SmoothL1Loss', loss_func_type='MSELoss'):
        super().__init__()
        self.label_func_type = label_func_type
        if label_func_type == 'MSELoss':
            self.label_func = MSELoss(reduction, 4.0)
        elif label_func_type == 'SmoothL1Loss':
            self.label_func = L1Loss(reduction, 4.0)  # sic: the reference builds an L1
        else:
            raise NotImplementedError
        if loss_func_type == 'MSELoss':
            self.loss_func = MSELoss(reduction, loss_weight)
        elif loss_func_type == 'SmoothL1Loss':
            self.loss_func = SmoothL1Loss(beta, reduction, loss_weight)
        else:
            raise NotImplementedError

    def forward(self, pred_side, pred, target, scale, center, prob, weight=None,
                avg_factor=None, reduction_override=None, **kwargs):
        target = Bbox2Surface(target)
        label_side = self.label_func(pred, target, None, None, 'none').detach()
        label_side = torch.where(label_side > 1, torch.ones_like(label_side), label_side)
        return self.loss_func(pred_side, label_side, weight, avg_factor, reduction_override)


# ---- axis-aligned IoU (axis_aligned_iou_loss.py:9-78, iou3d_loss.py:21-35) ----------------------
def axis_aligned_iou_loss(pred, target):
    """1 - IoU of one-to-one (…, 6) corner boxes (x1, y1, z1, x2, y2, z2) -> (…)."""
    return 1 - axis_aligned_bbox_overlaps_3d(pred, target, is_aligned=True)


def centre_size_to_corners(bbox):
    """(…, >= 6) centre + size (+ heading, ignored) -> (…, 6) corners (iou3d_loss.py:23-31)."""
    return torch.stack((bbox[..., 0] - bbox[..., 3] / 2, bbox[..., 1] - bbox[..., 4] / 2,
                        bbox[..., 2] - bbox[..., 5] / 2, bbox[..., 0] + bbox[..., 3] / 2,
                        bbox[..., 1] + bbox[..., 4] / 2, bbox[..., 2] + bbox[..., 5] / 2), dim=-1)


class AxisAlignedIoULoss(nn.Module):
    """1 - IoU of corner boxes, weighted and reduced (axis_aligned_iou_loss.py:28-78)."""

    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert reduction in ['none', 'sum', 'mean']
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        loss = axis_aligned_iou_loss(pred, target)
        if weight is not None and reduction != 'none':
            # reference :70-72 returns (pred * weight).sum() (== 0) when no weight is positive;
            # as IoU3DLoss: masking the unweighted entries gives that zero without the host sync
            loss = torch.where(weight > 0, loss, torch.zeros_like(loss))
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


# ---- IoU3D (iou3d_loss.py:12-14, 21-35, 38-76) --------------------------------------------------
class IoU3DLoss(nn.Module):
    """with_yaw: 1 - rotated IoU of (…, 7) boxes; without: 1 - axis-aligned IoU of (…, 7) or (…, 6)
    centre + size boxes, the heading ignored (iou3d_loss.py:72-75)."""

    def __init__(self, with_yaw=True, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.with_yaw = with_yaw
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None and weight.dim() > 1:
            weight = weight.mean(-1)
        if self.with_yaw:
            loss = 1 - cal_iou_3d(pred[None, ...], target[None, ...])  # (1, N)
        else:
            loss = axis_aligned_iou_loss(centre_size_to_corners(pred),
                                         centre_size_to_corners(target))  # (N,)
        if weight is not None:
            # reference :53-54 returns pred.sum() * weight.sum() (== 0) when no weight is
            # positive; masking the unweighted entries gives the same zeros without the
            # host sync of `if not torch.any(weight > 0)`.
            loss = torch.where(weight > 0, loss, torch.zeros_like(loss))
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


# ---- GIoU3D / DIoU3D (iou3d_loss.py:16-18, 38-68, 78-81) ---------------------------
class _EnclosingIoU3DLoss(nn.Module):
    """IoU3DMixin around an enclosing-box loss.  Deliberately not an ``IoU3DLoss``: the fused
    head-loss kernel computes plain IoU and must keep refusing a head with one of these."""

    loss_function = None

    def __init__(self, reduction='mean', loss_weight=1.0, enclosing_type='smallest'):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.enclosing_type = enclosing_type

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        if weight is not None and weight.dim() > 1:
            weight = weight.mean(-1)
        # the reference's `[0][0]`: the loss of (loss, iou), then the batch axis added here
        loss = type(self).loss_function(pred[None, ...], target[None, ...],
                                        self.enclosing_type)[0][0]  # (N,)
        if weight is not None:
            # as IoU3DLoss: zeros where no weight is positive, without the host sync of :53-54
            loss = torch.where(weight > 0, loss, torch.zeros_like(loss))
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


class GIoU3DLoss(_EnclosingIoU3DLoss):
    loss_function = staticmethod(cal_giou_3d)


class DIoU3DLoss(_EnclosingIoU3DLoss):
    """The reference has ``cal_diou_3d`` but no loss class; the name follows its pattern."""
    loss_function = staticmethod(cal_diou_3d)


# ---- quality focal loss (gfocal_loss.py:9-51, 80-139) ---------------------------
def quality_focal_loss(pred, target, beta=2.0, use_sigmoid=True):
    label, score = target
    if use_sigmoid:
        func = F.binary_cross_entropy_with_logits
        pred_sigmoid = pred.sigmoid()
    else:
        func = F.binary_cross_entropy
        pred_sigmoid = pred
    zerolabel = pred.new_zeros(pred.shape)
    loss = func(pred, zerolabel, reduction='none') * pred_sigmoid.pow(beta)
    bg_class_ind = pred.size(1)
    # positives (0 <= label < C) are supervised by the IoU score at their class column;
    # written as a dense one-hot select instead of the reference's nonzero()/index_put
    pos = ((label >= 0) & (label < bg_class_ind))
    onehot = F.one_hot(label.clamp(0, bg_class_ind - 1).long(), bg_class_ind).bool() \
        & pos.unsqueeze(1)
    score_b = score.unsqueeze(1).expand_as(pred)
    pos_loss = func(pred, score_b, reduction='none') * (score_b - pred_sigmoid).abs().pow(beta)
    loss = torch.where(onehot, pos_loss, loss)
    return loss.sum(dim=1, keepdim=False)


class GeneralQualityFocalLoss(nn.Module):
    def __init__(self, use_sigmoid=True, beta=2.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.use_sigmoid = use_sigmoid
        self.beta = beta
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        loss = quality_focal_loss(pred, target, beta=self.beta, use_sigmoid=self.use_sigmoid)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction, avg_factor)


# ---- distribution focal loss (gfocal_loss.py:54-76, 143-197) ---------------------
def distribution_focal_loss(pred, label, weight=None, reduction='mean', avg_factor=None):
    """pred (N, n+1) logits over the integral set, label (N,) real distances in [0, n): the two
    neighbouring integers' cross entropies, weighted by the distance to the other one -> weighted
    and reduced as ``weighted_loss`` does."""
    dis_left = label.long()
    dis_right = dis_left + 1
    weight_left = dis_right.float() - label
    weight_right = label - dis_left.float()
    loss = F.cross_entropy(pred, dis_left, reduction='none') * weight_left \
        + F.cross_entropy(pred, dis_right, reduction='none') * weight_right
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


class GeneralDistributionFocalLoss(nn.Module):
    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * distribution_focal_loss(
            pred, target, weight, reduction=reduction, avg_factor=avg_factor)


# ---- sigmoid focal loss (mmdet focal_loss.py; formulas of include/nesie_ops.h) ----
class _FocalTerms(Function):
    """Elementwise focal loss of logits against a boolean one-hot mask, in tensor ops of any dtype
    and device.  Forward and backward are the softplus formulas written out: autograd through
    ``max`` / ``abs`` would halve or double the slope at x == 0, and through ``exp`` it forms
    ``inf * 0`` at |x| ~ 3e38."""

    @staticmethod
    def _parts(pred, positive, gamma, alpha):
        z = torch.where(positive, pred, -pred)
        a = torch.where(positive, pred.new_tensor(alpha), pred.new_tensor(1 - alpha))
        e = torch.exp(-z.abs())
        log1p_e = torch.log1p(e)
        sp_pos = z.clamp(min=0) + log1p_e            # softplus(z)
        sp_neg = (-z).clamp(min=0) + log1p_e         # softplus(-z)
        return z, e, sp_neg, a * torch.exp(-(gamma * sp_pos))

    @staticmethod
    def forward(ctx, pred, positive, gamma, alpha):
        ctx.save_for_backward(pred, positive)
        ctx.gamma, ctx.alpha = gamma, alpha
        _, _, sp_neg, w = _FocalTerms._parts(pred, positive, gamma, alpha)
        return w * sp_neg

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pred, positive = ctx.saved_tensors
        z, e, sp_neg, w = _FocalTerms._parts(pred, positive, ctx.gamma, ctx.alpha)
        r = 1 / (1 + e)
        s_pos = torch.where(z >= 0, r, e * r)        # sigmoid(z)
        s_neg = torch.where(z >= 0, e * r, r)        # sigmoid(-z)
        dz = w * (ctx.gamma * s_pos * sp_neg + s_neg)
        return grad * torch.where(positive, -dz, dz), None, None, None


def py_sigmoid_focal_loss(pred, target, weight=None, gamma=2.0, alpha=0.25, reduction='mean',
                          avg_factor=None):
    """mmdet's tensor-op focal loss on the stable formulas.  pred (N, C) logits; target (N, C)
    one-hot (bool or any number type, positive where non-zero); weight (N,), (N, C) or of N * C
    elements."""
    loss = _FocalTerms.apply(pred, target != 0, float(gamma), float(alpha))
    if weight is not None:
        if weight.shape != loss.shape:
            if weight.size(0) == loss.size(0):
                # one weight per sample: broadcast over the classes
                weight = weight.view(-1, 1)
            else:
                assert weight.numel() == loss.numel()
                weight = weight.view(loss.size(0), -1)
        assert weight.dim() == loss.dim()
    return weight_reduce_loss(loss, weight, reduction, avg_factor)


class FocalLoss(nn.Module):
    """mmdet's ``FocalLoss`` for integer labels: pred (N, C), target (N,) with any value outside
    [0, C) as background.  float32 tensors served by the HIP back end go through
    ``csrc/focal_loss.hip`` (reduced forward fused, backward one launch, ``'none'`` with the weight
    applied in the launch); every other dtype and device, an empty input and a weight that requires a
    gradient take ``py_sigmoid_focal_loss``."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, 'Only sigmoid focal loss supported now.'
        self.use_sigmoid = use_sigmoid
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight

    @staticmethod
    def _native(pred):
        if pred.dtype != torch.float32 or not (pred.is_cuda or injected_backend() is not None):
            return False
        return getattr(backend_for(pred), 'name', '') == 'hip'

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        # the kernels differentiate the logits only: a weight or avg_factor that wants a gradient
        # goes through autograd
        wants_grad = any(torch.is_tensor(v) and v.requires_grad for v in (weight, avg_factor))
        if pred.numel() == 0 or wants_grad or not self._native(pred):
            num_classes = pred.size(1)
            onehot = target.view(-1, 1) == torch.arange(num_classes, device=pred.device)
            return self.loss_weight * py_sigmoid_focal_loss(
                pred, onehot, weight, self.gamma, self.alpha, reduction, avg_factor)
        if avg_factor is not None and reduction == 'sum':
            raise ValueError('avg_factor can not be used with reduction="sum"')
        n, c = pred.shape
        if weight is not None:
            assert weight.size(0) == n or weight.numel() == n * c
            weight = weight.to(torch.float32).contiguous()
        scale, scale_dev = float(self.loss_weight), None
        if reduction == 'mean':
            if avg_factor is None:
                scale /= n * c
            elif torch.is_tensor(avg_factor):
                # the kernels multiply by the device scalar: one small launch for its reciprocal
                scale_dev = avg_factor.to(pred.device, torch.float32).reshape(1).reciprocal()
            else:
                scale /= avg_factor
        return _FocalLossFn.apply(pred, target, weight, float(self.gamma), float(self.alpha),
                                  reduction != 'none', scale, scale_dev)


class _FocalLossFn(Function):
    @staticmethod
    def forward(ctx, pred, target, sample_weight, gamma, alpha, reduce, scale, scale_dev):
        pred, target = pred.contiguous(), target.long().contiguous()
        ctx.save_for_backward(pred, target, sample_weight, scale_dev)
        ctx.args = (gamma, alpha, reduce, scale)
        return focal_forward(pred, target, None, sample_weight, gamma, alpha, reduce, scale,
                             scale_dev)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        pred, target, sample_weight, scale_dev = ctx.saved_tensors
        gamma, alpha, reduce, scale = ctx.args
        return (focal_backward(grad, pred, target, None, sample_weight, gamma, alpha, reduce,
                               scale, scale_dev),) + (None,) * 7


def lovasz_grad(gt_sorted):
    """Gradient of the Lovasz extension w.r.t. the sorted errors (reference lovasz_loss.py:38-50,
    Alg. 1 of the paper), float32 like the reference's.  The reference differences
    ``1 - intersection / union`` of neighbouring entries; intersection and union are integer
    counts, so the difference is formed here in closed form from them in float64:
    ``1 / U`` at a foreground entry, ``I / (U (U - 1))`` at a background one."""
    fg = gt_sorted.reshape(-1) != 0
    cf = fg.cumsum(0)
    at = torch.arange(1, fg.numel() + 1, device=fg.device)
    union = (fg.sum() + (at - cf)).double()
    inter = (fg.sum() - cf).double()
    g = torch.where(fg, 1.0 / union, torch.where(
        union > 1, inter / (union * (union - 1)).clamp(min=1), torch.ones_like(union)))
    return g.float()


def flatten_probas(probas, labels, ignore=None):
    """(B, H, W) sigmoid output, (B, C, H, W) or (B, C, L, H, W) -> (P, C) probabilities and (P,)
    labels, the void points removed when ``ignore`` is given (reference lovasz_loss.py:86-106).
    Kept for code that calls it; ``lovasz_softmax`` itself neither permutes nor compacts."""
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)
    b, c = probas.shape[:2]
    probas = probas.reshape(b, c, -1).permute(0, 2, 1).reshape(-1, c)
    labels = labels.reshape(-1)
    if ignore is None:
        return probas, labels
    valid = labels != ignore
    return probas[valid], labels[valid]


def _lovasz_segments(probas, labels, classes, per_image, ignore):
    """probas (B, C, S) in any layout, labels (B, S) -> the loss; the checks the reference makes on
    the way (lovasz_loss.py:71-73)."""
    c = probas.shape[1]
    if c == 1:
        # the sigmoid form: one listed class k, foreground where the label is k
        if isinstance(classes, str) or len(classes) != 1:
            raise ValueError('Sigmoid output possible only with 1 class')
        k = int(classes[0])
        if k != 0:
            # k -> 0, everything else background (-1), void (-2) first as the reference compacts first
            fg = torch.where(labels == k, 0, -1)
            if ignore is not None:
                fg = torch.where(labels == ignore, -2, fg)
                ignore = -2
            labels, classes = fg, [0]
    return lovasz_softmax_op(probas, labels, classes, per_image, ignore)


def lovasz_softmax_flat(probas, labels, classes='present'):
    """Multi-class Lovasz-Softmax loss of probas (P, C) and labels (P,); ``classes``: 'all',
    'present' (the classes present in labels) or a list of classes to average (reference
    lovasz_loss.py:52-82).  The (P, C) tensor is read in place, on the device by the sort-and-scan
    kernels of csrc/lovasz.hip.  Equal errors are ordered by ascending point index."""
    assert probas.dim() == 2 and labels.numel() == probas.shape[0]
    return _lovasz_segments(probas.t().unsqueeze(0), labels.reshape(1, -1), classes, False, None)


def lovasz_softmax(probas, labels, classes='present', per_image=False, ignore=None):
    """Multi-class Lovasz-Softmax loss (reference lovasz_loss.py:109-126).  probas: (B, C, H, W)
    class probabilities, (B, C, L, H, W) for 3-D segmentation, or (B, H, W) as the output of a
    sigmoid; labels: (B, H, W) / (B, L, H, W) ground truth; ``per_image``: the mean of the images'
    losses instead of the loss of the batch; ``ignore``: the void label.

    Where the reference returns the Python int 0 (no class present) or an empty (0, C) tensor (no
    valid point), this returns a 0-d zero attached to the graph with a zero gradient: neither case
    is known without reading the device."""
    if probas.dim() == 3:
        probas = probas.unsqueeze(1)
    assert probas.dim() in (4, 5), 'probas: (B, H, W), (B, C, H, W) or (B, C, L, H, W)'
    b, c = probas.shape[:2]
    return _lovasz_segments(probas.reshape(b, c, -1), labels.reshape(b, -1), classes, per_image,
                            ignore)


class Lovasz3D(nn.Module):
    """Reference lovasz_loss.py:128-167: ``reduction`` is accepted and unused, ``weight`` only
    decides the all-zero early return.  ``ignore_index`` (keyword only) is an extension: the
    reference module never forwards ``ignore``."""

    def __init__(self, loss_function, reduction='mean', loss_weight=1.0, per_image=False,
                 classes='present', *, ignore_index=None):
        super().__init__()
        self.loss_function = loss_function
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.per_image = per_image
        self.classes = classes
        self.ignore_index = ignore_index

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None,
                **kwargs):
        if weight is not None and not torch.any(weight > 0):
            return pred.sum() * weight.sum()  # 0
        assert reduction_override in (None, 'none', 'mean', 'sum')
        if self.ignore_index is None:
            return self.loss_weight * self.loss_function(pred, target, self.classes,
                                                         self.per_image)
        return self.loss_weight * self.loss_function(pred, target, self.classes, self.per_image,
                                                     self.ignore_index)


class Lovasz3DLoss(Lovasz3D):
    def __init__(self, reduction='mean', loss_weight=1.0, per_image=False, classes='present', *,
                 ignore_index=None):
        super().__init__(lovasz_softmax, reduction, loss_weight, per_image, classes,
                         ignore_index=ignore_index)


_LOSSES = dict(ChamferDistance=ChamferDistance, CrossEntropyLoss=CrossEntropyLoss,
               Lovasz3DLoss=Lovasz3DLoss,
               FocalLoss=FocalLoss, GeneralDistributionFocalLoss=GeneralDistributionFocalLoss,
               IoU3DLoss=IoU3DLoss, GIoU3DLoss=GIoU3DLoss, DIoU3DLoss=DIoU3DLoss,
               AxisAlignedIoULoss=AxisAlignedIoULoss,
               GeneralQualityFocalLoss=GeneralQualityFocalLoss,
               SurfaceLoss=SurfaceLoss, SidePredLoss=SidePredLoss, MSELoss=MSELoss,
               L1Loss=L1Loss, SmoothL1Loss=SmoothL1Loss)


def build_loss(cfg):
    cfg = dict(cfg)
    return _LOSSES[cfg.pop('type')](**cfg)
