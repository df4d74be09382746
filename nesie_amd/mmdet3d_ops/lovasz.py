"""Lovasz-Softmax loss on ``csrc/lovasz.hip`` (reference mmdet3d/models/losses/lovasz_loss.py:38-126;
formulas, tie rule and void handling: include/nesie_ops.h).

``lovasz_softmax_op`` takes the probabilities as ``(B, C, S)`` of any dense strides (the flat
``(P, C)`` tensor is the view ``probas.t()[None]``), so nothing is permuted or compacted.  A HIP
tensor goes through one call of the kernel entry, which returns the loss AND d loss / d probas; the
backward is that saved gradient times the upstream scalar, one elementwise launch.  A CPU tensor
goes through ``lovasz_softmax_torch``, the same closed form and the same tie rule in torch ops: the
reference runs on the CPU, and ``tools/lovasz_bench.py`` times the kernels against this formulation
on the device.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ..kernels import backend_for

CLASS_MODES = {'all': 0, 'present': 1}      # 2: a class list, as counts per class
_masks = {}                                  # (classes, C, device) -> int32 counts on the device


def class_selector(classes, c, device):
    """``classes`` ('all', 'present' or a list of class numbers) -> (class_mode, class_mask): the
    mask counts how often each of the ``c`` classes is listed (the reference averages a class
    listed twice twice).  A listed class outside [0, c) is an IndexError, as indexing the
    probabilities with it is in the reference.  The mask of a list is built once per device."""
    if isinstance(classes, str):
        return CLASS_MODES[classes], None          # another string: KeyError
    listed = tuple(int(k) for k in classes)
    key = (listed, c, str(device))
    if key not in _masks:
        counts = [0] * c
        for k in listed:
            if not 0 <= k < c:
                raise IndexError(f'class {k} is out of range for {c} classes')
            counts[k] += 1
        _masks[key] = torch.tensor(counts, dtype=torch.int32, device=device)
    return 2, _masks[key]


def _dense(t):
    """Whether the elements of ``t`` tile its storage span without overlap or gap."""
    expect = 1
    for size, stride in sorted(((n, s) for n, s in zip(t.shape, t.stride()) if n != 1),
                               key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def lovasz_softmax_torch(probas, labels, per_image=False, ignore=None, class_mode=1,
                         class_mask=None):
    """probas (B, C, S), labels (B, S) -> (loss 0-d, d loss / d probas (B, C, S)) in torch ops on
    the tensors' device: the closed form of the Lovasz gradient from integer counts in float64,
    a stable descending sort (equal errors by ascending point index; +inf and NaN first), void
    points last with fg = 0.  The arguments are those of ``HipKernels.lovasz_softmax``."""
    with torch.no_grad():
        b, c, s = probas.shape
        dev = probas.device
        lab = labels.reshape(b, 1, s)
        void = (lab == ignore) if ignore is not None else torch.zeros_like(lab, dtype=torch.bool)
        fg = (lab == torch.arange(c, device=dev).view(1, c, 1)) & ~void
        e = (fg.to(torch.float32) - probas.to(torch.float32)).abs()
        void = void.expand(b, c, s)
        if per_image:
            rows = lambda t: t.reshape(b * c, s)
        else:
            rows = lambda t: t.permute(1, 0, 2).reshape(c, b * s)
        e, fg, void = rows(e), rows(fg), rows(void)
        key = torch.where(void, torch.full_like(e, -1.0), e)
        key = torch.where(torch.isfinite(key), key, torch.full_like(e, float('inf')))
        perm = torch.sort(key, dim=1, descending=True, stable=True)[1]
        fg_s, void_s, e_s = fg.gather(1, perm), void.gather(1, perm), e.gather(1, perm)
        g_count = fg.sum(1, keepdim=True)                               # G
        cf = fg_s.cumsum(1)
        at = torch.arange(1, e.shape[1] + 1, device=dev).view(1, -1)
        union = (g_count + (at - cf)).double()                          # U
        inter = (g_count - cf).double()                                 # I
        one = torch.ones_like(union)
        g = torch.where(fg_s, 1.0 / union,
                        torch.where(union > 1, inter / (union * (union - 1)).clamp(min=1), one))
        zero = torch.zeros_like(g)
        g = torch.where(void_s, zero, g)
        seg_loss = (torch.where(void_s, zero, e_s.double()) * g).sum(1)
        if class_mode == 0:
            weight = torch.ones_like(seg_loss)
        elif class_mode == 1:
            weight = (g_count.view(-1) > 0).double()
        else:
            weight = class_mask.clamp(min=0).double().repeat(b if per_image else 1)
        images = b if per_image else 1
        weight = weight.view(images, c)
        n = weight.sum(1, keepdim=True)
        scale = torch.where(n > 0, weight / (n.clamp(min=1) * images), torch.zeros_like(weight))
        seg_loss = seg_loss.view(images, c)
        loss = torch.where(weight > 0, scale * seg_loss, torch.zeros_like(seg_loss)).sum()
        grad_s = (torch.where(fg_s, -g, g) * scale.view(-1, 1)).to(torch.float32)
        grad = torch.zeros_like(grad_s).scatter_(1, perm, grad_s)
        if per_image:
            grad = grad.view(b, c, s)
        else:
            grad = grad.view(c, b, s).permute(1, 0, 2)
        return loss.to(torch.float32), grad


def lovasz_forward(probas, labels, per_image, ignore, class_mode, class_mask):
    """-> (loss 0-d, d loss / d probas in the layout of ``probas``): one back-end call on a HIP
    tensor, the torch formulation on a CPU one.  An empty input launches nothing."""
    if probas.numel() == 0:
        return probas.new_zeros(()), torch.zeros_like(probas)
    if not probas.is_cuda:
        return lovasz_softmax_torch(probas, labels, per_image, ignore, class_mode, class_mask)
    loss = probas.new_empty(1)
    grad = torch.empty_strided(probas.shape, probas.stride(), dtype=probas.dtype,
                               device=probas.device)
    backend_for(probas).lovasz_softmax(probas, labels, loss, grad, per_image, ignore, class_mode,
                                       class_mask)
    return loss.view(()), grad


class LovaszSoftmaxFunction(Function):

    @staticmethod
    def forward(ctx, probas, labels, per_image, ignore, class_mode, class_mask):
        loss, grad = lovasz_forward(probas, labels, per_image, ignore, class_mode, class_mask)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        return grad * grad_output, None, None, None, None, None


def lovasz_softmax_op(probas, labels, classes='present', per_image=False, ignore=None):
    """probas (B, C, S) class probabilities, labels (B, S) -> the 0-d Lovasz-Softmax loss,
    differentiable in ``probas``.  ``classes``: 'all', 'present' or a list of class numbers."""
    assert probas.dim() == 3 and labels.numel() == probas.shape[0] * probas.shape[2]
    b, c, s = probas.shape
    class_mode, class_mask = class_selector(classes, c, probas.device)
    if probas.dtype != torch.float32:
        probas = probas.float()
    if not _dense(probas):
        probas = probas.contiguous()
    labels = labels.reshape(b, s).long().contiguous()
    return LovaszSoftmaxFunction.apply(probas, labels, bool(per_image), ignore, class_mode,
                                       class_mask)
