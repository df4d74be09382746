"""Host referee of the BEV NMS (iou3d_cuda.nms_gpu / nms_normal_gpu): overlaps from the CPU
oracle's boxes_overlap_bev, IoU in float32 with the reference's formulas, a python greedy walk."""
import numpy as np
import torch

from nesie_amd import kernels
from nesie_amd.mmdet3d_ops import boxes_overlap_bev


def descending_order(scores):
    """Descending score, equal scores by ascending index, NaN last."""
    s = scores.numpy().astype(np.float32)
    key = np.where(np.isnan(s), np.float32(-np.inf), s)
    order = np.argsort(-key, kind='stable')
    return order[np.argsort(np.isnan(s[order]), kind='stable')]


def area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def iou_rows(oracle, a, bs, rotated):
    """IoU of box a (5,) (as box_a) with each row of bs (m,5): float32."""
    a1 = a.view(1, 5)
    if rotated:
        with kernels.use_backend(oracle):
            ov = boxes_overlap_bev(a1, bs)[0]
    else:
        w = torch.clamp(torch.minimum(a1[:, 2], bs[:, 2]) - torch.maximum(a1[:, 0], bs[:, 0]), min=0)
        h = torch.clamp(torch.minimum(a1[:, 3], bs[:, 3]) - torch.maximum(a1[:, 1], bs[:, 1]), min=0)
        ov = w * h
    return ov / torch.clamp(area(a1) + area(bs) - ov, min=1e-8)


def neighbours(boxes):
    """Pairs whose bounding circles meet (all others overlap by exactly 0): list of index arrays."""
    c = torch.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], 1).double()
    r = 0.5 * torch.hypot((boxes[:, 2] - boxes[:, 0]).double(), (boxes[:, 3] - boxes[:, 1]).double())
    out = []
    for i0 in range(0, len(boxes), 1024):
        d = torch.cdist(c[i0:i0 + 1024], c)
        near = d <= r[i0:i0 + 1024, None] + r[None, :] + 1e-3
        out += [torch.nonzero(row).view(-1) for row in near]
    return out


def referee_nms(oracle, boxes, scores, thr, rotated, valid=None, near_gap=1e-6):
    """-> (kept indices in pick order, smallest |iou - thr| over the pairs the walk looks at)."""
    order = descending_order(scores)
    if valid is not None:
        order = np.array([i for i in order if valid[i]], dtype=np.int64)
    pos = np.full(len(scores), -1)
    pos[order] = np.arange(len(order))
    nb = neighbours(boxes)
    removed = np.zeros(len(scores), dtype=bool)
    keep, gap = [], np.inf
    for i in order:
        js = nb[i]
        js = js[torch.from_numpy(pos[js.numpy()] > pos[i])]
        iou = iou_rows(oracle, boxes[i], boxes[js], rotated) if len(js) else torch.zeros(0)
        if len(js):
            gap = min(gap, float((iou - thr).abs().min()))
        if removed[i]:
            continue
        keep.append(int(i))
        removed[js[iou > thr].numpy()] = True
    return keep, gap


def pick_threshold(oracle, boxes, scores, rotated, candidates=(0.25, 0.2503, 0.2507, 0.31, 0.37)):
    """The first threshold no IoU pair lies within 1e-6 of -> (thr, referee keep)."""
    for thr in candidates:
        keep, gap = referee_nms(oracle, boxes, scores, thr, rotated)
        if gap > 1e-6:
            return thr, keep
    raise AssertionError('every candidate threshold has a pair within 1e-6')
