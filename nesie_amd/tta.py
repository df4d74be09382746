"""Test-time augmentation: the views of one scene and the merge of their detections
(``mmdet3d/core/post_processing/merge_augs.py``, ``core/bbox/transforms.py:4-23``,
``structures/utils.py:64-82``).

The merge maps every view's boxes back to the original frame, runs ONE batched BEV NMS
launch sequence over all classes (``nesie_bev_nms``; the reference calls ``nms_gpu`` once per
class) and orders the survivors as the reference does: class-major concatenation, then a
descending score sort (equal scores by ascending merged position), then ``max_num``.  The
result reaches the host in one transfer, at the end.

Config keys the shipped ``test_cfg``s lack: without ``use_rotate_nms`` the merge uses the
rotated BEV IoU (the boxes carry a yaw); without ``max_num`` nothing is cut.  (The reference
would raise on both.)
"""
import torch

from .mmdet3d_ops.iou3d import _bev_nms, batched_nms_bev, compact_kept
from .votenet.boxes import DepthInstance3DBoxes


def bbox3d_mapping_back(bboxes, scale_factor, flip_horizontal, flip_vertical):
    """Boxes of an augmented view back in the frame of the original scene: undo the flips,
    then scale by ``1 / scale_factor``."""
    new_bboxes = bboxes.clone()
    if flip_horizontal:
        new_bboxes.flip('horizontal')
    if flip_vertical:
        new_bboxes.flip('vertical')
    new_bboxes.scale(1 / scale_factor)
    return new_bboxes


def xywhr2xyxyr(boxes_xywhr):
    """(n,5) (x, y, w, h, r) -> (n,5) (x1, y1, x2, y2, r)."""
    boxes = torch.zeros_like(boxes_xywhr)
    half_w = boxes_xywhr[:, 2] / 2
    half_h = boxes_xywhr[:, 3] / 2
    boxes[:, 0] = boxes_xywhr[:, 0] - half_w
    boxes[:, 1] = boxes_xywhr[:, 1] - half_h
    boxes[:, 2] = boxes_xywhr[:, 0] + half_w
    boxes[:, 3] = boxes_xywhr[:, 1] + half_h
    boxes[:, 4] = boxes_xywhr[:, 4]
    return boxes


def _cfg(test_cfg, key, default=None):
    if isinstance(test_cfg, dict):
        return test_cfg.get(key, default)
    return getattr(test_cfg, key, default)


def _view_meta(img_meta):
    m = img_meta[0] if isinstance(img_meta, (list, tuple)) else img_meta
    return m['pcd_scale_factor'], m['pcd_horizontal_flip'], m['pcd_vertical_flip']


def _finish(kept, boxes, scores, labels, max_num):
    """kept (n) int64 merged rows of (boxes, scores, labels), -1 padded -> bbox3d2result of the
    reference's final order.  One device->host transfer."""
    from .votenet.detector import bbox3d2result
    live = kept >= 0
    idx = kept.clamp(min=0)
    s = torch.where(live, scores[idx], torch.full_like(scores[idx], float('nan')))
    nan = torch.isnan(s)
    # descending score, equal scores by merged position, NaN (and the padding after it) last
    order = torch.sort(torch.where(nan, torch.full_like(s, -float('inf')), s),
                       descending=True, stable=True)[1]
    order = order[torch.sort(nan[order].to(torch.uint8), stable=True)[1]]
    sel = idx[order]
    packed = torch.cat([boxes[sel], scores[sel].unsqueeze(1), labels[sel].unsqueeze(1).to(boxes.dtype),
                        live[order].unsqueeze(1).to(boxes.dtype)], 1).cpu()
    num = int(packed[:, -1].sum().item())
    if max_num is not None:
        num = min(num, int(max_num))
    out = DepthInstance3DBoxes(packed[:num, :7])
    return bbox3d2result(out, packed[:num, 7].contiguous(), packed[:num, 8].to(labels.dtype))


def merge_aug_bboxes_3d(aug_results, img_metas, test_cfg):
    """Merge the detections of several views of one scene (the reference's signature).
    aug_results: per view a dict with boxes_3d / scores_3d / labels_3d (host or device);
    img_metas: per view a one-element list of metas with pcd_scale_factor,
    pcd_horizontal_flip and pcd_vertical_flip.  -> dict of host results."""
    assert len(aug_results) == len(img_metas), \
        '"aug_results" should have the same length as "img_metas", got len(' \
        f'aug_results)={len(aug_results)} and len(img_metas)={len(img_metas)}'
    dev = aug_results[0]['scores_3d'].device
    if dev.type != 'cuda':
        dev = torch.device('cuda')   # the NMS runs on the GPU, as in the reference
    boxes, scores, labels = [], [], []
    for res, meta in zip(aug_results, img_metas):
        s, h, v = _view_meta(meta)
        boxes.append(bbox3d_mapping_back(res['boxes_3d'].to(dev), s, h, v))
        scores.append(res['scores_3d'].to(dev))
        labels.append(res['labels_3d'].to(dev))
    aug_boxes = DepthInstance3DBoxes.cat(boxes)
    aug_scores = torch.cat(scores, 0)
    aug_labels = torch.cat(labels, 0)
    max_num = _cfg(test_cfg, 'max_num')
    if len(aug_labels) == 0:
        from .votenet.detector import bbox3d2result
        return bbox3d2result(aug_boxes, aug_scores, aug_labels)
    kept, _ = batched_nms_bev(xywhr2xyxyr(aug_boxes.bev), aug_scores, aug_labels,
                              _cfg(test_cfg, 'nms_thr'), _cfg(test_cfg, 'use_rotate_nms', True))
    return _finish(kept, aug_boxes.tensor, aug_scores, aug_labels, max_num)


def merge_detect_tensors(tensors, img_metas, test_cfg, per_class_proposal):
    """The merge straight from a batch of views' ``detect_tensors`` (boxes (A,K,7), obj
    (A,K), sem (A,K,C), classes (A,K), selected (A,K)), with fixed shapes until the final
    transfer: segment c holds the A*K proposals in (view, proposal) order -- the order of
    the reference's per-view results -- and ``selected`` (and, without per-class proposals,
    the class) marks the ones that take part."""
    boxes, obj, sem, classes, selected = tensors
    A, K, C = sem.shape
    mapped = []
    for a in range(A):
        s, h, v = _view_meta(img_metas[a])
        bx = DepthInstance3DBoxes.__new__(DepthInstance3DBoxes)
        bx.tensor = boxes[a]
        mapped.append(bbox3d_mapping_back(bx, s, h, v))
    aug_boxes = DepthInstance3DBoxes.cat(mapped)                      # (A*K, 7)
    L = A * K
    cls_ids = torch.arange(C, device=boxes.device)
    if per_class_proposal:
        seg_scores = (obj.unsqueeze(-1) * sem).reshape(L, C).t()       # (C, L)
        valid = selected.reshape(1, L).expand(C, L)
    else:
        seg_scores = obj.reshape(1, L).expand(C, L)
        valid = selected.reshape(1, L) & (classes.reshape(1, L) == cls_ids.view(C, 1))
    nms_boxes = xywhr2xyxyr(aug_boxes.bev).unsqueeze(0).expand(C, L, 5).reshape(C * L, 5)
    offsets = (torch.arange(C + 1, device=boxes.device, dtype=torch.int32) * L)
    keep, count = _bev_nms(nms_boxes, seg_scores.reshape(-1), offsets, L,
                           _cfg(test_cfg, 'nms_thr'), _cfg(test_cfg, 'use_rotate_nms', True),
                           valid.reshape(-1))
    rows = torch.arange(C * L, device=boxes.device)
    kept, _ = compact_kept(rows, keep, count, offsets)
    flat_boxes = aug_boxes.tensor.repeat(C, 1)                          # row -> box
    flat_labels = cls_ids.to(classes.dtype).repeat_interleave(L)
    return _finish(kept, flat_boxes, seg_scores.reshape(-1), flat_labels,
                   _cfg(test_cfg, 'max_num'))


def tta_views(points, flips=((False, False), (True, False)), scales=(1.0,)):
    """Augmented views of ONE scene (N, C) on its device, in MultiScaleFlipAug3D's order (scale
    outer, flip inner): xyz scaled, then x negated for a horizontal flip and y for a vertical
    one (DepthPoints.flip).  -> (points, img_metas) in ``aug_test``'s format: one one-sample
    list per view."""
    views, metas = [], []
    for s in scales:
        for h, v in flips:
            p = points.clone()
            p[:, :3] *= s
            if h:
                p[:, 0] = -p[:, 0]
            if v:
                p[:, 1] = -p[:, 1]
            views.append([p])
            metas.append([dict(pcd_scale_factor=s, pcd_horizontal_flip=bool(h),
                               pcd_vertical_flip=bool(v), flip=bool(h or v),
                               box_type_3d=DepthInstance3DBoxes)])
    return views, metas


__all__ = ['bbox3d_mapping_back', 'xywhr2xyxyr', 'merge_aug_bboxes_3d', 'merge_detect_tensors',
           'tta_views']
