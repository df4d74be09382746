"""``mmdet3d.ops.iou3d`` (iou3d_utils.py, src/iou3d.cpp): the rotated BEV overlap behind
``BaseInstance3DBoxes.overlaps``, the BEV IoU and the two BEV NMS of test-time augmentation
(``merge_aug_bboxes_3d``).  The NMS runs as one fixed launch sequence for any number of
independent segments (``nesie_bev_nms``); the reference copies its suppression mask to the
host and walks it there."""
import torch

from ..kernels import backend_for

MAX_SEGMENT = 8192   # boxes per NMS segment the kernel is built for


def boxes_overlap_bev(boxes_a, boxes_b):
    """(N,5), (M,5) (x1, y1, x2, y2, ry) -> (N,M) overlap areas
    (``iou3d_cuda.boxes_overlap_bev_gpu``; the reference fills a caller-made tensor)."""
    ans = boxes_a.new_zeros((boxes_a.shape[0], boxes_b.shape[0]))
    backend_for(boxes_a).boxes_overlap_bev(boxes_a.contiguous().float(),
                                           boxes_b.contiguous().float(), ans)
    return ans


def boxes_iou_bev(boxes_a, boxes_b):
    """(M,5), (N,5) (x1, y1, x2, y2, ry) -> (M,N) BEV IoU (``iou3d_cuda.boxes_iou_bev_gpu``,
    iou_bev of iou3d_kernel.cu:244-250): overlap / max(area_a + area_b - overlap, 1e-8)."""
    a, b = boxes_a.contiguous().float(), boxes_b.contiguous().float()
    ov = boxes_overlap_bev(a, b)
    sa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    sb = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return ov / torch.clamp(sa.view(-1, 1) + sb.view(1, -1) - ov, min=1e-8)


def nms_workspace_bytes(n, max_segment):
    """Bytes of device workspace ``nesie_bev_nms`` needs: the (n, ceil(max_segment / 64))
    suppression mask, the sorted boxes and their order."""
    return n * (8 * ((max_segment + 63) // 64) + 24)


def _bev_nms(boxes, scores, offsets, max_segment, thresh, rotated, valid=None):
    """Segments given as device offsets (S+1) -> keep (n) int32, count (S) int32."""
    boxes = boxes.contiguous().float()
    scores = scores.contiguous().float()
    n, s = scores.shape[0], offsets.numel() - 1
    dev = boxes.device
    keep = torch.empty((n,), dtype=torch.int32, device=dev)
    count = torch.empty((s,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(nms_workspace_bytes(n, max_segment), 1),), dtype=torch.uint8,
                     device=dev)
    backend_for(boxes).bev_nms(
        boxes.reshape(n, 5), scores, None if valid is None else valid.to(torch.uint8).contiguous(),
        offsets.to(torch.int32).contiguous(), max_segment, thresh, rotated, keep, count, ws)
    return keep, count


def _descending_order(scores):
    """The kernel's candidate order: descending score, equal scores by ascending index, NaN
    last."""
    nan = torch.isnan(scores)
    order = torch.sort(torch.where(nan, torch.full_like(scores, -float('inf')), scores),
                       descending=True, stable=True)[1]
    return order[torch.sort(nan[order].to(torch.uint8), stable=True)[1]]


def _single_nms(boxes, scores, thresh, rotated, pre_maxsize=None):
    n = scores.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.long, device=boxes.device)
    valid = None
    if pre_maxsize is not None and pre_maxsize < n:
        valid = torch.zeros((n,), dtype=torch.uint8, device=boxes.device)
        valid[_descending_order(scores.float())[:pre_maxsize]] = 1
    offsets = torch.tensor([0, n], dtype=torch.int32, device=boxes.device)
    keep, count = _bev_nms(boxes, scores, offsets, n, thresh, rotated, valid)
    return keep[:int(count[0])].long()


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """Rotated BEV NMS (``iou3d_utils.nms_gpu``): boxes (N,5) (x1, y1, x2, y2, ry),
    scores (N) -> LongTensor of the kept indices, best score first.  N <= 8192."""
    keep = _single_nms(boxes, scores, thresh, True, pre_maxsize)
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


def nms_normal_gpu(boxes, scores, thresh):
    """Axis-aligned BEV NMS (``iou3d_utils.nms_normal_gpu``; ry is ignored): boxes (N,5),
    scores (N) -> LongTensor of the kept indices, best score first.  N <= 8192."""
    return _single_nms(boxes, scores, thresh, False)


def batched_nms_bev(boxes, scores, segment_ids, thresh, rotated=True, num_segments=None):
    """Independent BEV NMS per segment (e.g. per class) in one launch sequence.
    boxes (n,5), scores (n), segment_ids (n) in [0, num_segments) -> (keep, count): keep (n)
    int64 holds the kept input indices of each segment, best score first, segment after
    segment (segment t from sum(count[:t])); count (num_segments) int64.  Each segment holds
    at most 8192 boxes.  Without ``num_segments`` it is max(segment_ids) + 1, and the bound on
    the segment length is read back from the device (one synchronisation)."""
    n = scores.shape[0]
    dev = boxes.device
    seg = segment_ids.long()
    if num_segments is None:
        num_segments = int(seg.max()) + 1 if n else 0
    sizes = torch.bincount(seg, minlength=num_segments)[:num_segments]
    offsets = torch.zeros((num_segments + 1,), dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(sizes, 0)
    max_segment = int(sizes.max()) if num_segments and n else 0
    if max_segment > MAX_SEGMENT:
        raise ValueError(f'batched_nms_bev: a segment of {max_segment} boxes, built for '
                         f'<= {MAX_SEGMENT}')
    perm = torch.sort(seg, stable=True)[1]
    keep, count = _bev_nms(boxes.reshape(-1, 5)[perm], scores[perm], offsets, max_segment,
                           thresh, rotated)
    return compact_kept(perm, keep, count, offsets)


def compact_kept(rows, keep, count, offsets):
    """keep/count of ``nesie_bev_nms`` -> (kept ``rows`` segment after segment, count), both
    int64, on the device, without a synchronisation: the output keeps its full length n, the
    entries past sum(count) are -1."""
    n = keep.shape[0]
    count = count.long().clamp(min=0)
    if n == 0:
        return keep.long(), count
    last = count.numel() - 1
    pos = torch.arange(n, device=keep.device)
    seg = torch.searchsorted(offsets[1:].long(), pos, right=True).clamp(max=last)
    local = pos - offsets[:-1].long()[seg]
    live = local < count[seg]
    dest = (torch.cumsum(count, 0) - count)[seg] + local
    src = rows[keep.long().clamp(min=0, max=n - 1)]
    out = torch.full((n + 1,), -1, dtype=torch.long, device=keep.device)
    out.scatter_(0, torch.where(live, dest, torch.full_like(dest, n)), torch.where(live, src, -1))
    return out[:n], count
