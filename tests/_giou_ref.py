"""Referee of the enclosing-box losses (``nesie_giou3d_forward``): a torch restatement, in any float
dtype and differentiable by autograd, of ``cal_giou_3d`` / ``cal_diou_3d`` with the "smallest" and
"aligned" enclosing boxes.  The IoU chain is the oracle's (oracle/rotated_iou.py building blocks,
vertex order from the oracle's sort_vertices); the enclosing boxes are restated here:

  24 candidate lines, projection / distance ranges   rotated_iou/min_enclosing_box.py:26-172
  aligned box                                         rotated_iou/oriented_iou_loss.py:166-194
  GIoU / DIoU with z_range                            oriented_iou_loss.py:86-152

``cast_wh`` keeps the reference's ``w.float(), h.float()`` at the end of ``smallest_bounding_box``:
its float64 run rounds the two sides to float32 there, and so does the referee by default, which is
what lets it meet the recorded float64 results to 1e-10.
"""
import math

import torch

from oracle import rotated_iou as R

MODES = ('overlap', 'disjoint', 'yaw0', 'small_yaw', 'inside', 'identical', 'sizes')
ENCLOSING = ('smallest', 'aligned')
KINDS = ('giou', 'diou')

# candidate hull edges: corner pairs i < j of the 8 corners (0-3 first box, 4-7 second) except the
# two diagonals of either box, and for each the six corners that are not on the line
_DIAGONALS = {(0, 2), (1, 3), (4, 6), (5, 7)}
LINES = [(i, j) for i in range(8) for j in range(i + 1, 8) if (i, j) not in _DIAGONALS]
OTHERS = [[k for k in range(8) if k not in ij] for ij in LINES]
assert len(LINES) == 24


def _order(vertices, mask, num_valid):
    import oracle
    v = vertices.float().contiguous()
    idx = torch.empty(v.shape[0], v.shape[1], 9, dtype=torch.int32)
    oracle.OracleKernels().sort_vertices_forward(v, mask.contiguous(), num_valid.contiguous(), idx)
    return idx


def iou3d_verbose(box_a, box_b):
    """(B, N, 7) pairs -> iou3d, corners_a, corners_b (B, N, 4, 2), z_range, u3d."""
    ra = torch.cat([box_a[..., 0:2], box_a[..., 3:5], box_a[..., 6:7]], -1)
    rb = torch.cat([box_b[..., 0:2], box_b[..., 3:5], box_b[..., 6:7]], -1)
    ca, cb = R.bev_corners(ra), R.bev_corners(rb)
    inter2d = R.intersection_area(ca, cb, _order)
    union2d = ra[..., 2] * ra[..., 3] + rb[..., 2] * rb[..., 3] - inter2d
    iou2d = inter2d / union2d
    top_a, bot_a = box_a[..., 2] + box_a[..., 5] * 0.5, box_a[..., 2] - box_a[..., 5] * 0.5
    top_b, bot_b = box_b[..., 2] + box_b[..., 5] * 0.5, box_b[..., 2] - box_b[..., 5] * 0.5
    inter3d = iou2d * union2d * (torch.min(top_a, top_b) - torch.max(bot_a, bot_b)).clamp_min(0)
    u3d = box_a[..., 3] * box_a[..., 4] * box_a[..., 5] \
        + box_b[..., 3] * box_b[..., 4] * box_b[..., 5] - inter3d
    z_range = (torch.max(top_a, top_b) - torch.min(bot_a, bot_b)).clamp_min(0)
    return inter3d / u3d, ca, cb, z_range, u3d


def candidates(corners):
    """corners (..., 8, 2) -> per candidate line: projection range, distance range, area (with
    1e8 added where it is exactly 0), each (..., 24), and the line's direction angle (..., 24)."""
    li = torch.tensor([ij[0] for ij in LINES])
    lj = torch.tensor([ij[1] for ij in LINES])
    oth = torch.tensor(OTHERS)                                            # (24, 6)
    p1, p2 = corners[..., li, :], corners[..., lj, :]                     # (..., 24, 2)
    rest = corners[..., oth, :]                                           # (..., 24, 6, 2)
    every = torch.cat([p1.unsqueeze(-2), p2.unsqueeze(-2), rest], -2)     # (..., 24, 8, 2)
    x1, y1, x2, y2 = p1[..., 0:1], p1[..., 1:2], p2[..., 0:1], p2[..., 1:2]
    dx, dy = x2 - x1, y2 - y1
    slope = dy / (dx + 1e-8)
    length = torch.sqrt(1 + slope * slope)
    proj = (every[..., 0] + every[..., 1] * slope) / length
    w = proj.max(-1)[0] - proj.min(-1)[0]
    x, y = rest[..., 0], rest[..., 1]
    d = (dy * x - dx * y + x2 * y1 - y2 * x1) / torch.sqrt(dy * dy + dx * dx + 1e-14)
    h = torch.max(d.max(-1)[0] - d.min(-1)[0], d.abs().max(-1)[0])
    area = w * h
    area = area + 1e8 * (area == 0).to(area.dtype)
    return w, h, area, torch.atan2(dy, dx).squeeze(-1)


def smallest_box(corners, cast_wh=True):
    """-> w, h of the first candidate of minimal area, that area, its index."""
    w, h, area, _ = candidates(corners)
    best, idx = area.min(-1, keepdim=True)
    w, h = w.gather(-1, idx).squeeze(-1), h.gather(-1, idx).squeeze(-1)
    if cast_wh:
        w, h = w.float(), h.float()
    return w, h, best.squeeze(-1), idx.squeeze(-1)


def aligned_box(ca, cb):
    def span(a, b):
        hi = torch.max(a.max(-1)[0], b.max(-1)[0])
        lo = torch.min(a.min(-1)[0], b.min(-1)[0])
        return hi - lo
    return span(ca[..., 0], cb[..., 0]), span(ca[..., 1], cb[..., 1])


def enclosing_loss(kind, box_a, box_b, enclosing='smallest', cast_wh=True):
    """kind 'giou' | 'diou'; (B, N, 7) pairs -> (loss, iou3d), each (B, N)."""
    iou3d, ca, cb, z_range, u3d = iou3d_verbose(box_a, box_b)
    if enclosing == 'smallest':
        w, h = smallest_box(torch.cat([ca, cb], -2), cast_wh)[:2]
    else:
        w, h = aligned_box(ca, cb)
    if kind == 'giou':
        v_c = z_range * w * h
        return 1. - iou3d + (v_c - u3d) / v_c, iou3d
    off = box_a[..., :3] - box_b[..., :3]
    d2 = off[..., 0] * off[..., 0] + off[..., 1] * off[..., 1] + off[..., 2] * off[..., 2]
    c2 = w * w + h * h + z_range * z_range
    return 1. - iou3d + d2 / c2, iou3d


def loss_and_grad(kind, box_a, box_b, enclosing='smallest', dtype=torch.float64):
    """-> loss (N,), iou (N,), d loss.sum() / d box_a (N, 7), all in ``dtype`` on the CPU."""
    a = box_a.detach().cpu().reshape(1, -1, 7).to(dtype).requires_grad_(True)
    b = box_b.detach().cpu().reshape(1, -1, 7).to(dtype)
    loss, iou = enclosing_loss(kind, a, b, enclosing)
    (grad,) = torch.autograd.grad(loss.sum(), a)
    return loss.detach()[0], iou.detach()[0], grad[0]


def near_switch(box_a, box_b, rel=1e-4, angle=1e-3):
    """(N,) bool: pairs whose "smallest" winner is about to change direction.  In float64: the
    smallest area among the candidates whose direction differs from the winner's by more than
    ``angle`` rad (modulo pi/2) is within ``rel`` relative of the winner's.  Gradients of such a
    pair are not compared (the arg-min is piecewise constant: either side of the switch is right)."""
    a = box_a.detach().cpu().reshape(1, -1, 7).double()
    b = box_b.detach().cpu().reshape(1, -1, 7).double()
    _, ca, cb, _, _ = iou3d_verbose(a, b)
    _, _, area, direction = candidates(torch.cat([ca, cb], -2))
    best, idx = area.min(-1, keepdim=True)
    delta = torch.remainder(direction - direction.gather(-1, idx), math.pi / 2)
    delta = torch.min(delta, math.pi / 2 - delta)
    rival = torch.where(delta > angle, area, torch.full_like(area, float('inf'))).min(-1)[0]
    return ((rival - best.squeeze(-1)) <= rel * best.squeeze(-1))[0]
