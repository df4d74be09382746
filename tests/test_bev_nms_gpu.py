"""BEV NMS (nms_gpu / nms_normal_gpu / boxes_iou_bev / batched_nms_bev) on the GPU against a
host referee: the CPU oracle's rotated overlaps, the reference's IoU formulas in float32 and a
python greedy walk (tests/_bev_referee.py)."""
import pytest
import torch

from nesie_amd.mmdet3d_ops import boxes_iou_bev, nms_gpu, nms_normal_gpu
from nesie_amd.mmdet3d_ops.iou3d import batched_nms_bev

from tests._bev_referee import iou_rows, pick_threshold, referee_nms

pytestmark = pytest.mark.gpu


def make_boxes(n, seed, clustered=False, ties=False, zero_area=False, density=2.0):
    g = torch.Generator().manual_seed(seed)
    if clustered:   # a few clusters of heavily overlapping boxes
        centres = torch.rand(max(n // 50, 1), 2, generator=g) * 10
        c = centres[torch.randint(len(centres), (n,), generator=g)] + \
            torch.randn(n, 2, generator=g) * 0.15
    else:           # spread so that each box meets a few others
        side = (n * 0.8 / density) ** 0.5 + 1.0
        c = torch.rand(n, 2, generator=g) * side
    h = 0.2 + torch.rand(n, 2, generator=g) * 0.8
    if zero_area:
        h[::7, 0] = 0.0
        h[3::11, 1] = 0.0
    yaw = (torch.rand(n, 1, generator=g) - 0.5) * 6.3
    boxes = torch.cat([c - h / 2, c + h / 2, yaw], 1).float()
    scores = torch.rand(n, generator=g)
    if ties:
        scores = torch.round(scores * 20) / 20
    return boxes, scores


CASES = [(1, {}), (63, {}), (64, {}), (65, {}), (1000, {}), (1000, dict(clustered=True)),
         (1000, dict(ties=True)), (1000, dict(zero_area=True)), (4096, {}), (8192, {})]


@pytest.mark.parametrize("rotated", [True, False])
@pytest.mark.parametrize("n,kw", CASES)
def test_nms_matches_referee(oracle_kernels, hip_device, n, kw, rotated):
    boxes, scores = make_boxes(n, seed=n + 7 * len(kw), **kw)
    thr, want = pick_threshold(oracle_kernels, boxes, scores, rotated)
    fn = nms_gpu if rotated else nms_normal_gpu
    got = fn(boxes.to(hip_device), scores.to(hip_device), thr)
    assert got.dtype == torch.long and got.is_cuda
    assert got.cpu().tolist() == want
    if n >= 64:
        assert 0 < len(want) < n     # something was suppressed, something kept


def test_nms_pre_and_post_maxsize(oracle_kernels, hip_device):
    boxes, scores = make_boxes(1000, seed=5, clustered=True)
    thr, _ = pick_threshold(oracle_kernels, boxes, scores, True)
    top = torch.sort(scores, descending=True, stable=True)[1][:300]
    sub_keep, _ = referee_nms(oracle_kernels, boxes[top], scores[top], thr, True)
    want = [int(top[i]) for i in sub_keep]
    d_boxes, d_scores = boxes.to(hip_device), scores.to(hip_device)
    assert nms_gpu(d_boxes, d_scores, thr, pre_maxsize=300).cpu().tolist() == want
    assert nms_gpu(d_boxes, d_scores, thr, pre_maxsize=300, post_max_size=10).cpu().tolist() == want[:10]
    full, _ = referee_nms(oracle_kernels, boxes, scores, thr, True)
    assert nms_gpu(d_boxes, d_scores, thr, post_max_size=25).cpu().tolist() == full[:25]


def test_nan_scores_go_last(oracle_kernels, hip_device):
    boxes, scores = make_boxes(200, seed=11)
    scores[::9] = float('nan')
    thr, want = pick_threshold(oracle_kernels, boxes, scores, True)
    assert nms_gpu(boxes.to(hip_device), scores.to(hip_device), thr).cpu().tolist() == want


def test_boxes_iou_bev_matches_referee(oracle_kernels, hip_device):
    a, _ = make_boxes(150, seed=3, clustered=True)
    b, _ = make_boxes(130, seed=4, clustered=True)
    b[0] = a[0]
    want = torch.stack([iou_rows(oracle_kernels, a[i], b, True) for i in range(len(a))])
    got = boxes_iou_bev(a.to(hip_device), b.to(hip_device))
    assert got.shape == (150, 130) and got.is_cuda
    assert (got.cpu() - want).abs().max().item() <= 1e-6
    assert want.max() > 0.5
    assert boxes_iou_bev(torch.zeros(0, 5, device=hip_device), b.to(hip_device)).shape == (0, 130)


@pytest.mark.parametrize("rotated", [True, False])
def test_batched_equals_single_calls(hip_device, rotated):
    boxes, scores = make_boxes(3000, seed=9, clustered=True)
    g = torch.Generator().manual_seed(1)
    seg = torch.randint(18, (3000,), generator=g)
    seg[seg == 5] = 6                                 # one empty segment
    d = [t.to(hip_device) for t in (boxes, scores, seg)]
    keep, count = batched_nms_bev(d[0], d[1], d[2], 0.25, rotated, num_segments=18)
    keep, count = keep.cpu(), count.cpu()
    assert count.shape == (18,) and int(count[5]) == 0
    fn = nms_gpu if rotated else nms_normal_gpu
    at = 0
    for s in range(18):
        idx = torch.nonzero(seg == s).view(-1)
        want = idx[fn(boxes[idx].to(hip_device), scores[idx].to(hip_device), 0.25).cpu()] \
            if len(idx) else torch.zeros(0, dtype=torch.long)
        assert keep[at:at + int(count[s])].tolist() == want.tolist()
        at += int(count[s])
    assert (keep[at:] == -1).all()


def test_too_many_boxes_is_an_invalid_argument(hip_device):
    from nesie_amd import _lib
    boxes, scores = make_boxes(8193, seed=2)
    with pytest.raises(RuntimeError, match=r"nesie_bev_nms failed \(status 1\)"):
        nms_gpu(boxes.to(hip_device), scores.to(hip_device), 0.25)
    assert b"8192" in _lib.load().nesie_last_error()


def test_empty_inputs(hip_device):
    z = torch.zeros(0, 5, device=hip_device)
    assert nms_gpu(z, torch.zeros(0, device=hip_device), 0.25).shape == (0,)
    assert nms_normal_gpu(z, torch.zeros(0, device=hip_device), 0.25).shape == (0,)
    keep, count = batched_nms_bev(z, torch.zeros(0, device=hip_device),
                                  torch.zeros(0, dtype=torch.long, device=hip_device), 0.25,
                                  num_segments=4)
    assert keep.shape == (0,) and count.cpu().tolist() == [0, 0, 0, 0]


def test_two_runs_are_bit_identical(hip_device):
    boxes, scores = make_boxes(8192, seed=21, ties=True)
    d_boxes, d_scores = boxes.to(hip_device), scores.to(hip_device)
    a = nms_gpu(d_boxes, d_scores, 0.3)
    b = nms_gpu(d_boxes, d_scores, 0.3)
    assert torch.equal(a, b)
