"""VoteNet.aug_test (detectors/votenet.py:85-105) on the reduced model, Nesie and SAQE heads:
the batched forward of the views against simple_test per view, and the merged result against
a host referee of merge_aug_bboxes_3d applied to the per-view simple_test results."""
import torch
import pytest

from nesie_amd.tta import bbox3d_mapping_back, tta_views, xywhr2xyxyr
from nesie_amd.votenet import build_nesie_votenet
from nesie_amd.votenet.boxes import DepthInstance3DBoxes
from tests import _small
from tests._bev_referee import descending_order, referee_nms

pytestmark = pytest.mark.gpu

FLIPS = ((False, False), (True, False), (False, True))


def _model(head, device):
    cfg = _small.small_cfg()
    if head == 'SAQEHead':
        cfg['bbox_head'].update(
            angle_loss=dict(type='SmoothL1Loss', reduction='sum', loss_weight=10.0),
            angle_pred_loss=dict(type='MSELoss', reduction='sum', loss_weight=1.0))
        cfg['head_type'] = 'SAQEHead'
    torch.manual_seed(0)
    model = build_nesie_votenet(cfg).to(device)
    pts, _, _ = _small.small_batch(batch=2)
    model.train()
    model.bbox_head.jitter_noise = tuple(t.to(device) for t in _small.fixed_noise(2, 32))
    with torch.no_grad():
        model.bbox_head(model.extract_feat(pts.to(device)), 'vote')   # move the running stats
    model.eval()
    model.bbox_head.jitter_noise = None
    model.test_cfg['skip_jitter'] = True
    return model, pts[0].to(device)


@pytest.fixture(scope='module', params=['NesieHead', 'SAQEHead'])
def setup(request, hip_device):
    return _model(request.param, hip_device)


def referee_merge(oracle, per_view, metas, thr, rotated, max_num=None):
    """merge_aug_bboxes_3d on host results: map back, per-class greedy NMS with the referee
    IoU, class-major concatenation, descending stable score sort, max_num."""
    boxes = DepthInstance3DBoxes.cat([bbox3d_mapping_back(r['boxes_3d'], *(m[0][k] for k in (
        'pcd_scale_factor', 'pcd_horizontal_flip', 'pcd_vertical_flip'))) for r, m in zip(per_view, metas)])
    scores = torch.cat([r['scores_3d'] for r in per_view])
    labels = torch.cat([r['labels_3d'] for r in per_view])
    if len(labels) == 0:
        return boxes.tensor, scores, labels, float('inf')
    nms_boxes = xywhr2xyxyr(boxes.bev)
    picked, gap = [], float('inf')
    for c in range(int(labels.max()) + 1):
        inds = torch.nonzero(labels == c).view(-1)
        if len(inds) == 0:
            continue
        keep, g = referee_nms(oracle, nms_boxes[inds], scores[inds], thr, rotated)
        gap = min(gap, g)
        picked += [int(inds[k]) for k in keep]
    picked = torch.tensor(picked, dtype=torch.long)
    order = torch.from_numpy(descending_order(scores[picked]))
    if max_num is not None:
        order = order[:max_num]
    sel = picked[order]
    return boxes.tensor[sel], scores[sel], labels[sel], gap


def same(got, boxes, scores, labels):
    assert torch.equal(got['labels_3d'], labels)
    torch.testing.assert_close(got['scores_3d'], scores, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(got['boxes_3d'].tensor, boxes, rtol=1e-5, atol=1e-6)


def test_batched_views_equal_simple_test_per_view(setup):
    model, scene = setup
    views, metas = tta_views(scene, flips=FLIPS, scales=(1.0, 1.25))
    pts = torch.stack([v[0] for v in views])
    with torch.no_grad():
        x = model.extract_feat(pts)
        preds = model.bbox_head(x, model.test_cfg['sample_mod'])
        tensors = model.bbox_head.detect_tensors(pts, preds)
        batched = model.bbox_head.boxes_from_tensors(tuple(t.cpu() for t in tensors), None)
    for (bx, sc, lb), view, meta in zip(batched, views, metas):
        want = model.simple_test(view, meta)[0]
        assert len(lb) > 0
        same(want, bx.tensor, sc, lb)


@pytest.mark.parametrize("rotate,max_num", [(None, None), (True, 40), (False, None)])
def test_aug_test_equals_referee_merge(setup, oracle_kernels, rotate, max_num):
    model, scene = setup
    views, metas = tta_views(scene, flips=FLIPS)
    saved = dict(model.test_cfg)
    try:
        if rotate is not None:
            model.test_cfg['use_rotate_nms'] = rotate
        if max_num is not None:
            model.test_cfg['max_num'] = max_num
        for thr in (0.25, 0.2507, 0.31, 0.37):
            model.test_cfg['nms_thr'] = thr
            per_view = [model.simple_test(v, m)[0] for v, m in zip(views, metas)]
            want = referee_merge(oracle_kernels, per_view, metas, thr, rotate is not False, max_num)
            if want[3] > 1e-4:
                break
        else:
            pytest.fail('no threshold without a near-threshold pair')
        got = model.aug_test(views, metas)
        assert isinstance(got, list) and len(got) == 1
        assert not got[0]['scores_3d'].is_cuda
        assert len(want[2]) > 0
        if max_num is not None:
            assert len(want[2]) == max_num
        same(got[0], *want[:3])
    finally:
        model.test_cfg.clear()
        model.test_cfg.update(saved)


def test_aug_test_one_identity_view(setup, oracle_kernels):
    model, scene = setup
    views, metas = tta_views(scene, flips=((False, False),))
    thr = model.test_cfg['nms_thr']
    per_view = [model.simple_test(views[0], metas[0])[0]]
    want = referee_merge(oracle_kernels, per_view, metas, thr, True)
    assert want[3] > 1e-4
    same(model.aug_test(views, metas)[0], *want[:3])


def test_aug_test_nothing_selected(setup):
    model, scene = setup
    views, metas = tta_views(scene, flips=FLIPS)
    saved = model.test_cfg['score_thr']
    model.test_cfg['score_thr'] = 2.0
    try:
        got = model.aug_test(views, metas)[0]
    finally:
        model.test_cfg['score_thr'] = saved
    assert got['boxes_3d'].tensor.shape == (0, 7) and got['boxes_3d'].tensor.dtype == torch.float32
    assert got['scores_3d'].shape == (0,) and got['scores_3d'].dtype == torch.float32
    assert got['labels_3d'].shape == (0,) and got['labels_3d'].dtype == torch.int64
