"""Test-time augmentation helpers on the host: bbox3d_mapping_back, xywhr2xyxyr, the box
methods they use and the views of tta_views, on hand-computed cases."""
import math

import torch

from nesie_amd.tta import bbox3d_mapping_back, tta_views, xywhr2xyxyr
from nesie_amd.votenet.boxes import DepthInstance3DBoxes


def boxes():
    return DepthInstance3DBoxes(torch.tensor([[1.0, 2.0, 0.5, 1.0, 2.0, 0.5, 0.3],
                                              [-0.5, 0.25, 0.0, 0.4, 0.2, 1.5, -1.2]]))


def test_horizontal_flip_maps_yaw_to_pi_minus_yaw():
    out = bbox3d_mapping_back(boxes(), 1.0, True, False)
    want = torch.tensor([[-1.0, 2.0, 0.5, 1.0, 2.0, 0.5, math.pi - 0.3],
                         [0.5, 0.25, 0.0, 0.4, 0.2, 1.5, math.pi + 1.2]])
    torch.testing.assert_close(out.tensor, want, rtol=0, atol=1e-6)


def test_vertical_flip_negates_y_and_yaw():
    out = bbox3d_mapping_back(boxes(), 1.0, False, True)
    want = torch.tensor([[1.0, -2.0, 0.5, 1.0, 2.0, 0.5, -0.3],
                         [-0.5, -0.25, 0.0, 0.4, 0.2, 1.5, 1.2]])
    assert torch.equal(out.tensor, want)


def test_flip_then_map_back_is_the_identity():
    for h, v in [(True, False), (False, True), (True, True)]:
        view = boxes().clone()
        if h:
            view.flip('horizontal')
        if v:
            view.flip('vertical')
        back = bbox3d_mapping_back(view, 1.0, h, v).tensor
        torch.testing.assert_close(back[:, :6], boxes().tensor[:, :6], rtol=0, atol=0)
        # both flips: the yaw comes back 2 pi lower (h then v applied again, as in the reference)
        turn = torch.remainder(back[:, 6] - boxes().tensor[:, 6] + math.pi, 2 * math.pi) - math.pi
        assert turn.abs().max() < 1e-6


def test_scale_round_trips():
    view = boxes().clone()
    view.scale(1.25)
    torch.testing.assert_close(view.tensor[0, :6], torch.tensor([1.25, 2.5, 0.625, 1.25, 2.5, 0.625]))
    assert view.tensor[0, 6] == boxes().tensor[0, 6]          # yaw is not scaled
    back = bbox3d_mapping_back(view, 1.25, False, False)
    torch.testing.assert_close(back.tensor, boxes().tensor, rtol=1e-6, atol=1e-7)


def test_mapping_back_leaves_its_input_alone():
    b = boxes()
    bbox3d_mapping_back(b, 2.0, True, True)
    assert torch.equal(b.tensor, boxes().tensor)


def test_cat_and_clone():
    a, b = boxes(), boxes()[1:]
    c = DepthInstance3DBoxes.cat([a, b])
    assert len(c) == 3 and torch.equal(c.tensor[2], b.tensor[0])
    c.tensor[0, 0] = 9.0
    assert a.tensor[0, 0] == 1.0
    assert len(DepthInstance3DBoxes.cat([])) == 0
    d = a.clone()
    d.tensor[0, 0] = 7.0
    assert a.tensor[0, 0] == 1.0


def test_xywhr2xyxyr():
    got = xywhr2xyxyr(torch.tensor([[1.0, 2.0, 4.0, 1.0, 0.5], [0.0, 0.0, 0.0, 2.0, -1.0]]))
    assert torch.equal(got, torch.tensor([[-1.0, 1.5, 3.0, 2.5, 0.5], [0.0, -1.0, 0.0, 1.0, -1.0]]))
    assert torch.equal(xywhr2xyxyr(boxes().bev)[:, 4], boxes().tensor[:, 6])


def test_tta_views():
    pts = torch.tensor([[1.0, 2.0, 3.0, 0.5], [-1.0, 0.5, 0.0, 0.1]])
    views, metas = tta_views(pts, flips=((False, False), (True, False), (False, True)),
                             scales=(1.0, 1.25))
    assert len(views) == len(metas) == 6
    assert all(len(v) == 1 and len(m) == 1 for v, m in zip(views, metas))
    assert [(m[0]['pcd_scale_factor'], m[0]['pcd_horizontal_flip'], m[0]['pcd_vertical_flip'])
            for m in metas] == [(1.0, False, False), (1.0, True, False), (1.0, False, True),
                                (1.25, False, False), (1.25, True, False), (1.25, False, True)]
    assert torch.equal(views[0][0], pts)
    assert torch.equal(views[1][0], torch.tensor([[-1.0, 2.0, 3.0, 0.5], [1.0, 0.5, 0.0, 0.1]]))
    assert torch.equal(views[2][0], torch.tensor([[1.0, -2.0, 3.0, 0.5], [-1.0, -0.5, 0.0, 0.1]]))
    assert torch.equal(views[4][0], torch.tensor([[-1.25, 2.5, 3.75, 0.5], [1.25, 0.625, 0.0, 0.1]]))
    assert torch.equal(pts, torch.tensor([[1.0, 2.0, 3.0, 0.5], [-1.0, 0.5, 0.0, 0.1]]))
