"""Rotated GIoU / DIoU 3-D losses, the tier that needs no GPU: the referee against the reference's
recorded results (tests/golden/giou3d.npz), the tie cap of the fixture, the C entry's prototype and
argument checks, and the package / loss-registry surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

from nesie_amd import _lib
from tests import _giou_ref as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'giou3d.npz')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


def _pairs(golden, mode):
    return torch.from_numpy(golden[f'{mode}/box1']), torch.from_numpy(golden[f'{mode}/box2'])


@pytest.mark.parametrize('mode', G.MODES)
def test_referee_equals_the_recorded_float64_results(golden, mode):
    a, b = _pairs(golden, mode)
    assert a.shape == ((8, 7) if mode == 'identical' else (64, 7))
    for kind in G.KINDS:
        for enc in G.ENCLOSING:
            loss, iou, grad = G.loss_and_grad(kind, a, b, enc)
            key = f'{mode}/{kind}/{enc}/f64'
            np.testing.assert_allclose(loss.numpy(), golden[f'{key}/loss'], rtol=0, atol=1e-10)
            np.testing.assert_allclose(iou.numpy(), golden[f'{key}/iou'], rtol=0, atol=1e-10)
            assert torch.isfinite(grad).all()
    # the same winner wherever the recorded best two areas are apart
    _, ca, cb, _, _ = G.iou3d_verbose(a[None].double(), b[None].double())
    idx = G.smallest_box(torch.cat([ca, cb], -2))[3][0].numpy()
    best_two = golden[f'{mode}/best_two']
    clear = best_two[:, 1] - best_two[:, 0] > 1e-9 * best_two[:, 0]
    assert (idx[clear] == golden[f'{mode}/winner'][clear]).all()


def test_recorded_modes_are_what_they_claim(golden):
    a, b = _pairs(golden, 'disjoint')
    reach = 0.5 * (torch.hypot(a[:, 3], a[:, 4]) + torch.hypot(b[:, 3], b[:, 4]))
    assert ((a[:, :2] - b[:, :2]).norm(dim=1) > reach).all()
    assert (golden['disjoint/giou/smallest/f64/iou'] == 0).all()
    for mode in ('yaw0', 'small_yaw'):
        a, b = _pairs(golden, mode)
        assert (b[:, 6] == 0).all()
        assert (a[:, 6] == 0).all() if mode == 'yaw0' else (a[:, 6].abs() < 0.05).all()
    a, b = _pairs(golden, 'inside')
    vol = (a[:, 3] * a[:, 4] * a[:, 5] / (b[:, 3] * b[:, 4] * b[:, 5])).double().numpy()
    np.testing.assert_allclose(golden['inside/giou/aligned/f64/iou'], vol, rtol=1e-6)
    a, b = _pairs(golden, 'identical')
    assert torch.equal(a, b)
    for kind in G.KINDS:        # identical boxes: IoU 1, enclosing box = the box, loss 0
        np.testing.assert_allclose(golden[f'identical/{kind}/smallest/f64/loss'], 0, atol=1e-6)
    a, b = _pairs(golden, 'sizes')
    sizes = torch.cat([a[:, 3:6], b[:, 3:6]])
    assert sizes.min() >= 0.05 and sizes.max() <= 5.0 and sizes.min() < 0.1 and sizes.max() > 2.5


@pytest.mark.parametrize('mode', [m for m in G.MODES if m != 'identical'])
def test_tie_cap(golden, mode):
    """At most 5 % of a mode's pairs may sit near a switch of the winning direction (their
    gradients are left out of every comparison); 'identical' ties by construction and is compared
    on values only."""
    a, b = _pairs(golden, mode)
    near = G.near_switch(a, b)
    assert near.shape == (64,) and near.sum().item() <= 0.05 * 64


def test_near_switch_sees_a_switch():
    a = torch.tensor([[0., 0., 0., 1., 1., 1., 0.]])
    b = torch.tensor([[0.2, 0.1, 0., 1., 1., 1., 0.3]])
    assert not G.near_switch(a, b).item()
    # a square and its copy turned by 45 degrees about the same centre: the 8 corners are a
    # regular octagon, whose hull edges run in two directions 45 degrees apart (modulo 90) and
    # give the same area
    b = torch.tensor([[0., 0., 0., 1., 1., 1., 0.7853981633974483]])
    assert G.near_switch(a, b).item()
    # same-direction rivals do not count: two axis-aligned boxes tie along all eight edges
    b = torch.tensor([[0.3, 0.2, 0., 1., 2., 1., 0.]])
    assert not G.near_switch(a, b).item()


def test_entry_is_declared():
    c = ctypes
    assert _lib.SIGNATURES['nesie_giou3d_forward'] == (
        c.c_int, [c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p,
                  c.c_void_p, c.c_void_p])


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    null = (None,) * 3
    for kind in (0, 1):
        for enc in (0, 1):
            assert lib.nesie_giou3d_forward(0, None, None, kind, enc, *null, None) == 0
            # null pointers for a problem that is not empty are an argument error, not a crash
            assert lib.nesie_giou3d_forward(4, None, None, kind, enc, *null, None) == 1
            assert b'giou3d_forward' in lib.nesie_last_error()
    for n, kind, enc in ((-1, 0, 0), (4, 2, 0), (4, -1, 0), (4, 0, 2), (4, 0, -1), (0, 2, 0),
                         (0, 0, 2)):
        assert lib.nesie_giou3d_forward(n, None, None, kind, enc, *null, None) == 1, (n, kind, enc)
        assert b'giou3d_forward' in lib.nesie_last_error()
    # the plain IoU entry keeps its contract
    assert lib.nesie_iou3d_forward(0, None, None, None, None, None) == 0
    assert lib.nesie_iou3d_forward(4, None, None, None, None, None) == 1


def test_cal_giou_3d_is_the_real_op():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import cal_giou_3d
    from nesie_amd.mmdet3d_ops import rotated_iou
    assert 'cal_giou_3d' in mmdet3d_ops._HOT and 'cal_giou_3d' not in mmdet3d_ops._OUT_OF_SCOPE
    assert 'cal_giou_3d' in mmdet3d_ops.__all__
    assert cal_giou_3d is rotated_iou.cal_giou_3d
    # the reference's ops/__init__.py exports cal_giou_3d only; cal_diou_3d lives in the module
    assert 'cal_diou_3d' not in mmdet3d_ops.__all__ and callable(rotated_iou.cal_diou_3d)
    boxes = torch.rand(1, 4, 7) + 0.5
    for fn in (rotated_iou.cal_giou_3d, rotated_iou.cal_diou_3d):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(boxes, boxes)
        with pytest.raises(NotImplementedError, match='eigenvector_22'):
            fn(boxes, boxes, 'pca')
        with pytest.raises(ValueError, match='enclosing_type'):
            fn(boxes, boxes, 'convex')
    # the other names keep their stubs
    with pytest.raises(NotImplementedError):
        mmdet3d_ops.assign_score_withk()


def test_no_cpu_fallback_behind_an_injected_back_end(oracle_kernels):
    from nesie_amd import kernels
    from nesie_amd.mmdet3d_ops.rotated_iou import cal_diou_3d, cal_giou_3d
    boxes = torch.rand(1, 4, 7) + 0.5
    with kernels.use_backend(oracle_kernels):
        for fn in (cal_giou_3d, cal_diou_3d):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                fn(boxes, boxes)


def test_loss_modules_build_and_stay_off_the_fused_head_loss():
    from nesie_amd.votenet import losses as L
    giou = L.build_loss(dict(type='GIoU3DLoss'))
    diou = L.build_loss(dict(type='DIoU3DLoss'))
    assert (giou.reduction, giou.loss_weight, giou.enclosing_type) == ('mean', 1.0, 'smallest')
    assert (diou.reduction, diou.loss_weight, diou.enclosing_type) == ('mean', 1.0, 'smallest')
    built = L.build_loss(dict(type='GIoU3DLoss', reduction='sum', loss_weight=3.0,
                              enclosing_type='aligned'))
    assert (built.reduction, built.loss_weight, built.enclosing_type) == ('sum', 3.0, 'aligned')
    assert isinstance(giou, L.GIoU3DLoss) and isinstance(diou, L.DIoU3DLoss)
    for m in (giou, diou):
        assert not isinstance(m, L.IoU3DLoss)
    # the predicate of the fused head-loss path refuses a head that carries one of them
    from types import SimpleNamespace
    from nesie_amd.votenet import head_loss
    plain = L.build_loss(dict(type='IoU3DLoss', reduction='sum', loss_weight=3.0))
    head = SimpleNamespace(
        alpha=1.0, semantic_loss=L.CrossEntropyLoss(reduction='sum'),
        center_loss=L.ChamferDistance(mode='l2', reduction='sum'),
        surface_loss=L.SurfaceLoss(reduction='sum'), iou_loss=plain)
    assert head_loss.unsup_config_of(head) is not None
    for m in (giou, diou):
        head.iou_loss = m
        assert head_loss.unsup_config_of(head) is None
