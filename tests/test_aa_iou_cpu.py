"""Axis-aligned 3-D IoU / GIoU, the tier that needs no GPU: the tensor-op form (the definition)
against the reference's recorded results (tests/golden/aa_iou3d.npz), autograd's rules on the ties,
shapes and empty inputs, the loss modules, the C entries' prototypes and argument checks, and the
package / loss-registry surface."""
import ctypes

import numpy as np
import pytest
import torch

from nesie_amd import _lib
from nesie_amd.mmdet3d_ops import AxisAlignedBboxOverlaps3D, axis_aligned_bbox_overlaps_3d
from tests import _aa_iou as A


def _run(case, mode, form, dtype):
    z = A.golden()
    a = torch.from_numpy(z[f'{case}/box1']).to(dtype).requires_grad_(True)
    b = torch.from_numpy(z[f'{case}/box2']).to(dtype).requires_grad_(True)
    out = axis_aligned_bbox_overlaps_3d(a, b, mode, is_aligned=form == 'aligned')
    w = torch.ones_like(out) if form == 'aligned' else torch.from_numpy(z[f'{case}/gout']).to(dtype)
    g1, g2 = torch.autograd.grad((out * w).sum(), (a, b))
    return out.detach().numpy(), g1.numpy(), g2.numpy()


@pytest.mark.parametrize('mode', A.MODES)
@pytest.mark.parametrize('case', A.CASES)
def test_torch_form_equals_the_recorded_reference(case, mode):
    """float64 to 1e-12 (relative to the largest entry), float32 bit for bit: the same operations
    in the same order on the same library."""
    z = A.golden()
    for form in A.forms_of(case):
        key = f'{case}/{mode}/{form}'
        got = _run(case, mode, form, torch.float64)
        for what, g in zip(('out', 'grad1', 'grad2'), got):
            want = z[f'{key}/f64/{what}']
            assert g.shape == want.shape and g.dtype == np.float64
            np.testing.assert_allclose(g, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()),
                                       err_msg=f'{key} {what}')
        got = _run(case, mode, form, torch.float32)
        for what, g in zip(('out', 'grad1', 'grad2'), got):
            want = z[f'{key}/f32/{what}']
            assert g.dtype == np.float32
            np.testing.assert_array_equal(g, want, err_msg=f'{key} {what}')


def test_recorded_cases_are_what_they_claim():
    z = A.golden()
    for case in A.PAIRED:
        assert z[f'{case}/box1'].shape == (A.COUNT[case], 6) == z[f'{case}/box2'].shape
        assert z[f'{case}/box1'].dtype == np.float32
        assert z[f'{case}/iou/matrix/f32/out'].shape == (A.COUNT[case],) * 2
    assert z['matrix/box1'].shape == (2, 37, 6) and z['matrix/box2'].shape == (2, 53, 6)
    assert z['matrix/giou/matrix/f64/out'].shape == (2, 37, 53)
    assert 'matrix/iou/aligned/f64/out' not in z
    iou = {c: z[f'{c}/iou/aligned/f64/out'] for c in A.PAIRED}
    assert (iou['overlap'] > 0.05).all() and (iou['overlap'] < 0.95).all()
    assert (iou['disjoint'] == 0).all() and (z['disjoint/giou/aligned/f64/out'] < 0).all()
    a, b = z['inside/box1'], z['inside/box2']
    assert (a[:, :3] > b[:, :3]).all() and (a[:, 3:] < b[:, 3:]).all()
    vol = lambda x: np.prod(x[:, 3:].astype(np.float64) - x[:, :3], axis=1)  # noqa: E731
    np.testing.assert_allclose(iou['inside'], vol(a) / vol(b), rtol=1e-12)
    assert np.array_equal(z['identical/box1'], z['identical/box2']) and (iou['identical'] == 1).all()
    a, b = z['touching/box1'], z['touching/box2']
    flush = (a[:, 3:] == b[:, :3]) | (a[:, :3] == b[:, 3:])        # bit-equal faces
    assert (flush.sum(1) == 1).all() and (iou['touching'] == 0).all()
    assert (z['touching/iou/aligned/f64/grad1'] != 0).any(1).all()   # the clamp passes at 0
    for i in (6, 7):        # and an extent shared bit for bit: ties in max and min on another axis
        other = (i % 3 + 1) % 3
        assert a[i, other] == b[i, other] and a[i, 3 + other] == b[i, 3 + other]
    # tiny: the union is below eps, so the IoU is overlap / eps
    a, b = z['tiny/box1'], z['tiny/box2']
    assert (vol(a) + vol(b) < 1e-7).all() and (iou['tiny'] > 0).all() and (iou['tiny'] < 2e-3).all()
    assert (z['matrix/iou/matrix/f64/out'] > 0).mean() > 0.05
    assert (z['matrix/iou/matrix/f64/out'] == 0).mean() > 0.05


@pytest.mark.parametrize('mode', A.MODES)
def test_autograd_rules_on_the_ties(mode):
    """clamp(x, 0) passes the gradient at x == 0; max / min of equal arguments give one half each."""
    from nesie_amd.votenet.losses import axis_aligned_iou_loss, centre_size_to_corners
    box = torch.tensor([[0.3, -0.2, 0.1, 1.0, 2.0, 1.5]], requires_grad=True)
    same = box.detach().clone().requires_grad_(True)
    out = axis_aligned_bbox_overlaps_3d(centre_size_to_corners(box), centre_size_to_corners(same),
                                        mode, is_aligned=True)
    assert out.item() == 1.0
    g1, g2 = torch.autograd.grad(out.sum(), (box, same))
    assert (g1 == 0).all() and (g2 == 0).all()
    if mode == 'giou':
        return
    pred = torch.tensor([[0.5, 0.5, 0.5, 1.0, 2.0, 1.5]], requires_grad=True)
    target = torch.tensor([[1.5, 0.5, 0.5, 1.0, 2.0, 1.5]])
    loss = axis_aligned_iou_loss(centre_size_to_corners(pred), centre_size_to_corners(target))
    assert loss.item() == 1.0
    (g,) = torch.autograd.grad(loss.sum(), pred)
    assert torch.equal(g, torch.tensor([[-0.5, 0.0, 0.0, -0.25, 0.0, 0.0]]))


def test_shapes_and_empty_inputs():
    f = axis_aligned_bbox_overlaps_3d
    a, b = torch.rand(3, 6), torch.rand(5, 6)
    a[:, 3:] += 1
    b[:, 3:] += 1
    assert f(a, b).shape == (3, 5) and f(a, a, is_aligned=True).shape == (3,)
    assert f(a.expand(2, 4, 3, 6), b.expand(2, 4, 5, 6)).shape == (2, 4, 3, 5)
    assert f(a.expand(2, 4, 3, 6), a.expand(2, 4, 3, 6), 'giou', True).shape == (2, 4, 3)
    # the matrix form is the aligned form of every pair
    full = f(a, b, 'giou')
    pairs = f(a[:, None].expand(3, 5, 6).reshape(-1, 6), b[None].expand(3, 5, 6).reshape(-1, 6),
              'giou', is_aligned=True)
    assert torch.equal(full.reshape(-1), pairs)
    empty = torch.empty(0, 6)
    assert tuple(f(empty, b).shape) == (0, 5) and tuple(f(a, empty).shape) == (3, 0)
    assert tuple(f(empty, empty).shape) == (0, 0)
    assert tuple(f(empty, empty, is_aligned=True).shape) == (0,)
    assert tuple(f(torch.empty(0, 4), b).shape) == (0, 5)             # empty: any last dimension
    assert tuple(f(torch.empty(2, 0, 6), b.expand(2, 5, 6)).shape) == (2, 0, 5)
    assert f(empty, b).dtype == torch.float32 and f(empty.double(), b.double()).dtype == torch.float64
    with pytest.raises(AssertionError, match='Unsupported mode'):
        f(a, b, 'iof')
    with pytest.raises(AssertionError):
        f(a[:, :5], b)
    with pytest.raises(AssertionError):
        f(a, b, is_aligned=True)                                       # rows != cols
    with pytest.raises(AssertionError):
        f(a.expand(2, 3, 6), b.expand(4, 5, 6))                        # batch dimensions differ
    calc = AxisAlignedBboxOverlaps3D()
    assert repr(calc) == 'AxisAlignedBboxOverlaps3D()'
    assert torch.equal(calc(a, b, 'giou'), full) and calc(a, a, is_aligned=True).shape == (3,)
    with pytest.raises(AssertionError):
        calc(empty[:, :4], b)                                          # the class insists on 6


def _reference_loss(pred, target, weight, reduction, avg_factor, loss_weight, transform):
    """1 - the recorded formula on corner boxes, then mmdet's weight_reduce_loss, in float64."""
    from nesie_amd.mmdet3d_ops.axis_aligned_iou import _overlaps_torch
    from nesie_amd.votenet.losses import centre_size_to_corners, weight_reduce_loss
    if transform:
        pred, target = centre_size_to_corners(pred), centre_size_to_corners(target)
    loss = 1 - _overlaps_torch(pred.double(), target.double(), 'iou', True, 1e-6)
    return loss_weight * weight_reduce_loss(loss, None if weight is None else weight.double(),
                                            reduction, avg_factor)


@pytest.mark.parametrize('cls_name', ['IoU3DLoss', 'AxisAlignedIoULoss'])
def test_loss_modules(cls_name):
    from nesie_amd.votenet import losses as L
    g = torch.Generator().manual_seed(3)
    centre = torch.rand(40, 3, generator=g) * 2
    size = 0.4 + torch.rand(40, 3, generator=g)
    target7 = torch.cat([centre, size, torch.zeros(40, 1)], -1)
    pred7 = torch.cat([centre + (torch.rand(40, 3, generator=g) - 0.5) * 0.5,
                       size * (0.7 + 0.6 * torch.rand(40, 3, generator=g)),
                       torch.rand(40, 1, generator=g)], -1)           # the heading is ignored
    transform = cls_name == 'IoU3DLoss'
    extra = dict(with_yaw=False) if transform else {}
    if transform:
        inputs = [(pred7, target7), (pred7[:, :6], target7[:, :6])]
    else:
        inputs = [(L.centre_size_to_corners(pred7), L.centre_size_to_corners(target7))]
    w = torch.rand(40, generator=g)
    w[::4] = 0
    for pred, target in inputs:
        for weight in (None, w, torch.zeros(40)):
            for reduction, avg_factor in (('none', None), ('sum', None), ('mean', None),
                                          ('mean', 17.0), ('none', 17.0)):
                module = L.build_loss(dict(type=cls_name, reduction=reduction, loss_weight=3.0,
                                           **extra))
                p = pred.clone().requires_grad_(True)
                got = module(p, target, weight, avg_factor=avg_factor)
                want = _reference_loss(pred, target, weight, reduction, avg_factor, 3.0, transform)
                assert got.shape == want.shape
                torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
                # a reduction given at call time wins
                other = L.build_loss(dict(type=cls_name, reduction='sum', **extra))
                torch.testing.assert_close(
                    3.0 * other(pred, target, weight, avg_factor=avg_factor,
                                reduction_override=reduction), got)
                if weight is not None and not (weight > 0).any():
                    # the reference's early-out: zero, with a zero gradient
                    got.sum().backward()
                    assert (got == 0).all() and (p.grad == 0).all()
    with pytest.raises(ValueError):
        L.build_loss(dict(type=cls_name, reduction='sum', **extra))(*inputs[0], avg_factor=2.0)
    if transform:       # a per-side weight is averaged first (iou3d_loss.py:58-59)
        module = L.build_loss(dict(type=cls_name, reduction='sum', **extra))
        w6 = torch.rand(40, 6, generator=g)
        torch.testing.assert_close(module(pred7, target7, w6), module(pred7, target7, w6.mean(-1)))


def test_build_loss_accepts_the_axis_aligned_losses():
    from nesie_amd.votenet import losses as L
    m = L.build_loss(dict(type='IoU3DLoss', with_yaw=False))
    assert isinstance(m, L.IoU3DLoss) and m.with_yaw is False
    assert (m.reduction, m.loss_weight) == ('mean', 1.0)
    assert L.build_loss(dict(type='IoU3DLoss')).with_yaw is True
    m = L.build_loss(dict(type='AxisAlignedIoULoss', reduction='sum', loss_weight=2.0))
    assert isinstance(m, L.AxisAlignedIoULoss) and (m.reduction, m.loss_weight) == ('sum', 2.0)
    with pytest.raises(AssertionError):
        L.AxisAlignedIoULoss(reduction='max')
    # the fused head-loss path takes an IoU3DLoss of either kind and still refuses the others
    from types import SimpleNamespace
    from nesie_amd.votenet import head_loss
    head = SimpleNamespace(
        alpha=1.0, semantic_loss=L.CrossEntropyLoss(reduction='sum'),
        center_loss=L.ChamferDistance(mode='l2', reduction='sum'),
        surface_loss=L.SurfaceLoss(reduction='sum'),
        iou_loss=L.build_loss(dict(type='IoU3DLoss', with_yaw=False, reduction='sum')))
    assert head_loss.unsup_config_of(head) is not None
    for other in ('GIoU3DLoss', 'DIoU3DLoss', 'AxisAlignedIoULoss'):   # the last takes corner boxes
        head.iou_loss = L.build_loss(dict(type=other))
        assert head_loss.unsup_config_of(head) is None


def test_names_are_exported():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import axis_aligned_iou
    for name in ('AxisAlignedBboxOverlaps3D', 'axis_aligned_bbox_overlaps_3d'):
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__
        assert getattr(mmdet3d_ops, name) is getattr(axis_aligned_iou, name)


def test_entries_are_declared():
    c = ctypes
    i, f, p = c.c_int, c.c_float, c.c_void_p
    assert _lib.SIGNATURES['nesie_aa_iou3d_paired_forward'] == (i, [i, p, p, i, f, p, p, p, p])
    assert _lib.SIGNATURES['nesie_aa_iou3d_matrix_forward'] == (i, [i, i, i, p, p, i, f, p, p])
    assert _lib.SIGNATURES['nesie_aa_iou3d_matrix_backward'] == (
        i, [i, i, i, p, p, i, f, p, p, p, p])


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    paired, forward, backward = (lib.nesie_aa_iou3d_paired_forward,
                                 lib.nesie_aa_iou3d_matrix_forward,
                                 lib.nesie_aa_iou3d_matrix_backward)
    eps = 1e-6
    for mode in (0, 1):
        # nothing to do: success, nothing touched (every pointer is null)
        assert paired(0, None, None, mode, eps, None, None, None, None) == 0
        for b, m, n in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (0, 0, 0)):
            assert forward(b, m, n, None, None, mode, eps, None, None) == 0
            assert backward(b, m, n, None, None, mode, eps, None, None, None, None) == 0
        # null pointers for a problem that is not empty are an argument error, not a crash
        assert paired(4, None, None, mode, eps, None, None, None, None) == 1
        assert b'aa_iou3d_paired_forward' in lib.nesie_last_error()
        assert forward(2, 3, 4, None, None, mode, eps, None, None) == 1
        assert b'aa_iou3d_matrix_forward' in lib.nesie_last_error()
        assert backward(2, 3, 4, None, None, mode, eps, None, None, None, None) == 1
        assert b'aa_iou3d_matrix_backward' in lib.nesie_last_error()
    for mode in (-1, 2):
        for n in (0, 4):
            assert paired(n, None, None, mode, eps, None, None, None, None) == 1
            assert b'aa_iou3d_paired_forward' in lib.nesie_last_error()
            assert forward(1, n, n, None, None, mode, eps, None, None) == 1
            assert backward(1, n, n, None, None, mode, eps, None, None, None, None) == 1
    assert paired(-1, None, None, 0, eps, None, None, None, None) == 1
    assert forward(1, -1, 4, None, None, 0, eps, None, None) == 1
    assert backward(-1, 3, 4, None, None, 0, eps, None, None, None, None) == 1
    # rows are read as 8-byte pairs: a pointer that is not 8-byte aligned is refused (host memory
    # stands in; the check comes before any launch)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    assert base % 8 == 0
    assert paired(2, base + 4, base + 64, 0, eps, base + 128, None, None, None) == 1
    assert b'aligned8' in lib.nesie_last_error()
    # the label variant of the head loss is declared with one pointer more than the sigma variant
    sigma = _lib.SIGNATURES['nesie_head_loss_forward_sigma'][1]
    label = _lib.SIGNATURES['nesie_head_loss_forward_label'][1]
    assert len(label) == len(sigma) + 1 and label[11:14] == [ctypes.c_void_p] * 3
