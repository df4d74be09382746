"""Axis-aligned 3-D IoU / GIoU on the GPU: ``csrc/aa_iou3d.hip`` against the reference's recorded
results (tests/golden/aa_iou3d.npz), the shapes at which the launches can go wrong, the fixed-order
backward, the autograd op, graph capture, the loss modules and a head that trains with
``IoU3DLoss(with_yaw=False)``.

The bound (tests/_aa_iou.py ``bound``), per case, mode and form: 4 x the largest |float32 - float64|
of the reference's own results + 4 x 2^-24, the gradients' floor scaled by the largest float64
gradient entry of the case.  It is computed from the fixture at run time; every figure is printed
before it is asserted."""
import numpy as np
import pytest
import torch

from tests import _aa_iou as A
from tests import _small

pytestmark = pytest.mark.gpu

_cache = {}


def _backend(t):
    from nesie_amd.kernels import backend_for
    return backend_for(t)


def _paired(dev, a, b, mode, jac1=True, jac2=True, eps=1e-6):
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    n = a.shape[0]
    out = torch.full((n,), float('nan'), device=dev)
    j1 = torch.full((n, 6), float('nan'), device=dev) if jac1 else None
    j2 = torch.full((n, 6), float('nan'), device=dev) if jac2 else None
    _backend(a).aa_iou3d_paired_forward(a, b, A.MODES.index(mode), eps, out, j1, j2)
    return out, j1, j2


def _matrix(dev, a, b, mode, gout=None, grad1=True, grad2=True, eps=1e-6):
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    out = torch.full((a.shape[0], a.shape[1], b.shape[1]), float('nan'), device=dev)
    _backend(a).aa_iou3d_matrix_forward(a, b, A.MODES.index(mode), eps, out)
    if gout is None:
        return out, None, None
    g1 = torch.full(a.shape, float('nan'), device=dev) if grad1 else None
    g2 = torch.full(b.shape, float('nan'), device=dev) if grad2 else None
    _backend(a).aa_iou3d_matrix_backward(a, b, A.MODES.index(mode), eps,
                                         gout.to(dev).contiguous(), g1, g2)
    return out, g1, g2


def _case(case):
    z = A.golden()
    return torch.from_numpy(z[f'{case}/box1']), torch.from_numpy(z[f'{case}/box2'])


def _check(case, mode, form, got):
    """Print the figures of (out, grad1, grad2) against the recorded float64 results, then assert."""
    z = A.golden()
    lines, bad = [], []
    for what, g in zip(('out', 'grad1', 'grad2'), got):
        want = z[f'{case}/{mode}/{form}/f64/{what}']
        assert tuple(g.shape) == want.shape
        assert torch.isfinite(g).all()
        err = float(np.abs(g.cpu().double().numpy() - want).max())
        bound, ref = A.bound(case, mode, form, what)
        lines.append(f'{what} err {err:.3e} (reference {ref:.3e}, bound {bound:.3e})')
        if not err <= bound:
            bad.append((what, err, bound))
    print(f'{case:9s} {mode:4s} {form:7s}: ' + '  '.join(lines))
    assert not bad, (case, mode, form, bad)


@pytest.mark.parametrize('mode', A.MODES)
@pytest.mark.parametrize('case', A.PAIRED)
def test_paired_kernel_against_the_fixture(hip_device, case, mode):
    """Value and both Jacobians; 'identical' and 'touching' sit on the kinks of max, min and clamp,
    and their recorded gradients are autograd's choice there."""
    a, b = _case(case)
    _check(case, mode, 'aligned', _paired(hip_device, a, b, mode))


@pytest.mark.parametrize('mode', A.MODES)
@pytest.mark.parametrize('case', A.CASES)
def test_matrix_kernels_against_the_fixture(hip_device, case, mode):
    a, b = _case(case)
    gout = torch.from_numpy(A.golden()[f'{case}/gout'])
    if case != 'matrix':
        a, b, gout = a[None], b[None], gout[None]
    got = _matrix(hip_device, a, b, mode, gout)
    if case != 'matrix':
        got = tuple(g[0] for g in got)
    _check(case, mode, 'matrix', got)


def _pool():
    """Every paired case's boxes, one after the other: 168 pairs with the ties among them."""
    if 'pool' not in _cache:
        _cache['pool'] = (torch.cat([_case(c)[0] for c in A.PAIRED]),
                          torch.cat([_case(c)[1] for c in A.PAIRED]))
    return _cache['pool']


@pytest.mark.parametrize('mode', A.MODES)
def test_paired_sizes(hip_device, mode):
    """n around the 64 lanes of a wave, one pair, and several workgroups (256 pairs each): a pair's
    result does not depend on where it sits, so every size must reproduce the bits of the pool; a
    Jacobian that is not asked for changes no other output."""
    pa, pb = _pool()
    base = _paired(hip_device, pa, pb, mode)
    for n in (1, 63, 64, 65, 2048):
        idx = torch.arange(n) % pa.shape[0]
        got = _paired(hip_device, pa[idx], pb[idx], mode)
        for g, want in zip(got, base):
            assert torch.equal(g, want[idx.to(hip_device)]), n
        for jac1, jac2 in ((True, False), (False, True), (False, False)):
            part = _paired(hip_device, pa[idx], pb[idx], mode, jac1, jac2)
            assert torch.equal(part[0], got[0])
            assert part[1] is None if not jac1 else torch.equal(part[1], got[1])
            assert part[2] is None if not jac2 else torch.equal(part[2], got[2])


SHAPES = ((1, 1, 1), (2, 37, 53), (1, 64, 257), (3, 130, 5))


def _shape_case(shape):
    """Boxes of the pool laid out as (b, m, 6) x (b, n, 6), an upstream gradient, and the definition
    (the tensor-op form, which tests/test_aa_iou_cpu.py holds bit-equal to the reference) on them in
    float32 and float64 on the CPU: once per shape."""
    if shape not in _cache:
        from nesie_amd.mmdet3d_ops.axis_aligned_iou import _overlaps_torch
        b, m, n = shape
        pa, pb = _pool()
        g = torch.Generator().manual_seed(sum(shape))
        a = pa[torch.randint(0, pa.shape[0], (b * m,), generator=g)].view(b, m, 6)
        bx = pb[torch.randint(0, pb.shape[0], (b * n,), generator=g)].view(b, n, 6)
        gout = torch.rand(b, m, n, generator=g) * 3 - 1
        entry = dict(a=a, b=bx, gout=gout)
        for mode in A.MODES:
            res = {}
            for dtype in (torch.float32, torch.float64):
                p, q = (t.clone().to(dtype).requires_grad_(True) for t in (a, bx))
                out = _overlaps_torch(p, q, mode, False, 1e-6)
                g1, g2 = torch.autograd.grad((out * gout.to(dtype)).sum(), (p, q))
                res[dtype] = [t.detach().double() for t in (out, g1, g2)]
            entry[mode] = res
        _cache[shape] = entry
    return _cache[shape]


@pytest.mark.parametrize('mode', A.MODES)
@pytest.mark.parametrize('shape', SHAPES)
def test_matrix_shapes(hip_device, shape, mode):
    """Row and column tails of the forward tile (32 x 256), of the backward's 64-column groups and
    4-row groups, a column count above one LDS tile (257), one element, more than one batch entry.
    Forward: the bits of the paired kernel on the same pairs.  Backward: the fixture's rule with the
    definition's own float32 error on these inputs."""
    e = _shape_case(shape)
    b, m, n = shape
    out, g1, g2 = _matrix(hip_device, e['a'], e['b'], mode, e['gout'])
    pairs = _paired(hip_device, e['a'][:, :, None].expand(b, m, n, 6).reshape(-1, 6),
                    e['b'][:, None].expand(b, m, n, 6).reshape(-1, 6), mode, False, False)[0]
    assert torch.equal(out.view(-1), pairs)
    f32, f64 = e[mode][torch.float32], e[mode][torch.float64]
    scale = max(f64[1].abs().max().item(), f64[2].abs().max().item())
    bad = []
    for what, got, lo, hi in (('out', out, f32[0], f64[0]), ('grad1', g1, f32[1], f64[1]),
                              ('grad2', g2, f32[2], f64[2])):
        ref = (lo - hi).abs().max().item()
        bound = 4 * ref + A.FLOOR * (1.0 if what == 'out' else scale)
        err = (got.cpu().double() - hi).abs().max().item()
        print(f'{shape} {mode:4s} {what}: err {err:.3e} (definition in float32 {ref:.3e}, '
              f'bound {bound:.3e})')
        if not err <= bound:
            bad.append((what, err, bound))
    assert not bad, bad
    # a gradient that is not asked for changes nothing about the other
    only1 = _matrix(hip_device, e['a'], e['b'], mode, e['gout'], grad2=False)
    only2 = _matrix(hip_device, e['a'], e['b'], mode, e['gout'], grad1=False)
    assert only1[2] is None and only2[1] is None
    assert torch.equal(only1[1], g1) and torch.equal(only2[2], g2)


@pytest.mark.parametrize('mode', A.MODES)
def test_matrix_backward_is_bitwise_reproducible(hip_device, mode):
    for shape in ((2, 37, 53), (1, 64, 257)):
        e = _shape_case(shape)
        first = _matrix(hip_device, e['a'], e['b'], mode, e['gout'])
        second = _matrix(hip_device, e['a'], e['b'], mode, e['gout'])
        for x, y in zip(first, second):
            assert torch.equal(x, y)


@pytest.mark.parametrize('mode', A.MODES)
def test_autograd_op(hip_device, mode):
    from nesie_amd.mmdet3d_ops import AxisAlignedBboxOverlaps3D, axis_aligned_bbox_overlaps_3d
    pa, pb = _pool()
    pa, pb = pa[:160], pb[:160]
    k_out, k_j1, k_j2 = _paired(hip_device, pa, pb, mode)
    # aligned, with batch dimensions, both inputs differentiable
    p = pa.view(2, 4, 20, 6).to(hip_device).requires_grad_(True)
    q = pb.view(2, 4, 20, 6).to(hip_device).requires_grad_(True)
    out = axis_aligned_bbox_overlaps_3d(p, q, mode, is_aligned=True)
    assert out.shape == (2, 4, 20) and out.requires_grad
    assert torch.equal(out.detach().view(-1), k_out)
    scale = torch.linspace(-1, 2, 160, device=hip_device).view(2, 4, 20)
    (out * scale).sum().backward()
    assert torch.equal(p.grad.view(-1, 6), scale.view(-1, 1) * k_j1)
    assert torch.equal(q.grad.view(-1, 6), scale.view(-1, 1) * k_j2)
    # only the first input needs a gradient; none does
    p.grad = None
    axis_aligned_bbox_overlaps_3d(p, q.detach(), mode, is_aligned=True).sum().backward()
    assert torch.equal(p.grad.view(-1, 6), k_j1)
    with torch.no_grad():
        assert torch.equal(axis_aligned_bbox_overlaps_3d(p, q, mode, is_aligned=True), out.detach())
    # rows that start at an odd float of their storage, and strided rows, are copied first
    odd = torch.zeros(160 * 6 + 1, device=hip_device)
    odd[1:] = pa.to(hip_device).view(-1)
    assert odd[1:].data_ptr() % 8 == 4
    wide = torch.zeros(160, 7, device=hip_device)
    wide[:, :6] = pb.to(hip_device)
    assert torch.equal(axis_aligned_bbox_overlaps_3d(odd[1:].view(160, 6), wide[:, :6], mode,
                                                     is_aligned=True), k_out)
    # the matrix form through the calculator class, batch dimensions flattened and restored
    e = _shape_case((2, 37, 53))
    m_out, m_g1, m_g2 = _matrix(hip_device, e['a'], e['b'], mode, e['gout'])
    a = e['a'].view(2, 1, 37, 6).to(hip_device).requires_grad_(True)
    b = e['b'].view(2, 1, 53, 6).to(hip_device).requires_grad_(True)
    res = AxisAlignedBboxOverlaps3D()(a, b, mode)
    assert res.shape == (2, 1, 37, 53) and torch.equal(res.detach().view(2, 37, 53), m_out)
    (res * e['gout'].to(hip_device).view(2, 1, 37, 53)).sum().backward()
    assert torch.equal(a.grad.view(2, 37, 6), m_g1) and torch.equal(b.grad.view(2, 53, 6), m_g2)
    # float64 on the device is the tensor-op form: the recorded float64 results
    z = A.golden()
    a64, b64 = (t.double().to(hip_device) for t in _case('overlap'))
    got = axis_aligned_bbox_overlaps_3d(a64, b64, mode, is_aligned=True)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.cpu().numpy(), z[f'overlap/{mode}/aligned/f64/out'], rtol=0,
                               atol=1e-12)
    # empty inputs on the device
    assert tuple(axis_aligned_bbox_overlaps_3d(a64[:0], b64, mode).shape) == (0, 64)
    assert tuple(axis_aligned_bbox_overlaps_3d(pa[:0].to(hip_device), pb[:0].to(hip_device), mode,
                                               is_aligned=True).shape) == (0,)


def _capture_and_replay(hip_device, step, inputs, flipped):
    """``step(*tensors) -> outputs`` eagerly on ``inputs`` and on ``flipped``, then captured on
    static copies: two replays give the first, a replay after refilling the buffers the second."""
    eager = [t.clone() for t in step(*[t.clone().requires_grad_(True) for t in inputs])]
    other = [t.clone() for t in step(*[t.clone().requires_grad_(True) for t in flipped])]
    static = [t.clone().requires_grad_(True) for t in inputs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up off the default stream, as torch asks
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    for t in static:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got.detach(), want)
    with torch.no_grad():                            # the replay computes, it does not remember
        for t, new in zip(static, flipped):
            t.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, other):
        assert torch.equal(got.detach(), want)


@pytest.mark.parametrize('form', A.FORMS)
def test_graph_capture(hip_device, form):
    from nesie_amd.mmdet3d_ops import axis_aligned_bbox_overlaps_3d
    if form == 'aligned':
        a, b = (t.to(hip_device) for t in _case('overlap'))
        weight = None
    else:
        e = _shape_case((2, 37, 53))
        a, b, weight = e['a'].to(hip_device), e['b'].to(hip_device), e['gout'].to(hip_device)

    def step(p, q):
        p.grad = q.grad = None
        out = axis_aligned_bbox_overlaps_3d(p, q, 'giou', is_aligned=form == 'aligned')
        (out.sum() if weight is None else (out * weight).sum()).backward()
        return out.detach(), p.grad, q.grad

    _capture_and_replay(hip_device, step, (a, b), (a.flip(-2), b.flip(-2)))


@pytest.mark.parametrize('cls_name', ['IoU3DLoss', 'AxisAlignedIoULoss'])
def test_loss_modules(hip_device, cls_name):
    """On the device the modules are 1 - the paired kernel: against the recorded float64 IoU of
    'overlap', per element within the kernel's bound, sums scaled by their weights."""
    from nesie_amd.votenet import losses as L
    z = A.golden()
    a, b = _case('overlap')
    want = torch.from_numpy(1 - z['overlap/iou/aligned/f64/out'])
    bound = A.bound('overlap', 'iou', 'aligned', 'out')[0] + 2.0 ** -24     # + the rounding of 1 - x
    if cls_name == 'IoU3DLoss':       # centre + size + a heading that is ignored
        def to7(x):
            return torch.cat([(x[:, :3] + x[:, 3:]) / 2, x[:, 3:] - x[:, :3], torch.rand(64, 1)], -1)
        pred, target, extra = to7(a), to7(b), dict(with_yaw=False)
        bound += 4 * 2.0 ** -24       # the corners are rebuilt from centre and size in float32
    else:
        pred, target, extra = a, b, {}
    pred, target = pred.to(hip_device), target.to(hip_device)
    g = torch.Generator().manual_seed(5)
    w = torch.rand(64, generator=g)
    w[::4] = 0
    for weight in (None, w):
        ref = want if weight is None else torch.where(weight.double() > 0, want, torch.zeros_like(want))
        mass = 64.0 if weight is None else weight.double().sum().item()
        for reduction, avg_factor in (('none', None), ('sum', None), ('mean', None), ('mean', 17.0)):
            module = L.build_loss(dict(type=cls_name, reduction=reduction, loss_weight=3.0, **extra))
            got = module(pred, target, None if weight is None else weight.to(hip_device),
                         avg_factor=avg_factor)
            ref_r = 3.0 * L.weight_reduce_loss(ref, None if weight is None else weight.double(),
                                               reduction, avg_factor)
            scale = 3.0 * {'none': 1.0, 'sum': mass, 'mean': mass / (avg_factor or 64.0)}[reduction]
            err = (got.cpu().double() - ref_r).abs().max().item()
            print(f'{cls_name} weight {weight is not None} {reduction} avg {avg_factor}: err '
                  f'{err:.3e} bound {bound * max(scale, 1.0):.3e}')
            assert got.shape == ref_r.shape and err <= bound * max(scale, 1.0)
    # no weight is positive: zero, with a zero gradient
    p = pred.clone().requires_grad_(True)
    out = L.build_loss(dict(type=cls_name, reduction='sum', **extra))(
        p, target, torch.zeros(64, device=hip_device))
    out.backward()
    assert out.item() == 0 and (p.grad == 0).all()


# ---- a head that trains with the axis-aligned IoU loss ---------------------------------------------
AA_LOSS = dict(type='IoU3DLoss', with_yaw=False, reduction='sum', loss_weight=3.0)


def _head_model(hip_device, iou_loss, saqe=False, zero_heading=False):
    from nesie_amd.votenet import build_nesie_votenet
    cfg = _small.small_cfg()
    if saqe:
        from nesie_amd.votenet.detector import saqe_votenet_scannet_cfg
        scfg = saqe_votenet_scannet_cfg()
        cfg['bbox_head'].update(angle_loss=scfg['bbox_head']['angle_loss'],
                                angle_pred_loss=scfg['bbox_head']['angle_pred_loss'])
        cfg['head_type'] = 'SAQEHead'
    cfg['bbox_head']['iou_loss'] = dict(iou_loss)
    cfg['train_cfg'].update(pos_distance_thr=1.0, neg_distance_thr=1.5)     # positives at random init
    torch.manual_seed(0)
    model = build_nesie_votenet(cfg).to(hip_device).train()
    model.bbox_head.train_cfg = model.train_cfg
    if zero_heading:        # sin = 0, cos = 1 whatever the features: every proposal is upright
        conv = model.bbox_head.conv_pred.conv_heading
        with torch.no_grad():
            conv.weight.zero_()
            conv.bias.copy_(torch.tensor([0.0, 1.0]))
    return model


def _assert_same_step(want, got):
    """The comparison of tests/test_head_loss_gpu.py, fused against module by module."""
    assert list(got[0]) == list(want[0])
    for k in want[0]:
        assert want[0][k].abs().item() > 0, k
        torch.testing.assert_close(got[0][k], want[0][k], rtol=2e-5, atol=1e-6, msg=k)
    for k in want[1]:
        scale = want[1][k].abs().max().item()
        torch.testing.assert_close(got[1][k], want[1][k], rtol=1e-4,
                                   atol=2e-5 * max(scale, 1e-6), msg=k)
    flat_w = torch.cat([want[2][n].flatten() for n in sorted(want[2])]).double()
    flat_g = torch.cat([got[2][n].flatten() for n in sorted(want[2])]).double()
    assert ((flat_g - flat_w).norm() / flat_w.norm()).item() < 1e-4


def test_head_fused_loss_matches_the_module_by_module_loss(hip_device):
    """``loss`` and ``unsup_loss`` of a NesieHead with IoU3DLoss(with_yaw=False): the one-launch
    path is usable and agrees with the module-by-module evaluation.  The proposals keep the heading
    of a random initialisation, so the IoU the loss weighs (upright) and the IoU-quality label
    (rotated, as the reference computes it) are different numbers here."""
    from nesie_amd.votenet import head_loss
    from nesie_amd.votenet import losses as L
    from nesie_amd.votenet.nesie_head import GTBatch
    from tests.test_head_loss_gpu import _run, _run_unsup
    model = _head_model(hip_device, AA_LOSS)
    head = model.bbox_head
    assert isinstance(head.iou_loss, L.IoU3DLoss) and head.iou_loss.with_yaw is False
    assert head_loss.config_of(head) is not None and head_loss.unsup_config_of(head) is not None
    pts, boxes, labels = _small.small_batch(batch=3)
    pts = pts.to(hip_device)
    head.jitter_noise = tuple(t.to(hip_device) for t in _small.fixed_noise(3, 32))
    gt = GTBatch.collate(boxes, labels, hip_device)
    with torch.no_grad():
        preds = head(model.extract_feat(pts), 'vote')
        assert head_loss.usable(head, preds) and head_loss.usable(head, preds, unsup=True)
        assert (preds['bbox_preds'][..., 6].abs() > 0.1).any()
    weights = dict(vote_loss=1.0, objectness_loss=0.7, semantic_loss=1.3, center_loss=0.9,
                   surface_loss=1.1, iou_loss=0.8, iou_pred_loss=1.2, side_loss=0.6)
    _assert_same_step(_run(model, pts, gt, False, weights), _run(model, pts, gt, True, weights))
    # pseudo labels = the ground truth with seeded side qualities, one scene without any pseudo box
    boxes[1], labels[1] = boxes[1][:0], labels[1][:0]
    T = max(b.shape[0] for b in boxes)
    g = torch.Generator().manual_seed(11)
    quality = torch.zeros(3, max(T, 1), 6)
    for i, b in enumerate(boxes):
        quality[i, :b.shape[0]] = torch.rand(b.shape[0], 6, generator=g)
    quality = quality.to(hip_device)
    want = _run_unsup(model, pts, boxes, labels, quality, False)
    got = _run_unsup(model, pts, boxes, labels, quality, True)
    assert len(want[0]) == 4
    _assert_same_step(want, got)


def test_saqe_head_fused_loss_matches_the_module_by_module_loss(hip_device):
    """SAQEHead.loss with the axis-aligned IoU loss and headings that are alive: the fused path
    (nesie_head_loss_forward_label without uncertainties) against the module-by-module one."""
    from nesie_amd.votenet import head_loss
    from nesie_amd.votenet.nesie_head import GTBatch
    model = _head_model(hip_device, AA_LOSS, saqe=True)
    assert type(model.bbox_head).__name__ == 'SAQEHead'
    pts, boxes, labels = _small.small_batch(batch=3)
    for b in boxes:
        b[:, 6] = torch.linspace(-1.2, 1.4, b.shape[0])
    pts = pts.to(hip_device)
    gt = GTBatch.collate(boxes, labels, hip_device)
    model.bbox_head.jitter_noise = tuple(t.to(hip_device) for t in _small.fixed_noise(3, 32))
    weights = dict(vote_loss=1.0, objectness_loss=0.7, semantic_loss=1.3, center_loss=0.9,
                   surface_loss=1.1, iou_loss=0.8, iou_pred_loss=1.2, side_loss=0.6, angle_loss=1.4,
                   angle_pred_loss=0.5)
    keys = ('_cls_all', 'bbox_preds', 'surface_pred', '_side_all', '_iou_all', '_rot_all', '_robj_all')

    def run(fused):
        head_loss.ENABLED = fused
        try:
            for p in model.parameters():
                p.grad = None
            preds = model.bbox_head(model.extract_feat(pts), 'vote')
            keep = {}
            for k in keys:
                preds[k].retain_grad()
                keep[k] = preds[k]
            assert head_loss.saqe_usable(model.bbox_head, preds) == fused
            losses = model.bbox_head.loss(preds, pts, gt, None)
            sum(losses[k] * weights[k] for k in losses).backward()
            return ({k: v.detach().clone() for k, v in losses.items()},
                    {k: (v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v))
                     for k, v in keep.items()}, _small.grads_of(model))
        finally:
            head_loss.ENABLED = True
    _assert_same_step(run(False), run(True))


def test_upright_head_agrees_with_the_rotated_iou_head(hip_device):
    """With heading-0 proposals and targets the upright IoU is the rotated IoU: per proposal, and
    in ``iou_loss``, the two heads agree within the margin tests/test_giou_gpu.py allows the
    rotated kernel on its yaw-0 pairs (twice the reference chain's own float32 error there, from
    tests/golden/giou3d.npz, + 1e-6), weighted as the loss weighs the proposals."""
    import os
    from nesie_amd.votenet.nesie_head import GTBatch
    z = dict(np.load(os.path.join(os.path.dirname(A.GOLDEN), 'giou3d.npz')))
    key = 'yaw0/giou/smallest'
    margin = 2 * float(np.abs(z[f'{key}/f32/loss'].astype(np.float64) - z[f'{key}/f64/loss']).max()) \
        + 1e-6
    pts, boxes, labels = _small.small_batch(batch=2)
    for b in boxes:
        b[:, 6] = 0
    pts = pts.to(hip_device)
    gt = GTBatch.collate(boxes, labels, hip_device)
    seen = {}
    for name, cfg in (('upright', AA_LOSS),
                      ('rotated', dict(type='IoU3DLoss', reduction='sum', loss_weight=3.0))):
        model = _head_model(hip_device, cfg, zero_heading=True)
        head = model.bbox_head
        head.jitter_noise = tuple(t.to(hip_device) for t in _small.fixed_noise(2, 32))
        preds = head(model.extract_feat(pts), 'vote')
        assert (preds['bbox_preds'][..., 6] == 0).all()
        targets = head.get_targets(pts, gt, None, bbox_preds=preds)
        iou, _ = head._loss_iou(preds['bbox_preds'], targets[3])
        coef = 3.0 * torch.exp(-head._sigma(preds).mean(dim=-1)).reshape(-1) * targets[8].reshape(-1)
        losses = head.loss(preds, pts, gt, None)
        seen[name] = (iou.detach().double().cpu(), coef.detach().double().cpu(),
                      losses['iou_loss'].detach().double().item())
    (iou_u, coef_u, loss_u), (iou_r, coef_r, loss_r) = seen['upright'], seen['rotated']
    assert torch.equal(coef_u, coef_r) and (coef_u > 0).sum() >= 4 and (iou_r > 0).sum() >= 4
    err = (iou_u - iou_r).abs().max().item()
    bound = margin * coef_u.sum().item() + 4 * 2.0 ** -24 * abs(loss_r)     # + the sum's rounding
    print(f'upright vs rotated IoU: per proposal {err:.3e} (margin {margin:.3e}); iou_loss '
          f'{loss_u:.7f} vs {loss_r:.7f}, difference {abs(loss_u - loss_r):.3e} (bound {bound:.3e})')
    assert err <= margin
    assert abs(loss_u - loss_r) <= bound
