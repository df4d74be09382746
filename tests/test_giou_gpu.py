"""Rotated GIoU / DIoU 3-D losses on the GPU: ``nesie_giou3d_forward`` against the float64 referee
(tests/_giou_ref.py) within a bound taken from the reference's own float32 error as recorded in
tests/golden/giou3d.npz, the autograd op, the loss modules, graph capture and a head.

The bound, per input mode and per (kind, enclosing): twice the largest |float32 - float64| of the
reference's own results over the mode's pairs (for gradients: over the pairs that are not near a
switch of the winning direction, and over the 7 components), plus 1e-6.  The factor 2 allows for
a different but equally valid rounding order inside one expression.  It is computed from the
fixture at run time."""
import os

import numpy as np
import pytest
import torch

from tests import _giou_ref as G
from tests import _small

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'giou3d.npz')
SIZES = (1, 7, 8, 9, 257)        # around the eight pairs of a 64-thread workgroup, and a partial last one
_cache = {}


def _fixture():
    """The recorded pairs and results, the float64 referee on them and the switch set: once."""
    if not _cache:
        z = dict(np.load(GOLDEN))
        for mode in G.MODES:
            a, b = torch.from_numpy(z[f'{mode}/box1']), torch.from_numpy(z[f'{mode}/box2'])
            near = G.near_switch(a, b)
            if mode == 'identical':      # every direction of the box ties: values only
                near = torch.ones_like(near)
            entry = dict(box1=a, box2=b, compare_grad=~near)
            for kind in G.KINDS:
                for enc in G.ENCLOSING:
                    loss, iou, grad = G.loss_and_grad(kind, a, b, enc)
                    key = f'{mode}/{kind}/{enc}'
                    ref_v = np.abs(z[f'{key}/f32/loss'].astype(np.float64) - z[f'{key}/f64/loss'])
                    ref_g = np.abs(z[f'{key}/f32/grad'].astype(np.float64) - z[f'{key}/f64/grad'])
                    keep = (~near).numpy()
                    entry[kind, enc] = dict(
                        loss=loss, iou=iou, grad=grad,
                        ref_err_value=float(ref_v.max()),
                        ref_err_grad=float(ref_g[keep].max()) if keep.any() else 0.0)
            _cache[mode] = entry
    return _cache


def _launch(dev, a, b, kind, enc, want_iou=True, want_jac=True):
    from nesie_amd.kernels import backend_for
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    n = a.shape[0]
    loss = torch.full((n,), float('nan'), device=dev)
    iou = torch.full((n,), float('nan'), device=dev) if want_iou else None
    jac = torch.full((n, 7), float('nan'), device=dev) if want_jac else None
    backend_for(a).giou3d_forward(a, b, G.KINDS.index(kind), G.ENCLOSING.index(enc), loss, iou, jac)
    return loss, iou, jac


def _check_against_referee(dev, mode, kind, enc, index, what):
    """Launch on the fixture pairs ``index`` of ``mode``; print the figures, then assert."""
    e = _fixture()[mode]
    want = e[kind, enc]
    loss, iou, jac = _launch(dev, e['box1'][index], e['box2'][index], kind, enc)
    err_v = (loss.cpu().double() - want['loss'][index]).abs().max().item()
    err_i = (iou.cpu().double() - want['iou'][index]).abs().max().item()
    bound_v = 2 * want['ref_err_value'] + 1e-6
    keep = e['compare_grad'][index]
    err_g, bound_g = 0.0, 2 * want['ref_err_grad'] + 1e-6
    assert torch.isfinite(jac).all()
    if keep.any():
        err_g = (jac.cpu().double() - want['grad'][index])[keep].abs().max().item()
    print(f'{what} {mode:9s} {kind} {enc:8s} n={len(index):3d}: value err {err_v:.3e} (reference '
          f'{want["ref_err_value"]:.3e}, bound {bound_v:.3e})  grad err {err_g:.3e} (reference '
          f'{want["ref_err_grad"]:.3e}, bound {bound_g:.3e})  iou err {err_i:.3e}')
    assert err_v <= bound_v, (mode, kind, enc, err_v, bound_v)
    assert err_i <= bound_v, (mode, kind, enc, err_i, bound_v)
    assert err_g <= bound_g, (mode, kind, enc, err_g, bound_g)
    return loss, iou, jac


@pytest.mark.parametrize('enc', G.ENCLOSING)
@pytest.mark.parametrize('kind', G.KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_values_and_jacobian_against_the_float64_referee(hip_device, n, kind, enc):
    """Prefixes (n <= 9) and tilings (n = 257) of every mode's pairs.  The launcher takes the
    eight-threads-per-pair form whenever a Jacobian is asked for and the one-thread form
    otherwise, at every n: there is no size at which it switches."""
    for mode in G.MODES:
        count = _fixture()[mode]['box1'].shape[0]
        _check_against_referee(hip_device, mode, kind, enc, torch.arange(n) % count, 'referee')


@pytest.mark.parametrize('enc', G.ENCLOSING)
@pytest.mark.parametrize('kind', G.KINDS)
def test_null_jacobian_and_null_iou_return_the_same_loss_bits(hip_device, kind, enc):
    fx = _fixture()
    a = torch.cat([fx[m]['box1'] for m in G.MODES])
    b = torch.cat([fx[m]['box2'] for m in G.MODES])
    full = _launch(hip_device, a, b, kind, enc)
    no_jac = _launch(hip_device, a, b, kind, enc, want_jac=False)
    no_iou = _launch(hip_device, a, b, kind, enc, want_iou=False)
    neither = _launch(hip_device, a, b, kind, enc, want_iou=False, want_jac=False)
    for other in (no_jac, no_iou, neither):
        assert torch.equal(other[0], full[0])
    assert torch.equal(no_jac[1], full[1]) and torch.equal(no_iou[2], full[2])
    # and the IoU is the plain kernel's, bit for bit
    from nesie_amd.kernels import backend_for
    iou = torch.empty_like(full[0])
    jac = torch.empty_like(full[2])
    backend_for(iou).iou3d_forward(a.to(hip_device), b.to(hip_device), iou, jac)
    assert torch.equal(iou, full[1])
    backend_for(iou).iou3d_forward(a.to(hip_device), b.to(hip_device), iou, None)
    assert torch.equal(iou, full[1])


@pytest.mark.parametrize('enc', G.ENCLOSING)
@pytest.mark.parametrize('kind', G.KINDS)
def test_disjoint_pairs_get_a_gradient(hip_device, kind, enc):
    """What the feature exists for: the plain IoU has no gradient for a proposal that does not
    overlap its target, the enclosing-box losses pull it towards the target."""
    from nesie_amd.kernels import backend_for
    e = _fixture()['disjoint']
    a, b = e['box1'].to(hip_device), e['box2'].to(hip_device)
    iou, jac = torch.empty(64, device=hip_device), torch.empty(64, 7, device=hip_device)
    backend_for(a).iou3d_forward(a, b, iou, jac)
    assert (iou == 0).all() and (jac == 0).all()
    _, giou_iou, giou_jac = _check_against_referee(hip_device, 'disjoint', kind, enc,
                                                   torch.arange(64), 'disjoint')
    assert (giou_iou == 0).all()
    # the aligned box of GIoU does not change with x (y) while the target spans the prediction
    # there, so per pair the centre gradient is non-zero as a vector; otherwise in x and in y
    assert (giou_jac[:, :2] != 0).any(1).all()
    if (kind, enc) != ('giou', 'aligned'):
        assert (giou_jac[:, 0] != 0).all() and (giou_jac[:, 1] != 0).all()
    # a step against the gradient brings the centres closer (the recorded float64 gradients of
    # these pairs have this product >= 0.1)
    towards = ((b[:, :2] - a[:, :2]) * -giou_jac[:, :2]).sum(1)
    assert (towards > 0).all()


@pytest.mark.parametrize('fn_name', ['cal_giou_3d', 'cal_diou_3d'])
def test_autograd(hip_device, fn_name):
    from nesie_amd.mmdet3d_ops import rotated_iou
    from nesie_amd.mmdet3d_ops.rotated_iou import cal_iou_3d
    fn = getattr(rotated_iou, fn_name)
    kind = 'giou' if fn_name == 'cal_giou_3d' else 'diou'
    e = _fixture()['overlap']
    for enc in G.ENCLOSING:
        pred = e['box1'].view(2, 32, 7).to(hip_device).requires_grad_(True)
        target = e['box2'].view(2, 32, 7).to(hip_device)
        loss, iou = fn(pred, target, enc)
        assert loss.shape == (2, 32) and iou.shape == (2, 32)
        assert loss.requires_grad and not iou.requires_grad
        loss.sum().backward()
        k_loss, k_iou, k_jac = _launch(hip_device, e['box1'], e['box2'], kind, enc)
        assert torch.equal(loss.detach().view(-1), k_loss)
        assert torch.equal(pred.grad.view(-1, 7), k_jac)
        assert torch.equal(iou, cal_iou_3d(pred.detach(), target))
        # an upstream gradient scales the rows
        pred.grad = None
        scale = torch.linspace(-1, 2, 64, device=hip_device).view(2, 32)
        (fn(pred, target, enc)[0] * scale).sum().backward()
        assert torch.equal(pred.grad.view(-1, 7), scale.view(-1, 1) * k_jac)
        # without requires_grad no Jacobian is computed, the values are the same bits
        with torch.no_grad():
            assert torch.equal(fn(pred, target, enc)[0], loss.detach())
    with pytest.raises(RuntimeError, match='second box'):
        fn(pred, target.clone().requires_grad_(True))


@pytest.mark.parametrize('cls_name', ['GIoU3DLoss', 'DIoU3DLoss'])
def test_loss_modules(hip_device, cls_name):
    from nesie_amd.votenet import losses as L
    kind = 'giou' if cls_name == 'GIoU3DLoss' else 'diou'
    e = _fixture()['overlap']
    want = e[kind, 'smallest']
    bound = 2 * want['ref_err_value'] + 1e-6         # per element; sums scale with their weights
    pred, target = e['box1'].to(hip_device), e['box2'].to(hip_device)
    g = torch.Generator().manual_seed(5)
    w1 = torch.rand(64, generator=g)
    w1[::4] = 0
    w2 = torch.rand(64, 6, generator=g)
    w2[1::5] = 0
    for weight in (None, w1, w2):
        flat = weight if weight is None or weight.dim() == 1 else weight.mean(-1)
        ref = want['loss'] if flat is None else \
            torch.where(flat.double() > 0, want['loss'], torch.zeros_like(want['loss']))
        mass = 64.0 if flat is None else flat.double().abs().sum().item()
        for reduction, avg_factor in (('none', None), ('sum', None), ('mean', None),
                                      ('mean', 17.0), ('none', 17.0)):
            module = L.build_loss(dict(type=cls_name, reduction=reduction, loss_weight=3.0))
            got = module(pred, target, None if weight is None else weight.to(hip_device),
                         avg_factor=avg_factor)
            ref_r = 3.0 * L.weight_reduce_loss(ref, None if flat is None else flat.double(),
                                               reduction, avg_factor)
            assert got.shape == ref_r.shape
            scale = 3.0 * {'none': 1.0, 'sum': mass,
                           'mean': mass / (avg_factor or 64.0)}[reduction]
            err = (got.cpu().double() - ref_r).abs().max().item()
            print(f'{cls_name} weight {None if weight is None else tuple(weight.shape)} '
                  f'{reduction} avg {avg_factor}: err {err:.3e} bound {bound * max(scale, 1.0):.3e}')
            assert err <= bound * max(scale, 1.0)
    with pytest.raises(ValueError):
        L.build_loss(dict(type=cls_name, reduction='sum'))(pred, target, avg_factor=2.0)
    # no weight is positive: zero, with a zero gradient
    p = pred.clone().requires_grad_(True)
    out = L.build_loss(dict(type=cls_name, reduction='sum'))(p, target, torch.zeros(64, device=hip_device))
    out.backward()
    assert out.item() == 0 and (p.grad == 0).all()


def test_graph_capture(hip_device):
    from nesie_amd.mmdet3d_ops import cal_giou_3d
    e = _fixture()['small_yaw']
    a, b = e['box1'].to(hip_device), e['box2'].to(hip_device)

    def step(pred, target):
        pred.grad = None
        loss, iou = cal_giou_3d(pred[None], target[None])
        loss.sum().backward()
        return loss.detach(), iou, pred.grad

    eager_pred = a.clone().requires_grad_(True)
    eager = [t.clone() for t in step(eager_pred, b)]
    other = [t.clone() for t in step(eager_pred.detach().flip(0).requires_grad_(True), b.flip(0))]
    static_pred = a.clone().requires_grad_(True)
    static_target = b.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up off the default stream, as torch asks
        step(static_pred, static_target)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    static_pred.grad = None
    with torch.cuda.graph(graph):
        loss, iou = cal_giou_3d(static_pred[None], static_target[None])
        loss.sum().backward()
    outs = (loss, iou, static_pred.grad)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got.detach(), want)
    # new inputs in the captured buffers: the replay computes, it does not remember
    with torch.no_grad():
        static_pred.copy_(a.flip(0))
        static_target.copy_(b.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, other):
        assert torch.equal(got.detach(), want)


@pytest.mark.parametrize('head_type', ['NesieHead', 'SAQEHead'])
def test_head_trains_a_step_with_giou(hip_device, head_type):
    from nesie_amd.votenet import build_nesie_votenet, head_loss
    from nesie_amd.votenet import losses as L
    from nesie_amd.votenet.detector import saqe_votenet_scannet_cfg
    pts, boxes, labels = _small.small_batch(batch=2)
    pts = pts.to(hip_device)
    results = {}
    for loss_type in ('GIoU3DLoss', 'IoU3DLoss'):
        cfg = _small.small_cfg()
        if head_type == 'SAQEHead':
            scfg = saqe_votenet_scannet_cfg()
            cfg['bbox_head'].update(angle_loss=scfg['bbox_head']['angle_loss'],
                                    angle_pred_loss=scfg['bbox_head']['angle_pred_loss'])
            cfg['head_type'] = 'SAQEHead'
        cfg['bbox_head']['iou_loss'] = dict(type=loss_type, reduction='sum', loss_weight=3.0)
        cfg['train_cfg'].update(pos_distance_thr=1.0, neg_distance_thr=1.5)   # positives at random init
        torch.manual_seed(0)
        model = build_nesie_votenet(cfg).to(hip_device).train()
        head = model.bbox_head
        assert type(head).__name__ == head_type
        head.jitter_noise = tuple(t.to(hip_device) for t in _small.fixed_noise(2, 32))
        fused = head_loss.config_of(head) is not None
        assert fused == (loss_type == 'IoU3DLoss')                  # GIoU: module-by-module path
        assert (head_loss.unsup_config_of(head) is not None) == (loss_type == 'IoU3DLoss')
        assert isinstance(head.iou_loss, getattr(L, loss_type))
        losses, grads = _small.train_step_losses(model, pts, boxes, labels)
        for k, v in losses.items():
            assert torch.isfinite(v).all(), k
        for k, g in grads.items():
            assert torch.isfinite(g).all(), k
        assert grads and any(g.abs().max() > 0 for g in grads.values())
        results[loss_type] = losses
    assert set(results['GIoU3DLoss']) == set(results['IoU3DLoss'])
    giou, iou = results['GIoU3DLoss']['iou_loss'].item(), results['IoU3DLoss']['iou_loss'].item()
    print(f'{head_type}: iou_loss with GIoU3DLoss {giou:.6f}, with IoU3DLoss {iou:.6f}')
    assert giou > 0 and iou > 0 and giou != iou
    assert giou >= iou          # the enclosing-box term is never negative
