"""Sigmoid focal loss on the device against the float64 referee (``tests/_focal_ref.py`` derives the
bound: no element excused, (16 + 8 gamma softplus(z)) u relative plus 2^-126; a reduced scalar the
sum of its elements' bounds plus gamma_{m+3} S)."""
import functools
import itertools

import pytest
import torch

from tests import _focal_head as H
from tests import _focal_ref as R
from tests import _small

pytestmark = pytest.mark.gpu

GAMMAS = (0, 0.5, 2, 5)
ALPHAS = (0.25, 0.5)
SCALES = (3, 30)
# the reduction cuts the flat index into chunks of 4096 elements: one chunk (one launch), an odd
# element count below and above one chunk, and 74 chunks with a ragged last one of 882 elements
SHAPES = [(1, 1), (3, 2), (64, 1), (257, 19), (1000, 3), (4099, 10), (29989, 10)]


@functools.lru_cache(maxsize=None)
def inputs(n, c, scale, limit=None):
    """``limit=104`` for every test of a SUM: see ``R.case``."""
    x, t = R.case(n, c, scale, seed=n * 31 + c, limit=limit)
    g = torch.Generator().manual_seed(n + c)
    # weights in (0.25, 1]: 3e38 times a weight above 1 would leave float32
    return dict(x=x, t=t, cw=torch.rand(c, generator=g) * 0.75 + 0.25,
                sw_row=torch.rand(n, generator=g) * 0.75 + 0.25,
                sw_elem=torch.rand(n, c, generator=g) * 0.75 + 0.25,
                up=torch.randn(n, c, generator=g))


@functools.lru_cache(maxsize=None)
def referee(n, c, scale, gamma, alpha, limit=None):
    i = inputs(n, c, scale, limit)
    return R.reference(i['x'], i['t'], gamma, alpha)


def nan_like(*shape, device):
    return torch.full(shape, float('nan'), device=device)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_kernel_values_against_float64(hip_device, shape):
    from nesie_amd.kernels import backend_for
    n, c = shape
    worst = {g: 0.0 for g in GAMMAS}
    for scale in SCALES:
        host = inputs(n, c, scale)
        dev = {k: v.to(hip_device) for k, v in host.items()}
        hip = backend_for(dev['x'])
        # the terms at -3e38 and 3e38 add up to 3e38: every scale stays below 1
        quarter = torch.tensor([0.25], device=hip_device)
        for gamma, alpha in itertools.product(GAMMAS, ALPHAS):
            loss64, grad64, sp = referee(n, c, scale, gamma, alpha)
            for cw, sw in itertools.product((None, 'cw'), (None, 'sw_row', 'sw_elem')):
                what = f'{shape} scale {scale} gamma {gamma} alpha {alpha} {cw} {sw}'
                f = R.factor(host['t'], n, c, cw and host[cw], sw and host[sw])
                cwd, swd = cw and dev[cw], sw and dev[sw]
                loss = nan_like(n, c, device=hip_device)
                hip.sigmoid_focal_loss_forward(dev['x'], dev['t'], cwd, loss, gamma, alpha, swd, 0.5)
                total = nan_like(1, device=hip_device)
                hip.sigmoid_focal_loss_forward_sum(dev['x'], dev['t'], cwd, total, gamma, alpha, swd,
                                                   0.5, quarter)
                g_elem, g_scalar = nan_like(n, c, device=hip_device), nan_like(n, c, device=hip_device)
                hip.sigmoid_focal_loss_backward(dev['x'], dev['t'], cwd, g_elem, gamma, alpha, swd,
                                                grad_output=dev['up'], scale=0.5)
                hip.sigmoid_focal_loss_backward(dev['x'], dev['t'], cwd, g_scalar, gamma, alpha, swd,
                                                grad_scalar=quarter, scale=0.5, scale_dev=quarter)
                ratios = (
                    R.check(loss, loss64 * f * 0.5, sp, gamma, what + ' loss'),
                    R.check(g_elem, grad64 * f * host['up'].double() * 0.5, sp, gamma,
                            what + ' grad (elementwise upstream)'),
                    R.check(g_scalar, grad64 * f * 0.03125, sp, gamma, what + ' grad (scalar upstream)'))
                R.check_sum(total[0], loss64 * f * 0.125, sp, gamma, what + ' sum')
                worst[gamma] = max(worst[gamma], *ratios)
    print(f'focal worst error / bound at {shape}: '
          + ', '.join(f'gamma {g}: {r:.3f}' for g, r in worst.items()))


# 11, 74 and 289 partials, each with a ragged last chunk; 289 gives the finish's threads two
# partials each (0 .. 32) or one
SUM_SHAPES = [(4099, 10), (29989, 10), (131101, 9)]


@pytest.mark.parametrize('shape', SUM_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_multi_chunk_sums_against_float64(hip_device, shape):
    """The reduced scalar on inputs clamped to |x| <= 104, held to the bound of the kernel's own
    tree (``R.device_sum_depth``): gamma_{depth+3} S is a few 1e-6 of S, a lost element of a
    hundred-thousandth of the sum would show, a lost chunk or partial by orders of magnitude."""
    from nesie_amd.kernels import backend_for
    from nesie_amd.votenet.losses import FocalLoss
    n, c = shape
    depth = R.device_sum_depth(n * c)
    assert depth == 23 + 8 + (2 if n * c > 256 * R.CHUNK else 1)
    worst = 0.0
    for scale, gamma in itertools.product(SCALES, (0.5, 2)):
        host = inputs(n, c, scale, 104)
        x, t, cw, sw = (host[k].to(hip_device) for k in ('x', 't', 'cw', 'sw_row'))
        hip = backend_for(x)
        loss64, _, sp = referee(n, c, scale, gamma, 0.25, 104)
        weighted = loss64 * R.factor(host['t'], n, c, host['cw'], host['sw_row'])
        what = f'{shape} scale {scale} gamma {gamma}'
        total = nan_like(1, device=hip_device)
        hip.sigmoid_focal_loss_forward_sum(x, t, None, total, gamma, 0.25)
        worst = max(worst, R.check_sum(total[0], loss64, sp, gamma, what + ' sum', depth))
        total = nan_like(1, device=hip_device)
        hip.sigmoid_focal_loss_forward_sum(x, t, cw, total, gamma, 0.25, sw, 0.5)
        worst = max(worst, R.check_sum(total[0], 0.5 * weighted, sp, gamma, what + ' weighted sum',
                                       depth))
        plain = loss64 * R.factor(host['t'], n, c, None, host['sw_row'])
        out = FocalLoss(gamma=gamma, reduction='sum', loss_weight=2.0)(x, t, sw)
        worst = max(worst, R.check_sum(out, 2.0 * plain, sp, gamma, what + ' FocalLoss sum', depth))
        out = FocalLoss(gamma=gamma, reduction='mean')(x, t, sw)
        worst = max(worst, R.check_sum(out, plain / (n * c), sp, gamma, what + ' FocalLoss mean',
                                       depth))
    print(f'focal sums at {shape}: worst error / bound {worst:.3f}')


def test_unaligned_base_takes_the_scalar_lanes_and_gives_the_same_bits(hip_device):
    from nesie_amd.kernels import backend_for
    n, c = 4099, 10
    host = inputs(n, c, 3)
    x, t = host['x'].to(hip_device), host['t'].to(hip_device)
    shifted = torch.empty(n * c + 1, device=hip_device)[1:].view(n, c).copy_(x)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    hip = backend_for(x)
    got = []
    for pred in (x, shifted):
        loss, total, grad = (nan_like(n, c, device=hip_device), nan_like(1, device=hip_device),
                             nan_like(n, c, device=hip_device))
        hip.sigmoid_focal_loss_forward(pred, t, None, loss, 2.0, 0.25)
        hip.sigmoid_focal_loss_forward_sum(pred, t, None, total, 2.0, 0.25)
        hip.sigmoid_focal_loss_backward(pred, t, None, grad, 2.0, 0.25, grad_scalar=total)
        got.append((loss, total, grad))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    loss64, _, sp = referee(n, c, 3, 2.0, 0.25)
    R.check(got[1][0], loss64, sp, 2.0)


@pytest.mark.parametrize('weighted', [False, True])
def test_function_equals_the_back_end_bit_for_bit(hip_device, weighted):
    from nesie_amd.kernels import backend_for
    from nesie_amd.mmdet3d_ops import SigmoidFocalLoss, sigmoid_focal_loss
    n, c = 4099, 10
    host = inputs(n, c, 3, 104)
    x, t = host['x'].to(hip_device), host['t'].to(hip_device)
    cw = host['cw'].to(hip_device) if weighted else None
    up = host['up'].to(hip_device)
    hip = backend_for(x)
    for reduction, scale in (('none', 1.0), ('sum', 1.0), ('mean', 1.0 / n)):
        leaf = x.clone().requires_grad_(True)
        out = sigmoid_focal_loss(leaf, t, 1.5, 0.4, cw, reduction)
        want_grad = nan_like(n, c, device=hip_device)
        if reduction == 'none':
            want = nan_like(n, c, device=hip_device)
            hip.sigmoid_focal_loss_forward(x, t, cw, want, 1.5, 0.4)
            out.backward(up)
            hip.sigmoid_focal_loss_backward(x, t, cw, want_grad, 1.5, 0.4, grad_output=up)
        else:
            want = nan_like(1, device=hip_device)
            hip.sigmoid_focal_loss_forward_sum(x, t, cw, want, 1.5, 0.4, None, scale)
            (out * 0.7).backward()
            seven = torch.tensor([0.7], device=hip_device)
            hip.sigmoid_focal_loss_backward(x, t, cw, want_grad, 1.5, 0.4, grad_scalar=seven, scale=scale)
        assert out.shape == ((n, c) if reduction == 'none' else ())
        assert torch.equal(out.reshape(want.shape), want), reduction
        assert torch.equal(leaf.grad, want_grad), reduction
        # the module is the function
        again = SigmoidFocalLoss(1.5, 0.4, cw, reduction)(x, t)
        assert torch.equal(again, out.detach())
    # 'mean' is over the N rows
    loss64, _, sp = R.reference(x, t, 1.5, 0.4, cw)
    R.check_sum(sigmoid_focal_loss(x, t, 1.5, 0.4, cw, 'mean'), loss64 / n, sp, 1.5, 'mean',
                depth=R.device_sum_depth(n * c))


def test_zero_upstream_gives_exact_zeros_and_no_grad_means_no_launch(hip_device):
    from nesie_amd import kernels
    from nesie_amd.mmdet3d_ops import sigmoid_focal_loss
    from tests._launch_recorder import LaunchRecorder
    host = inputs(257, 19, 30)
    x, t = host['x'].to(hip_device), host['t'].to(hip_device)
    for reduction in ('none', 'sum'):
        leaf = x.clone().requires_grad_(True)
        out = sigmoid_focal_loss(leaf, t, 0.5, 0.25, None, reduction)
        out.backward(torch.zeros_like(out))
        assert (leaf.grad == 0).all()
    with kernels.use_backend(LaunchRecorder()) as rec:
        out = sigmoid_focal_loss(x, t, 2.0, 0.25, None, 'sum')
        assert not out.requires_grad
        assert [e[0] for e in rec.log] == ['sigmoid_focal_loss_forward_sum']


AVG = (None, 7.5, 'tensor')


@pytest.mark.parametrize('weight', [None, 'sw_row', 'sw_elem'])
def test_focal_loss_module(hip_device, weight):
    from nesie_amd.kernels import backend_for
    from nesie_amd.votenet.losses import FocalLoss
    n, c = 4099, 10                                   # eleven partials, a ragged last one
    host = inputs(n, c, 3, 104)
    x, t = host['x'].to(hip_device), host['t'].to(hip_device)
    w = weight and host[weight].to(hip_device)
    loss64, grad64, sp = referee(n, c, 3, 2.0, 0.25, 104)
    f = R.factor(host['t'], n, c, None, weight and host[weight])
    for reduction, avg in itertools.product(('none', 'mean', 'sum'), AVG):
        module = FocalLoss(reduction='mean' if reduction == 'sum' else 'sum', loss_weight=0.5)
        avg_arg = torch.tensor(7.5, device=hip_device) if avg == 'tensor' else avg
        if reduction == 'sum' and avg is not None:
            with pytest.raises(ValueError):
                module(x, t, w, avg_factor=avg_arg, reduction_override=reduction)
            continue
        leaf = x.clone().requires_grad_(True)
        out = module(leaf, t, w, avg_factor=avg_arg, reduction_override=reduction)
        what = f'{reduction} avg_factor {avg}'
        if reduction == 'none':
            want = nan_like(n, c, device=hip_device)
            backend_for(x).sigmoid_focal_loss_forward(x, t, None, want, 2.0, 0.25, w, 0.5)
            assert torch.equal(out, want), what
            R.check(out, 0.5 * loss64 * f, sp, 2.0, what)
            out.sum().backward()
            R.check(leaf.grad, 0.5 * grad64 * f, sp, 2.0, what + ' grad')
            continue
        div = 1.0 if reduction == 'sum' else (n * c if avg is None else 7.5)
        assert out.shape == ()
        R.check_sum(out, 0.5 * loss64 * f / div, sp, 2.0, what, depth=R.device_sum_depth(n * c))
        out.backward()
        R.check(leaf.grad, 0.5 * grad64 * f / div, sp, 2.0, what + ' grad')


@pytest.mark.parametrize('dtype', [torch.float64, torch.bfloat16])
def test_other_dtypes_take_the_torch_path(hip_device, dtype):
    from nesie_amd import kernels
    from nesie_amd.votenet.losses import FocalLoss
    host = inputs(257, 19, 3)
    x = host['x'].clamp(-50, 50).to(hip_device, dtype).requires_grad_(True)
    t = host['t'].to(hip_device)

    class Refuses:
        name = 'hip'

        def __getattr__(self, method):
            raise AssertionError(f'{method} launched for {dtype}')
    with kernels.use_backend(Refuses()):
        out = FocalLoss(reduction='sum')(x, t)
        out.backward()
    assert out.dtype == dtype and x.grad.dtype == dtype
    # the logits are float32 values in either dtype, so the referee sees exactly what the module saw;
    # bfloat16 keeps 8 bits per term
    loss64, _, _ = R.reference(x.detach().float(), t, 2.0, 0.25)
    rtol = 1e-12 if dtype == torch.float64 else 2e-2
    torch.testing.assert_close(out.detach().double().cpu(), loss64.sum(), rtol=rtol, atol=0)
    assert torch.isfinite(x.grad).all()


def _forward_backward(module, x, t, w):
    leaf = x.clone().requires_grad_(True)
    out = module(leaf, t, w)
    out.backward()
    return out.detach(), leaf.grad


def test_same_bits_twice_under_a_cu_budget_and_on_a_side_stream(hip_device):
    from nesie_amd.kernels import HipKernels
    from nesie_amd.votenet.losses import FocalLoss
    n, c = 29989, 10                                  # 74 partials
    host = inputs(n, c, 3)
    x, t, w = (host[k].to(hip_device) for k in ('x', 't', 'sw_row'))
    module = FocalLoss(reduction='mean', loss_weight=2.0)
    first = _forward_backward(module, x, t, w)
    again = _forward_backward(module, x, t, w)
    with HipKernels.cu_budget(232):
        budget = _forward_backward(module, x, t, w)
    side = torch.cuda.Stream(hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        streamed = _forward_backward(module, x, t, w)
    torch.cuda.current_stream(hip_device).wait_stream(side)
    for other in (again, budget, streamed):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


def test_graph_replay_equals_eager(hip_device):
    from nesie_amd.votenet.losses import FocalLoss
    n, c = 4099, 10                                   # two launches forward, one backward
    host = inputs(n, c, 3)
    x, t, w = (host[k].to(hip_device) for k in ('x', 't', 'sw_row'))
    module = FocalLoss(reduction='sum')
    eager = _forward_backward(module, x, t, w)
    static_x = torch.zeros_like(x).requires_grad_(True)
    side = torch.cuda.Stream(hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):                     # warm-up off the capture
        module(static_x, t, w).backward()
    torch.cuda.current_stream(hip_device).wait_stream(side)
    static_x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = module(static_x, t, w)
        out.backward()
    with torch.no_grad():
        static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize(hip_device)
    assert torch.equal(out.detach(), eager[0]) and torch.equal(static_x.grad, eager[1])


def test_head_takes_a_focal_objectness_loss(hip_device):
    from nesie_amd.votenet import head_loss
    model = H.head_model().to(hip_device)
    head = model.bbox_head
    assert head_loss.config_of(head) is None
    pts, boxes, labels = _small.small_batch()
    head.jitter_noise = tuple(n.to(hip_device) for n in _small.fixed_noise(2, 32))
    losses, scores, targets, weights = H.head_run(model, pts.to(hip_device), boxes, labels)
    sum(losses.values()).backward()
    assert scores.shape == (64, 2) and 0 < int(targets.sum()) < 64
    ref, _, sp = R.reference(scores, targets, 2.0, 0.25, sample_weight=weights)
    R.check_sum(losses['objectness_loss'], 5.0 * ref, sp, 2.0, 'objectness_loss')
    grad = head.conv_pred.conv_cls.weight.grad
    assert torch.isfinite(grad).all() and grad[:2].abs().sum() > 0
