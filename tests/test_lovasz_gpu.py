"""Lovasz-Softmax kernels on the device against the float64 referee (``tests/_lovasz_ref.py``),
through the C ABI's back-end method and through autograd.

Bounds: the sign and zero pattern of the gradient exact; the loss within
4 * 2^-24 relative (every term is nonnegative, g and the sums are double, one rounding to float32
follows, the factor leaves a margin); a gradient element within 8 * 2^-24 relative (g times the
divisor in double, one rounding; an upstream scale adds one more)."""
import functools

import numpy as np
import pytest
import torch

from tests import _lovasz_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
VOID = 255


@functools.lru_cache(maxsize=None)
def inputs(b, c, s, kind='plain'):
    """(probas (B, C, S) float32, labels (B, S)) as read-only arrays.  kind: 'plain' softmax of
    3 * randn; 'saturated' probabilities rounded to quarters (exact 0 and 1, equal errors inside and
    across foreground and background); 'void' 20 % void labels; 'mixed' void labels, labels outside
    [0, C), class 2 missing from image 1; 'one_class' every label 1; 'all_void'."""
    rng = np.random.RandomState(b * 1000003 + c * 1009 + s)
    logits = torch.from_numpy(3.0 * rng.randn(b, c, s)).float()
    p = (torch.sigmoid(logits) if c == 1 else torch.softmax(logits, dim=1)).numpy()
    labels = rng.randint(0, max(c, 2), size=(b, s)).astype(np.int64)
    if kind == 'saturated':
        p = (np.round(p * 4) / 4).astype(np.float32)
    if kind in ('void', 'mixed'):
        labels[rng.rand(b, s) < 0.2] = VOID
    if kind == 'mixed':
        labels[1][labels[1] == 2] = 0
        labels[0, :3] = c + 4
        labels[b - 1, -3:] = -2
    if kind == 'one_class':
        labels[:] = 1
    if kind == 'all_void':
        labels[:] = VOID
    p.setflags(write=False); labels.setflags(write=False)
    return p, labels


@functools.lru_cache(maxsize=None)
def referee(b, c, s, kind, classes, per_image, ignore):
    p, labels = inputs(b, c, s, kind)
    return R.lovasz(p, labels, list(classes) if isinstance(classes, tuple) else classes, per_image,
                    ignore)


def device_probas(p, device, layout):
    """(B, C, S) on the device, channel-first contiguous or the view of a points-major (B, S, C)
    tensor (B = 1: the flat (P, C) form)."""
    t = torch.from_numpy(np.array(p)).to(device)
    if layout == 'flat':
        t = t.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert t.shape[1] == 1 or t.stride(1) == 1
    return t


def run_kernel(device, p, labels, classes, per_image, ignore, layout='channel_first'):
    from nesie_amd.kernels import backend_for
    from nesie_amd.mmdet3d_ops.lovasz import class_selector
    probas = device_probas(p, device, layout)
    lab = torch.from_numpy(np.array(labels)).to(device)
    mode, mask = class_selector(list(classes) if isinstance(classes, tuple) else classes,
                                p.shape[1], device)
    loss = torch.full((1,), float('nan'), device=device)
    grad = torch.full_like(probas, float('nan'))
    assert grad.stride() == probas.stride()
    backend_for(probas).lovasz_softmax(probas, lab, loss, grad, per_image, ignore, mode, mask)
    return loss.cpu(), grad.cpu()


def check(loss, grad, want, want_grad, what, scale=1.0):
    print(f'{what}: loss {float(loss):.9g} referee {want * scale:.17g}')
    got = grad.numpy().astype(np.float64)
    want_grad = want_grad * scale
    assert np.array_equal(np.sign(got), np.sign(want_grad)), what
    assert abs(float(loss) - want * scale) <= 4 * U * abs(want * scale), what
    err = np.abs(got - want_grad)
    with np.errstate(divide='ignore', invalid='ignore'):
        print(f'  worst gradient error {np.nanmax(np.where(want_grad != 0, err / np.abs(want_grad), 0)) / U:.3f} u')
    assert np.all(err <= 8 * U * np.abs(want_grad)), what


# (B, C, S), kind, classes, per_image, ignore
CASES = [
    ((1, 2, 1), 'plain', 'present', False, None),
    ((1, 2, 1), 'plain', 'all', True, None),
    ((1, 1, 1023), 'plain', (0,), False, None),
    ((1, 1, 1024), 'plain', (0,), False, None),
    ((1, 1, 1025), 'plain', (0,), False, None),
    ((1, 2, 1023), 'plain', 'present', False, None),
    ((1, 2, 1024), 'plain', 'all', False, None),
    ((1, 2, 1025), 'plain', 'present', False, None),
    ((1, 3, 700), 'plain', 'present', False, None),
    ((1, 3, 700), 'saturated', 'all', False, None),
    ((1, 7, 5000), 'plain', 'present', False, None),
    ((2, 7, 2500), 'void', (1, 3, 3, 6), False, VOID),
    ((3, 4, 1500), 'mixed', 'present', True, VOID),
    ((3, 4, 1500), 'mixed', 'all', True, VOID),
    ((3, 4, 1500), 'mixed', (2, 3), True, VOID),
    ((3, 4, 1500), 'mixed', 'present', False, VOID),
    ((3, 4, 1500), 'saturated', 'present', True, None),
    # class 0, 2 and 3 absent: G = 0 and g_0 = 1 under 'all' and the list, left out under 'present'
    ((2, 4, 1100), 'one_class', 'present', False, None),
    ((2, 4, 1100), 'one_class', 'all', False, None),
    ((2, 4, 1100), 'one_class', (0, 1), True, None),
    ((2, 3, 1100), 'all_void', 'present', False, VOID),
    ((2, 3, 1100), 'all_void', 'all', True, VOID),
]


def case_id(case):
    (b, c, s), kind, classes, per_image, ignore = case
    name = classes if isinstance(classes, str) else 'list'
    return f'{b}x{c}x{s}-{kind}-{name}-{"image" if per_image else "batch"}'


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_kernel_against_float64(hip_device, case):
    (b, c, s), kind, classes, per_image, ignore = case
    p, labels = inputs(b, c, s, kind)
    want, want_grad = referee(b, c, s, kind, classes, per_image, ignore)
    loss, grad = run_kernel(hip_device, p, labels, classes, per_image, ignore)
    check(loss, grad, want, want_grad, case_id(case))
    # the points-major layout (B = 1: the flat (P, C) tensor) on the same data: the same bits
    loss2, grad2 = run_kernel(hip_device, p, labels, classes, per_image, ignore, 'flat')
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    if kind == 'all_void':
        assert float(loss) == 0.0 and torch.count_nonzero(grad) == 0


def test_forty_thousand_points_twenty_classes(hip_device):
    b, c, s = 2, 20, 20000
    p, labels = inputs(b, c, s, 'void')
    want, want_grad = referee(b, c, s, 'void', 'present', False, VOID)
    loss, grad = run_kernel(hip_device, p, labels, 'present', False, VOID)
    check(loss, grad, want, want_grad, '40000 x 20')
    again = run_kernel(hip_device, p, labels, 'present', False, VOID)
    assert torch.equal(loss, again[0]) and torch.equal(grad, again[1])


def test_two_runs_give_the_same_bits(hip_device):
    p, labels = inputs(3, 4, 1500, 'mixed')
    first = run_kernel(hip_device, p, labels, 'present', True, VOID)
    for _ in range(2):
        again = run_kernel(hip_device, p, labels, 'present', True, VOID)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_nan_and_inf_reach_the_loss(hip_device):
    p, labels = inputs(1, 3, 700, 'plain')
    for bad in (float('nan'), float('inf')):
        q = p.copy()
        fg = int(np.flatnonzero(labels[0] == 1)[0])
        q[0, 1, fg] = bad                     # a foreground point of class 1: g > 0 there
        loss, grad = run_kernel(hip_device, q, labels, 'present', False, None)
        assert not np.isfinite(float(loss)), bad
        assert np.isnan(float(loss)) if np.isnan(bad) else float(loss) == float('inf')
        assert torch.isfinite(grad).all()     # g comes from the counts alone
        # the bad error sorts first: the entry's gradient is the first foreground one, -1 / G / n
        big_g = int((labels[0] == 1).sum())
        assert abs(float(grad[0, 1, fg]) + 1.0 / big_g / 3) <= 8 * U / big_g / 3


def test_autograd_against_float64(hip_device):
    from nesie_amd.votenet import losses as L
    b, c, s = 3, 4, 1500
    p, labels = inputs(b, c, s, 'mixed')
    lab = torch.from_numpy(np.array(labels)).to(hip_device)
    for classes, per_image in (('present', True), ((2, 3), False)):
        want, want_grad = referee(b, c, s, 'mixed', classes, per_image, VOID)
        probas = device_probas(p, hip_device, 'channel_first').reshape(b, c, 30, 50)
        probas.requires_grad_(True)
        arg = list(classes) if isinstance(classes, tuple) else classes
        loss = L.lovasz_softmax(probas, lab.reshape(b, 30, 50), arg, per_image, VOID)
        (0.375 * loss).backward()
        check(loss.detach().cpu(), probas.grad.reshape(b, c, s).cpu() / 0.375, want, want_grad,
              f'autograd {classes}')
        module = L.build_loss(dict(type='Lovasz3DLoss', loss_weight=2.0, classes=arg,
                                   per_image=per_image, ignore_index=VOID))
        assert float(module(probas.detach().reshape(b, c, 3, 10, 50),
                            lab.reshape(b, 3, 10, 50))) == 2.0 * float(loss.detach())
    # the flat form and the sigmoid form
    p, labels = inputs(1, 3, 700, 'plain')
    want, want_grad = referee(1, 3, 700, 'plain', 'present', False, None)
    flat = torch.from_numpy(np.array(p[0].T)).to(hip_device).requires_grad_(True)
    loss = L.lovasz_softmax_flat(flat, torch.from_numpy(labels[0].copy()).to(hip_device))
    loss.backward()
    check(loss.detach().cpu(), flat.grad.t()[None].cpu(), want, want_grad, 'flat')
    p, labels = inputs(1, 1, 1025, 'plain')
    want, want_grad = R.lovasz(p, np.where(labels == 1, 0, -1), [0])     # C = 1: the listed label is class 0
    sig = torch.from_numpy(p.reshape(1, 25, 41).copy()).to(hip_device).requires_grad_(True)
    loss = L.lovasz_softmax(sig, torch.from_numpy(labels.reshape(1, 25, 41).copy()).to(hip_device), [1])
    loss.backward()
    check(loss.detach().cpu(), sig.grad.reshape(1, 1, 1025).cpu(), want, want_grad, 'sigmoid')


def test_graph_replay_equals_eager(hip_device):
    from nesie_amd.votenet import losses as L
    b, c, s = 3, 4, 1500
    p, labels = inputs(b, c, s, 'mixed')
    x = device_probas(p, hip_device, 'channel_first').reshape(b, c, 30, 50)
    lab = torch.from_numpy(np.array(labels)).to(hip_device).reshape(b, 30, 50)

    def run(probas):
        out = L.lovasz_softmax(probas, lab, [0, 2, 3], True, VOID)
        out.backward()
        return out

    eager_x = x.clone().requires_grad_(True)
    eager = run(eager_x)
    static_x = torch.zeros_like(x).requires_grad_(True)
    side = torch.cuda.Stream(hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):                     # warm-up off the capture
        run(static_x)
    torch.cuda.current_stream(hip_device).wait_stream(side)
    static_x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static_x)
    with torch.no_grad():
        static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize(hip_device)
    assert torch.equal(out.detach(), eager.detach()) and torch.equal(static_x.grad, eager_x.grad)


def test_refusals_come_before_any_launch(hip_device):
    """Sizes and arguments the entry refuses: a status and a message, nothing written."""
    from nesie_amd import _lib
    lib = _lib.load()
    n = None
    call = lib.nesie_lovasz_softmax
    assert call(-1, 2, 4, n, 0, 0, 0, n, 0, 0, 0, 0, n, n, n, n, 0, n) == 1
    assert b'lovasz_softmax' in lib.nesie_last_error()
    assert call(1, 2, -4, n, 0, 0, 0, n, 0, 0, 0, 0, n, n, n, n, 0, n) == 1
    assert call(1, 2, 4, n, 0, 0, 0, n, 0, 0, 0, 3, n, n, n, n, 0, n) == 1       # class_mode
    assert call(1, 2, 4, n, 0, 0, 0, n, 0, 0, 0, 0, n, n, n, n, 0, n) == 1       # null tensors
    assert call(1, 2, 2 ** 30, n, 0, 0, 0, n, 0, 0, 0, 0, n, n, n, n, 0, n) == 2  # P * C > IX_MAX_N
    assert call(70000, 70000, 1, n, 0, 0, 0, n, 0, 0, 0, 0, n, n, n, n, 0, n) == 2
    assert b'at most 2147482623' in lib.nesie_last_error()
    assert lib.nesie_lovasz_softmax_workspace_bytes(1, 2, 2 ** 30) == 0
    assert lib.nesie_lovasz_softmax_workspace_bytes(-1, 2, 4) == 0
    assert call(0, 2, 4, n, 0, 0, 0, n, 0, 0, 0, 0, n, n, n, n, 0, n) == 0       # empty: no launch
    need = lib.nesie_lovasz_softmax_workspace_bytes(1, 2, 4)
    assert need > 0 and need % 8 == 0
    assert lib.nesie_lovasz_softmax_workspace_bytes(3, 4, 1500) >= need
    # real tensors, a workspace one byte short, a mask missing: refused, outputs untouched
    p, labels = inputs(1, 2, 1, 'plain')
    probas = torch.from_numpy(p.copy()).to(hip_device)
    lab = torch.from_numpy(labels.copy()).to(hip_device)
    loss = torch.full((1,), 7.0, device=hip_device)
    grad = torch.full_like(probas, 7.0)
    need = lib.nesie_lovasz_softmax_workspace_bytes(1, 2, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=hip_device)
    args = (1, 2, 1, probas.data_ptr(), 2, 1, 1, lab.data_ptr(), 0, 0, 0)
    tail = (loss.data_ptr(), grad.data_ptr(), ws.data_ptr())
    assert call(*args, 0, n, *tail, need - 1, n) == 1
    assert call(*args, 2, n, *tail, need, n) == 1
    assert call(*args, 0, n, loss.data_ptr(), grad.data_ptr(), ws.data_ptr() + 4, need, n) == 1
    torch.cuda.synchronize(hip_device)
    assert float(loss) == 7.0 and bool((grad == 7.0).all())
    # an empty input through the public function: a zero attached to the graph
    from nesie_amd.votenet import losses as L
    empty = torch.zeros(2, 3, 0, 5, device=hip_device, requires_grad=True)
    out = L.lovasz_softmax(empty, torch.zeros(2, 0, 5, dtype=torch.long, device=hip_device))
    assert float(out.detach()) == 0.0 and out.requires_grad
