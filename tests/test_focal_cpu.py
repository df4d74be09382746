"""Sigmoid focal loss without a GPU: the names that were stubs, the tensor-op formulation against the
float64 referee (``tests/_focal_ref.py``, which derives the bound), FocalLoss's host logic, the
distribution focal loss, what the native path launches, the declared C entries and the head."""
import ctypes
import itertools

import pytest
import torch

from nesie_amd import _lib, kernels, mmdet3d_ops
from nesie_amd.mmdet3d_ops import focal_loss as FL
from nesie_amd.votenet import head_loss, losses as L
from tests import _focal_head as H
from tests import _focal_ref as R
from tests import _small
from tests._launch_recorder import LaunchRecorder

GAMMAS = (0, 0.5, 2, 5)


# ---- stub yesterday, real now ------------------------------------------------------------------
def test_the_losses_build_from_a_config():
    loss = L.build_loss(dict(type='FocalLoss', use_sigmoid=True, gamma=1.5, alpha=0.4,
                             reduction='sum', loss_weight=5.0))
    assert isinstance(loss, L.FocalLoss)
    assert (loss.use_sigmoid, loss.gamma, loss.alpha, loss.reduction, loss.loss_weight) == \
        (True, 1.5, 0.4, 'sum', 5.0)
    dfl = L.build_loss(dict(type='GeneralDistributionFocalLoss'))
    assert isinstance(dfl, L.GeneralDistributionFocalLoss)
    assert (dfl.reduction, dfl.loss_weight) == ('mean', 1.0)
    with pytest.raises(AssertionError):
        L.FocalLoss(use_sigmoid=False)


def test_the_mmcv_names_are_real_and_the_pinned_stubs_still_raise():
    for name in ('sigmoid_focal_loss', 'SigmoidFocalLoss'):
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__
    assert mmdet3d_ops.sigmoid_focal_loss == FL.sigmoid_focal_loss
    assert mmdet3d_ops.sigmoid_focal_loss.__self__ is FL.SigmoidFocalLossFunction
    assert mmdet3d_ops.SigmoidFocalLoss is FL.SigmoidFocalLoss
    for name in ('assign_score_withk', 'PAConv', 'SparseBottleneck'):
        assert name in mmdet3d_ops._OUT_OF_SCOPE
        with pytest.raises(NotImplementedError):
            getattr(mmdet3d_ops, name)()


def test_module_keeps_its_weight_as_a_buffer():
    m = FL.SigmoidFocalLoss(2.0, 0.25, weight=torch.tensor([1.0, 2.0]), reduction='sum')
    assert 'weight' in dict(m.named_buffers()) and m.reduction == 'sum'
    assert dict(FL.SigmoidFocalLoss(2.0, 0.25).named_buffers()) == {}


# ---- the tensor-op formulation against float64 -------------------------------------------------
@pytest.mark.parametrize('gamma', GAMMAS)
@pytest.mark.parametrize('scale', [3, 30])
def test_torch_formulation_meets_the_bound(gamma, scale):
    x, t = R.case(257, 19, scale, seed=11)
    x.requires_grad_(True)
    onehot = t.view(-1, 1) == torch.arange(19)
    loss = L.py_sigmoid_focal_loss(x, onehot, None, gamma, 0.25, 'none')
    loss.sum().backward()
    ref, gref, sp = R.reference(x, t, gamma, 0.25)
    R.check(loss, ref, sp, gamma, 'loss')
    R.check(x.grad, gref, sp, gamma, 'grad')


@pytest.mark.parametrize('gamma', GAMMAS)
def test_bare_focal_loss_on_cpu_tensors_takes_the_torch_path(gamma):
    x, t = R.case(64, 3, 10, seed=12, limit=104)      # a sum is checked: see R.case
    x.requires_grad_(True)
    w = torch.rand(64) * 0.75 + 0.25
    out = L.FocalLoss(gamma=gamma, alpha=0.5, reduction='sum', loss_weight=0.5)(x, t, weight=w)
    out.backward()
    ref, gref, sp = R.reference(x, t, gamma, 0.5, sample_weight=w)
    R.check_sum(out, 0.5 * ref, sp, gamma, 'sum')
    R.check(x.grad, 0.5 * gref, sp, gamma, 'grad')


@pytest.mark.parametrize('shape', [(4099, 10), (29989, 10)])
def test_the_sum_check_of_the_device_tests_notices_a_lost_chunk(shape):
    """What ``tests/test_focal_gpu.py`` relies on: on inputs clamped to |x| <= 104 and with the bound
    of the device's tree, a sum that lost its ragged last chunk, its first chunk or just its largest
    term fails; on the unclamped inputs (terms of 3e38) one chunk alone would pass for the sum."""
    n, c = shape
    depth = R.device_sum_depth(n * c)
    x, t = R.case(n, c, 3, seed=21, limit=104)
    ref, _, sp = R.reference(x, t, 2.0, 0.25)
    flat = ref.reshape(-1)
    R.check_sum(flat.sum().float(), ref, sp, 2.0, depth=depth)
    last = (n * c // R.CHUNK) * R.CHUNK
    for wrong in (flat[:last].sum(), flat[R.CHUNK:].sum(), flat.sum() - flat.max()):
        with pytest.raises(AssertionError):
            R.check_sum(wrong.float(), ref, sp, 2.0, depth=depth)
    x, t = R.case(n, c, 3, seed=21)
    ref, _, sp = R.reference(x, t, 2.0, 0.25)
    R.check_sum(ref.reshape(-1)[:R.CHUNK].sum().float(), ref, sp, 2.0)


def test_finite_where_the_textbook_form_is_not():
    values = torch.tensor([88.0, -88.0, 104.0, -104.0, 1e4, -1e4, 3e38, -3e38])
    x = values.view(-1, 1).repeat(1, 2).requires_grad_(True)
    t = torch.zeros(len(values), dtype=torch.long)       # column 0 positive, column 1 negative
    loss = L.FocalLoss(gamma=0.5, reduction='none')(x, t)
    loss.sum().backward()
    assert torch.isfinite(loss).all() and torch.isfinite(x.grad).all()
    ref, gref, sp = R.reference(x, t, 0.5, 0.25)
    R.check(loss, ref, sp, 0.5, 'loss')
    R.check(x.grad, gref, sp, 0.5, 'grad')
    # the form both mmcv's kernel and mmdet's fallback restate: (1 - p)^gamma by subtraction
    y = x.detach().clone().requires_grad_(True)
    p = y.sigmoid()
    onehot = torch.nn.functional.one_hot(t, 2).float()
    pt = (1 - p) * onehot + p * (1 - onehot)
    textbook = torch.nn.functional.binary_cross_entropy_with_logits(y, onehot, reduction='none') \
        * pt.pow(0.5)
    textbook.sum().backward()
    assert not torch.isfinite(y.grad).all()


# ---- host logic ----------------------------------------------------------------------------------
N, C = 23, 4


def _expected(ref, weight, reduction, avg_factor, loss_weight):
    loss = ref if weight is None else ref * (weight.double().view(N, 1) if weight.numel() == N
                                             else weight.double().view(N, C))
    if reduction == 'none':
        return loss_weight * loss
    if reduction == 'sum':
        return loss_weight * loss.sum()
    return loss_weight * (loss.mean() if avg_factor is None else loss.sum() / float(avg_factor))


@pytest.mark.parametrize('weight_shape', [None, (N,), (N, C), (N * C,)])
def test_every_reduction_avg_factor_and_override(weight_shape):
    x, t = R.case(N, C, 3, seed=13)
    x = x.clamp(-104, 104)      # 3e38 times the loss weight would leave float32
    weight = None if weight_shape is None else torch.rand(*weight_shape) + 0.5
    ref, _, _ = R.reference(x, t, 2.0, 0.25)
    for own, override, avg in itertools.product(('none', 'mean', 'sum'), (None, 'none', 'mean', 'sum'),
                                                (None, 7.5, torch.tensor(7.5), torch.tensor([7.5]))):
        module = L.FocalLoss(reduction=own, loss_weight=3.0)
        reduction = override or own
        if reduction == 'sum' and avg is not None:
            with pytest.raises(ValueError):
                module(x, t, weight, avg_factor=avg, reduction_override=override)
            continue
        got = module(x, t, weight, avg_factor=avg, reduction_override=override)
        want = _expected(ref, weight, reduction, avg, 3.0)
        assert got.numel() == want.numel()
        torch.testing.assert_close(got.double().reshape(want.shape), want, rtol=1e-5, atol=1e-7)
    with pytest.raises(AssertionError):
        L.FocalLoss()(x, t, reduction_override='average')
    with pytest.raises(AssertionError):
        L.FocalLoss()(x, t, weight=torch.ones(N + 1))


def test_labels_outside_the_classes_give_all_negative_rows():
    x = torch.randn(1, C).repeat(4, 1)
    t = torch.tensor([C, -1, 2 ** 31 + 3, 1])
    loss = L.FocalLoss(reduction='none')(x, t)
    assert torch.equal(loss[0], loss[1]) and torch.equal(loss[0], loss[2])
    assert not torch.equal(loss[0], loss[3])
    all_negative = L.py_sigmoid_focal_loss(x[:1], torch.zeros(1, C), None, 2.0, 0.25, 'none')
    assert torch.equal(loss[:1], all_negative)
    ref, _, sp = R.reference(x, t, 2.0, 0.25)
    R.check(loss, ref, sp, 2.0)


def test_empty_input_gives_what_the_torch_formulation_gives():
    x, t = torch.zeros(0, C, requires_grad=True), torch.zeros(0, dtype=torch.long)
    for reduction in ('none', 'mean', 'sum'):
        got = L.FocalLoss(reduction=reduction)(x, t)
        want = L.py_sigmoid_focal_loss(x, torch.zeros(0, C), None, 2.0, 0.25, reduction)
        torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)
    assert L.FocalLoss(reduction='none')(x, t).shape == (0, C)
    assert L.FocalLoss(reduction='sum')(x, t).item() == 0
    L.FocalLoss(reduction='sum')(x, t).backward()
    assert x.grad.shape == (0, C)


# ---- distribution focal loss ---------------------------------------------------------------------
def test_distribution_focal_loss_by_hand():
    g = torch.Generator().manual_seed(14)
    pred = torch.randn(37, 17, generator=g)
    label = torch.rand(37, generator=g) * 15.999
    weight = torch.rand(37, generator=g)
    logp = torch.log_softmax(pred.double(), dim=1)
    left = label.long()
    w_left = (left + 1).double() - label.double()
    w_right = label.double() - left.double()
    rows = torch.arange(37)
    want = -(logp[rows, left] * w_left + logp[rows, left + 1] * w_right)
    torch.testing.assert_close(L.distribution_focal_loss(pred, label, reduction='none'),
                               want.float())
    torch.testing.assert_close(L.distribution_focal_loss(pred, label, weight, avg_factor=4.0),
                               ((want * weight.double()).sum() / 4.0).float())
    module = L.GeneralDistributionFocalLoss(reduction='sum', loss_weight=0.25)
    torch.testing.assert_close(module(pred, label, weight),
                               (0.25 * (want * weight.double()).sum()).float())
    torch.testing.assert_close(module(pred, label, reduction_override='mean'),
                               (0.25 * want.mean()).float())
    with pytest.raises(AssertionError):
        module(pred, label, reduction_override='average')


# ---- what the native path launches ----------------------------------------------------------------
def _nc_float_storages(log, n, c):
    found = set()

    def walk(v):
        if isinstance(v, dict) and 'T' in v:
            if v['T'][2] == [n, c] and v['T'][4] == 'float32':
                found.add(v['T'][0])
        elif isinstance(v, dict):
            for e in v.values():
                walk(e)
        elif isinstance(v, list):
            for e in v:
                walk(e)
    for _, args, kwargs in log:
        walk(args)
        walk(kwargs)
    return found


@pytest.mark.parametrize('reduction', ['sum', 'mean'])
@pytest.mark.parametrize('surface', ['function', 'module'])
def test_reduced_forward_and_backward_launch_one_entry_each(reduction, surface):
    n, c = 40, 5
    x, t = R.case(n, c, 3, seed=15)
    x.requires_grad_(True)
    with kernels.use_backend(LaunchRecorder()) as rec:
        if surface == 'function':
            out = FL.sigmoid_focal_loss(x, t, 2.0, 0.25, torch.ones(c), reduction)
        else:
            avg = torch.tensor(3.0) if reduction == 'mean' else None
            out = L.FocalLoss(reduction=reduction)(x, t, weight=torch.ones(n), avg_factor=avg)
        assert out.shape == ()
        assert [e[0] for e in rec.log] == ['sigmoid_focal_loss_forward_sum']
        assert _nc_float_storages(rec.log, n, c) == {0}              # pred, seen first
        out.backward()
        assert [e[0] for e in rec.log] == ['sigmoid_focal_loss_forward_sum',
                                           'sigmoid_focal_loss_backward']
        assert len(_nc_float_storages(rec.log, n, c)) == 2           # pred and grad_x
    assert x.grad.shape == (n, c)


def test_unreduced_forward_applies_the_weight_in_the_launch():
    n, c = 40, 5
    x, t = R.case(n, c, 3, seed=16)
    x.requires_grad_(True)
    w = torch.ones(n, c)
    with kernels.use_backend(LaunchRecorder()) as rec:
        out = L.FocalLoss(reduction='none', loss_weight=2.0)(x, t, weight=w)
        out.sum().backward()
    assert out.shape == (n, c)
    assert [e[0] for e in rec.log] == ['sigmoid_focal_loss_forward', 'sigmoid_focal_loss_backward']
    bound = dict(zip(('input', 'target', 'weight', 'output', 'gamma', 'alpha', 'sample_weight',
                      'scale'), rec.log[0][1]))
    assert bound['sample_weight']['T'][2] == [n, c] and bound['scale'] == 2.0


def test_a_weight_that_wants_a_gradient_goes_through_autograd():
    x, t = R.case(40, 5, 3, seed=19)
    x = x.clamp(-50, 50).requires_grad_(True)
    w = torch.rand(40, requires_grad=True)
    with kernels.use_backend(LaunchRecorder()) as rec:
        L.FocalLoss(reduction='sum')(x, t, weight=w).backward()
    assert rec.log == []
    ref, _, _ = R.reference(x, t, 2.0, 0.25)
    torch.testing.assert_close(w.grad.double(), ref.sum(1), rtol=1e-5, atol=1e-7)


def test_function_checks_and_reductions():
    x, t = R.case(8, 3, 3, seed=17)
    with kernels.use_backend(LaunchRecorder()):
        assert FL.sigmoid_focal_loss(x, t, 2.0, 0.25, None, 'none').shape == (8, 3)
        with pytest.raises(KeyError):
            FL.sigmoid_focal_loss(x, t, 2.0, 0.25, None, 'average')
        for bad in ((x.view(-1), t), (x, t.int()), (x, t[:-1]), (x, t.view(-1, 1))):
            with pytest.raises(AssertionError):
                FL.sigmoid_focal_loss(*bad)
        for bad_weight in (torch.ones(4), torch.ones(3, 1)):
            with pytest.raises(AssertionError):
                FL.sigmoid_focal_loss(x, t, 2.0, 0.25, bad_weight)


def test_function_on_an_empty_input_launches_nothing_and_agrees_with_focal_loss():
    x, t = torch.zeros(0, 3, requires_grad=True), torch.zeros(0, dtype=torch.long)
    with kernels.use_backend(LaunchRecorder()) as rec:
        for reduction in ('none', 'sum', 'mean'):       # 'mean' = sum / N = 0 / 0
            got = FL.sigmoid_focal_loss(x, t, 2.0, 0.25, None, reduction)
            want = L.FocalLoss(reduction=reduction)(x, t)
            torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)
        assert torch.isnan(FL.sigmoid_focal_loss(x, t, 2.0, 0.25, None, 'mean'))
        FL.sigmoid_focal_loss(x, t, 2.0, 0.25, None, 'sum').backward()
        assert rec.log == [] and x.grad.shape == (0, 3)


def test_no_cpu_fallback():
    x, t = R.case(8, 3, 3, seed=18)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FL.sigmoid_focal_loss(x, t)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        FL.SigmoidFocalLoss(2.0, 0.25)(x, t)


# ---- the C entries ---------------------------------------------------------------------------------
def test_entries_are_declared():
    i, f, p, z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    sig = _lib.SIGNATURES
    operands = [i, i, p, p, p, p, i, f, f]          # n, c, x, target, class w, sample w, mode, gamma, alpha
    assert sig['nesie_sigmoid_focal_loss_forward'] == (i, operands + [f, p, p])
    assert sig['nesie_sigmoid_focal_loss_workspace_bytes'] == (z, [i, i])
    assert sig['nesie_sigmoid_focal_loss_forward_sum'] == (i, operands + [f, p, p, p, z, p])
    assert sig['nesie_sigmoid_focal_loss_backward'] == (i, operands + [p, p, f, p, p, p])
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in sig if name.startswith('nesie_sigmoid_focal'))
    assert lib.nesie_abi_version() == 2


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    n = None
    INVALID, UNSUPPORTED = 1, 2
    host = ctypes.create_string_buffer(64)
    a = ctypes.addressof(host)          # never dereferenced: every call below stops at a check

    def fwd(rows, cols, x=n, t=n, sw=n, mode=0, gamma=2.0, out=n):
        return lib.nesie_sigmoid_focal_loss_forward(rows, cols, x, t, n, sw, mode, gamma, 0.25, 1.0,
                                                    out, n)

    def fsum(rows, cols, x=n, t=n, out=n, ws=n, ws_bytes=0):
        return lib.nesie_sigmoid_focal_loss_forward_sum(rows, cols, x, t, n, n, 0, 2.0, 0.25, 1.0, n,
                                                        out, ws, ws_bytes, n)

    def bwd(rows, cols, x=n, t=n, g=n, gs=n, out=n):
        return lib.nesie_sigmoid_focal_loss_backward(rows, cols, x, t, n, n, 0, 2.0, 0.25, g, gs, 1.0,
                                                     n, out, n)

    for rows, cols in ((0, 5), (5, 0), (0, 0)):       # nothing to do: success, nothing touched
        assert fwd(rows, cols) == 0 and fsum(rows, cols) == 0 and bwd(rows, cols) == 0
    for call in (fwd, fsum, bwd):
        assert call(-1, 5) == INVALID and call(5, -1) == INVALID
        assert call(4, 5) == INVALID                   # null operands of a problem that is not empty
        assert b'sigmoid_focal_loss' in lib.nesie_last_error()
        assert call(65536, 32768) == UNSUPPORTED       # 2^31 elements
    assert fwd(4, 5, a, a) == INVALID                  # no output
    assert fwd(4, 5, a, a, out=a, gamma=-1.0) == INVALID
    assert fwd(4, 5, a, a, out=a, gamma=float('nan')) == INVALID
    assert fwd(4, 5, a, a, out=a, mode=3) == INVALID
    assert fwd(4, 5, a, a, out=a, mode=1) == INVALID   # a mode without its weight
    assert fwd(4, 5, a, a, out=a, sw=a, mode=0) == INVALID
    assert bwd(4, 5, a, a, out=a) == INVALID           # neither upstream gradient
    assert bwd(4, 5, a, a, g=a, gs=a, out=a) == INVALID   # both
    # the reduction's scratch: one float per chunk of 4096 elements once there is more than one
    ws = lib.nesie_sigmoid_focal_loss_workspace_bytes
    assert ws(1, 4096) == 0 and ws(4097, 1) == 16 and ws(4096, 5) == 32
    assert ws(-1, 5) == 0 and ws(65536, 32768) == 0
    assert fsum(4097, 1, a, a, out=a) == INVALID       # two chunks and no scratch
    assert fsum(4097, 1, a, a, out=a, ws=a, ws_bytes=4) == INVALID


# ---- the head ----------------------------------------------------------------------------------------
def test_head_takes_a_focal_objectness_loss(oracle_kernels):
    model = H.head_model()
    head = model.bbox_head
    assert isinstance(head.objectness_loss, L.FocalLoss) and head_loss.config_of(head) is None
    pts, boxes, labels = _small.small_batch()
    head.jitter_noise = _small.fixed_noise(2, 32)
    with kernels.use_backend(oracle_kernels):
        losses, scores, targets, weights = H.head_run(model, pts, boxes, labels)
        sum(losses.values()).backward()
    assert scores.shape == (64, 2) and 0 < int(targets.sum()) < 64
    ref, _, sp = R.reference(scores, targets, 2.0, 0.25, sample_weight=weights)
    R.check_sum(losses['objectness_loss'], 5.0 * ref, sp, 2.0, 'objectness_loss')
    grad = head.conv_pred.conv_cls.weight.grad
    assert torch.isfinite(grad).all() and grad[:2].abs().sum() > 0
