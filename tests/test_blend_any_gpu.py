"""The general blend backward (nesie_blend_conv_backward_any): the shapes the 64 x 64-tile kernels
refuse -- against the oracle, bitwise reproducible, fully written, under the norm fold, inside a
captured graph and at model level."""
import copy

import pytest
import torch

from nesie_amd import kernels
from nesie_amd import mmdet3d_ops as ops
from tests import _small
from tests.test_blend_any_cpu import GENERAL_SHAPES

pytestmark = pytest.mark.gpu


def _blend_case(k, segs, g, c, seed, b=2, m=300):
    gen = torch.Generator().manual_seed(seed)
    n = k * segs * g
    idx = torch.randint(0, m, (b, n, 3), generator=gen, dtype=torch.int32)
    w = torch.rand(b, n, 3, generator=gen)
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    rel = torch.randn(b, n, 3, generator=gen)
    return gen, b, m, n, idx, w, rel


def _hip(dev):
    return kernels.backend_for(torch.empty(1, device=dev))


class _Spy:
    """Records (bn fold given?) for every call of HipKernels.blend_conv_backward_any."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = kernels.HipKernels.blend_conv_backward_any
        spy = self

        def wrapped(self_, *a, **kw):
            spy.calls.append(kw.get('bn_z') is not None and kw.get('bnb') is not None)
            return real(self_, *a, **kw)
        monkeypatch.setattr(kernels.HipKernels, 'blend_conv_backward_any', wrapped)


@pytest.mark.parametrize("k,segs,g,c,m", GENERAL_SHAPES)
def test_blend_conv_matches_oracle_at_general_shapes(oracle_kernels, hip_device, monkeypatch, k, segs, g, c, m):
    """BlendConv forward + backward on the device in the default (deterministic) mode against the
    oracle, with the tolerances of test_kernels_gpu.test_blend_conv_matches_oracle."""
    assert kernels.HipKernels.DETERMINISTIC
    spy = _Spy(monkeypatch)
    gen, b, m, n, idx, w, rel = _blend_case(k, segs, g, c, k + c, m=m)
    table = torch.randn(b, m, segs * c, generator=gen)
    wx = torch.randn(segs, c, 3, generator=gen)
    go = torch.randn(b, segs, c, k * g, generator=gen)
    with kernels.use_backend(oracle_kernels):
        t0, x0 = table.clone().requires_grad_(True), wx.clone().requires_grad_(True)
        want = ops.blend_conv(t0, x0, idx, w, rel, segs, g)
        want.backward(go)
    t1 = table.to(hip_device).requires_grad_(True)
    x1 = wx.to(hip_device).requires_grad_(True)
    got = ops.blend_conv(t1, x1, idx.to(hip_device), w.to(hip_device), rel.to(hip_device), segs, g)
    got.backward(go.to(hip_device))
    assert spy.calls == [False]
    torch.testing.assert_close(got.detach().cpu(), want.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(t1.grad.cpu(), t0.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(x1.grad.cpu(), x0.grad, rtol=1e-4, atol=2e-3)


def _skewed(k, segs, g, c, hot, dev):
    """The input of test_staged_blend_backward_is_reproducible_and_equals_the_atomic_form: 70 % of
    the taps on `hot` seeds, the rest on the upper half of m = 96; and its float64 scatter."""
    gen = torch.Generator().manual_seed(k + c)
    b, m = 2, 96
    n = k * segs * g
    hot_idx = torch.randint(0, hot, (b, n, 3), generator=gen)
    cold_idx = torch.randint(m // 2, m, (b, n, 3), generator=gen)
    idx = torch.where(torch.rand(b, n, 3, generator=gen) < 0.7, hot_idx, cold_idx).int()
    w = torch.rand(b, n, 3, generator=gen)
    rel = torch.randn(b, n, 3, generator=gen)
    dy = torch.randn(b, segs, c, n // segs, generator=gen)
    want = torch.zeros(b, m, segs, c, dtype=torch.float64)
    dyc = dy.double().view(b, segs, c, k, g)
    idc = idx.long().view(b, k, segs, g, 3)
    wc = w.double().view(b, k, segs, g, 3)
    for bi in range(b):
        for s_ in range(segs):
            rows = idc[bi, :, s_].reshape(-1, 3)
            contrib = dyc[bi, s_].reshape(c, k * g).t().unsqueeze(1) * wc[bi, :, s_].reshape(-1, 3).unsqueeze(-1)
            want[bi, :, s_].index_add_(0, rows.reshape(-1), contrib.reshape(-1, c))
    return b, m, n, idx, w, rel, dy, want


@pytest.mark.parametrize("k,segs,g,c,hot", [(128, 6, 9, 48, 1), (128, 6, 9, 48, 3), (64, 1, 64, 64, 1),
                                            (64, 1, 64, 64, 3)])
def test_general_blend_backward_is_reproducible_written_in_full_and_accurate(oracle_kernels, hip_device,
                                                                             k, segs, g, c, hot):
    """Three backend-level calls into a NaN-filled table at the skewed input (one seed collects
    about 14 000 taps at the first shape): same bits, no NaN, zero rows for seeds without taps.
    Accuracy against the float64 scatter: at most twice the error of the oracle's fp32 backward
    (the reference's serial order) on the same inputs, plus 1e-6 max|want|."""
    hip = _hip(hip_device)
    b, m, n, idx, w, rel, dy, want = _skewed(k, segs, g, c, hot, hip_device)
    dev = [t.to(hip_device) for t in (idx, w, rel, dy)]
    outs = []
    for _ in range(3):
        d_table = torch.full((b, m, segs * c), float('nan'), device=hip_device)
        d_wx = torch.full((segs, c, 3), float('nan'), device=hip_device)
        hip.blend_conv_backward_any(dev[3], c, dev[0], dev[1], dev[2], d_table, d_wx, segs, g)
        outs.append((d_table.clone(), d_wx.clone()))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
    assert not torch.isnan(outs[0][0]).any() and not torch.isnan(outs[0][1]).any()
    assert float(outs[0][0][:, hot:m // 2].abs().max()) == 0.0          # seeds no tap landed on
    # the routed call takes the same path in both modes
    for det in (True, False):
        prev = hip.set_deterministic(det)
        try:
            d_table = torch.full((b, m, segs * c), float('nan'), device=hip_device)
            d_wx = torch.empty(segs, c, 3, device=hip_device)
            if kernels.blend_backward_form(c, n // segs, m, det) == 'any':
                hip.blend_conv_backward(dev[3], c, dev[0], dev[1], dev[2], d_table, d_wx, segs, g)
                assert torch.equal(d_table, outs[0][0]) and torch.equal(d_wx, outs[0][1])
        finally:
            hip.set_deterministic(prev)
    ref_table = torch.zeros(b, m, segs * c)
    ref_wx = torch.zeros(segs, c, 3)
    oracle_kernels.blend_conv_backward(dy, c, idx, w, rel, ref_table, ref_wx, segs, g)
    scale = want.abs().max().item()
    ref_err = (ref_table.double().view(b, m, segs, c) - want).abs().max().item()
    err = (outs[0][0].double().cpu().view(b, m, segs, c) - want).abs().max().item()
    print(f'blend_any skewed ({k},{segs},{g},{c}) hot={hot}: kernel err {err:.3e}, oracle fp32 err '
          f'{ref_err:.3e}, max|want| {scale:.3e}')
    assert err <= 2 * ref_err + 1e-6 * scale, (err, ref_err, scale)
    want_wx = torch.einsum('bsckg,bksgd->scd', dy.double().view(b, segs, c, k, g),
                           rel.double().view(b, k, segs, g, 3))
    wx_ref_err = (ref_wx.double() - want_wx).abs().max().item()
    wx_err = (outs[0][1].double().cpu() - want_wx).abs().max().item()
    print(f'  d_wx: kernel err {wx_err:.3e}, oracle fp32 err {wx_ref_err:.3e}')
    assert wx_err <= 2 * wx_ref_err + 1e-6 * want_wx.abs().max().item(), (wx_err, wx_ref_err)


@pytest.mark.parametrize("with_bn", [False, True])
def test_general_form_agrees_with_the_staged_form_at_a_tile_shape(hip_device, with_bn):
    """The new entry called directly at (64, 6, 16, 128, 300), a shape the staged form serves: two
    fixed orders of the same terms (rtol 1e-5, atol 1e-5 max, as staged against atomic)."""
    k, segs, g, c = 64, 6, 16, 128
    hip = _hip(hip_device)
    gen, b, m, n, idx, w, rel = _blend_case(k, segs, g, c, 11)
    dy = torch.randn(b, segs, c, k * g, generator=gen).to(hip_device)
    idx, w, rel = idx.to(hip_device), w.to(hip_device), rel.to(hip_device)
    kw = {}
    if with_bn:
        z = torch.randn(b, segs, c, k * g, generator=gen).to(hip_device)
        bnb = torch.randn(segs * c, 8, generator=gen).to(hip_device)
        kw = dict(bn_z=z, bnb=bnb)
    assert kernels.blend_backward_form(c, n // segs, m, True) == 'staged'
    res = []
    prev = hip.set_deterministic(True)
    try:
        for fn in (hip.blend_conv_backward, hip.blend_conv_backward_any):
            d_table = torch.full((b, m, segs * c), float('nan'), device=hip_device)
            d_wx = torch.full((segs, c, 3), float('nan'), device=hip_device)
            fn(dy, c, idx, w, rel, d_table, d_wx, segs, g, **kw)
            res.append((d_table, d_wx))
    finally:
        hip.set_deterministic(prev)
    (t0, x0), (t1, x1) = res
    torch.testing.assert_close(t1, t0, rtol=1e-5, atol=1e-5 * float(t0.abs().max()))
    torch.testing.assert_close(x1, x0, rtol=1e-5, atol=1e-5 * float(x0.abs().max()))


# Generator seed per seed count.  The two legs form the second norm's input with different
# roundings (see the test this repeats), so of the ~3 M normalised activations a few may sit on a
# ReLU knife-edge and flip between the legs; one flip changes a whole 256-channel row of da0 and, over
# M >= 2048 seeds with 1.5 taps per (seed, face), stands out of a table gradient row.  The seeds are
# chosen off such ties, as that test's own seed is; the kernel itself is within 2e-7 max|want| of
# a float64 scatter of the folded expression at these seed counts.
_FOLD_SEEDS = {2048: 22, 2100: 24}


def _fold_case(dev, M, gseed):
    """-> (want, got, calls): the module-by-module leg, the fused leg, and whether each call of the
    general form came with the norm fold."""
    from nesie_amd.mmdet3d_ops import fused_mlp
    from nesie_amd.votenet.side_pooling import DeferredBlendConv, MiniPointNet, grouped_mini_pointnets
    S, G = 6, 16
    torch.manual_seed(2)
    nets = [MiniPointNet(259, 128).to(dev) for _ in range(S)]
    with torch.no_grad():
        for n in nets:
            for m in n.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.uniform_(-1.0, 1.5)
                    m.bias.normal_(0, 0.3)
    B, H, K = 2, 256, 64
    g = torch.Generator(device=dev).manual_seed(gseed)
    table0 = torch.randn(B, M, S * H, device=dev, generator=g) * 0.5
    wx0 = torch.randn(S, H, 3, device=dev, generator=g)
    n = K * S * G
    idx = torch.randint(0, M, (B, n, 3), device=dev, generator=g, dtype=torch.int32)
    w = torch.rand(B, n, 3, device=dev, generator=g) + 0.05
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    rel = torch.randn(B, n, 3, device=dev, generator=g) * 0.3
    pick = torch.linspace(-1, 1, B * S * 128 * K, device=dev)
    calls = []
    real = kernels.HipKernels.blend_conv_backward_any

    def spy(self_, *a, **kw):
        calls.append(kw.get('bn_z') is not None and kw.get('bnb') is not None)
        return real(self_, *a, **kw)

    def run(fused):
        local = copy.deepcopy(nets)
        params = [p_ for net in local for p_ in net.parameters()]
        table, wx = table0.clone().requires_grad_(True), wx0.clone().requires_grad_(True)
        d = DeferredBlendConv(table, wx, idx, w, rel, S, G, K)
        fused_mlp.ENABLED = fused
        try:
            if fused:
                assert d.has_stats
                out = grouped_mini_pointnets(local, d)
            else:
                c0, stats = d.materialize()
                out = grouped_mini_pointnets(local, c0, c0_stats=stats)
            (out * pick.view_as(out)).sum().backward()
        finally:
            fused_mlp.ENABLED = True
        stats_ = [b_.clone() for net in local for b_ in net.buffers()]
        return out.detach(), table.grad, wx.grad, [None if p_.grad is None else p_.grad.clone() for p_ in params], stats_

    kernels.HipKernels.blend_conv_backward_any = spy
    try:
        want = run(False)
        got = run(True)
    finally:
        kernels.HipKernels.blend_conv_backward_any = real
    return want, got, calls


def _fold_check(want, got):
    torch.testing.assert_close(got[0], want[0], rtol=1e-4, atol=1e-4)
    for a, b in ((got[1], want[1]), (got[2], want[2])):   # (two fp32 orders of the same sums)
        torch.testing.assert_close(a, b, rtol=1e-3, atol=6e-4 * b.abs().max().item())
    scale = max(b.abs().max().item() for b in want[3] if b is not None)
    kinks = 0
    for a, b in zip(got[3], want[3]):
        assert (a is None) == (b is None)
        if a is not None:
            # (ReLU knife-edges: see the test this one repeats)
            tol = 1e-3 * b.abs() + 3e-4 * max(b.abs().max().item(), 1e-2 * scale)
            off = (a - b).abs() > tol
            assert int(off.sum()) <= 3 and float((a - b).abs().max()) <= 0.15 * scale, \
                (int(off.sum()), float((a - b).abs().max()), scale)
            kinks += int(off.sum())
    assert kinks <= 6, kinks
    for a, b in zip(got[4], want[4]):
        torch.testing.assert_close(a.float(), b.float(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('M', [2048, 2100])
def test_deferred_blend_into_fused_mini_pointnets_over_many_seeds(hip_device, M):
    """tests/test_pwconv_gpu.test_deferred_blend_into_fused_mini_pointnets, case (S, G) = (6, 16),
    B = 2, H = 256, K = 64, over 2048 and 2100 seeds, with its tolerances: BlendMiniHeadFn hands the
    norm backward to the general form."""
    want, got, calls = _fold_case(hip_device, M, _FOLD_SEEDS[M])
    # the materialised BlendConv of the first leg: plain backward; the fused node: with the fold
    assert calls == [False, True], calls
    _fold_check(want, got)


def test_no_queries_write_zeros(hip_device):
    hip = _hip(hip_device)
    b, m, segs, c, g = 2, 37, 6, 19, 9
    d_table = torch.full((b, m, segs * c), float('nan'), device=hip_device)
    d_wx = torch.full((segs, c, 3), float('nan'), device=hip_device)
    dy = torch.empty(b, segs, c, 0, device=hip_device)
    idx = torch.empty(b, 0, 3, dtype=torch.int32, device=hip_device)
    w = torch.empty(b, 0, 3, device=hip_device)
    hip.blend_conv_backward(dy, c, idx, w, w.clone(), d_table, d_wx, segs, g)
    assert float(d_table.abs().max()) == 0.0 and float(d_wx.abs().max()) == 0.0


def test_general_blend_backward_captures_into_a_graph(hip_device):
    """BlendConv forward + backward at (24, 6, 27, 128, 300) under torch.cuda.graph: two replays equal
    the eager bits, and a replay over new inputs in the captured buffers equals their eager result."""
    k, segs, g, c = 24, 6, 27, 128
    gen, b, m, n, idx, w, rel = _blend_case(k, segs, g, c, 5)
    table = torch.randn(b, m, segs * c, generator=gen).to(hip_device)
    wx = torch.randn(segs, c, 3, generator=gen).to(hip_device)
    go = torch.randn(b, segs, c, k * g, generator=gen).to(hip_device)
    idx, w, rel = idx.to(hip_device), w.to(hip_device), rel.to(hip_device)
    _, _, _, _, idx2, w2, rel2 = _blend_case(k, segs, g, c, 6)
    idx2, w2, rel2 = idx2.to(hip_device), w2.to(hip_device), rel2.to(hip_device)

    def step(t, x, i, ww, r, gout):
        t.grad = x.grad = None
        out = ops.blend_conv(t, x, i, ww, r, segs, g)
        out.backward(gout)
        return out.detach(), t.grad, x.grad

    t_e, x_e = table.clone().requires_grad_(True), wx.clone().requires_grad_(True)
    eager = [v.clone() for v in step(t_e, x_e, idx, w, rel, go)]
    t_o, x_o = table.flip(0).clone().requires_grad_(True), wx.clone().requires_grad_(True)
    other = [v.clone() for v in step(t_o, x_o, idx2, w2, rel2, go.flip(0).contiguous())]
    s_t, s_x = table.clone().requires_grad_(True), wx.clone().requires_grad_(True)
    s_idx, s_w, s_rel, s_go = idx.clone(), w.clone(), rel.clone(), go.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up off the default stream, as torch asks
        step(s_t, s_x, s_idx, s_w, s_rel, s_go)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    s_t.grad = s_x.grad = None
    with torch.cuda.graph(graph):
        out = ops.blend_conv(s_t, s_x, s_idx, s_w, s_rel, segs, g)
        out.backward(s_go)
    outs = (out, s_t.grad, s_x.grad)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got.detach(), want)
    with torch.no_grad():
        s_t.copy_(table.flip(0)); s_idx.copy_(idx2); s_w.copy_(w2); s_rel.copy_(rel2)
        s_go.copy_(go.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, other):
        assert torch.equal(got.detach(), want)


def _train_cfg(cfg):
    cfg['train_cfg'].update(pos_distance_thr=1.0, neg_distance_thr=1.5)   # positives at random init
    return cfg


def test_saqe_head_with_24_proposals_trains_a_step(hip_device, monkeypatch):
    """2 K 27 = 1296 queries per face in the SAQE box grid: no whole 64-query tiles."""
    from nesie_amd.votenet import build_nesie_votenet
    from nesie_amd.votenet.detector import saqe_votenet_scannet_cfg
    spy = _Spy(monkeypatch)
    pts, boxes, labels = _small.small_batch(batch=2)
    pts = pts.to(hip_device)
    cfg = _small.small_cfg()
    scfg = saqe_votenet_scannet_cfg()
    cfg['bbox_head'].update(angle_loss=scfg['bbox_head']['angle_loss'],
                            angle_pred_loss=scfg['bbox_head']['angle_pred_loss'])
    cfg['head_type'] = 'SAQEHead'
    cfg['bbox_head']['vote_aggregation_cfg'].update(num_point=24)
    cfg['bbox_head']['grid_conv_cfg'].update(num_proposal=24)
    _train_cfg(cfg)
    torch.manual_seed(0)
    model = build_nesie_votenet(cfg).to(hip_device).train()
    head = model.bbox_head
    assert type(head).__name__ == 'SAQEHead'
    head.jitter_noise = tuple(t.to(hip_device) for t in _small.fixed_noise(2, 24))
    losses, grads = _small.train_step_losses(model, pts, boxes, labels)
    for name, v in losses.items():
        assert torch.isfinite(v).all(), name
    for name, gr in grads.items():
        assert torch.isfinite(gr).all(), name
    nets = len(head.grid_conv.mlps_before)
    assert nets == 6                 # (the SAQE variant has the six face nets and no box-grid net)
    for i in range(nets):
        name = f'bbox_head.grid_conv.mlps_before.{i}.first_conv.0.weight'
        assert name in grads and float(grads[name].abs().max()) > 0, name
    assert spy.calls, 'the general blend backward did not run'


def test_nesie_head_over_2048_seeds_is_bitwise_reproducible(hip_device, monkeypatch):
    """A backbone whose second level keeps 2048 seeds (one more than the staged index takes): two
    steps from identically seeded models give the same bits in every loss term and gradient."""
    from nesie_amd.mmdet3d_ops import fused_mlp
    from nesie_amd.votenet import build_nesie_votenet
    assert kernels.HipKernels.DETERMINISTIC
    spy = _Spy(monkeypatch)
    heads = []
    real = fused_mlp.BlendMiniHeadFn.forward

    def fwd(*a, **kw):
        heads.append(True)
        return real(*a, **kw)
    monkeypatch.setattr(fused_mlp.BlendMiniHeadFn, 'forward', staticmethod(fwd))
    pts, boxes, labels = _small.small_batch(batch=2, n=8192)
    pts = pts.to(hip_device)
    cfg = _small.small_cfg()
    cfg['backbone'].update(num_points=(4096, 2048, 256, 128), num_samples=(16, 16, 8, 8))
    _train_cfg(cfg)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = build_nesie_votenet(cfg).to(hip_device).train()
        assert type(model.bbox_head).__name__ == 'NesieHead'
        model.bbox_head.jitter_noise = tuple(t.to(hip_device) for t in _small.fixed_noise(2, 32))
        runs.append(_small.train_step_losses(model, pts, boxes, labels))
    (l0, g0), (l1, g1) = runs
    assert heads, 'BlendMiniHeadFn did not run'
    assert spy.calls and any(spy.calls), 'the general form did not run with the norm fold'
    assert set(l0) == set(l1) and set(g0) == set(g1) and g0
    for name in l0:
        assert torch.isfinite(l0[name]).all(), name
        assert torch.equal(l0[name], l1[name]), name
    for name in g0:
        assert torch.isfinite(g0[name]).all(), name
        assert torch.equal(g0[name], g1[name]), name
