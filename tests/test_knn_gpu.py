"""kNN grouping on the GPU: the kernel against the numpy referee bit for bit (tests/_knn_ref.py),
the ``knn`` op, ``QueryAndGroup(max_radius=None)`` against the literal composition,
``uniform_sample`` and a kNN set-abstraction level."""
import numpy as np
import pytest
import torch

from tests import _knn_ref, _np_ref

pytestmark = pytest.mark.gpu


def _hip():
    from nesie_amd.kernels import HipKernels
    return HipKernels()


def _uniform(seed, b, n, m):
    rng = np.random.default_rng(seed)
    return (rng.random((b, n, 3)) * [4.0, 4.0, 2.5]).astype(np.float32), \
        (rng.random((b, m, 3)) * [4.0, 4.0, 2.5]).astype(np.float32)


def _lattice(seed, b, n, m):
    """Coordinates from a 4 x 4 x 4 integer lattice: hundreds of exactly equal distances per
    centre and many points on the centre itself."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, (b, n, 3)).astype(np.float32), \
        rng.integers(0, 4, (b, m, 3)).astype(np.float32)


def _self(seed, b, n, m):
    assert n == m
    xyz = _uniform(seed, b, n, m)[0]
    return xyz, xyz.copy()


def _run_kernel(dev, xyz, centres, k):
    b, n = xyz.shape[:2]
    m = centres.shape[1]
    p, c = torch.from_numpy(xyz).to(dev), torch.from_numpy(centres).to(dev)
    # start from values the kernel must overwrite
    idx = torch.full((b, m, k), -7, dtype=torch.int32, device=dev)
    dist2 = torch.full((b, m, k), -1.0, dtype=torch.float32, device=dev)
    _hip().knn_wrapper(b, n, m, k, p, c, idx, dist2)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist2.cpu().numpy()


def _check_against_referee(dev, xyz, centres, k):
    got_idx, got_d = _run_kernel(dev, xyz, centres, k)
    want_idx, want_d = _knn_ref.knn_batch(centres, xyz, k)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)), "dist2 differs"
    assert np.array_equal(got_idx, want_idx), "idx differs"
    return got_idx, got_d


CASES = [
    (2, 64, 16, 1, _uniform),         # one tile, k = 1
    (1, 100, 7, 16, _uniform),        # n not a multiple of 64
    (2, 257, 33, 64, _uniform),       # one point past a 64-point step, the full one-key-per-lane list
    (1, 300, 20, 65, _uniform),       # first size of the two-keys-per-lane instantiation
    (1, 1000, 50, 100, _uniform),     # the reference's own maximum
    (1, 500, 9, 128, _uniform),       # our maximum
    (1, 10, 4, 16, _uniform),         # n < k: padding index 0, distance 1e10
    (2, 512, 64, 32, _lattice),       # exact ties: the (distance, index) rule
    (1, 2048, 2048, 16, _self),       # centres = the points: self first at distance 0
    (8, 4096, 256, 32, _uniform),     # several scenes and several LDS tiles, batch stride
    (1, 1025, 5, 64, _uniform),       # one point past an LDS tile
    (2, 70, 3, 128, _uniform),        # n < k in the two-keys-per-lane instantiation
]


@pytest.mark.parametrize('b,n,m,k,make', CASES,
                         ids=[f'{b}x{n}x{m}_k{k}_{f.__name__[1:]}' for b, n, m, k, f in CASES])
def test_kernel_matches_the_referee_bit_for_bit(hip_device, b, n, m, k, make):
    xyz, centres = make(1000 + n + k, b, n, m)
    idx, d = _check_against_referee(hip_device, xyz, centres, k)
    if n < k:
        assert (idx[..., n:] == 0).all() and (d[..., n:] == np.float32(1e10)).all()
    if make is _self:
        assert np.array_equal(idx[0, :, 0], np.arange(n)) and (d[..., 0] == 0).all()
    if make is _lattice:    # the case is about ties: make sure it has them
        assert (d[..., 1:] == d[..., :-1]).sum() > 100 * b


@pytest.mark.parametrize('form', [1, 2])
def test_distance_forms(hip_device, form):
    hip = _hip()
    try:
        hip.set_distance_form(form)
        _np_ref.FORM = form
        assert hip.get_distance_form() == form
        _check_against_referee(hip_device, *_lattice(1544, 2, 512, 64), 32)
        _check_against_referee(hip_device, *_uniform(1321, 2, 257, 33), 64)
    finally:
        hip.set_distance_form(0)
        _np_ref.FORM = 0
    assert hip.get_distance_form() == 0


def test_no_points_fills_the_padding(hip_device):
    idx, d = _run_kernel(hip_device, np.zeros((2, 0, 3), np.float32), _uniform(5, 2, 8, 6)[1], 5)
    assert (idx == 0).all() and (d == np.float32(1e10)).all()


def test_knn_op(hip_device):
    from nesie_amd.mmdet3d_ops import knn
    xyz_np, cen_np = _uniform(77, 2, 300, 40)
    xyz, cen = torch.from_numpy(xyz_np).to(hip_device), torch.from_numpy(cen_np).to(hip_device)
    k_idx, k_d = _run_kernel(hip_device, xyz_np, cen_np, 12)
    idx = knn(12, xyz.clone().requires_grad_(True), cen)
    assert idx.shape == (2, 12, 40) and idx.dtype == torch.int32 and not idx.requires_grad
    assert idx.is_contiguous()
    assert np.array_equal(idx.cpu().numpy(), k_idx.transpose(0, 2, 1))
    assert torch.equal(knn(12, xyz.transpose(1, 2).contiguous(), cen.transpose(1, 2).contiguous(),
                           True), idx)
    assert torch.equal(knn(12, xyz), knn(12, xyz, xyz))
    assert knn(12, xyz).shape == (2, 12, 300)
    idx2, d2 = knn(12, xyz.clone().requires_grad_(True), cen, False, True)
    assert torch.equal(idx2, idx) and not d2.requires_grad and d2.dtype == torch.float32
    assert np.array_equal(d2.cpu().numpy(), k_d.transpose(0, 2, 1))
    with pytest.raises(RuntimeError, match="unsupported|knn_wrapper"):
        knn(129, xyz)


def _group_inputs(dev, b=2, n=512, m=64, c=8, seed=9):
    g = torch.Generator(device=dev).manual_seed(seed)
    xyz = torch.rand(b, n, 3, device=dev, generator=g)
    centres = xyz[:, torch.randperm(n, device=dev, generator=g)[:m]].contiguous()
    feats = torch.randn(b, c, n, device=dev, generator=g)
    return xyz, centres, feats


def _literal(xyz, centres, feats, k):
    from nesie_amd.mmdet3d_ops import grouping_operation, knn
    idx = knn(k, xyz, centres, False).transpose(1, 2).contiguous()
    grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx)
    grouped_xyz = grouped_xyz - centres.transpose(1, 2).unsqueeze(-1)
    return torch.cat([grouped_xyz, grouping_operation(feats, idx)], dim=1), grouped_xyz, idx


def test_query_and_group_knn_equals_the_literal_composition(hip_device):
    from nesie_amd.mmdet3d_ops import QueryAndGroup
    hip = _hip()
    xyz, centres, feats = _group_inputs(hip_device)
    grouper = QueryAndGroup(None, 16)
    prev = hip.set_deterministic(True)
    try:
        want_f = feats.clone().requires_grad_(True)
        want, want_xyz, want_idx = _literal(xyz, centres, want_f, 16)
        grad_out = torch.randn(want.shape, device=hip_device,
                               generator=torch.Generator(device=hip_device).manual_seed(4))
        want.backward(grad_out)
        grads = []
        for _ in range(2):
            f = feats.clone().requires_grad_(True)
            out = grouper(xyz, centres, f)
            assert out.shape == (2, 3 + 8, 64, 16) and torch.equal(out, want)
            out.backward(grad_out)
            grads.append(f.grad)
        assert torch.equal(grads[0], want_f.grad) and torch.equal(grads[0], grads[1])
    finally:
        hip.set_deterministic(prev)
    assert torch.equal(grouper.ball_indices(xyz, centres), want_idx)
    # the self-neighbour comes first: every centre is one of the points
    assert (want_xyz[:, :, :, 0] == 0).all()
    # min_radius is ignored in kNN mode
    assert torch.equal(QueryAndGroup(None, 16, min_radius=0.3)(xyz, centres, feats), want)

    out, gxyz = QueryAndGroup(None, 16, return_grouped_xyz=True)(xyz, centres, feats)
    assert torch.equal(out, want) and torch.equal(gxyz, want_xyz)
    out, gidx = QueryAndGroup(None, 16, return_grouped_idx=True)(xyz, centres, feats)
    assert torch.equal(out, want) and torch.equal(gidx, want_idx)
    out, gxyz, gidx = QueryAndGroup(None, 16, return_grouped_xyz=True,
                                    return_grouped_idx=True)(xyz, centres, feats)
    assert torch.equal(out, want) and torch.equal(gxyz, want_xyz) and torch.equal(gidx, want_idx)
    # coordinates that carry a gradient take the literal path and get one
    x = xyz.clone().requires_grad_(True)
    out = grouper(x, centres, feats)
    assert torch.equal(out, want)
    out.sum().backward()
    assert x.grad is not None and x.grad.shape == xyz.shape


def test_uniform_sample_rows_and_unique_count(hip_device):
    from nesie_amd.mmdet3d_ops import QueryAndGroup, ball_query, grouping_operation
    xyz, centres, feats = _group_inputs(hip_device, seed=21)
    raw = ball_query(0, 0.12, 16, xyz, centres)        # small radius: rows hold repeats
    grouper = QueryAndGroup(0.12, 16, uniform_sample=True, return_unique_cnt=True,
                            return_grouped_xyz=True, return_grouped_idx=True)
    grouper.generator = torch.Generator(device=hip_device).manual_seed(5)
    out, gxyz, cnt, idx = grouper(xyz, centres, feats)
    assert cnt.shape == (2, 64) and cnt.dtype == torch.float32
    assert idx.shape == raw.shape and idx.dtype == torch.int32
    raw_c, idx_c, cnt_c = raw.cpu(), idx.cpu(), cnt.cpu()
    assert (cnt_c < 16).any() and (cnt_c > 1).any()    # the case has rows with repeats
    for r_in, r_out, c in zip(raw_c.reshape(-1, 16), idx_c.reshape(-1, 16), cnt_c.reshape(-1)):
        distinct = torch.unique(r_in)
        assert float(c) == distinct.numel()
        assert torch.equal(r_out[:distinct.numel()], distinct)
        assert torch.isin(r_out[distinct.numel():], distinct).all()
    # the literal grouping over the resampled indices
    want_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) \
        - centres.transpose(1, 2).unsqueeze(-1)
    assert torch.equal(gxyz, want_xyz)
    assert torch.equal(out, torch.cat([want_xyz, grouping_operation(feats, idx)], dim=1))
    # the same seed gives the same rows
    grouper.generator = torch.Generator(device=hip_device).manual_seed(5)
    assert torch.equal(grouper(xyz, centres, feats)[3], idx)


def _knn_sa(dev, widths):
    from nesie_amd.mmdet3d_ops import PointSAModule
    torch.manual_seed(0)
    sa = PointSAModule(num_point=64, radius=None, num_sample=16, mlp_channels=widths).to(dev)
    with torch.no_grad():
        for mod in sa.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0, 0.3)
    return sa


@pytest.mark.parametrize('widths,stacked', [([8, 16, 16, 32], False), ([8, 64, 64, 128], True)])
def test_knn_sa_module_against_a_plain_torch_composition(hip_device, monkeypatch, widths, stacked):
    """``stacked``: the widths are ones the fused SA stacks (training and evaluation) serve: their
    pooling epilogue is built for whole row tiles, not for a 32-channel last layer."""
    from nesie_amd.mmdet3d_ops import fused_mlp
    sa = _knn_sa(hip_device, widths)
    xyz, _, feats = _group_inputs(hip_device, seed=33)

    decided, served = [], []
    supported, stack = fused_mlp.sa_stack_supported, fused_mlp.sa_stack
    monkeypatch.setattr(fused_mlp, 'sa_stack_supported',
                        lambda *a: decided.append(supported(*a)) or decided[-1])
    monkeypatch.setattr(fused_mlp, 'sa_stack', lambda *a: served.append(1) or stack(*a))

    def run(**kw):
        for p in sa.parameters():
            p.grad = None
        f = feats.clone().requires_grad_(True)
        new_xyz, out, indices = sa(xyz, f, **kw)
        (out * torch.linspace(-1, 1, out.numel(), device=hip_device).view_as(out)).sum().backward()
        return new_xyz, out.detach(), indices, f.grad, [p.grad.clone() for p in sa.parameters()]

    got = run()
    assert got[1].shape == (2, widths[-1], 64) and got[0].shape == (2, 64, 3)
    # a kNN level goes through the fused stack whenever the stack serves its shapes
    assert len(served) == sum(decided) == int(stacked)
    pre = sa.sample_and_group_indices(xyz)
    assert pre['group_idx'][0].shape == (2, 64, 16)
    again = run(precomputed=pre)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    assert torch.equal(again[2], got[2])

    # plain torch over the same kNN indices and the same weights
    idx = pre['group_idx'][0].long()
    layers = []
    for layer in sa.mlps[0]:
        conv = torch.nn.Conv2d(layer.conv.in_channels, layer.conv.out_channels, 1, bias=False)
        bn = torch.nn.BatchNorm2d(layer.conv.out_channels)
        conv.weight.data.copy_(layer.conv.weight.data.view_as(conv.weight))
        bn.weight.data.copy_(layer.norm.weight.data)
        bn.bias.data.copy_(layer.norm.bias.data)
        layers += [conv, bn, torch.nn.ReLU()]
    plain = torch.nn.Sequential(*layers).to(hip_device).train()
    f = feats.clone().requires_grad_(True)
    b, m, k = idx.shape
    flat = idx.reshape(b, 1, m * k)
    grouped_xyz = torch.gather(xyz.transpose(1, 2), 2, flat.expand(-1, 3, -1)).view(b, 3, m, k) \
        - pre['new_xyz'].transpose(1, 2).unsqueeze(-1)
    grouped_f = torch.gather(f, 2, flat.expand(-1, f.shape[1], -1)).view(b, -1, m, k)
    want = plain(torch.cat([grouped_xyz, grouped_f], dim=1)).max(dim=3)[0]
    (want * torch.linspace(-1, 1, want.numel(), device=hip_device).view_as(want)).sum().backward()
    want_params = [p.grad for p in plain.parameters()]
    assert len(want_params) == len(got[4])
    # the tolerances of test_pwconv_gpu.test_fused_sa_stack_matches_the_module_by_module_path
    torch.testing.assert_close(got[1], want.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(got[3], f.grad, rtol=1e-3, atol=1e-4 * f.grad.abs().max().item())
    for a, w in zip(got[4], want_params):
        torch.testing.assert_close(a, w.view_as(a), rtol=1e-3,
                                   atol=2e-4 * max(w.abs().max().item(), 1e-3))

    # evaluation mode without autograd: the running statistics, through sa_stack_eval where its
    # pooled tail is built for the widths and module by module otherwise (the tolerance of
    # test_pwconv_gpu.test_eval_mode_sa_stack_matches_the_module_by_module_path)
    for layer, bn in zip(sa.mlps[0], [mod for mod in plain if isinstance(mod, torch.nn.BatchNorm2d)]):
        bn.running_mean.copy_(layer.norm.running_mean)
        bn.running_var.copy_(layer.norm.running_var)
    eval_decided, eval_supported = [], fused_mlp.sa_stack_eval_supported
    monkeypatch.setattr(fused_mlp, 'sa_stack_eval_supported',
                        lambda *a: eval_decided.append(eval_supported(*a)) or eval_decided[-1])
    sa.eval(), plain.eval()
    with torch.no_grad():
        got_eval = sa(xyz, feats, precomputed=pre)[1]
        want_eval = plain(torch.cat([grouped_xyz, grouped_f], dim=1)).max(dim=3)[0]
    assert eval_decided == [stacked]
    torch.testing.assert_close(got_eval, want_eval, rtol=1e-4, atol=1e-4)
