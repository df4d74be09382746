"""Backward of the MiniPointNet tail (conv4 256 -> 128 pooled directly over G samples,
side_pooling_module.py:343-370) from the max-pool's ENTRIES instead of the dense gradient of conv4's
output: nesie_pool_tail_pack, nesie_pw_dgrad_bn_reduce_sparse (bit for bit the dense launch) and
nesie_pw_wgrad_sparse (a sparse product on the vector ALUs that leaves the dense launch's partials: against
float64, and bit for bit the dense weight gradient).

Measured on MI355X: the relative L2 error of dW4 against float64 is the dense kernel's to the last digit
(4.45e-8 ... 1.12e-7 over the eight shapes), the results being bit-equal.
The whole MiniPointNet chain on this route against float64 autograd is in tests/test_fused_chains_fp64_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, H2 = 128, 256

# (nb, ng, G, P, CU budget | None)
# The library sizes its grids for multiples of 8 CUs, 8 at the least (nesie_set_cu_count): a budget of
# 8 gives ONE workgroup per net in both launches here -- what any smaller budget would give too -- so a
# workgroup walks every tile of its net, across batch elements.  40 CUs: six workgroups per net over 16
# tiles per batch element (tiles_per_batch does not divide the stride of a workgroup's walk).
SHAPES = [
    (12, 6, 16, 1024, None),   # the fused-MiniPointNet test's size, six nets
    (2, 1, 64, 4096, None),    # the box grid's group size
    (6, 6, 16, 64, None),      # one tile per element, fewer tiles than workgroups
    (12, 6, 16, 1024, 8),      # several tiles per workgroup, runs crossing batch elements
    (12, 6, 16, 1024, 40),
]
# the weight gradient also where a net has more than 1024 32-position tiles: plain (not tiled) partials
WGRAD_SHAPES = SHAPES + [
    (2, 1, 16, 32768, None),
    (2, 1, 64, 32768, 16),     # groups of 64: half a group per tile; 16 workgroups over 2048 tiles
    (6, 6, 16, 36864, None),   # six nets
]
IDS = ['%dx%d_G%d_P%d_cu%s' % s for s in SHAPES]
WGRAD_IDS = ['%dx%d_G%d_P%d_cu%s' % s for s in WGRAD_SHAPES]


def _dev():
    return torch.device('cuda:0')


def _hip():
    from nesie_amd import kernels
    return kernels.backend_for(torch.zeros(1, device=_dev()))


def _budget(cu):
    import contextlib
    from nesie_amd.kernels import HipKernels
    return HipKernels.cu_budget(cu) if cu else contextlib.nullcontext()


def _inputs(nb, ng, G, P):
    """Pooled gradient with exact zeros and negative values, arg-max positions that include 0 and
    G - 1, one group in which all 128 channels name the same position; y, its folded norm, W4."""
    g = torch.Generator(device=_dev()).manual_seed(1000 * nb + 10 * G + ng)
    M = P // G
    dout = torch.randn(nb, F, M, device=_dev(), generator=g)
    dout[torch.rand(nb, F, M, device=_dev(), generator=g) < 0.1] = 0.0
    arg = torch.randint(0, G, (nb, F, M), device=_dev(), generator=g).to(torch.uint8)
    arg[0, :F // 2, 0] = 0
    arg[0, F // 2:, 0] = G - 1
    arg[nb - 1, :, M - 1] = 3          # every channel of this group at one position
    arg[nb - 1, 0, 0] = G - 1
    assert (dout == 0).any() and (dout < 0).any() and (arg == 0).any() and (arg == G - 1).any()
    y = torch.randn(nb, H2, P, device=_dev(), generator=g)
    coef = torch.empty(ng * H2, 4, device=_dev())
    coef[:, 0] = torch.rand(ng * H2, device=_dev(), generator=g) * 2.5 - 1.0     # scale, either sign
    coef[:, 1] = torch.randn(ng * H2, device=_dev(), generator=g) * 0.3
    coef[:, 2] = torch.randn(ng * H2, device=_dev(), generator=g) * 0.1
    coef[:, 3] = torch.rand(ng * H2, device=_dev(), generator=g) + 0.5
    w4 = torch.randn(ng, F, H2, device=_dev(), generator=g) / 16
    return dout, arg, y, coef, w4


def _dense_dz(hip, dout, arg, G):
    nb, _, M = dout.shape
    dz = torch.empty(nb, F, M, G, device=_dev())
    hip.group_max_pool_backward(dout, arg, dz)
    return dz.view(nb, F, M * G)


def _both_dgrads(hip, nb, ng, G, P):
    dout, arg, y, coef, w4 = _inputs(nb, ng, G, P)
    dz = _dense_dz(hip, dout, arg, G)
    da_d = torch.empty(nb, H2, P, device=_dev())
    part_d = hip.pw_dgrad_bn_reduce(dz, w4.transpose(1, 2), y, coef, da_d, ng=ng)
    ent = hip.pool_tail_pack(dout, arg)
    da_s = torch.full((nb, H2, P), float('nan'), device=_dev())
    part_s = hip.pw_dgrad_bn_reduce_sparse(ent, G, w4.transpose(1, 2), y, coef, da_s, ng=ng)
    torch.cuda.synchronize()
    return da_d, part_d, da_s, part_s


@pytest.mark.parametrize('nb,ng,G,P,cu', SHAPES, ids=IDS)
def test_sparse_input_gradient_is_the_dense_launch_bit_for_bit(nb, ng, G, P, cu):
    hip = _hip()
    with _budget(cu):
        da_d, part_d, da_s, part_s = _both_dgrads(hip, nb, ng, G, P)
    assert da_d.abs().max().item() > 0
    assert part_s.shape == part_d.shape
    assert torch.equal(da_s, da_d)
    assert torch.equal(part_s, part_d)


def _child_mirrored():
    """(runs in a child process started with NESIE_PW_REV_MB=1: both launches walk their tiles mirrored)"""
    hip = _hip()
    da_d, part_d, da_s, part_s = _both_dgrads(hip, 12, 6, 16, 1024)
    assert 12 * F * 1024 * 4 >= 1000000
    ok = torch.equal(da_s, da_d) and torch.equal(part_s, part_d) and da_d.abs().max().item() > 0
    # ... and the weight gradient, whose walk follows the same threshold
    from nesie_amd.mmdet3d_ops import fused_mlp
    dout, arg, y, coef, w4 = _inputs(12, 6, 16, 1024)
    dense = fused_mlp._wgrad(hip, _dense_dz(hip, dout, arg, 16), y, coef, ng=6)
    new = torch.full((6, F, H2), float('nan'), device=_dev())
    hip.pw_wgrad_sparse(hip.pool_tail_pack(dout, arg), 16, y, new, ng=6, x_coef=coef)
    ok = ok and torch.equal(new, dense.view(6, F, H2))
    print('MIRRORED_EQUAL' if ok else 'MIRRORED_DIFFER')


def test_sparse_input_gradient_mirrored_walk_in_a_fresh_process():
    """The walk direction is read once at library load: a fresh child with a 1 MB threshold runs the
    dense launch mirrored, and the sparse one must follow the size of the dense tensor it replaces."""
    env = dict(os.environ, NESIE_PW_REV_MB='1')
    r = subprocess.run([sys.executable, '-c',
                        'import tests.test_mini_tail_sparse_gpu as t; t._child_mirrored()'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'MIRRORED_EQUAL' in r.stdout, r.stdout + r.stderr


def _rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize('nb,ng,G,P,cu', WGRAD_SHAPES, ids=WGRAD_IDS)
def test_sparse_weight_gradient_against_fp64(nb, ng, G, P, cu):
    from nesie_amd.mmdet3d_ops import fused_mlp
    hip = _hip()
    assert hip.pw_wgrad_sparse_supported(F, H2, P, G)
    dout, arg, y, coef, w4 = _inputs(nb, ng, G, P)
    dz = _dense_dz(hip, dout, arg, G)
    # reference: dz @ relu(coef1 . y)^T per net, float64 on the device
    c = coef.double().view(ng, H2, 4)
    ref = torch.stack([torch.einsum('ncp,nkp->ck', dz[g::ng].double(),
                                    (y[g::ng].double() * c[g, :, 0, None] + c[g, :, 1, None]).clamp_min(0))
                       for g in range(ng)])
    ent = hip.pool_tail_pack(dout, arg)
    with _budget(cu):
        dense = fused_mlp._wgrad(hip, dz, y, coef, ng=ng)
        new = torch.full((ng, F, H2), float('nan'), device=_dev())
        hip.pw_wgrad_sparse(ent, G, y, new, ng=ng, x_coef=coef)
        again = torch.full((ng, F, H2), float('nan'), device=_dev())
        hip.pw_wgrad_sparse(ent, G, y, again, ng=ng, x_coef=coef)
    torch.cuda.synchronize()
    e_new, e_dense = _rel_l2(new, ref), _rel_l2(dense.view(ng, F, H2), ref)
    print('mini tail dW4 (nb %d, ng %d, G %d, P %d, cu %s): relative L2 error new %.3e dense %.3e'
          % (nb, ng, G, P, cu, e_new, e_dense))
    assert ref.abs().max().item() > 0
    assert torch.equal(new, again)
    assert e_new <= 1.5 * e_dense
    # the same chain of fused multiply-adds per element as the MFMA form over the expanded tensor
    assert torch.equal(new, dense.view(ng, F, H2))
    torch.testing.assert_close(new.double(), ref, rtol=1e-3, atol=3e-4 * ref.abs().max().item())


@pytest.mark.parametrize('S,G', [(6, 16), (1, 64)])
def test_whole_mini_pointnet_backward_sparse_against_dense(S, G):
    from nesie_amd.mmdet3d_ops import fused_mlp
    from nesie_amd.votenet.side_pooling import MiniPointNet, grouped_mini_pointnets
    torch.manual_seed(1)
    nets = [MiniPointNet(259, 128).to(_dev()) for _ in range(S)]
    with torch.no_grad():
        for n in nets:
            for m in n.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.uniform_(-1.0, 1.5)
                    m.bias.normal_(0, 0.3)
    B, H, K = 2, 256, 64
    g = torch.Generator(device=_dev()).manual_seed(G)
    c0 = torch.randn(B, S, H, K, G, device=_dev(), generator=g)
    flat = c0.permute(1, 2, 0, 3, 4).reshape(S * H, B * K * G // 64, 64).double()
    part = torch.stack([flat.sum(-1), (flat ** 2).sum(-1)], -1).float().contiguous()
    params = [p_ for n in nets for p_ in n.parameters()]
    w4_ids = {id(n.second_conv[3].weight) for n in nets}
    real = fused_mlp.MiniTailFn.backward
    seen = []

    def spy(ctx, dout):
        out = real(ctx, dout)
        seen.append([None if t is None else t.detach().clone() for t in out])
        return out

    def run(sparse):
        fused_mlp.MINI_TAIL_SPARSE = sparse
        seen.clear()
        for p_ in params:
            p_.grad = None
        x = c0.clone().requires_grad_(True)
        out = grouped_mini_pointnets(nets, x, c0_stats=part)
        (out * torch.linspace(-1, 1, out.numel(), device=_dev()).view_as(out)).sum().backward()
        assert len(seen) == 1, 'the nets did not go through MiniTailFn'
        return out.detach(), x.grad.clone(), [None if p_.grad is None else p_.grad.clone() for p_ in params], list(seen[0])

    fused_mlp.MiniTailFn.backward = staticmethod(spy)
    try:
        assert fused_mlp.mini_tail_sparse_supported(_hip(), F, H2, G, K * G)
        want = run(False)
        got = run(True)
    finally:
        fused_mlp.MINI_TAIL_SPARSE = True
        fused_mlp.MiniTailFn.backward = staticmethod(real)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert want[1].abs().max().item() > 0
    # MiniTailFn.backward -> (dc, dsmall, -, -, dW_l, dgamma, dbeta, dW4)
    for j in (0, 1, 4, 5, 6):
        assert torch.equal(got[3][j], want[3][j]), j
    dw_new, dw_dense = got[3][7], want[3][7]
    assert torch.equal(dw_new, dw_dense)
    torch.testing.assert_close(dw_new, dw_dense, rtol=1e-3, atol=3e-4 * dw_dense.abs().max().item())
    checked = 0
    for p_, a, b in zip(params, got[2], want[2]):
        assert (a is None) == (b is None)
        if a is None:
            continue
        if id(p_) in w4_ids:
            torch.testing.assert_close(a, b, rtol=1e-3, atol=3e-4 * dw_dense.abs().max().item())
            checked += 1
        else:
            assert torch.equal(a, b)
    assert checked == S
