"""Kernel instantiations that a launcher selects from a runtime value (csrc/dispatch.h) and that no
other test launches: each at the smallest shape that selects it, against float64 at the tolerance
the op's other tests use.

* group_bwd_csr_rows_kernel<CH, EDIV>: CH = 8, 4, 2, 1 channel rows per workgroup (the largest that
  still leaves 256 workgroups: 2 scenes x 1024 / 512 / 256 / 9 channels), EDIV = 1 (grouped columns)
  and 3 (three weighted taps per column).
* group_bwd_lds_kernel<CH>: CH = 2, 4, 8 (b * c / 512, at most 8).
* blend_bwd_rows_kernel<CPT, BNB, STAGED>: c = 64 .. 256, with and without the norm backward on the
  tile load, staged and atomic form, one 64-query tile per face.
* the non-temporal (NT) forms of bn_apply / bn_bwd_reduce / bn_bwd_apply / affine_apply: tensors of
  192 MB, the size from which the norm passes stream (bn.hip, stream_nt)."""
import pytest
import torch

from nesie_amd import kernels

pytestmark = pytest.mark.gpu


def _hip(dev):
    return kernels.backend_for(torch.empty(1, device=dev))


# ---- group_bwd_csr_rows_kernel<CH, EDIV> ----------------------------------------------------------
@pytest.mark.parametrize("c", [1024, 512, 256, 9])      # CH = 8, 4, 2, 1
@pytest.mark.parametrize("ediv", [1, 3])
def test_csr_rows_for_every_rows_per_workgroup(hip_device, c, ediv):
    hip = _hip(hip_device)
    b, n, m, ns = 2, 37, 8, 6
    g = torch.Generator().manual_seed(c + ediv)
    idx = torch.randint(0, n - 5, (b, m, ns), generator=g).int()          # the last 5 points: no entry
    want = torch.zeros(b, c, n, dtype=torch.float64)
    gp = torch.full((b, c, n), float('nan'), device=hip_device)           # written in full
    if ediv == 1:
        go = torch.randn(b, c, m, ns, generator=g)
        order, sources = hip.inverted_index(idx.to(hip_device), n)
        hip.group_points_backward_csr(go.to(hip_device), order, sources, gp)
        want.scatter_add_(2, idx.view(b, 1, -1).expand(-1, c, -1).long(), go.reshape(b, c, -1).double())
    else:
        nq = m * ns // 3
        idx3 = idx.view(b, nq, 3).contiguous()
        w3 = torch.rand(b, nq, 3, generator=g)
        go = torch.randn(b, c, nq, generator=g)
        order, sources = hip.inverted_index(idx3.to(hip_device), n)
        hip.three_interpolate_grad_csr(go.to(hip_device), w3.to(hip_device), order, sources, gp)
        contrib = (go.double().unsqueeze(-1) * w3.double().unsqueeze(1)).reshape(b, c, -1)
        want.scatter_add_(2, idx3.view(b, 1, -1).expand(-1, c, -1).long(), contrib)
    err = (gp.cpu().double() - want).abs().max().item()
    assert err <= 2e-6 * want.abs().max().item(), err
    assert float(gp[:, :, n - 5:].abs().max()) == 0.0


# ---- group_bwd_lds_kernel<CH> ---------------------------------------------------------------------
@pytest.mark.parametrize("c", [512, 1024, 2048])        # CH = 2, 4, 8
def test_atomic_group_backward_for_every_rows_per_workgroup(hip_device, c):
    hip = _hip(hip_device)
    b, n, m, ns = 2, 8, 8, 4                                              # m * ns >= 4 n: the LDS form
    g = torch.Generator().manual_seed(c)
    idx = torch.randint(0, n, (b, m, ns), generator=g).int()
    go = torch.randn(b, c, m, ns, generator=g)
    gp = torch.zeros(b, c, n, device=hip_device)
    hip.group_points_backward(b, c, n, m, ns, go.to(hip_device), idx.to(hip_device), gp)
    want = torch.zeros(b, c, n, dtype=torch.float64)
    want.scatter_add_(2, idx.view(b, 1, -1).expand(-1, c, -1).long(), go.reshape(b, c, -1).double())
    err = (gp.cpu().double() - want).abs().max().item()
    assert err <= 2e-5 * want.abs().max().item(), err


# ---- blend_bwd_rows_kernel<CPT, BNB, STAGED> ------------------------------------------------------
@pytest.mark.parametrize("c", [64, 128, 192, 256])
@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("staged", [False, True])
def test_blend_backward_tile_forms_at_every_width(hip_device, c, with_bn, staged):
    """One 64-query tile per face.  float64 referee: dZ = a g + (e0 - (z - mean) d1) with
    g = dA [z scale + shift > 0] (the columns of bnb; z kept off the mask's edge), scattered through
    the taps; d_wx = sum dZ x rel."""
    hip = _hip(hip_device)
    b, m, k, segs, gq = 2, 40, 4, 2, 16
    n = k * segs * gq
    gen = torch.Generator().manual_seed(c + 2 * with_bn + staged)
    idx = torch.randint(0, m - 3, (b, n, 3), generator=gen, dtype=torch.int32)   # the last 3 seeds: no tap
    w = torch.rand(b, n, 3, generator=gen)
    rel = torch.randn(b, n, 3, generator=gen)
    dy = torch.randn(b, segs, c, k * gq, generator=gen)
    dz, kw = dy.double(), {}
    if with_bn:
        z = torch.randn(b, segs, c, k * gq, generator=gen)
        bnb = torch.randn(segs * c, 8, generator=gen)
        cf = bnb.double().view(1, segs, c, 8, 1)
        pre = z.double() * cf[..., 0, :] + cf[..., 1, :]
        z = torch.where(pre.abs() < 1e-3, z + 1.0, z)
        pre = z.double() * cf[..., 0, :] + cf[..., 1, :]
        assert float(pre.abs().min()) > 1e-5
        gmask = torch.where(pre > 0, dy.double(), torch.zeros((), dtype=torch.float64))
        dz = cf[..., 2, :] * gmask + ((cf[..., 3, :] - z.double()) * cf[..., 4, :] + cf[..., 5, :])
        kw = dict(bn_z=z.to(hip_device), bnb=bnb.to(hip_device))
    want = torch.zeros(b, m, segs, c, dtype=torch.float64)
    dzc = dz.view(b, segs, c, k, gq)
    idc = idx.long().view(b, k, segs, gq, 3)
    wc = w.double().view(b, k, segs, gq, 3)
    for bi in range(b):
        for s_ in range(segs):
            contrib = dzc[bi, s_].reshape(c, k * gq).t().unsqueeze(1) * wc[bi, :, s_].reshape(-1, 3).unsqueeze(-1)
            want[bi, :, s_].index_add_(0, idc[bi, :, s_].reshape(-1), contrib.reshape(-1, c))
    want_wx = torch.einsum('bsckg,bksgd->scd', dzc, rel.double().view(b, k, segs, gq, 3))
    assert kernels.blend_backward_form(c, n // segs, m, staged) == ('staged' if staged else 'atomic')
    prev = hip.set_deterministic(staged)
    try:
        # staged: written in full; atomic: added into a zeroed table
        d_table = torch.full((b, m, segs * c), float('nan') if staged else 0.0, device=hip_device)
        d_wx = torch.empty(segs, c, 3, device=hip_device)
        hip.blend_conv_backward(dy.to(hip_device), c, idx.to(hip_device), w.to(hip_device), rel.to(hip_device),
                                d_table, d_wx, segs, gq, **kw)
    finally:
        hip.set_deterministic(prev)
    err = (d_table.double().cpu().view(b, m, segs, c) - want).abs().max().item()
    assert err <= 3e-6 * want.abs().max().item(), err
    assert float(d_table[:, m - 3:].abs().max()) == 0.0
    torch.testing.assert_close(d_wx.double().cpu(), want_wx, rtol=1e-4, atol=2e-3)


# ---- the non-temporal norm passes -----------------------------------------------------------------
NT_SHAPE = (2, 24, 1 << 20)      # 2 * 24 * 2^20 floats = 192 MB exactly: the first size that streams


@pytest.mark.parametrize("relu", [True, False])
def test_norm_passes_at_the_streaming_size(hip_device, relu):
    """FusedBNReLU1d forward, backward and evaluation forward on 192 MB: bn_apply, bn_bwd_reduce,
    bn_bwd_apply and affine_apply with NT loads / stores.  float64 closed forms on the device; the
    ReLU mask of the backward is the kernel's own (test_fused_bn_relu_matches_aten says why)."""
    from nesie_amd.mmdet3d_ops.norm import FusedBNReLU1d
    assert NT_SHAPE[0] * NT_SHAPE[1] * NT_SHAPE[2] * 4 == 192 << 20
    C = NT_SHAPE[1]
    g = torch.Generator(device=hip_device).manual_seed(7 + relu)
    x = torch.randn(NT_SHAPE, device=hip_device, generator=g) * 2.0 + 3.0
    go = torch.randn(NT_SHAPE, device=hip_device, generator=g)
    mine = FusedBNReLU1d(C, relu=relu).to(hip_device)
    with torch.no_grad():
        mine.weight.copy_(torch.rand(C, device=hip_device, generator=g) + 0.5)
        mine.bias.copy_(torch.randn(C, device=hip_device, generator=g))
    gam, bet = mine.weight.detach().double().view(1, C, 1), mine.bias.detach().double().view(1, C, 1)
    xg = x.clone().requires_grad_(True)
    yg = mine(xg)
    yg.backward(go)
    xd = x.double()
    cnt = xd.numel() // C
    mean = xd.mean((0, 2), keepdim=True)
    var = xd.var((0, 2), unbiased=False, keepdim=True)
    invstd = 1.0 / torch.sqrt(var + mine.eps)
    xhat = (xd - mean) * invstd
    pre = xhat * gam + bet
    want = torch.relu(pre) if relu else pre
    torch.testing.assert_close(yg.detach().double(), want, rtol=1e-5, atol=2e-5)
    del pre, want
    torch.testing.assert_close(mine.running_mean.double(), 0.1 * mean.view(C), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(mine.running_var.double(), 0.9 + 0.1 * var.view(C) * cnt / (cnt - 1),
                               rtol=1e-5, atol=1e-6)
    gmask = go.double() * (yg.detach() > 0) if relu else go.double()
    dbeta = gmask.sum((0, 2))
    dgamma = (gmask * xhat).sum((0, 2))
    dx = gam * invstd * (gmask - dbeta.view(1, C, 1) / cnt - xhat * dgamma.view(1, C, 1) / cnt)
    del gmask, xhat
    scale = max(dx.abs().max().item(), 1e-3)
    assert (xg.grad.double() - dx).abs().max().item() <= 1e-4 * scale
    del dx
    torch.testing.assert_close(mine.weight.grad.double(), dgamma, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(mine.bias.grad.double(), dbeta, rtol=1e-4, atol=1e-4)
    # evaluation mode: y = relu?(scale x + shift) from the running statistics
    mine.eval()
    with torch.no_grad():
        ye = mine(x)
    s_ = mine.weight.detach().double() / torch.sqrt(mine.running_var.double() + mine.eps)
    t_ = mine.bias.detach().double() - mine.running_mean.double() * s_
    want = xd * s_.view(1, C, 1) + t_.view(1, C, 1)
    if relu:
        want = torch.relu(want)
    torch.testing.assert_close(ye.double(), want, rtol=1e-5, atol=2e-5)


def test_norm_backward_apply_pass_at_the_streaming_size(hip_device):
    """nesie_bn_relu_backward_apply (the apply pass alone, from ready sums; x is the raw input of a
    fused norm + ReLU) on 192 MB: bn_bwd_apply_kernel<true, NT>.  float64 closed form; x kept off
    the edge of the mask, which the kernel re-derives as fma(x, scale, shift) > 0."""
    hip = _hip(hip_device)
    b, C, p = NT_SHAPE
    g = torch.Generator(device=hip_device).manual_seed(11)
    x = torch.randn(NT_SHAPE, device=hip_device, generator=g) * 1.5 + 0.3
    dy = torch.randn(NT_SHAPE, device=hip_device, generator=g)
    gamma = torch.rand(C, device=hip_device, generator=g) + 0.5
    beta = torch.randn(C, device=hip_device, generator=g) * 0.3
    mean = x.double().mean((0, 2))
    invstd = (x.double().var((0, 2), unbiased=False) + 1e-5).rsqrt()
    coef = torch.stack([gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd, mean, invstd],
                       1).float().contiguous()
    cd = coef.double()
    pre = x.double() * cd[:, 0].view(1, C, 1) + cd[:, 1].view(1, C, 1)
    x = torch.where(pre.abs() < 1e-4, x + 1.0, x)
    pre = x.double() * cd[:, 0].view(1, C, 1) + cd[:, 1].view(1, C, 1)
    assert float(pre.abs().min()) > 1e-6
    gm = torch.where(pre > 0, dy.double(), torch.zeros((), dtype=torch.float64, device=hip_device))
    del pre
    xhat = (x.double() - cd[:, 2].view(1, C, 1)) * cd[:, 3].view(1, C, 1)
    sums = torch.stack([gm.sum((0, 2)), (gm * xhat).sum((0, 2))], 1)               # (C, 2)
    cnt = b * p
    want = (gamma.double() * cd[:, 3]).view(1, C, 1) * (gm - sums[:, 0].view(1, C, 1) / cnt
                                                         - xhat * sums[:, 1].view(1, C, 1) / cnt)
    del gm, xhat
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty(C, device=hip_device), torch.empty(C, device=hip_device)
    hip.bn_relu_backward_apply(dy, x, gamma, coef[:, 3].contiguous(), coef, sums.float().view(C, 1, 2).contiguous(),
                               dx, dgamma, dbeta)
    assert (dx.double() - want).abs().max().item() < 2e-5 * want.abs().max().item()
    torch.testing.assert_close(dgamma.double(), sums[:, 1], rtol=1e-4, atol=1e-4 * sums[:, 1].abs().max().item())
    torch.testing.assert_close(dbeta.double(), sums[:, 0], rtol=1e-4, atol=1e-4 * sums[:, 0].abs().max().item())
