"""The statistics -> coefficients step (csrc/bn_coef.h: bn_coef_finish) through each of the five
finishers that end in it, at the branches of its tail, against the closed form in float64:

    n == 1                      var = 0, and running_var moves by momentum * 0 (the n > 1 guard of
                                the unbiased rule)
    gamma and beta absent       scale = invstd, bias = -mean * invstd
    running statistics absent   coef still complete
    chan_bias (pw_stats_finalize only): the running mean is shifted by it, coef is not

Each finisher keeps its own summation; the closed form is evaluated in float64 on the very values
the finisher is handed (fp32 partials, float64 moments), so what is compared is the tail.  The
tolerances are those of each route's neighbouring test: test_fused_bn_relu_matches_aten's running
statistics (bn_relu_forward), _syncbn_ref.check_running (syncbn_forward_apply),
test_k4_statistics_from_input_moments_against_float64 and test_layer_forward_matches_fp64
(test_pwconv_gpu.py).  mlp_stat_finalize has no neighbour: see MLP_TOL."""
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS, MOM = 1e-5, 0.1
RM0, RV0 = 0.25, 1.5      # running statistics before the call


def _hip():
    from nesie_amd.kernels import HipKernels
    return HipKernels()


def _closed(n, mean, var, gamma, beta, biased=False, chan_bias=None):
    """float64 (coef (C, 4), running_mean, running_var) of channels with count n, mean, biased var."""
    invstd = 1.0 / torch.sqrt(var + EPS)
    g = torch.ones_like(mean) if gamma is None else gamma.double().cpu()
    b = torch.zeros_like(mean) if beta is None else beta.double().cpu()
    coef = torch.stack([g * invstd, b - mean * g * invstd, mean, invstd], -1)
    shown = mean if chan_bias is None else mean + chan_bias.double().cpu()
    spread = var if biased or n <= 1 else var * n / (n - 1)
    return coef, (1 - MOM) * RM0 + MOM * shown, (1 - MOM) * RV0 + MOM * spread


def _params(c, dev, affine, running, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev) if affine else None
    beta = torch.randn(c, generator=g).to(dev) if affine else None
    rm = torch.full((c,), RM0, device=dev) if running else None
    rv = torch.full((c,), RV0, device=dev) if running else None
    return gamma, beta, rm, rv


def _close(got, want, rtol, atol):
    torch.testing.assert_close(got.double().cpu(), want, rtol=rtol, atol=atol)


# (gamma and beta given, running statistics given): the third is the plain case the others vary
BRANCHES = [(False, True), (True, False), (True, True)]


@pytest.mark.parametrize('affine,running', BRANCHES)
@pytest.mark.parametrize('shape', [(1, 2, 1), (3, 2, 5), (2, 2, 8)])
def test_bn_relu_forward(hip_device, shape, affine, running):
    hip, c = _hip(), shape[1]
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))) * 2 + 3).to(hip_device)
    gamma, beta, rm, rv = _params(c, hip_device, affine, running, 1)
    y, coef = torch.empty_like(x), torch.empty(c, 4, device=hip_device)
    sm, si = torch.empty(c, device=hip_device), torch.empty(c, device=hip_device)
    hip.bn_relu_forward(x, gamma, beta, rm, rv, MOM, EPS, False, y, sm, si, coef)
    xd = x.double().cpu()
    n = shape[0] * shape[2]
    want, wrm, wrv = _closed(n, xd.mean((0, 2)), xd.var((0, 2), unbiased=False), gamma, beta)
    _close(coef, want, 1e-5, 1e-6)
    _close(sm, want[:, 2], 1e-5, 1e-6)
    _close(si, want[:, 3], 1e-5, 1e-6)
    _close(y, xd * want[:, 0].view(1, c, 1) + want[:, 1].view(1, c, 1), 1e-5, 2e-5)
    if running:
        _close(rm, wrm, 1e-5, 1e-6)
        _close(rv, wrv, 1e-5, 1e-6)


@pytest.mark.parametrize('affine,running', BRANCHES)
@pytest.mark.parametrize('shape', [(1, 2, 1), (3, 2, 5)])
def test_syncbn_forward_apply_takes_the_biased_variance(hip_device, shape, affine, running):
    hip, c = _hip(), 2
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))) - 1.5).to(hip_device)
    xd = x.double().cpu()
    n = shape[0] * shape[2]
    moments = torch.stack([torch.full((c,), float(n), dtype=torch.float64), xd.sum((0, 2)),
                           xd.square().sum((0, 2))], -1).to(hip_device)
    gamma, beta, rm, rv = _params(c, hip_device, affine, running, 2)
    y, coef = torch.empty_like(x), torch.empty(c, 4, device=hip_device)
    hip.syncbn_forward_apply(x, moments, gamma, beta, rm, rv, MOM, EPS, False, y, coef)
    mean = xd.sum((0, 2)) / n
    want, wrm, wrv = _closed(n, mean, (xd.square().sum((0, 2)) / n - mean * mean).clamp_min(0), gamma,
                             beta, biased=True)
    _close(coef, want, 1e-5, 1e-6)
    if running:
        _close(rm, wrm, 1e-5, 1e-6)
        _close(rv, wrv, 1e-5, 1e-6)


# mlp_stat_finalize has no neighbouring test.  Its outputs are float64 results rounded to float
# once, so against the same closed form in float64 the error relative to max(1, |want|) is about one
# rounding (2^-24 = 6.0e-8; momentum is a float, 0.1f - 0.1 = 1.5e-9, on top).  The largest error
# over these 18 cases at the commit before bn_coef.h existed was 6.495e-08 (MLP_PARENT_ERR, and the
# same with it); allowed: twice that.
MLP_PARENT_ERR = 6.495e-8
MLP_TOL = 2 * MLP_PARENT_ERR


@pytest.mark.parametrize('affine,running', BRANCHES)
@pytest.mark.parametrize('channel_major', [False, True])
@pytest.mark.parametrize('parts,per', [(1, 1), (1, 7), (300, 7)])
def test_mlp_stat_finalize(hip_device, parts, per, channel_major, affine, running):
    hip, c = _hip(), 2
    n = parts * per
    g = torch.Generator().manual_seed(parts + per)
    v = torch.randn(parts, c, per, generator=g).double() * 0.5 + 0.75
    if n == 1:
        v[:] = 1.5             # its square is exact in fp32, so var == 0 exactly
    part = torch.stack([v.sum(-1), v.square().sum(-1)], -1).float()       # (parts, C, 2)
    pd = part.double()
    mean = pd[..., 0].sum(0) / n
    gamma, beta, rm, rv = _params(c, hip_device, affine, running, 3)
    want, wrm, wrv = _closed(n, mean, (pd[..., 1].sum(0) / n - mean * mean).clamp_min(0), gamma, beta)
    coef = torch.empty(c, 4, device=hip_device)
    dev_part = (part.transpose(0, 1).contiguous() if channel_major else part).to(hip_device)
    hip.mlp_stat_finalize(dev_part, float(n), gamma, beta, rm, rv, MOM, EPS, coef, channel_major=channel_major)
    pairs = [(coef, want)] + ([(rm, wrm), (rv, wrv)] if running else [])
    err = max(((a.double().cpu() - b).abs() / b.abs().clamp_min(1.0)).max().item() for a, b in pairs)
    print(f'mlp_stat_finalize parts={parts} per={per} cm={channel_major} affine={affine} '
          f'running={running}: err {err:.3e}')
    assert err <= MLP_TOL


def _k4_single_point_moments(x, dev):
    """The (256, 20) float64 partial moments nesie_k4_moments leaves, for ONE point x (4,): row 0
    holds sum x_j at [j] and sum x_j x_k at [4 + 4 j + k], k >= j; the other rows are empty."""
    mom = torch.zeros(256, 20, dtype=torch.float64)
    xd = x.double()
    mom[0, :4] = xd
    for j in range(4):
        for k in range(j, 4):
            mom[0, 4 + 4 * j + k] = xd[j] * xd[k]
    return mom.to(dev)


@pytest.mark.parametrize('affine,running', BRANCHES)
@pytest.mark.parametrize('single', [True, False])
def test_k4_stat_finalize(hip_device, single, affine, running):
    hip = _hip()
    g = torch.Generator().manual_seed(5)
    x4 = torch.randn(1, 4, 4, generator=g).to(hip_device)
    x4[:, 3] = x4[:, 3].abs() * 0.7 + 1.3
    w0 = torch.randn(64, 4, generator=g).to(hip_device)
    gamma, beta, rm, rv = _params(64, hip_device, affine, running, 4)
    coef = torch.empty(64, 4, device=hip_device)
    if single:
        n, mom = 1, _k4_single_point_moments(x4[0, :, 0].cpu(), hip_device)
        z = (w0.double().cpu() @ x4[0, :, :1].double().cpu()).unsqueeze(0)
    else:
        n, mom = 4, hip.k4_moments(x4)
        z = torch.einsum('cj,njp->ncp', w0.double().cpu(), x4.double().cpu())
    hip.k4_stat_finalize(mom, w0, gamma, beta, rm, rv, MOM, EPS, float(n), coef)
    want, wrm, wrv = _closed(n, z.mean((0, 2)), z.var((0, 2), unbiased=False), gamma, beta)
    _close(coef, want, 2e-5, 2e-5)
    if running:
        _close(rm, wrm, 1e-5, 1e-6)
        _close(rv, wrv, 1e-5, 1e-6)


@pytest.mark.parametrize('affine,running,bias', [(False, True, False), (True, False, False),
                                                 (True, True, False), (True, True, True)])
@pytest.mark.parametrize('slots,single', [(1, True), (1, False), (65, True), (65, False)])
def test_pw_stats_finalize(hip_device, slots, single, affine, running, bias):
    hip, ng, cout, per = _hip(), 2, 2, 6
    g = torch.Generator().manual_seed(slots)
    v = (torch.randn(ng, slots, cout, per, generator=g) * 0.5 + 2.0).float().double()
    cnt = torch.full((ng, slots, cout), float(per), dtype=torch.float64)
    if single:                      # one value in one slot, every other slot empty (count 0)
        cnt[:] = 0.0
        cnt[:, slots // 2] = 1.0
    live = torch.arange(per).view(1, 1, 1, per) < cnt.unsqueeze(-1)
    shift = v[..., 0]
    d = (v - shift.unsqueeze(-1)) * live
    part = torch.stack([cnt, shift, d.sum(-1), d.square().sum(-1)], -1).float()      # (ng, slots, Cout, 4)
    pd = part.double()
    n_i, s1, s2 = pd[..., 0], pd[..., 2], pd[..., 3]
    safe = n_i.clamp_min(1.0)
    mean_i = pd[..., 1] + s1 / safe
    m2_i = (s2 - s1 * s1 / safe).clamp_min(0) * (n_i > 0)
    n = int(n_i.sum(1)[0, 0].item())
    mean = (n_i * mean_i).sum(1) / n                                                  # (ng, Cout)
    var = (m2_i + n_i * (mean_i - mean.unsqueeze(1)).square()).sum(1) / n
    gamma, beta, rm, rv = _params(ng * cout, hip_device, affine, running, 6)
    cb = torch.randn(ng * cout, generator=g).to(hip_device) if bias else None
    want, wrm, wrv = _closed(n, mean.reshape(-1), var.reshape(-1), gamma, beta, chan_bias=cb)
    coef = torch.empty(ng * cout, 4, device=hip_device)
    hip.pw_stats_finalize(part.to(hip_device), gamma, beta, rm, rv, MOM, EPS, coef, chan_bias=cb)
    _close(coef[:, 2], want[:, 2], 1e-5, 1e-6)
    _close(coef[:, 3], want[:, 3], 2e-5, 0)
    _close(coef[:, 0], want[:, 0], 2e-5, 0)
    _close(coef[:, 1], want[:, 1], 1e-4, 1e-5)      # chan_bias or not: the same coef
    if running:
        _close(rm, wrm, 1e-5, 1e-6)
        _close(rv, wrv, 2e-5, 0)
