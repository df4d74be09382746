"""float64 referee of the sigmoid focal loss (formulas: include/nesie_ops.h), evaluated on the
float32-rounded inputs, and the bound a float32 implementation is held to.

With z = x, a = alpha for a positive element (label == column) and z = -x, a = 1 - alpha otherwise:

    loss      = a * exp(-gamma * softplus(z)) * softplus(-z)
    d loss/dz = -a * exp(-gamma * softplus(z)) * (gamma * sigmoid(z) * softplus(-z) + sigmoid(-z))
    softplus(v) = max(v, 0) + log1p(exp(-|v|))

The elementwise bound, no element excused, with u = 2^-24:

    |dev - f64| <= (16 + 8 * gamma * softplus(z)) * u * |f64| + 2^-126

exp at 3 ulp and log1p at 2 ulp (the OpenCL full-profile limits) give each softplus at most 6 u; the
exponent gamma * softplus(z) then carries at most 6.5 u relative, that is 6.5 * gamma * softplus(z) * u
absolute, which the second exp turns into a relative error of the result; that exp, the products
(weights and upstream gradient included: they enter both sides) and the sum inside the gradient add
less than 10 u.  The floor lets a result below the smallest normal be flushed.

A reduced scalar is held to the sum of its elements' bounds plus gamma_{m+3} * S, m the number of
elements, gamma_m = m u / (1 - m u), S the sum of the absolute terms: valid for any order of the sum,
the 3 covering the scale factors.  Where the order is known (the device's: a tree of depth
``device_sum_depth(m)``) the tests also hold the scalar to gamma_{depth+3} * S, the bound of that
tree, on inputs clamped to |x| <= 104: only there can a lost partial show."""
import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -126


SPECIAL = (0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4, 3e38, -3e38)


def case(n, c, scale, seed, device='cpu', limit=None):
    """Seeded logits ``randn * scale`` (N, C) and labels uniform in [0, C] (C = background).  The
    first rows carry the SPECIAL values in a positive column (the label's) and in a negative one
    where there is one, then come a row labelled -1 and one labelled 2^31 + 3, as far as N allows.
    ``limit``: clamp every logit to [-limit, limit].  A sum over the unclamped case is dominated by
    the two terms of 3e38, whose own error bound (1e31) hides every other term: a test of a SUM
    takes limit=104, so that no term exceeds 104 and a lost term shows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * scale
    t = torch.randint(0, c + 1, (n,), generator=g)
    k = min(len(SPECIAL), n)
    special = torch.tensor(SPECIAL[:k])
    t[:k] = 0
    x[:k, 0] = special
    if c > 1:
        x[:k, 1] = special
    for row, label in ((k, -1), (k + 1, 2 ** 31 + 3)):
        if row < n:
            t[row] = label
    if limit is not None:
        x = x.clamp(-limit, limit)
    return x.to(device), t.to(device)


CHUNK = 4096        # elements per partial of the device's reduction (csrc/focal_loss.hip)


def device_sum_depth(m):
    """Roundings on the longest path of the device's sum over m elements, from its fixed order
    (DESIGN 7k): a thread adds 16 terms (15), 64 lanes fold in 6 steps, 4 waves in 2; with more
    than one chunk the finish adds ceil(chunks / 256) partials per thread and folds again (6 + 2)."""
    chunks = -(-m // CHUNK)
    return 23 if chunks <= 1 else 23 + -(-chunks // 256) + 8


def _f32(v):
    return float(np.float32(v))


def reference(x, target, gamma, alpha, class_weight=None, sample_weight=None):
    """x (N, C) float32, target (N,) int64, class_weight (C,), sample_weight (N,) / (N, C) / (N*C,)
    -> (loss, d loss/dx, softplus(z)), each (N, C) float64 on the CPU, the weights multiplied in."""
    x = x.detach().cpu().to(torch.float32).double()
    target = target.detach().cpu().long()
    n, c = x.shape
    gamma, alpha = _f32(gamma), _f32(alpha)
    pos = target.view(-1, 1) == torch.arange(c)
    z = torch.where(pos, x, -x)
    a = torch.where(pos, torch.tensor(alpha, dtype=torch.float64),
                    torch.tensor(1.0 - alpha, dtype=torch.float64))
    e = torch.exp(-z.abs())
    log1p_e = torch.log1p(e)
    sp_pos = z.clamp(min=0) + log1p_e
    sp_neg = (-z).clamp(min=0) + log1p_e
    w = a * torch.exp(-gamma * sp_pos)
    s_pos = torch.where(z >= 0, 1 / (1 + e), e / (1 + e))
    s_neg = torch.where(z >= 0, e / (1 + e), 1 / (1 + e))
    dz = -w * (gamma * s_pos * sp_neg + s_neg)
    f = factor(target, n, c, class_weight, sample_weight)
    return w * sp_neg * f, torch.where(pos, dz, -dz) * f, sp_pos


def factor(target, n, c, class_weight=None, sample_weight=None):
    """The weight of every element, (N, C) or (1, 1) float64: class_weight[label], 1.0 for a label
    outside [0, C), times the sample weight of the row or of the element."""
    target = target.detach().cpu().long()
    f = torch.ones(1, 1, dtype=torch.float64)
    if class_weight is not None:
        cw = class_weight.detach().cpu().to(torch.float32).double()
        inside = (target >= 0) & (target < c)
        row = torch.where(inside, cw[target.clamp(0, max(c - 1, 0))], torch.ones(n, dtype=torch.float64))
        f = f * row.view(n, 1)
    if sample_weight is not None:
        sw = sample_weight.detach().cpu().to(torch.float32).double()
        f = f * (sw.view(n, 1) if sw.numel() == n else sw.view(n, c))
    return f


def element_bound(ref, softplus_z, gamma):
    return (16 + 8 * _f32(gamma) * softplus_z) * U * ref.abs() + FLOOR


def check(dev, ref, softplus_z, gamma, what=''):
    """Asserts the elementwise bound on every element; -> the worst error / bound ratio."""
    dev = dev.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(dev).all(), f'{what}: {int((~torch.isfinite(dev)).sum())} non-finite values'
    if ref.numel() == 0:
        return 0.0
    ratio = (dev - ref).abs() / element_bound(ref, softplus_z, gamma)
    worst = int(ratio.argmax())
    r = float(ratio.reshape(-1)[worst])
    assert r <= 1.0, (f'{what}: element {worst} of shape {tuple(ref.shape)}: got '
                      f'{float(dev.reshape(-1)[worst])!r}, float64 {float(ref.reshape(-1)[worst])!r}, '
                      f'error / bound = {r:.3f}')
    return r


def check_sum(dev, terms, softplus_z, gamma, what='', depth=None):
    """``dev``: a float32 scalar that should be ``terms.sum()`` (terms (N, C) float64, scale factors
    multiplied in).  Asserts the sum bound; -> error / bound.  ``depth``: the roundings on the longest
    path of a sum whose order is known (``device_sum_depth``); the summation term is then
    gamma_{depth+3} * S, which is what that order can lose at the most and is far below gamma_{m+3} * S
    (1.8 % of S at 3e5 elements, where a whole lost chunk would hide)."""
    dev = float(dev.detach().cpu().double())
    assert np.isfinite(dev), f'{what}: {dev}'
    m = terms.numel()
    k = ((m if depth is None else min(depth, m)) + 3) * U
    bound = float(element_bound(terms, softplus_z, gamma).sum()) + k / (1 - k) * float(terms.abs().sum())
    err = abs(dev - float(terms.sum()))
    assert err <= bound, f'{what}: got {dev!r}, float64 {float(terms.sum())!r}, error / bound = {err / bound:.3f}'
    return err / bound
