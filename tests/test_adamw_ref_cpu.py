"""tests/_adamw_ref.py IS the reference's optimiser (torch.optim.AdamW behind clip_grad_norm_, in
float64), its magnitudes dominate its outputs, and its float32 bounds are attainable: a float32
numpy transcription of csrc/optim.hip stays inside them at every step count the GPU tests use.
No GPU."""
import numpy as np
import pytest
import torch

from tests import _adamw_ref as R

U = R.U
STEP_COUNTS = (1, 2, 3, 10, 100, 1000, 10_000, 100_000)     # tests/test_flat_adamw_fp64_gpu.py


def rounded_hyper(max_norm):
    h = R.HYPER
    return dict(lr=R.rounded(h['lr']), betas=tuple(R.rounded(b) for b in h['betas']),
                eps=R.rounded(h['eps']), wd=R.rounded(h['wd']), max_norm=max_norm)


@pytest.mark.parametrize('scale,max_norm', [(5.0, 10.0), (1e-2, 10.0), (5.0, None)],
                         ids=['clip-active', 'clip-inactive', 'no-max-norm'])
def test_step_chained_is_torch_adamw_behind_clip_grad_norm_in_float64(scale, max_norm):
    n, h = 257, rounded_hyper(max_norm)
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * scale).astype(np.float32) for _ in range(6)]
    w = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.AdamW([w], lr=h['lr'], betas=h['betas'], eps=h['eps'], weight_decay=h['wd'])
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, start=1):
        w.grad = torch.tensor(g, dtype=torch.float64)
        if max_norm is not None:
            want_norm = float(torch.nn.utils.clip_grad_norm_([w], max_norm=max_norm))
        opt.step()
        r = R.step(p, g, m, v, t, **h)
        p, m, v = r.p, r.m, r.v
        if max_norm is not None:
            assert r.norm == pytest.approx(want_norm, rel=1e-12)
            assert (r.coef < 1) == (scale == 5.0)
            np.testing.assert_allclose(r.g, w.grad.numpy(), rtol=1e-12, atol=0)
        else:
            assert r.coef == 1.0 and np.array_equal(r.g, g.astype(np.float64))
        st = opt.state[w]
        np.testing.assert_allclose(r.p, w.detach().numpy(), rtol=1e-12, atol=0, err_msg=str(t))
        np.testing.assert_allclose(r.m, st['exp_avg'].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(r.v, st['exp_avg_sq'].numpy(), rtol=1e-12, atol=0)
    # the free run is the same chain
    last, kept = R.trajectory(p0, grads, keep=(3, 6), **h)
    assert np.array_equal(last.p, p) and np.array_equal(kept[6].m, m) and kept[3].t == 3


@pytest.mark.parametrize('t', STEP_COUNTS)
def test_the_magnitudes_dominate_the_outputs(t):
    p, g, m, v = R.case(4097, t, 4.0, seed=t)
    r = R.step(p, g, m, v, t, **R.HYPER)
    for out, mag in ((r.p, r.S_p), (r.g, r.S_g), (r.m, r.S_m), (r.v, r.S_v)):
        assert (np.abs(out) <= mag).all()
    assert r.norm == pytest.approx(4.0 * R.rounded(R.HYPER['max_norm']), rel=1e-6)


# ---- csrc/optim.hip in float32 numpy, operation for operation ------------------------------------
f32 = np.float32


def _block_tree(per_thread):
    """(..., 256) float32 per-thread sums -> (...,): wave_sum (xor 32, 16, ... 1 over each 64
    lanes), then (sh0 + sh1) + (sh2 + sh3)."""
    w = per_thread.reshape(per_thread.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    sh = w[..., 0]
    return (sh[..., 0] + sh[..., 1]) + (sh[..., 2] + sh[..., 3])


def kernel_norm_float32(g):
    n = g.size
    per = -(-n // R.PARTS)
    rounds = -(-per // R.BLOCK)
    idx = (np.arange(R.PARTS)[:, None, None] * per + np.arange(rounds)[None, :, None] * R.BLOCK
           + np.arange(R.BLOCK)[None, None, :])
    inside = (idx < np.minimum((np.arange(R.PARTS) + 1) * per, n)[:, None, None])
    sq = np.where(inside, (g * g)[np.minimum(idx, n - 1)], f32(0))
    s = np.zeros((R.PARTS, R.BLOCK), f32)
    for k in range(rounds):
        s = s + sq[:, k]
    part = _block_tree(s)
    s = np.zeros(R.BLOCK, f32)
    for k in range(R.PARTS // R.BLOCK):
        s = s + part[k * R.BLOCK:(k + 1) * R.BLOCK]
    return np.sqrt(_block_tree(s))


def kernel_step_float32(p, g, m, v, t, lr, betas, eps, wd, max_norm):
    """adamw_clip_kernel's arithmetic with exact, once-rounded bias corrections."""
    lr, b1, b2, eps, wd, mx = (f32(x) for x in (lr, betas[0], betas[1], eps, wd, max_norm or 0.0))
    total = kernel_norm_float32(g)
    c = mx / (total + f32(1e-6)) if mx > 0 else f32(1)
    coef = c if c < 1 else f32(1)
    bc1, bc2 = f32(1 - float(b1) ** t), f32(1 - float(b2) ** t)
    step_size, inv_sqrt_bc2 = lr / bc1, f32(1) / np.sqrt(bc2)
    gi = g * coef
    pi = p - p * (lr * wd)
    mi = b1 * m + (f32(1) - b1) * gi
    vi = b2 * v + (f32(1) - b2) * (gi * gi)
    denom = np.sqrt(vi) * inv_sqrt_bc2 + eps
    out = pi - step_size * (mi / denom), gi, mi, vi, total
    assert all(o.dtype == np.float32 for o in out)
    return out


@pytest.mark.parametrize('n,t,ratio', [(4097, t, 4.0) for t in STEP_COUNTS]
                         + [(1025, 7, 4.0), (262_145, 7, 4.0), (4097, 7, 1 - 1e-3), (4097, 7, 1 + 1e-3)])
def test_a_float32_transcription_of_the_kernel_stays_inside_the_bounds(n, t, ratio):
    p, g, m, v = R.case(n, t, ratio, seed=100 + t)
    r = R.step(p, g, m, v, t, **R.HYPER)
    b = R.bounds(r)
    got = kernel_step_float32(p, g, m, v, t, **R.HYPER)
    for name, dev, ref in zip('pgmv', got, (r.p, r.g, r.m, r.v)):
        err = np.abs(dev.astype(np.float64) - ref)
        assert (err <= b[name]).all(), (name, float((err / np.maximum(b[name], 1e-300)).max()))
    assert abs(float(got[4]) - r.norm) <= b['norm']
    # and the bounds are no wider than a few parts in a million of the norm and the moment
    assert b['norm'] <= 2e-6 * r.norm and (b['m'] <= 2e-6 * r.S_m + R.TINY).all()


def test_the_abi_rounding_of_beta2_is_217_u_of_the_second_moment():
    p, g, m, v = R.case(63, 1, 0.5, seed=3)                  # first step: v' = (1 - beta2) g'^2
    h = dict(R.HYPER)
    b2, b2f = h['betas'][1], R.rounded(h['betas'][1])
    as_abi = R.step(p, g, m, v, 1, **h)
    as_double = R.step(p, g, m, v, 1, round_hyper=False, **h)
    want = abs(1 - (1 - b2f) / (1 - b2))
    live = as_double.v > 0
    assert live.sum() >= 60
    got = np.abs(as_abi.v[live] / as_double.v[live] - 1)
    assert np.abs(got / want - 1).max() <= 1e-9
    assert 216 * U < want < 218 * U
