"""csrc/optim.hip (sumsq_partials_kernel + adamw_clip_kernel) against the float64 referee of
tests/_adamw_ref.py under its a-priori bounds, at every launch edge: the sizes around the norm
kernel's 1024 ranges and the update kernel's 256-thread workgroups, 4096-element chunks and 1024
workgroup cap; step counts from the cancellation in 1 - beta^t at t = 1 to a powf of a large
exponent; every branch of the clip; the host-scalar entry; a non-finite gradient; n = 0; the
workspace's extent; run-to-run bits; then 200 free-running steps and FlatTrainState end to end.

Single steps are teacher-forced: HipKernels.flat_adamw_step on float32 device tensors with the
step scalar preset to t - 1.  No element is excused.  Each case prints, per output, dev_err (max
|device - float64|), ref_err (the same for float32 torch.optim.AdamW + clip_grad_norm_ on the
device) and the largest err / bound."""
import copy

import numpy as np
import pytest
import torch

from tests import _adamw_ref as R

pytestmark = pytest.mark.gpu

U = R.U
H = R.HYPER
N_EDGE = 4097
CAP = 1024 * 4096          # the update kernel's workgroup count saturates here
SIZES = (1, 63, 64, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 262_145,
         CAP - 1, CAP, CAP + 1, 2 * CAP + 5)
STEP_COUNTS = (1, 2, 3, 10, 100, 1000, 10_000, 100_000)
OUTPUTS = ('p', 'g', 'm', 'v')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_step(dev, arrays, t, hyper=H, norm_out=True, hyper_dev=None, counts=True):
    """One call of HipKernels.flat_adamw_step -> numpy p, g, m, v, norm (None without norm_out)."""
    from nesie_amd.kernels import HipKernels
    p, g, m, v = (torch.from_numpy(np.array(a, dtype=np.float32)).to(dev) for a in arrays)
    step = torch.tensor(float(t - 1), dtype=torch.float32, device=dev)
    norm = torch.full((), -1.0, dtype=torch.float32, device=dev) if norm_out else None
    if hyper_dev is not None:
        hyper_dev = torch.tensor(hyper_dev, dtype=torch.float32, device=dev)
    HipKernels().flat_adamw_step(p, g, m, v, step, hyper['lr'], hyper['betas'], hyper['eps'],
                                 hyper['wd'], hyper['max_norm'], norm, hyper=hyper_dev)
    torch.cuda.synchronize()
    assert float(step) == (t if counts else t - 1)
    out = {k: a.cpu().numpy() for k, a in zip(OUTPUTS, (p, g, m, v))}
    out['norm'] = float(norm) if norm_out else None
    return out


def torch_step(dev, arrays, t, hyper=H):
    """The same single step by float32 torch.optim.AdamW behind clip_grad_norm_ on the device."""
    p, g, m, v = (torch.from_numpy(np.array(a, dtype=np.float32)).to(dev) for a in arrays)
    w = torch.nn.Parameter(p)
    w.grad = g
    opt = torch.optim.AdamW([w], lr=hyper['lr'], betas=hyper['betas'], eps=hyper['eps'],
                            weight_decay=hyper['wd'])
    opt.state[w] = dict(step=torch.tensor(float(t - 1)), exp_avg=m, exp_avg_sq=v)
    if hyper['max_norm'] and hyper['max_norm'] > 0:
        norm = torch.nn.utils.clip_grad_norm_([w], hyper['max_norm'])
    else:
        norm = g.double().norm()
    opt.step()
    out = {k: a.detach().cpu().numpy() for k, a in zip(OUTPUTS, (w, w.grad, m, v))}
    out['norm'] = float(norm)
    return out


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact."""
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


def check(label, got, r, b, ref=None, keep=None):
    """Print dev_err, ref_err and max err / bound of every output, then assert every element
    (``keep``: a mask, for the case that sets one element to NaN on purpose)."""
    keep = slice(None) if keep is None else keep
    ratios, cells = {}, []
    for k in OUTPUTS:
        want = getattr(r, k)[keep]
        err = np.abs(got[k].astype(np.float64)[keep] - want)
        ref_err = np.abs(ref[k].astype(np.float64)[keep] - want).max() if ref and err.size else float('nan')
        ratios[k] = worst(err, np.broadcast_to(b[k], getattr(r, k).shape)[keep])
        cells.append(f'{k}: dev_err {err.max() if err.size else 0.0:.3e} ref_err {ref_err:.3e} '
                     f'err/bound {ratios[k]:.3f}')
    if got['norm'] is not None and np.isfinite(r.norm):
        err = abs(got['norm'] - r.norm)
        ref_err = abs(ref['norm'] - r.norm) if ref else float('nan')
        ratios['norm'] = worst(np.float64(err), np.float64(b['norm']))
        cells.append(f'norm: dev_err {err:.3e} ref_err {ref_err:.3e} err/bound {ratios["norm"]:.3f}')
    print(f'\n[{label}] ' + ' | '.join(cells))
    for k, q in ratios.items():
        assert q <= 1.0, f'{label}: {k} is {q:.3f} of its bound'
    for k in OUTPUTS:
        assert np.isfinite(got[k][keep]).all()
    return ratios


def run_case(dev, label, arrays, t, hyper=H, **kw):
    r = R.step(*arrays, t, **hyper)
    b = R.bounds(r)
    got = device_step(dev, arrays, t, hyper, **kw)
    check(label, got, r, b, torch_step(dev, arrays, t, hyper))
    return got, r, b


# ---- launch geometry ------------------------------------------------------------------------------

@pytest.mark.parametrize('n', SIZES)
def test_every_size_edge_with_the_clip_active(hip_device, n):
    """t = 7, norm = 4 max_norm.  1 .. 1023: most norm workgroups own an empty range; 255 / 256 /
    257 and 4095 / 4096 / 4097: one thread round, one workgroup of the update; 1024 * 4096 and
    past it: the workgroup count stays 1024 and each walks more than 4096 elements."""
    arrays = R.case(n, 7, 4.0, seed=n % 1000)
    got, r, b = run_case(hip_device, f'n={n}', arrays, 7)
    assert r.coef < 1 and b['e_coef'] > 0


# ---- step counts ----------------------------------------------------------------------------------

# what reading a bias correction back from the outputs adds (derived in the test below)
NOISE_BC1, NOISE_BC2 = 3 * U * R.SECOND_ORDER, 22 * U * R.SECOND_ORDER


@pytest.mark.parametrize('t', STEP_COUNTS)
def test_bias_corrections_from_the_first_step_to_a_large_exponent(hip_device, t):
    """n = 4097 at step counts 1 .. 100 000 (zero moments at t = 1), all outputs inside their
    bounds, and the two bias corrections read back in isolation:

    bc1 at EPS_ONLY (p = 0, g = 0, v = 0): the update is fl(fl(lr / bc1) * fl(m' / eps)) = -p'', so
    bc1 = lr (m' / eps) / -p'' within 3 roundings.
    bc2 at FIRST (p = m = v = 0): -p'' = fl(fl(lr / bc1) * fl(m' / denom)) gives denom within the 3 u
    of bc1's reading and 3 more; denom = fl(fl(sqrtf(v') * inv) + eps) gives inv within 3 more (two
    roundings and sqrtf's); inv = fl(1 / fl(sqrtf(bc2))) gives sqrt(bc2) within 2 more, 11 u, and bc2
    within 22 u.
    Each must lie within ``bc_rel_bound`` (powf within E_POW_ULPS ulp, the subtraction) plus that
    reading noise.  Printed: the relative error in u, and the absolute error in ulps of beta^t."""
    arrays = R.case(N_EDGE, t, 4.0, seed=t % 1000)
    got, r, b = run_case(hip_device, f't={t}', arrays, t)
    lr, eps = R.rounded(H['lr']), R.rounded(H['eps'])
    p, m, v = (got[k].astype(np.float64) for k in 'pmv')
    bc1 = lr * (m[R.EPS_ONLY] / eps) / -p[R.EPS_ONLY]
    denom = (lr / bc1) * m[R.FIRST] / -p[R.FIRST]
    bc2 = (np.sqrt(v[R.FIRST]) / (denom - eps)) ** 2
    for name, rec, true, beta, e, noise in (('bc1', bc1, r.bc1, r.b1, b['e_bc1'], NOISE_BC1),
                                            ('bc2', bc2, r.bc2, r.b2, b['e_bc2'], NOISE_BC2)):
        rel = abs(rec - true) / true
        ulp = float(np.spacing(np.float32(beta ** t)))
        in_ulps = f'{abs(rec - true) / ulp:.2f} ulp of beta^t' if beta ** t > 1e-3 else 'beta^t below 1e-3'
        print(f'[t={t}] {name}: read {rec:.9e} true {true:.9e} rel err {rel / U:.2f} u = {in_ulps}; '
              f'bound {e / U:.2f} u (powf {R.E_POW_ULPS:g} ulp) + reading {noise / U:.0f} u')
        assert rel <= e + noise, name


# ---- the clip's branches --------------------------------------------------------------------------

@pytest.mark.parametrize('ratio', [0.0, 1e-3, 1 - 1e-3, 1 + 1e-3, 40.0])
def test_clip_branches_by_norm_over_max_norm(hip_device, ratio):
    """norm / max_norm = 0 (total 0: the coefficient max_norm / 1e-6 is clamped to 1), far below,
    just below, just above and far above 1.  1 -+ 1e-3 is far outside the norm's bound, so the branch
    is determined; which one is the referee's answer (below 1 the 1e-6 of the denominator can still
    push the coefficient under 1, as in torch).  Where no clipping can happen the gradient left
    behind is the input bit for bit."""
    arrays = R.case(N_EDGE, 7, ratio, seed=17)
    got, r, b = run_case(hip_device, f'norm/max={ratio:g}', arrays, 7)
    assert (r.coef_raw > 1) == (ratio < 1)
    if r.coef == 1.0 and b['e_coef'] == 0:
        assert ratio < 1 and np.array_equal(bits(got['g']), bits(arrays[1]))
    else:
        assert ratio > 1 and r.coef < 1 and not np.array_equal(bits(got['g']), bits(arrays[1]))
    if ratio == 0:
        assert got['norm'] == 0.0 and (got['g'] == 0).all()
        assert (np.abs(got['v']) <= np.abs(arrays[3])).all()        # the moments only decay
        assert (np.abs(got['m']) <= np.abs(arrays[2])).all()


@pytest.mark.parametrize('max_norm', [None, 0, -1])
def test_without_a_max_norm_the_gradient_is_untouched_and_the_norm_still_written(hip_device, max_norm):
    arrays = R.case(N_EDGE, 7, 4.0, seed=19)
    got, r, b = run_case(hip_device, f'max_norm={max_norm}', arrays, 7, dict(H, max_norm=max_norm))
    assert r.coef == 1.0 and r.norm > 39
    assert np.array_equal(bits(got['g']), bits(arrays[1]))
    assert abs(got['norm'] - r.norm) <= b['norm']


def test_a_null_grad_norm_out_changes_no_other_output(hip_device):
    arrays = R.case(N_EDGE, 7, 4.0, seed=23)
    with_norm = device_step(hip_device, arrays, 7)
    without = device_step(hip_device, arrays, 7, norm_out=False)
    for k in OUTPUTS:
        assert np.array_equal(bits(with_norm[k]), bits(without[k])), k


def test_host_scalar_entry_equals_the_device_vector_and_the_vector_wins(hip_device):
    """nesie_flat_adamw_step (hyper=None, which dp.FlatAdamW never takes) and
    nesie_flat_adamw_step_dev with [lr, wd] at the same values: identical bits.  A vector that
    differs from the lr / weight_decay arguments is the one that is applied."""
    arrays = R.case(N_EDGE, 7, 4.0, seed=29)
    host, r, b = run_case(hip_device, 'hyper=None', arrays, 7)
    vector = device_step(hip_device, arrays, 7, hyper_dev=[H['lr'], H['wd']])
    for k in OUTPUTS:
        assert np.array_equal(bits(host[k]), bits(vector[k])), k
    assert vector['norm'] == host['norm']
    other = dict(H, lr=2e-3, wd=0.05)
    wins = device_step(hip_device, arrays, 7, hyper_dev=[other['lr'], other['wd']])
    r2 = R.step(*arrays, 7, **other)
    check('hyper vector wins', wins, r2, R.bounds(r2), torch_step(hip_device, arrays, 7, other))
    assert not np.array_equal(bits(wins['p']), bits(host['p']))


def test_a_non_finite_gradient_follows_clip_grad_norm(hip_device):
    """One +inf at element 5.  torch's rule, which the reference's hook has (pinned here, not
    recommended): the norm is inf, the coefficient max_norm / inf = 0, every finite gradient becomes
    0 and inf * 0 is NaN -- in exactly that element of p, g, m and v.  Every other element is the
    referee's with that gradient zeroed and the coefficient 0."""
    p, g, m, v = R.case(N_EDGE, 7, 4.0, seed=31)
    g[5] = np.inf
    got = device_step(hip_device, (p, g, m, v), 7)
    assert got['norm'] == np.inf
    at5 = np.arange(N_EDGE) == 5
    for k in OUTPUTS:
        assert np.array_equal(np.isnan(got[k]), at5), k
    finite_g = g.copy()
    finite_g[5] = 0
    r = R.step(p, finite_g, m, v, 7, coef=0.0, **H)
    got['norm'] = None
    check('inf at 5', got, r, R.bounds(r), keep=~at5)
    assert (got['g'][~at5] == 0).all()


def test_an_empty_vector_returns_without_counting_the_step(hip_device):
    """n = 0: the call returns, ``step`` keeps its value and nothing is written, the norm included.
    This is the kernel's present contract (the launcher returns before either launch)."""
    empty = tuple(np.zeros(0, np.float32) for _ in range(4))
    got = device_step(hip_device, empty, 7, counts=False)
    assert got['norm'] == -1.0 and all(got[k].size == 0 for k in OUTPUTS)


# ---- workspace and repeatability ------------------------------------------------------------------

def raw_step_dev(dev, tensors, step, hyper, norm, ws_ptr, ws_bytes):
    """nesie_flat_adamw_step_dev through the ctypes binding -> status."""
    from nesie_amd import _lib
    p, g, m, v = tensors
    with torch.cuda.device(dev):
        return _lib.load().nesie_flat_adamw_step_dev(
            p.numel(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(),
            hyper.data_ptr(), H['betas'][0], H['betas'][1], H['eps'], H['max_norm'],
            norm.data_ptr(), ws_ptr, ws_bytes, torch.cuda.current_stream(dev).cuda_stream)


def test_workspace_extent_guard_bands_and_a_short_workspace(hip_device):
    """The workspace is exactly nesie_flat_adamw_workspace_bytes() inside a buffer with 4096-byte
    bands of 0xA5 on both sides: the bands are intact afterwards.  One byte less is refused with
    NESIE_ERR_INVALID_ARG (1) and nothing is written."""
    from nesie_amd import _lib
    band = 4096
    need = _lib.load().nesie_flat_adamw_workspace_bytes()
    arrays = R.case(N_EDGE, 7, 4.0, seed=37)

    def fresh():
        tensors = [torch.from_numpy(a.copy()).to(hip_device) for a in arrays]
        step = torch.tensor(6.0, device=hip_device)
        hyper = torch.tensor([H['lr'], H['wd']], dtype=torch.float32, device=hip_device)
        norm = torch.full((), -1.0, device=hip_device)
        buf = torch.full((need + 2 * band,), 0xA5, dtype=torch.uint8, device=hip_device)
        return tensors, step, hyper, norm, buf

    tensors, step, hyper, norm, buf = fresh()
    status = raw_step_dev(hip_device, tensors, step, hyper, norm, buf.data_ptr() + band, need)
    torch.cuda.synchronize()
    assert status == 0 and float(step) == 7
    assert bool((buf[:band] == 0xA5).all()) and bool((buf[band + need:] == 0xA5).all())
    plain = device_step(hip_device, arrays, 7, hyper_dev=[H['lr'], H['wd']])
    for k, a in zip(OUTPUTS, tensors):
        assert np.array_equal(bits(a.cpu().numpy()), bits(plain[k])), k
    assert float(norm) == plain['norm']

    tensors, step, hyper, norm, buf = fresh()
    status = raw_step_dev(hip_device, tensors, step, hyper, norm, buf.data_ptr() + band, need - 1)
    torch.cuda.synchronize()
    assert status == 1
    assert b'workspace_bytes' in _lib.load().nesie_last_error()
    assert float(step) == 6 and float(norm) == -1.0 and bool((buf == 0xA5).all())
    for a, before in zip(tensors, arrays):
        assert np.array_equal(bits(a.cpu().numpy()), bits(before))


@pytest.mark.parametrize('n', [N_EDGE, CAP + 1])
def test_two_runs_give_the_same_bits(hip_device, n):
    """The header comment's fixed summation order: a second run from the same inputs repeats every
    output bit, the norm included.  There is no arm under HipKernels.cu_budget: the optimiser does
    not honour the budget (its grids are 1024 and min(ceil(n / 4096), 1024) workgroups whatever
    nesie_set_cu_count says), so that arm would run the same launches a third time."""
    arrays = R.case(n, 7, 4.0, seed=41)
    a = device_step(hip_device, arrays, 7)
    b = device_step(hip_device, arrays, 7)
    for k in OUTPUTS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a['norm'] == b['norm']


# ---- free run, and the flat state end to end ------------------------------------------------------

def test_200_free_running_steps_drift_no_more_than_torch_float32(hip_device):
    """dp.FlatAdamW.step for 200 steps, the clip switching on and off, beside the float64
    trajectory and float32 torch.optim.AdamW + clip_grad_norm_ on the device.  Errors are measured on
    the movement p - p0 (max |error| over max |movement|): the accumulated movement is what the
    optimiser produces and the parameter's own magnitude would hide it.  dev_err <= 2 ref_err at
    steps 1, 10, 50 and 200: both are float32 evaluations of one recurrence in a different rounding
    order, and the factor 2 is the margin for that difference and nothing else."""
    from nesie_amd import dp
    n, marks = 20_011, (1, 10, 50, 200)
    rng = np.random.default_rng(43)
    p0 = rng.standard_normal(n).astype(np.float32)
    scales = (1e-3, 5.0, 1e-2, 40.0)
    grads = [(rng.standard_normal(n) * scales[i % 4]).astype(np.float32) for i in range(200)]
    _, kept = R.trajectory(p0, grads, keep=marks, **H)
    a = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(hip_device))
    b = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(hip_device))
    opt_a = dp.FlatAdamW(a, lr=H['lr'], betas=H['betas'], eps=H['eps'], weight_decay=H['wd'],
                         max_norm=H['max_norm'])
    opt_b = torch.optim.AdamW([b], lr=H['lr'], betas=H['betas'], eps=H['eps'], weight_decay=H['wd'])
    clipped = 0
    for t, g in enumerate(grads, start=1):
        a.grad = torch.from_numpy(g.copy()).to(hip_device)
        b.grad = torch.from_numpy(g.copy()).to(hip_device)
        torch.nn.utils.clip_grad_norm_([b], H['max_norm'])
        opt_a.step()
        opt_b.step()
        if t in marks:
            want = kept[t].p - p0
            dev_err, ref_err = (np.abs(w.detach().cpu().numpy().astype(np.float64) - p0 - want).max()
                                / np.abs(want).max() for w in (a, b))
            clipped += kept[t].coef < 1
            print(f'\n[free run t={t}] dev_err {dev_err:.3e} ref_err {ref_err:.3e} '
                  f'ratio {dev_err / ref_err:.3f}')
            assert dev_err <= 2 * ref_err, t
    assert float(opt_a.state[a]['step']) == 200
    assert clipped == 3                       # step 1 runs unclipped (scale 1e-3); 10, 50, 200 clipped


def test_flat_train_state_against_its_float64_twin_and_the_gaps_stay_zero(hip_device):
    """Linear(6, 5) / ReLU / Linear(5, 3) through FlatTrainState + FlatAdamW(max_norm=10) on the
    device beside a float64 CPU copy under per-parameter torch.optim.AdamW + clip_grad_norm_ over all
    its parameters, three steps.  Every parameter stays within the sum of the per-step bounds the
    referee gives on the float64 trajectory, grad_norm within the norm's bound, and the alignment
    gaps (sizes 30, 5, 15, 3 start at 0, 32, 40, 56 of 60) hold +0.0 in the parameter, the
    gradient and both moments after every step -- by their bits, so that -0.0 would fail."""
    from nesie_amd import dp
    torch.manual_seed(47)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))
    twin = copy.deepcopy(model).double()
    model = model.to(hip_device)
    state = dp.FlatTrainState(model.parameters())
    opt = dp.FlatAdamW(state.flat_param, lr=H['lr'], betas=H['betas'], eps=H['eps'],
                       weight_decay=H['wd'], max_norm=H['max_norm'])
    h64 = dict(lr=R.rounded(H['lr']), betas=tuple(R.rounded(x) for x in H['betas']),
               eps=R.rounded(H['eps']), weight_decay=R.rounded(H['wd']))
    opt64 = torch.optim.AdamW(twin.parameters(), **h64)
    total, spans = state.flat.numel(), [(o, p.numel()) for o, p in zip(state.offsets, state.params)]
    assert total == 60 and [o for o, _ in spans] == [0, 32, 40, 56]
    gap = np.ones(total, dtype=bool)
    for o, k in spans:
        gap[o:o + k] = False
    assert gap.sum() == 7

    def flat64(tensors):
        out = np.zeros(total)
        for (o, k), x in zip(spans, tensors):
            out[o:o + k] = x.detach().numpy().reshape(-1)
        return out

    xs = [torch.randn(7, 6, dtype=torch.float64) for _ in range(3)]
    m64, v64, allowed = np.zeros(total), np.zeros(total), np.zeros(total)
    for t, x in enumerate(xs, start=1):
        state.begin()
        model(x.float().to(hip_device)).square().sum().backward()
        state.collect()
        opt.step()
        opt64.zero_grad()
        twin(x).square().sum().backward()
        p_before = flat64(list(twin.parameters()))
        r = R.step(p_before, flat64([p.grad for p in twin.parameters()]), m64, v64, t, **H)
        b = R.bounds(r)
        norm64 = float(torch.nn.utils.clip_grad_norm_(twin.parameters(), H['max_norm']))
        opt64.step()
        m64, v64 = r.m, r.v
        assert r.norm == pytest.approx(norm64, rel=1e-12)
        np.testing.assert_allclose(r.p, flat64(list(twin.parameters())), rtol=1e-11, atol=1e-300)
        allowed += b['p']
        got = state.flat_param.detach().cpu().numpy()
        err = np.abs(got.astype(np.float64) - r.p)
        norm_err = abs(float(opt.grad_norm) - r.norm)
        print(f'\n[flat state t={t}] p: dev_err {err.max():.3e} err/bound {worst(err, allowed):.3f} | '
              f'norm: dev_err {norm_err:.3e} err/bound {norm_err / b["norm"]:.3f} '
              f'(coef {r.coef:.4f})')
        assert worst(err, allowed) <= 1.0
        assert norm_err <= b['norm']
        st = opt.state[state.flat_param]
        for name, vec in (('flat_param', state.flat_param), ('grad', state.flat_param.grad),
                          ('exp_avg', st['exp_avg']), ('exp_avg_sq', st['exp_avg_sq'])):
            assert (bits(vec.detach().cpu().numpy())[gap] == 0).all(), (name, t)
    assert state.flat_param.grad.data_ptr() == state.flat.data_ptr()
