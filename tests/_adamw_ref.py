"""Referee of the flat optimiser tests (nesie_amd/csrc/optim.hip): clip by global norm + AdamW in
plain numpy float64.  It shares no code with the package.

The hyper-parameters are the ABI's.  ``nesie_flat_adamw_step`` takes lr, beta1, beta2, eps,
weight_decay and max_norm as ``float`` and the kernel forms ``1.f - beta2`` from the rounded value.
float(0.999) is 0.99900001287, so ``1.f - beta2`` lies 1.29e-5 below 0.001, relatively: about 217 u
with u = 2^-24.  The kernel is self-consistent as "Adam with beta = float(beta)": at t = 1 the same
deficit sits in v and in the bias correction and cancels, and the update is within a few u of the
float64 form THAT USES THE FLOAT-ROUNDED HYPER-PARAMETERS.  Against float64 with the double 0.999
the second moment is 217 u off; that offset is the ABI's rounding, not a kernel error.  ``step``
therefore rounds every hyper-parameter to float32 first and widens it again
(tests/test_adamw_ref_cpu.py asserts the 217 u as a fact about the ABI).

``step``        one step, with the magnitude S of each output (the same formulas on absolute
                operands): what the bounds are stated in, so that a moment or an update that cancels
                to near zero is judged by the size of its terms (the ``absolute=True`` idea of
                tests/_spconv_ref.py).
``bounds``      a-priori float32 bounds k * u * S per output, k counted from the kernel source.
``trajectory``  free-running float64 steps from given gradients.
"""
import types

import numpy as np

U = 2.0 ** -24
PARTS, BLOCK = 1024, 256          # OPT_PARTS, OPT_BLOCK of optim.hip
TINY = 2.0 ** -126                # one float32 min normal: a product that underflows (or is flushed)

# powf of the device library.  The ROCm installation carries no accuracy table for the device math
# functions (its share/doc holds the HIP runtime API and licences only), so the figure is the one
# the public HIP documentation states: "HIP math API", single-precision mathematical functions,
# powf: maximum ULP difference 1.
E_POW_ULPS = 1.0

# first-order sums of roundings are closed by this factor: the largest relative bound in use is about
# 1100 u = 6.6e-5, its square 4e-9 of itself
SECOND_ORDER = 1.001


def rounded(x):
    """A hyper-parameter as the C ABI carries it: float32, widened."""
    return float(np.float32(x))


def step(p, g, m, v, t, lr, betas, eps, wd, max_norm, coef=None, round_hyper=True):
    """One step on float32 arrays, widened here (float64 arrays are taken as they are: a float64
    trajectory); ``t`` is the step count AFTER the increment.
    lr, beta1, beta2, eps, wd and max_norm are each rounded to float32 first (module docstring).
    ``max_norm`` None, 0 or negative: no clipping.  ``coef``: overrides the clip coefficient (the
    non-finite case of the GPU tests).  ``round_hyper=False`` keeps the hyper-parameters double:
    only to measure what the ABI's rounding costs.

      norm = sqrt(sum g^2);  c = max_norm / (norm + 1e-6), coef = min(1, c)  (1 without clipping)
      g' = g coef;  p' = p - p (lr wd);  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
      p'' = p' - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

    -> namespace: p, g, m, v (float64), norm, coef, coef_raw (c before the clamp; inf without
    clipping), bc1, bc2, denom, S_p, S_g, S_m, S_v, S_u, and the inputs of ``bounds``."""
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    cut = rounded if round_hyper else float
    lr, b1, b2, eps, wd = (cut(x) for x in (lr, betas[0], betas[1], eps, wd))
    mx = cut(max_norm) if max_norm else 0.0
    with np.errstate(all='ignore'):
        norm = float(np.sqrt(np.sum(g * g)))
        raw = mx / (norm + 1e-6) if mx > 0 else float('inf')
        if coef is None:
            coef = min(1.0, raw)
        g1 = g * coef
        decay = np.abs(p) * (lr * wd)
        p1 = p - p * (lr * wd)
        m1 = b1 * m + (1 - b1) * g1
        v1 = b2 * v + (1 - b2) * g1 * g1
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        denom = np.sqrt(v1) / np.sqrt(bc2) + eps
        p2 = p1 - (lr / bc1) * m1 / denom
        s_m = np.abs(b1 * m) + np.abs((1 - b1) * g1)
        s_u = (lr / bc1) * s_m / denom
    return types.SimpleNamespace(
        p=p2, g=g1, m=m1, v=v1, norm=norm, coef=coef, coef_raw=raw, bc1=bc1, bc2=bc2, denom=denom,
        S_p=np.abs(p) + decay + s_u, S_g=np.abs(g1), S_m=s_m, S_v=v1, S_u=s_u, decay=decay,
        n=int(p.size), t=t, b1=b1, b2=b2, clipping=mx > 0, coef_forced=coef != min(1.0, raw))


def gamma(k):
    return k * U / (1 - k * U)


def norm_chain(n):
    """The longest chain of float32 additions an element of the squared norm sees, plus one for
    its square: ceil(ceil(n / 1024) / 256) serial adds in a thread of sumsq_partials_kernel, 6 for
    the wave sum, 2 for the block; then the fold of the 1024 partials in adamw_clip_kernel: 4
    serial, 6 for the wave, 2 for the block."""
    per = -(-n // PARTS)
    return -(-per // BLOCK) + 6 + 2 + (4 + 6 + 2) + 1


def norm_rel_bound(n):
    """|norm_dev - norm64| <= (gamma_k / 2 + 2 u) norm64: the sum of squares is within gamma_k, the
    square root halves that and adds its own rounding (the second u closes the second order)."""
    return gamma(norm_chain(n)) / 2 + 2 * U


def bc_rel_bound(beta, t):
    """Relative bound of bc = fl(1 - fl(powf(beta, t))).  powf is within E_POW_ULPS ulp of beta^t
    (absolute: E_POW_ULPS * spacing(beta^t), at least TINY for a flushed denormal), so bc carries
    that absolute error over 1 - beta^t -- at t = 1 and beta2 = 0.999 about 1000 u -- and one
    rounding of the subtraction (exact by Sterbenz for beta^t >= 0.5, counted all the same)."""
    x = beta ** t
    ulp = float(np.spacing(np.float32(x))) if x >= TINY else 0.0
    return max(E_POW_ULPS * ulp, TINY) / (1 - x) + U


def bounds(r):
    """A-priori bounds of a float32 evaluation of ``r = step(...)`` in the kernel's operation order
    (optim.hip is built with -ffp-contract=off: every operation rounds once).  u = 2^-24; each line
    is one rounding, relative to the magnitude S of the output it ends in.

    coefficient, relative e_c (0 when no clipping can happen: max_norm <= 0, or c (1 - e) >= 1, or
    the coefficient was forced):
        the norm's bound (``norm_rel_bound``)
      + u  total + 1e-6f
      + u  max_norm / (...)
      + u  the constant 1e-6f itself, at most u of the denominator
    g' (2):  e_c, and
      1  g * coef
    m' (4):  e_c, and on the g' term of the sum
      1  g'                          (above)
      1  1.f - beta1                 (exact for beta1 >= 0.5; counted)
      1  (1.f - beta1) * g'
      1  the sum
      (the other term carries 2, beta1 * m and the sum: the larger count is taken for both)
    v' (6):  2 e_c, and
      2  g', twice in the square
      1  g' * g'
      1  1.f - beta2
      1  (1.f - beta2) * (...)
      1  the sum
    update (15):  2 e_c + e_bc1 + e_bc2 / 2, and
      4  m'                          (above)
      3  sqrtf(v'): half of v's 6
      1  sqrtf's own rounding
      1  sqrtf(bc2)                  (e_bc2 / 2 from its operand)
      1  1.f / sqrtf(bc2)
      1  sqrtf(v') * inv_sqrt_bc2
      1  ... + eps                   (both terms positive: the sum's relative error is at most the
                                      larger term's, plus this rounding)
      1  m' / denom
      1  lr / bc1                    (e_bc1 from its operand)
      1  step_size * (...)
      (v's e_c enters the denominator once, 2 e_c / 2, and m's once: 2 e_c)
    p'':  the update's bound, and
      2  lr * wd and p * (lr wd), on |p| lr wd
      1  p - p (lr wd), on |p'| <= S_p
      1  p' - update, on |p''| <= S_p
    e_bc1, e_bc2: ``bc_rel_bound``.  Every bound is closed by SECOND_ORDER and gets TINY for a
    product that underflows.  -> dict p, g, m, v (arrays), norm (absolute), e_coef, e_bc1, e_bc2."""
    e_norm = norm_rel_bound(r.n)
    e_c = e_norm + 3 * U
    if not r.clipping or r.coef_forced or r.coef_raw * (1 - e_c) >= 1:
        e_c = 0.0
    e_bc1, e_bc2 = bc_rel_bound(r.b1, r.t), bc_rel_bound(r.b2, r.t)
    k = SECOND_ORDER
    b_g = k * (e_c + (U if r.coef != 1.0 else 0.0)) * r.S_g
    b_m = k * (4 * U + e_c) * r.S_m + TINY
    b_v = k * (6 * U + 2 * e_c) * r.S_v + TINY
    b_u = k * (15 * U + 2 * e_c + e_bc1 + e_bc2 / 2) * r.S_u + TINY
    b_p = b_u + k * U * (2 * r.decay + 2 * r.S_p)
    return dict(p=b_p, g=b_g, m=b_m, v=b_v, norm=k * e_norm * r.norm, e_coef=e_c, e_bc1=e_bc1,
                e_bc2=e_bc2)


def trajectory(p0, grads, lr, betas, eps, wd, max_norm, keep=()):
    """Free-running float64 steps from zero moments: gradient i (float32) drives step i + 1 and
    the state stays float64 between steps.  -> (the last step's namespace, {t: the namespace of
    step t for t in keep})."""
    p = np.asarray(p0, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    kept, r = {}, None
    for t, g in enumerate(grads, start=1):
        r = step(p, g, m, v, t, lr, betas, eps, wd, max_norm)
        p, m, v = r.p, r.m, r.v
        if t in keep:
            kept[t] = r
    return r, kept


# ---- the inputs of the tests: a mid-training state with the awkward elements at fixed places ------
HYPER = dict(lr=8e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.01, max_norm=10.0)
ZERO_G, CANCEL, EPS_ONLY, BIG_P, SMALL_P, FIRST = 1, 2, 3, 4, 5, 6


def case(n, t, ratio, seed, hyper=HYPER):
    """float32 p, g, m, v of n elements for a step that ends at count ``t``:
    p ~ N(0, 1), m ~ 0.3 N(0, 1), v = (0.05 + U(0, 1)) min(1, t (1 - beta2)) (zero moments at
    t = 1, as in a real first step, but for EPS_ONLY's m), g ~ N(0, 1) scaled in float64 so that
    its norm is ``ratio`` * max_norm (all zero for ratio 0).  For n > 6, at fixed places:
      ZERO_G    an exact zero gradient
      CANCEL    g with beta1 m = -(1 - beta1) g coef to within rounding (t > 1, and only where that g
                fits inside the wanted norm)
      EPS_ONLY  v = 0 and g = 0, so the denominator is eps alone; p = 0 and m = 0.25, so that
                -p'' is the update itself and bc1 can be read from it
      BIG_P, SMALL_P   parameters of magnitude 1e4 and 1e-4
      FIRST     m = v = p = 0 with a gradient: a first step's element, from which bc2 can be read
      n - 1     a gradient of half the norm: a range that stops short of n then shows in the norm
                whatever n is (one average element of four million would hide below its rounding)."""
    rng = np.random.default_rng(seed)
    b1, mx = rounded(hyper['betas'][0]), rounded(hyper['max_norm'])
    b2 = rounded(hyper['betas'][1])
    p, g = rng.standard_normal(n), rng.standard_normal(n)
    m = 0.3 * rng.standard_normal(n)
    v = (0.05 + rng.random(n)) * min(1.0, t * (1 - b2))
    if t == 1:
        m[:], v[:] = 0, 0
    special = n > FIRST
    if special:
        p[BIG_P], p[SMALL_P] = 1e4, 1e-4
        p[EPS_ONLY], m[EPS_ONLY], v[EPS_ONLY] = 0, 0.25, 0
        p[FIRST], m[FIRST], v[FIRST], g[FIRST] = 0, 0, 0, 1.0
        if t > 1:
            m[CANCEL] = 0.25
        g[ZERO_G] = g[EPS_ONLY] = 0
    m = m.astype(np.float32)
    if ratio == 0:
        g[:] = 0
    else:
        target, fixed = ratio * mx, 0.0
        rest = np.ones(n, dtype=bool)
        if special and t > 1:
            gc = -(b1 * float(m[CANCEL])) / ((1 - b1) * min(1.0, mx / (target + 1e-6)))
            if abs(gc) < target / 2:
                g[CANCEL], rest[CANCEL], fixed = gc, False, gc * gc
        if special:
            g[n - 1], rest[n - 1], fixed = 0.5 * target, False, fixed + 0.25 * target * target
        g[rest] *= np.sqrt(target * target - fixed) / np.sqrt(np.sum(g[rest] ** 2))
    return tuple(a.astype(np.float32) for a in (p, g, m, v))
