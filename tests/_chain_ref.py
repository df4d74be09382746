"""A float64 restatement of the fused MLP chains (``mmdet3d_ops/fused_mlp.py``) in plain torch:
differentiable, written from the docstrings of the five autograd functions, with no call into
``nesie_amd.kernels``.  tests/test_fused_chains_fp64_gpu.py holds the device's outputs and
gradients against it; tests/test_chain_ref_cpu.py holds IT against the project's own modules
evaluated module by module in float64 (a referee for the referee).

Every evaluation also records the decisions of the network: every layer's normalised
pre-activation (the ReLU's input) and, for pooled layers, the values the maximum is taken over.
From them comes the decision margin of a case: ``E_ref`` = the largest difference between the
float32 and the float64 evaluation of any normalised pre-activation, ``margin = 4 E_ref``.  A seed
QUALIFIES when the float64 evaluation has no pre-activation within the margin of zero and no pooled
group whose two largest values are closer than the margin (both positive, where a ReLU sits in
front of the maximum; for a maximum over values that no ReLU clipped and no norm scaled, the margin
is taken from the float32 error of those values where that is larger).  At such a seed a float32
evaluation in any summation order takes the decisions of float64, so gradients can be compared at
rounding level with no element excused.

``python -m tests._chain_ref`` searches seeds 0..199 per data set and prints the first that
qualifies; that seed is committed in ``DATA`` below and re-checked by the CPU tier.

Data: inputs ``randn``, weights ``randn / sqrt(Cin)``, norm scales uniform in [-1, 1.5] (a negative
scale sends the pooled layers through their minima), shifts N(0, 0.3), upstream gradients ``randn``.
Everything is generated in float32 on the CPU from the seed alone."""
import math

import torch

MOMENTUM, EPS = 0.1, 1e-5       # nn.BatchNorm's defaults, which the modules keep
SEEDS = range(200)
MARGIN_FACTOR = 4.0


class Trace:
    """What one evaluation decided: ``pre`` = the normalised pre-activations, ``pools`` =
    [(values with the pooled axis last, a ReLU sits in front)], ``stats`` = the running (mean,
    variance) every norm leaves behind."""

    def __init__(self):
        self.pre, self.pools, self.stats = [], [], []


# ---- the layers --------------------------------------------------------------------------------------

def batch_norm(trace, z, gamma, beta, bn, axes, chan_bias=None):
    """Training-mode BatchNorm of z over ``axes`` (every other axis indexes a channel, in the order
    of gamma's entries): biased variance in the values; the running statistics move by
    ``momentum`` towards the batch mean (+ ``chan_bias``: the bias of the conv in front, which the
    values never see) and the UNBIASED batch variance."""
    rm, rv, momentum, eps = bn
    n = math.prod(z.shape[a] for a in axes)
    mean = z.mean(axes, keepdim=True)
    var = (z - mean).square().mean(axes, keepdim=True)
    a = (z - mean) * torch.rsqrt(var + eps) * gamma.view(mean.shape) + beta.view(mean.shape)
    with torch.no_grad():
        m = mean.reshape(-1) if chan_bias is None else mean.reshape(-1) + chan_bias.reshape(-1)
        trace.stats.append(((1 - momentum) * rm.to(z.dtype) + momentum * m,
                            (1 - momentum) * rv.to(z.dtype) + momentum * var.reshape(-1) * (n / (n - 1))))
    trace.pre.append(a)
    return a


def eval_norm(trace, z, gamma, beta, bn, shape):
    rm, rv, _, eps = bn
    a = (z - rm.view(shape)) * torch.rsqrt(rv.view(shape) + eps) * gamma.view(shape) + beta.view(shape)
    trace.pre.append(a)
    return a


def group_max(trace, v, relu):
    """Maximum over the last axis."""
    trace.pools.append((v, relu))
    return v.max(-1).values


def sa_stack(trace, x, params, bufs, training=True):
    """SAStackFn: x (B, C0, M, ns) -> max_ns relu(bn_L(conv_L(... relu(bn_1(conv_1 x))))) (B, C_L, M);
    params = [W (Cout, Cin, 1, 1), gamma, beta] per layer."""
    a = x
    for l, bn in enumerate(bufs):
        w, gamma, beta = params[3 * l:3 * l + 3]
        z = torch.einsum('oc,bcmn->bomn', w.flatten(1), a)
        if training:
            a = torch.relu(batch_norm(trace, z, gamma, beta, bn, (0, 2, 3)))
        else:
            a = torch.relu(eval_norm(trace, z, gamma, beta, bn, (1, -1, 1, 1)))
    return group_max(trace, a, True)


def grouped_conv(w, a):
    """w (S, Cout, Cin), a (B, S, Cin, P) -> (B, S, Cout, P): net s has its own matrix."""
    return torch.einsum('soc,bscp->bsop', w, a)


def stack1d(trace, x, layers, S, tensors):
    """Stack1dFn: x (NB, C0, P), batch n uses weight group n % S.  ``layers`` = [(bias, bn | None)],
    ``tensors`` = per layer W (S, Cout, Cin), bias (S * Cout) if any, gamma, beta (S * Cout) if a
    norm.  A bias in front of a norm leaves the values alone and enters the running mean; a last
    layer with a norm returns the activation, one without W a + b."""
    NB, c0, P = x.shape
    a = x.view(NB // S, S, c0, P)
    i = 0
    for bias, bn in layers:
        w = tensors[i]
        b = tensors[i + 1] if bias else None
        i += 1 + bool(bias)
        z = grouped_conv(w, a)
        if bn is not None:
            gamma, beta = tensors[i], tensors[i + 1]
            i += 2
            a = torch.relu(batch_norm(trace, z, gamma, beta, bn, (0, 3),
                                      chan_bias=None if b is None else b.detach()))
        else:
            a = z if b is None else z + b.view(1, S, -1, 1)
    return a.reshape(NB, -1, P)


def mini_head(trace, c0, bn0, G, gamma0, beta0, w3, coef0=None):
    """MiniHeadFn: c0 (B, S, H0, K*G) -> c = W3 . relu(bn0(c0)) (B, S, half, K*G), g = max_G c.
    ``coef0`` (S*H0, 4): evaluation mode, relu(scale c0 + shift) from its first two columns."""
    B, S, H0, P = c0.shape
    if coef0 is None:
        a0 = batch_norm(trace, c0, gamma0, beta0, bn0, (0, 3))
    else:
        a0 = c0 * coef0[:, 0].view(1, S, H0, 1) + coef0[:, 1].view(1, S, H0, 1)
        trace.pre.append(a0)
    c = grouped_conv(w3, torch.relu(a0))
    return c, group_max(trace, c.view(B, S, -1, P // G, G), False)


def mini_tail(trace, c, small, bn1, G, wl, gamma1, beta1, w4, coef1=None):
    """MiniTailFn: max_G W4 . relu(bn1(W_l c + small)), small (B, S, H2, K) a row bias per group of
    G positions -> (B, S, F, K)."""
    B, S, half, P = c.shape
    H2 = wl.shape[1]
    y = grouped_conv(wl, c) + small.repeat_interleave(G, dim=-1)
    if coef1 is None:
        a1 = batch_norm(trace, y, gamma1, beta1, bn1, (0, 3))
    else:
        a1 = y * coef1[:, 0].view(1, S, H2, 1) + coef1[:, 1].view(1, S, H2, 1)
        trace.pre.append(a1)
    out = grouped_conv(w4, torch.relu(a1))
    return group_max(trace, out.view(B, S, -1, P // G, G), False)


def blend_conv(table, wx, idx, weight, rel, segs, seg_len):
    """The first conv of ``segs`` MiniPointNets through the 3-NN blend (``interpolate.BlendConv``,
    include/nesie_ops.h): the n = K * segs * seg_len queries are ordered (proposal k, face s, grid
    point g); query (k, s, g) lands at out[b, s, ch, k * seg_len + g] =
    sum_j weight[q, j] table[b, idx[q, j], s * H + ch] + wx[s, ch] . rel[q]."""
    b, m, pitch = table.shape
    h = pitch // segs
    n = idx.shape[1]
    k = n // (segs * seg_len)
    rows = table[torch.arange(b).view(b, 1, 1), idx.long()]             # (b, n, 3, pitch)
    mixed = (rows * weight.unsqueeze(-1)).sum(2).view(b, k, segs, seg_len, segs, h)
    face = torch.stack([mixed[:, :, s, :, s] for s in range(segs)], 1)  # (b, segs, k, seg_len, h)
    r = rel.view(b, k, segs, seg_len, 3).permute(0, 2, 1, 3, 4)
    out = face + torch.einsum('shj,bskgj->bskgh', wx, r)
    return out.permute(0, 1, 4, 2, 3).reshape(b, segs, h, k * seg_len)


def stat_partials(c0):
    """(sum, sum of squares) of c0 (B, S, H, P) per 64-position tile in the blend kernel's layout
    (S*H, B*P/64, 2), summed in float64."""
    B, S, H, P = c0.shape
    flat = c0.permute(1, 2, 0, 3).reshape(S * H, B * P // 64, 64).double()
    return torch.stack([flat.sum(-1), flat.square().sum(-1)], -1).float().contiguous()


# ---- data ----------------------------------------------------------------------------------------------
# name -> what is generated and the committed seed (python -m tests._chain_ref prints them).  Several
# cases of the device test share one data set: they differ in the route, not in the numbers.
B = 2
H0, HALF, H2, F = 256, 128, 256, 128       # the MiniPointNets' built widths

DATA = {
    'sa1': dict(family='sa', chans=(4, 64, 64, 128), ns=64, M=2, seed=7),
    'sa2': dict(family='sa', chans=(131, 128, 128, 256), ns=32, M=2, seed=1),
    'sa_no_lead': dict(family='sa', chans=(128, 128, 256), ns=32, M=2, seed=1),
    'sa_two': dict(family='sa', chans=(4, 64, 128), ns=16, M=4, seed=1),
    'sa_259': dict(family='sa', chans=(259, 128, 128), ns=16, M=4, seed=4),
    # evaluation mode is forward only: values are continuous across a decision, any seed serves
    'sa2_eval': dict(family='sa', chans=(131, 128, 128, 256), ns=32, M=2, training=False, seed=0, search=False),
    'sa_two_eval': dict(family='sa', chans=(4, 64, 128), ns=16, M=4, training=False, seed=0, search=False),
    's1d_bias_norm_then_bias': dict(family='s1d', S=2, c0=64, P=64, spec=[(128, True, True), (32, True, False)],
                                    seed=1),
    's1d_norm_everywhere': dict(family='s1d', S=1, c0=64, P=64,
                                spec=[(128, False, True), (128, True, True), (64, True, True)], seed=0),
    's1d_single_bias_layer': dict(family='s1d', S=2, c0=32, P=64, spec=[(256, True, False)], seed=0),
    's1d_input_without_grad': dict(family='s1d', S=1, c0=64, P=64, spec=[(128, True, True), (16, True, False)],
                                   seed=0),
    's1d_input_grad_matmul': dict(family='s1d', S=2, c0=64, P=64, spec=[(128, True, True), (32, False, False)],
                                  seed=1),
    's1d_sliced_gradient': dict(family='s1d', S=1, c0=64, P=64, spec=[(128, False, True), (16, True, False)],
                                seed=0),
    's1d_ragged_220': dict(family='s1d', S=1, c0=64, P=64, spec=[(128, False, True), (220, True, False)],
                           seed=0),
    's1d_slots': dict(family='s1d', S=1, c0=64, P=64,
                      spec=[(128, True, True), (128, False, True), (16, True, False)], seed=0),
    'mini_s2_g16': dict(family='mini', S=2, G=16, P=64, seed=47),
    'mini_s1_g64': dict(family='mini', S=1, G=64, P=128, seed=12),
    'mini_eval_s2_g16': dict(family='mini', S=2, G=16, P=64, training=False, seed=0, search=False),
    'mini_eval_s1_g64': dict(family='mini', S=1, G=64, P=128, training=False, seed=0, search=False),
    'blend': dict(family='blend', S=2, G=16, P=64, m=16, seed=0),
}


class _Gen:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(int(seed))

    def randn(self, *shape, scale=1.0):
        return torch.randn(*shape, generator=self.g) * scale

    def weight(self, *shape):           # (..., Cout, Cin[, 1, 1])
        cin = shape[-1] if shape[-1] != 1 else shape[-3]
        return torch.randn(*shape, generator=self.g) / math.sqrt(cin)

    def gamma(self, n):
        return torch.rand(n, generator=self.g) * 2.5 - 1.0

    def beta(self, n):
        return torch.randn(n, generator=self.g) * 0.3

    def running(self, n, training):
        """A norm's buffers: fresh ones for a training step, non-trivial ones for evaluation."""
        if training:
            return torch.zeros(n), torch.ones(n)
        return torch.randn(n, generator=self.g) * 0.3, torch.rand(n, generator=self.g) + 0.5


def make(name, seed=None):
    """-> {tensor name: float32 CPU tensor} of data set ``name``: the differentiable leaves, the
    constants, the norms' buffers (``rm<i>``, ``rv<i>``) and the upstream gradients (``g_<output>``)."""
    cfg = DATA[name]
    gen = _Gen(cfg['seed'] if seed is None else seed)
    training = cfg.get('training', True)
    d = {}
    fam = cfg['family']
    if fam == 'sa':
        chans = cfg['chans']
        d['x'] = gen.randn(B, chans[0], cfg['M'], cfg['ns'])
        for l, (cin, cout) in enumerate(zip(chans, chans[1:])):
            d[f'w{l}'], d[f'gamma{l}'], d[f'beta{l}'] = gen.weight(cout, cin, 1, 1), gen.gamma(cout), gen.beta(cout)
            d[f'rm{l}'], d[f'rv{l}'] = gen.running(cout, training)
        d['g_out'] = gen.randn(B, chans[-1], cfg['M'])
    elif fam == 's1d':
        S, cin = cfg['S'], cfg['c0']
        d['x'] = gen.randn(B * S, cin, cfg['P'])
        for l, (cout, bias, norm) in enumerate(cfg['spec']):
            d[f'w{l}'] = gen.weight(S, cout, cin)
            if bias:
                d[f'b{l}'] = gen.randn(S * cout, scale=0.5)
            if norm:
                d[f'gamma{l}'], d[f'beta{l}'] = gen.gamma(S * cout), gen.beta(S * cout)
                d[f'rm{l}'], d[f'rv{l}'] = gen.running(S * cout, True)
            cin = cout
        d['g_out'] = gen.randn(B * S, cin, cfg['P'])
    elif fam in ('mini', 'blend'):
        S, G, P = cfg['S'], cfg['G'], cfg['P']
        if fam == 'blend':
            m, n = cfg['m'], S * P
            d['table'] = gen.randn(B, m, S * H0, scale=0.5)
            d['wx'] = gen.randn(S, H0, 3)
            d['idx'] = torch.randint(0, m, (B, n, 3), generator=gen.g, dtype=torch.int32)
            w = torch.rand(B, n, 3, generator=gen.g) + 0.05
            d['weight'] = (w / w.sum(-1, keepdim=True)).contiguous()
            d['rel'] = gen.randn(B, n, 3, scale=0.3)
        else:
            d['c0'] = gen.randn(B, S, H0, P)
        d['gamma0'], d['beta0'] = gen.gamma(S * H0), gen.beta(S * H0)
        d['rm0'], d['rv0'] = gen.running(S * H0, training)
        d['w3'] = gen.weight(S, HALF, H0)
        if fam == 'blend':
            d['g_c'], d['g_g'] = gen.randn(B, S, HALF, P), gen.randn(B, S, HALF, P // G)
        else:
            d['w'] = gen.weight(S, H2, 2 * HALF)                # second_conv[0]: (global half, local half)
            d['bias'] = gen.randn(S * H2, scale=0.5)            # W_g b3 + W_l b3 of the modules
            d['gamma1'], d['beta1'] = gen.gamma(S * H2), gen.beta(S * H2)
            d['rm1'], d['rv1'] = gen.running(S * H2, training)
            d['w4'] = gen.weight(S, F, H2)
            d['g_out'], d['g_c'] = gen.randn(B, S, F, P // G), gen.randn(B, S, HALF, P)
    else:
        raise KeyError(fam)
    return d


def eval_coef(gamma, beta, rm, rv, eps=EPS):
    """(C, 4) = (scale, shift, 0, 0) of an evaluation-mode norm, formed in float64 and rounded to
    float32 once: the device and both reference evaluations apply the same coefficients."""
    scale = gamma.double() * torch.rsqrt(rv.double() + eps)
    shift = beta.double() - rm.double() * scale
    return torch.stack([scale, shift, torch.zeros_like(scale), torch.zeros_like(scale)], 1).float().contiguous()


# ---- one evaluation --------------------------------------------------------------------------------------

CONSTANTS = ('idx', 'weight', 'rel')


class Result:
    """outs / grads: {name: tensor}; ``trace``: the decisions; ``stats`` = [(running mean, variance)]."""

    def __init__(self, outs, grads, trace):
        self.outs, self.grads, self.trace, self.stats = outs, grads, trace, trace.stats


def leaf_names(data):
    return [k for k in data if not (k.startswith(('g_', 'rm', 'rv')) or k in CONSTANTS)]


def evaluate(name, data, dtype, second_consumer=False, backward=True):
    """The restatement on ``data`` in ``dtype`` -> Result.  Gradients are those of
    sum_o <output o, g_o> with respect to every leaf (and ``small`` for the MiniPointNets); a leaf
    the function does not depend on (the bias in front of a norm) gets zeros.  ``second_consumer``:
    the MiniPointNets' ``c`` also feeds <c, g_c>."""
    cfg = DATA[name]
    fam, training = cfg['family'], cfg.get('training', True)
    t = {k: (v if k == 'idx' else v.detach().clone().to(dtype)) for k, v in data.items()}
    leaves = {k: t[k].requires_grad_(backward) for k in leaf_names(data)}
    trace = Trace()

    def bn(i):
        return t[f'rm{i}'], t[f'rv{i}'], MOMENTUM, EPS
    outs, extra = {}, {}
    if fam == 'sa':
        L = len(cfg['chans']) - 1
        params = [t[f'{k}{l}'] for l in range(L) for k in ('w', 'gamma', 'beta')]
        outs['out'] = sa_stack(trace, t['x'], params, [bn(l) for l in range(L)], training)
    elif fam == 's1d':
        layers, tensors = [], []
        for l, (cout, bias, norm) in enumerate(cfg['spec']):
            tensors.append(t[f'w{l}'])
            if bias:
                tensors.append(t[f'b{l}'])
            if norm:
                tensors += [t[f'gamma{l}'], t[f'beta{l}']]
            layers.append((bias, bn(l) if norm else None))
        outs['out'] = stack1d(trace, t['x'], layers, cfg['S'], tensors)
    else:
        S, G = cfg['S'], cfg['G']
        coef0 = coef1 = None
        if not training:
            coef0 = eval_coef(data['gamma0'], data['beta0'], data['rm0'], data['rv0']).to(dtype)
            coef1 = eval_coef(data['gamma1'], data['beta1'], data['rm1'], data['rv1']).to(dtype)
        c0 = t['c0'] if fam == 'mini' else blend_conv(t['table'], t['wx'], t['idx'], t['weight'], t['rel'], S, G)
        c, g = mini_head(trace, c0, bn(0), G, t['gamma0'], t['beta0'], t['w3'], coef0)
        if fam == 'blend':
            outs['c'], outs['g'] = c, g
        else:
            w_g, w_l = t['w'].split(HALF, dim=2)
            small = grouped_conv(w_g, g) + t['bias'].view(1, S, H2, 1)
            extra['small'] = small
            outs['out'] = mini_tail(trace, c, small, bn(1), G, w_l, t['gamma1'], t['beta1'], t['w4'], coef1)
            if second_consumer or not training:
                outs['c'] = c
            if not training:
                outs['g'] = g
    grads = {}
    if backward:
        loss = sum((outs[k] * t['g_' + k]).sum() for k in outs)
        wrt = dict(leaves, **extra)
        got = torch.autograd.grad(loss, list(wrt.values()), allow_unused=True)
        grads = {k: (torch.zeros_like(v) if g_ is None else g_).detach() for (k, v), g_ in zip(wrt.items(), got)}
    return Result({k: v.detach() for k, v in outs.items()}, grads, trace)


# ---- the decision margin ----------------------------------------------------------------------------------

def reference_errors(r32, r64):
    """-> (E_ref, E_pool): the largest float32 error of a normalised pre-activation, and of a value
    that a maximum without a ReLU in front is taken over."""
    def err(a, b):
        return float((a.detach().double() - b.detach()).abs().max())
    if r64.trace.pre:
        e_ref = max(err(a, b) for a, b in zip(r32.trace.pre, r64.trace.pre))
    else:       # a chain without a norm decides nothing: the float32 error of what it returns
        e_ref = max(err(r32.outs[k], r64.outs[k]) for k in r64.outs)
    e_pool = max([err(a, b)
                  for (a, relu), (b, _) in zip(r32.trace.pools, r64.trace.pools) if not relu], default=0.0)
    return e_ref, e_pool


def margins(r32, r64):
    """-> (margin, the margin of the maxima that no ReLU precedes)."""
    e_ref, e_pool = reference_errors(r32, r64)
    return MARGIN_FACTOR * e_ref, MARGIN_FACTOR * max(e_ref, e_pool)


def violations(r64, margin, pool_margin):
    """How many decisions of the float64 evaluation lie within the margin."""
    bad = sum(int((a.abs() <= margin).sum()) for a in r64.trace.pre)
    for v, relu in r64.trace.pools:
        top = v.topk(2, dim=-1).values
        gap = top[..., 0] - top[..., 1]
        bad += int(((top[..., 1] > 0) & (gap <= margin)).sum()) if relu else int((gap <= pool_margin).sum())
    return bad


def same_decisions(r32, r64):
    """The float32 evaluation's ReLU masks and arg-max equal float64's."""
    for a, b in zip(r32.trace.pre, r64.trace.pre):
        if not torch.equal(a > 0, b > 0):
            return False
    for (a, relu), (b, _) in zip(r32.trace.pools, r64.trace.pools):
        live = b.max(-1).values > 0 if relu else torch.ones_like(b[..., 0], dtype=torch.bool)
        if not torch.equal(a.argmax(-1)[live], b.argmax(-1)[live]):
            return False
    return True


def qualifies(name, seed, second_consumer=False):
    """-> (qualifies, margin, r32, r64) of data set ``name`` at ``seed``."""
    data = make(name, seed)
    backward = DATA[name].get('training', True)
    r32 = evaluate(name, data, torch.float32, second_consumer, backward)
    r64 = evaluate(name, data, torch.float64, second_consumer, backward)
    margin, pool_margin = margins(r32, r64)
    return violations(r64, margin, pool_margin) == 0, margin, r32, r64


def search(name):
    for seed in SEEDS:
        if qualifies(name, seed)[0]:
            return seed
    return None


if __name__ == '__main__':
    import sys
    for name_, cfg_ in DATA.items():
        if cfg_.get('search', True) and (len(sys.argv) == 1 or name_ in sys.argv[1:]):
            found = search(name_)
            print(f'{name_}: seed {found}' + ('' if found == cfg_['seed'] else f'   (table: {cfg_["seed"]})'), flush=True)
