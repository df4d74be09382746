"""Every backward branch of the fused MLP chains (``mmdet3d_ops/fused_mlp.py``: SAStackFn, Stack1dFn,
MiniHeadFn, MiniTailFn, BlendMiniHeadFn) on the device against float64 autograd at rounding-level
tolerance, with no element excused.

The reference is tests/_chain_ref.py, a plain-torch float64 restatement that shares no code with the
kernels (tests/test_chain_ref_cpu.py holds it against the modules in float64).  The routes are the
ones tests/test_fused_mlp_trace_cpu.py pins as launch traces -- the case names mirror its ``CASES``
-- taken here by the REAL back end with chosen answers (tests/_forced_hip.py: an answer can only
turn a library "yes" into a "no").

Why rounding-level works: every data set runs at a committed seed at which the float64 evaluation
takes no decision (ReLU mask, arg-max) within ``margin = 4 E_ref`` of its threshold, ``E_ref`` being
the restatement's own float32 error on the normalised pre-activations.  What each case asserts:

* route: the launches that define the branch are present / absent in the back end's launch list;
* forward: max |out_dev - out_f64| <= margin (absolute: the outputs are of order 1); running
  statistics the same, scaled by their largest entry;
* gradients, per returned tensor: max |g_dev - g_f64| <= 8 ref_err with ref_err = the largest of
  max |g_ref32 - g_f64|, 2^-23 max |g_f64| and 2^-23 times the largest entry of any gradient of the
  case (the floor for tensors whose true value is near zero).  The factor 8: the device sums partials
  per workgroup and per slot in another order than torch does.  ``BOUNDS`` lists the tensors that need
  more, each with the cause that can be read in the kernel ("chains against float64");
* the bias in front of a norm: an exact zero tensor (None with a gradient slot);
* a frozen parameter: no gradient at all; a gradient slot of the quality head's functions: bit for bit
  what the same route returns without slots;
* housekeeping: module switches and the injected back end restored, no weight-gradient reduction
  left pending.

Every figure is printed before it is asserted (``-s`` shows the ratio table)."""
import contextlib

import pytest
import torch

from nesie_amd import _lib, grad_slots
from nesie_amd.kernels import HipKernels
from nesie_amd.mmdet3d_ops import fused_mlp
from tests import _chain_ref as ref
from tests._forced_hip import forced_hip

pytestmark = pytest.mark.gpu

GRAD_FACTOR = 8.0
# (case, tensor) -> bound on dev_err / ref_err where the default 8 does not hold: twice the measured
# ratio, never above 64; the cause of each is stated in DESIGN.md ("chains against float64")
BOUNDS = {}
SENTINEL = -7777.0
APPLY_PASS = {'pool_tail_supported': False, 'pw_wgrad_bn_supported': False}
ATEN_WGRAD = dict(APPLY_PASS, pw_wgrad_tiled=False, pw_wgrad_supported=False)


def _refuse(*shape):
    """An answer that refuses exactly the product (k, cout) = ``shape``: the input-gradient one."""
    return lambda k, cout, p: (k, cout) != shape


# ---- the reference, evaluated once per data set ----------------------------------------------------------

_REFERENCE = {}


def _reference(data_name, second_consumer=False):
    """-> (data, margin, float32 Result, float64 Result); computed once, shared, never modified."""
    key = (data_name, second_consumer)
    if key not in _REFERENCE:
        ok, margin, r32, r64 = ref.qualifies(data_name, ref.DATA[data_name]['seed'], second_consumer)
        assert ok or not ref.DATA[data_name].get('search', True), f'{data_name}: the committed seed does not qualify'
        _REFERENCE[key] = (ref.make(data_name), margin, r32, r64)
    return _REFERENCE[key]


# ---- running a case --------------------------------------------------------------------------------------

@contextlib.contextmanager
def _route(answers, switches, atomic=False):
    keep = {k: getattr(fused_mlp, k) for k in switches}
    deterministic = HipKernels.DETERMINISTIC
    try:
        for k, v in switches.items():
            setattr(fused_mlp, k, v)
        if atomic:
            HipKernels.set_deterministic(False)
        with forced_hip(answers) as backend:
            yield backend
    finally:
        HipKernels.set_deterministic(deterministic)
        for k, v in keep.items():
            setattr(fused_mlp, k, v)


class _Owner:
    """Stand-in for dp.FlatTrainState on the device: one flat gradient vector with a slot per
    parameter, filled with a sentinel so that a slot nobody wrote is seen; the deferred-reduction
    window is opened as FlatTrainState.begin() does and closed as collect() does."""

    def __init__(self, params):
        self.flat = torch.full((sum(p.numel() for p in params),), SENTINEL, device=params[0].device)
        self.views, off = [], 0
        for p in params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        grad_slots.register(self, params, self.views, [])
        grad_slots.begin(self)
        HipKernels.begin_deferred_reductions()

    def collect(self):
        HipKernels.flush_deferred_reductions(close=True)
        grad_slots.close(self)


def _leaf(t, dev, grad=True):
    return t.to(dev).clone().requires_grad_(grad)


def _bufs(d, i, dev):
    return d[f'rm{i}'].to(dev).clone(), d[f'rv{i}'].to(dev).clone(), ref.MOMENTUM, ref.EPS


def _run_sa(cfg, case, d, dev):
    L = len(cfg['chans']) - 1
    x = _leaf(d['x'], dev, case.get('x_grad', False))
    names = [f'{k}{l}' for l in range(L) for k in ('w', 'gamma', 'beta')]
    params = [_leaf(d[n], dev) for n in names]
    for i in case.get('frozen', ()):
        params[i].requires_grad_(False)
    bufs = [_bufs(d, l, dev) for l in range(L)]
    owner = _Owner(params) if case.get('slots') else None
    out = fused_mlp.SAStackFn.apply(x, bufs, case.get('fixed_lead', 0), *params)
    out.backward(d['g_out'].to(dev))
    grads = {}
    if owner is not None:
        owner.collect()
        grads = dict(zip(names, owner.views))       # the flat vector itself
    else:
        grads = {n: p.grad for n, p in zip(names, params) if p.requires_grad}
        assert all(p.grad is None for p in params if not p.requires_grad)
    if x.requires_grad:
        dx = x.grad
        if case.get('fixed_lead', 0) == 3:      # nobody consumes the coordinate rows' gradient: exact zeros
            assert not dx[:, :3].any()
            grads['x[3:]'] = dx[:, 3:]
        else:
            grads['x'] = dx
    return {'out': out.detach()}, grads, [(b[0], b[1]) for b in bufs]


def _run_sa_eval(cfg, case, d, dev):
    from nesie_amd.kernels import injected_backend
    from nesie_amd.mmdet3d_ops.pointnet_modules import ConvModule
    chans = cfg['chans']
    layers = []
    for l, (cin, cout) in enumerate(zip(chans, chans[1:])):
        m = ConvModule(cin, cout, norm_cfg=dict(type='BN2d')).to(dev).eval()
        with torch.no_grad():
            m.conv.weight.copy_(d[f'w{l}'])
            m.norm.weight.copy_(d[f'gamma{l}'])
            m.norm.bias.copy_(d[f'beta{l}'])
            m.norm.running_mean.copy_(d[f'rm{l}'])
            m.norm.running_var.copy_(d[f'rv{l}'])
        layers.append(m)
    with torch.no_grad():
        x = d['x'].to(dev)
        assert fused_mlp.sa_stack_eval_supported(injected_backend(), x, layers)
        out = fused_mlp.sa_stack_eval(x, layers)
    return {'out': out}, {}, []


def _run_s1d(cfg, case, d, dev):
    S, P = cfg['S'], cfg['P']
    x = _leaf(d['x'], dev, case.get('x_grad', True))
    layers, tensors, leaves, bufs, zero_bias = [], [], {}, [], []
    for l, (cout, bias, norm) in enumerate(cfg['spec']):
        if S == 1:      # as fused_mlp.stack1d passes a single module's weight: a view of the parameter
            w = _leaf(d[f'w{l}'][0].unsqueeze(-1), dev)
            tensors.append(w.flatten(1).unsqueeze(0))
        else:
            w = _leaf(d[f'w{l}'], dev)
            tensors.append(w)
        leaves[f'w{l}'] = w
        if bias:
            leaves[f'b{l}'] = _leaf(d[f'b{l}'], dev)
            tensors.append(leaves[f'b{l}'])
            if norm:
                zero_bias.append(f'b{l}')
        if norm:
            leaves[f'gamma{l}'], leaves[f'beta{l}'] = _leaf(d[f'gamma{l}'], dev), _leaf(d[f'beta{l}'], dev)
            tensors += [leaves[f'gamma{l}'], leaves[f'beta{l}']]
            bufs.append(_bufs(d, l, dev))
        layers.append(fused_mlp.Stack1dLayer(bias, bufs[-1] if norm else None))
    plain_bias = [f'b{l}' for l, (_, bias, norm) in enumerate(cfg['spec']) if bias and not norm]
    owner = _Owner([t for n, t in leaves.items() if n not in plain_bias]) if case.get('slots') else None
    out = fused_mlp.Stack1dFn.apply(x, tuple(layers), S, *tensors)
    g = d['g_out'].to(dev)
    if case.get('sliced'):      # the consumer concatenates: the gradient arrives as a batch-strided channel slice
        pad = torch.randn(g.shape[0], 5, P, device=dev)
        torch.cat([out, pad.clone().requires_grad_(True)], 1).backward(torch.cat([g, pad], 1))
    else:
        out.backward(g)
    grads = {}
    if owner is not None:
        owner.collect()
        slotted = dict(zip([n for n in leaves if n not in plain_bias], owner.views))
        for n in zero_bias:     # left to collect()'s zero fill: nobody may have written it
            assert leaves[n].grad is None and bool((slotted.pop(n) == SENTINEL).all()), n
        grads.update(slotted)
        grads.update({n: leaves[n].grad for n in plain_bias})
    else:
        for n in zero_bias:     # identically zero: an exact zero tensor, not rounding noise and not None
            assert leaves[n].grad is not None and not leaves[n].grad.any(), n
        grads.update({n: t.grad for n, t in leaves.items()})
    grads = {n: (v.reshape(d[n].shape) if v is not None else v) for n, v in grads.items()}
    if x.requires_grad:
        grads['x'] = x.grad
    return {'out': out.detach()}, grads, [(b[0], b[1]) for b in bufs]


def _small(backend, g, w_g, bias, S):
    """The per-proposal term as side_pooling.fused_mini_pointnets forms it: a one-layer ``Stack1dFn``
    where the layer kernel serves K proposals, tensor ops otherwise (K < 64 at these shapes)."""
    Bn, _, half, K = g.shape
    gx = g.reshape(Bn * S, half, K)
    if fused_mlp.stack1d_supported(backend, gx, [(half, ref.H2)], [None], S):
        return fused_mlp.Stack1dFn.apply(gx, (fused_mlp.Stack1dLayer(True, None),), S, w_g, bias).view(Bn, S, ref.H2, K)
    return torch.matmul(w_g.unsqueeze(0), g) + bias.view(1, S, ref.H2, 1)


# the parameters of the quality head's functions that have a gradient slot ('w', which W_g and W_l are
# split from, is filled by autograd's concatenation)
_SLOTTED = {'mini': ('gamma0', 'beta0', 'w3', 'gamma1', 'beta1', 'w4'), 'blend': ('gamma0', 'beta0', 'w3')}


def _leaves(d, names, case, family, dev):
    """-> ({name: leaf} with the case's frozen ones requiring no gradient, the owner of their slots | None)."""
    t = {n: _leaf(d[n], dev, n not in case.get('frozen', ())) for n in names}
    return t, _Owner([t[n] for n in _SLOTTED[family]]) if case.get('slots') else None


def _gradients(t, case, family, owner):
    """{name: gradient} of the leaves ``t``: the flat vector itself where there are slots; a frozen leaf has none."""
    frozen = case.get('frozen', ())
    assert all(t[n].grad is None for n in frozen)
    grads = {n: v.grad for n, v in t.items() if n not in frozen}
    if owner is not None:
        owner.collect()
        grads.update(zip(_SLOTTED[family], owner.views))
    return grads


def _run_mini(cfg, case, d, dev):
    from nesie_amd.kernels import injected_backend
    S, G = cfg['S'], cfg['G']
    names = ('c0', 'gamma0', 'beta0', 'w3', 'w', 'bias', 'gamma1', 'beta1', 'w4')
    t, owner = _leaves(d, names, case, 'mini', dev)
    bufs = [_bufs(d, 0, dev), _bufs(d, 1, dev)]
    part = ref.stat_partials(d['c0']).to(dev)
    c, g = fused_mlp.MiniHeadFn.apply(t['c0'], part, bufs[0], G, t['gamma0'], t['beta0'], t['w3'])
    w_g, w_l = t['w'].split(ref.HALF, dim=2)
    small = _small(injected_backend(), g, w_g, t['bias'], S)
    small.retain_grad()
    out = fused_mlp.MiniTailFn.apply(c, small, bufs[1], G, w_l, t['gamma1'], t['beta1'], t['w4'])
    loss = (out * d['g_out'].to(dev)).sum()
    outs = {'out': out.detach()}
    if case.get('second_consumer'):     # autograd sums the two gradients of c: a tensor without the mark
        loss = loss + (c * d['g_c'].to(dev)).sum()
        outs['c'] = c.detach()
    loss.backward()
    grads = _gradients(t, case, 'mini', owner)
    grads['small'] = small.grad
    return outs, grads, [(b[0], b[1]) for b in bufs]


def _run_mini_eval(cfg, case, d, dev):
    from nesie_amd.kernels import injected_backend
    backend = injected_backend()
    S, G = cfg['S'], cfg['G']
    coef0 = ref.eval_coef(d['gamma0'], d['beta0'], d['rm0'], d['rv0']).to(dev)
    coef1 = ref.eval_coef(d['gamma1'], d['beta1'], d['rm1'], d['rv1']).to(dev)
    with torch.no_grad():
        w = d['w'].to(dev)
        w_g, w_l = (h.contiguous() for h in w.split(ref.HALF, dim=2))
        c, g, _ = fused_mlp.mini_head_kernels(backend, d['c0'].to(dev), coef0, d['w3'].to(dev), G)
        small = (torch.matmul(w_g.unsqueeze(0), g) + d['bias'].to(dev).view(1, S, ref.H2, 1)).contiguous()
        y, _ = fused_mlp.mini_tail_first(backend, c, small, w_l, G)
        out, _ = fused_mlp.mini_tail_second(backend, y, coef1, d['w4'].to(dev), G)
    return {'c': c, 'g': g, 'out': out}, {}, []


def _run_blend(cfg, case, d, dev):
    S, G = cfg['S'], cfg['G']
    names = ('table', 'wx', 'gamma0', 'beta0', 'w3')
    t, owner = _leaves(d, names, case, 'blend', dev)
    bufs = [_bufs(d, 0, dev)]
    c, g = fused_mlp.BlendMiniHeadFn.apply(t['table'], t['wx'], d['idx'].to(dev), d['weight'].to(dev),
                                           d['rel'].to(dev), S, G, bufs[0], G, t['gamma0'], t['beta0'], t['w3'])
    ((c * d['g_c'].to(dev)).sum() + (g * d['g_g'].to(dev)).sum()).backward()
    return {'c': c.detach(), 'g': g.detach()}, _gradients(t, case, 'blend', owner), [(bufs[0][0], bufs[0][1])]


_RUN = {'sa': _run_sa, 'sa_eval': _run_sa_eval, 's1d': _run_s1d, 'mini': _run_mini, 'mini_eval': _run_mini_eval,
        'blend': _run_blend}


def _err(dev_t, want):
    return float((dev_t.detach().double().cpu() - want).abs().max())


def _run(family, cfg, case, d, dev):
    """-> (outs, grads, stats, the back end) of ``case`` on its route."""
    try:
        with _route(case.get('answers', {}), case.get('switches', {}), case.get('atomic', False)) as backend:
            result = _RUN[family](cfg, case, d, dev)
            torch.cuda.synchronize()
    finally:
        if HipKernels._deferred is not None:        # a case that failed inside its window
            HipKernels.begin_deferred_reductions()
            HipKernels._deferred = None
    return (*result, backend)


def check_case(name, case, dev):
    """Run ``case`` and assert everything the module docstring lists; -> [(tensor, ratio)]."""
    cfg = ref.DATA[case['data']]
    family = cfg['family'] + ('' if cfg.get('training', True) else '_eval')
    d, margin, r32, r64 = _reference(case['data'], bool(case.get('second_consumer')))
    outs, grads, stats, backend = _run(family, cfg, case, d, dev)
    launched = backend.launched
    if case.get('slots') and family in _SLOTTED:
        # a slot holds exactly what the same route returns without slots
        plain = _run(family, cfg, dict(case, slots=False), d, dev)[1]
        for k in _SLOTTED[family]:
            same = torch.equal(grads[k].reshape(plain[k].shape), plain[k])
            print(f'SLOT {name} {k} equals the unslotted gradient bit for bit: {same}')
            assert same, f'{name}: the slot of {k} differs from the unslotted gradient'
    # route
    for m in case.get('present', ()):
        assert m in launched, f'{name}: {m} was not launched: {launched}'
    for m in case.get('absent', ()):
        assert m not in launched, f'{name}: {m} was launched: {launched}'
    for m, n in case.get('count', {}).items():
        assert launched.count(m) == n, f'{name}: {m} launched {launched.count(m)} times, not {n}: {launched}'
    failures = []
    # forward
    for k, v in outs.items():
        e = _err(v, r64.outs[k])
        print(f'FORWARD {name} {k} err {e:.3e} margin {margin:.3e}')
        if not e <= margin:
            failures.append(f'{k}: forward error {e:.3e} > margin {margin:.3e}')
    assert len(stats) == len(r64.stats) or not stats
    for i, (got, want) in enumerate(zip(stats, r64.stats)):
        for what, g_, w_ in (('mean', got[0], want[0]), ('variance', got[1], want[1])):
            e, bound = _err(g_, w_), margin * float(w_.abs().max())
            print(f'STATS {name} running {what} {i} err {e:.3e} bound {bound:.3e}')
            if not e <= bound:
                failures.append(f'running {what} {i}: {e:.3e} > {bound:.3e}')
    # gradients
    rows = []
    if grads:
        case_scale = max(float(v.abs().max()) for v in r64.grads.values())
        for k, g_dev in grads.items():
            key = 'x' if k == 'x[3:]' else k
            g64, g32 = r64.grads[key], r32.grads[key].double()
            if k == 'x[3:]':
                g64, g32 = g64[:, 3:], g32[:, 3:]
            assert g_dev is not None, f'{name}: no gradient for {k}'
            ref_err = max(float((g32 - g64).abs().max()), 2.0 ** -23 * float(g64.abs().max()), 2.0 ** -23 * case_scale)
            ratio = _err(g_dev.reshape(g64.shape), g64) / ref_err
            bound = BOUNDS.get((name, k), GRAD_FACTOR)
            rows.append((k, ratio))
            print(f'RATIO {name} {k} dev_err/ref_err {ratio:.2f} bound {bound:g} ref_err {ref_err:.3e}')
            if not ratio <= bound:
                failures.append(f'd{k}: dev_err / ref_err = {ratio:.2f} > {bound:g}')
        # every gradient of the reference is compared, but: the input's where the case asks for none, an
        # identically zero one that a slot leaves to the zero fill, a frozen parameter's
        skip = set() if case.get('x_grad', cfg['family'] != 'sa') else {'x'}
        if case.get('frozen'):      # (a set-abstraction case names them by position, the others by name)
            sa_names = [f'{k}{l}' for l in range(len(cfg.get('chans', ())) - 1) for k in ('w', 'gamma', 'beta')]
            skip |= {i if isinstance(i, str) else sa_names[i] for i in case['frozen']}
        missing = [k for k in r64.grads if k not in grads and k not in skip and r64.grads[k].any()
                   and not (k == 'x' and 'x[3:]' in grads)]
        assert not missing, f'{name}: gradients not compared: {missing}'
    assert not failures, f'{name}: ' + '; '.join(failures)
    assert _lib.load().nesie_pw_wgrad_pending() == 0
    return rows


def _cases(table):
    return pytest.mark.parametrize('name', sorted(table))


# ---- set-abstraction stacks ------------------------------------------------------------------------------
# (names as in test_fused_mlp_trace_cpu.CASES where the route is pinned there)
SA_CASES = {
    'sa1_k4_tail': dict(data='sa1', present=('pw_layer_forward_k4', 'pw_wgrad_bn_backward_k4_fused', 'pool_tail_backward'),
                        absent=('bn_relu_maxpool_backward', 'mlp_stream_forward')),
    'sa1_stream_tail': dict(data='sa1', answers={'k4_supported': False},
                            present=('mlp_stream_forward', 'pool_tail_backward'), absent=('pw_layer_forward_k4',)),
    'sa1_stream_dense_pool': dict(data='sa1', answers={'k4_supported': False, 'pool_tail_supported': False},
                                  present=('mlp_stream_forward', 'bn_relu_maxpool_backward'),
                                  absent=('pool_tail_backward', 'pw_layer_forward_k4')),
    'sa1_k4_switch_off': dict(data='sa1', switches={'SA1_K4': False}, present=('mlp_stream_forward',),
                              absent=('k4_moments', 'pw_layer_forward_k4')),
    'sa_frozen_middle_weight': dict(data='sa1', frozen=(3,),
                                    present=('mlp_stream_forward', 'pool_tail_backward'), absent=('k4_moments',)),
    'sa_frozen_middle_dense': dict(data='sa1', frozen=(3,), answers=APPLY_PASS,
                                   present=('bn_relu_maxpool_backward', 'bn_relu_backward_apply'),
                                   absent=('pool_tail_backward', 'pw_wgrad_bn_backward')),
    'sa_nothing_needs_grad': dict(data='sa1', x_grad=True, frozen=range(9),
                                  present=('bn_relu_backward_apply',),
                                  absent=('pw_wgrad', 'pw_wgrad_bn_backward', 'conv_wgrad', 'k4_moments')),
    # (the pooled tail is built for 64 -> 128 only: a 256-wide last layer always pools densely)
    'sa2_folded': dict(data='sa2', x_grad=True, present=('pw_wgrad_bn_backward', 'bn_relu_maxpool_backward'),
                       absent=('bn_relu_backward_apply',), count={'pw_layer_forward': 4}),
    'sa2_unfolded_switch': dict(data='sa2', x_grad=True, switches={'FOLD_NORM_BWD': False},
                                present=('bn_relu_backward_apply', 'pw_wgrad'), absent=('pw_wgrad_bn_backward',)),
    'sa2_apply_pass_lead0': dict(data='sa2', x_grad=True, fixed_lead=0, answers=APPLY_PASS,
                                 present=('bn_relu_maxpool_backward', 'bn_relu_backward_apply'),
                                 absent=('pool_tail_backward', 'pw_wgrad_bn_backward')),
    'sa2_apply_pass_lead3': dict(data='sa2', x_grad=True, fixed_lead=3, answers=APPLY_PASS,
                                 present=('bn_relu_maxpool_backward', 'bn_relu_backward_apply'),
                                 absent=('pool_tail_backward', 'pw_wgrad_bn_backward')),
    # pw_supported refused for the input-gradient product only: three layer launches (the forward's)
    # instead of four, the input gradient through torch.bmm
    'sa2_input_grad_bmm': dict(data='sa2', x_grad=True, answers=dict(APPLY_PASS, pw_supported=_refuse(128, 128)),
                               present=('bn_relu_backward_apply',), count={'pw_layer_forward': 3}),
    'sa2_wgrad_aten': dict(data='sa2', x_grad=True, answers=ATEN_WGRAD, present=('affine_relu_forward',),
                           absent=('pw_wgrad', 'pw_wgrad_bn_backward', 'conv_wgrad')),
    'sa_no_lead_rows': dict(data='sa_no_lead', x_grad=True, present=('pw_wgrad_bn_backward', 'bn_relu_maxpool_backward')),
    'sa_two_layers': dict(data='sa_two', present=('mlp_stream_forward', 'pool_tail_backward', 'conv_wgrad')),
    'sa_two_layers_dense_pool': dict(data='sa_two', answers={'pool_tail_supported': False},
                                     present=('bn_relu_maxpool_backward', 'conv_wgrad'), absent=('pool_tail_backward',)),
    'sa_lead_rows_259': dict(data='sa_259', x_grad=True, count={'pw_layer_forward': 3}),
    'sa1_slots': dict(data='sa1', slots=True, present=('pw_wgrad_bn_backward_k4_fused',)),
    'sa2_slots_wgrad_paths': dict(data='sa2', x_grad=True, slots=True, answers=ATEN_WGRAD,
                                  present=('affine_relu_forward',), absent=('pw_wgrad', 'pw_wgrad_bn_backward')),
    'sa_eval': dict(data='sa2_eval', present=('pw_layer_forward', 'pw_pool_finish'), absent=('pw_stats_finalize',)),
    'sa_eval_ns16': dict(data='sa_two_eval', present=('pw_layer_forward', 'pw_pool_finish'), absent=('pw_stats_finalize',)),
}


@_cases(SA_CASES)
def test_sa_stack_against_float64(name, hip_device):
    check_case(name, SA_CASES[name], hip_device)


# ---- 1-D chains ------------------------------------------------------------------------------------------
S1D_CASES = {
    's1d_s2_bias_norm_then_bias': dict(data='s1d_bias_norm_then_bias', present=('channel_sum', 'pw_dgrad_bn_reduce')),
    's1d_s1_norm_everywhere': dict(data='s1d_norm_everywhere', present=('bn_relu_backward', 'pw_wgrad_bn_backward'),
                                   absent=('bn_relu_backward_apply',)),
    's1d_s1_unfolded': dict(data='s1d_norm_everywhere', answers={'pw_wgrad_bn_supported': False},
                            present=('bn_relu_backward', 'bn_relu_backward_apply', 'pw_wgrad'),
                            absent=('pw_wgrad_bn_backward',)),
    's1d_single_bias_layer': dict(data='s1d_single_bias_layer', present=('channel_sum', 'pw_wgrad'),
                                  count={'pw_layer_forward': 2}),
    's1d_input_without_grad': dict(data='s1d_input_without_grad', x_grad=False,
                                   count={'pw_layer_forward': 2}),
    # pw_supported refused for the input-gradient product only: the gradient through torch.matmul
    's1d_input_grad_matmul': dict(data='s1d_input_grad_matmul', answers={'pw_supported': _refuse(128, 64)},
                                  count={'pw_layer_forward': 2}),
    's1d_sliced_gradient': dict(data='s1d_sliced_gradient', sliced=True, present=('channel_sum',)),
    's1d_ragged_220': dict(data='s1d_ragged_220', present=('channel_sum', 'pw_wgrad')),
    's1d_slots': dict(data='s1d_slots', slots=True, present=('channel_sum',)),
}


@_cases(S1D_CASES)
def test_stack1d_against_float64(name, hip_device):
    check_case(name, S1D_CASES[name], hip_device)


def test_single_bias_layer_runs_at_the_smallest_accepted_length(hip_device):
    """The single-layer case runs at P = 64, which is also the smallest length ``nesie_pw_supported``
    accepts for it (whole 64-position tiles): there is no shorter device case to add."""
    accept = _lib.load().nesie_pw_supported
    assert accept(32, 256, 64) and not any(accept(32, 256, p) for p in range(1, 64))


# ---- MiniPointNets ---------------------------------------------------------------------------------------
_SPARSE = dict(present=('pool_tail_pack', 'pw_wgrad_sparse', 'pw_dgrad_bn_reduce_sparse', 'pw_wgrad_bn_backward'),
               absent=('group_max_pool_backward',), count={'bn_relu_backward_apply': 1})     # (the head's first norm)
_DENSE = dict(switches={'MINI_TAIL_SPARSE': False}, present=('group_max_pool_backward', 'pw_wgrad_bn_backward'),
              absent=('pool_tail_pack', 'pw_wgrad_sparse'))
_UNFOLDED = dict(answers={'pw_wgrad_bn_supported': False}, present=('pool_tail_pack',),
                 absent=('pw_wgrad_bn_backward',), count={'bn_relu_backward_apply': 2})
MINI_CASES = {
    'mini_s2_g16': dict(data='mini_s2_g16', **_SPARSE),
    'mini_s1_g64': dict(data='mini_s1_g64', **_SPARSE),
    'mini_s2_g16_dense': dict(data='mini_s2_g16', **_DENSE),
    'mini_s1_g64_dense': dict(data='mini_s1_g64', **_DENSE),
    'mini_s2_g16_unfolded': dict(data='mini_s2_g16', **_UNFOLDED),
    'mini_s1_g64_unfolded': dict(data='mini_s1_g64', **_UNFOLDED),
    'mini_s2_g16_unmarked_dc': dict(data='mini_s2_g16', second_consumer=True, present=('group_max_pool_backward_add',)),
    'mini_s2_g16_slots': dict(data='mini_s2_g16', slots=True, **_SPARSE),
    'mini_s1_g64_dense_slots': dict(data='mini_s1_g64', slots=True, **_DENSE),
    # W_l (the whole weight it is split from) without a gradient: the norm backward as its own apply pass
    'mini_s2_g16_frozen_wl': dict(data='mini_s2_g16', frozen=('w',), present=('pool_tail_pack', 'pw_wgrad_sparse'),
                                  absent=('pw_wgrad_bn_backward',), count={'bn_relu_backward_apply': 2}),
    'mini_s1_g64_frozen_w4': dict(data='mini_s1_g64', frozen=('w4',),
                                  present=('pool_tail_pack', 'pw_dgrad_bn_reduce_sparse', 'pw_wgrad_bn_backward'),
                                  absent=('pw_wgrad_sparse', 'group_max_pool_backward')),
    'mini_s2_g16_frozen_w3': dict(data='mini_s2_g16', frozen=('w3',), **dict(_SPARSE, absent=('group_max_pool_backward',
                                                                                              'pw_wgrad'))),
    'mini_eval_s2_g16': dict(data='mini_eval_s2_g16', present=('pw_layer_forward', 'pw_pool_finish')),
    'mini_eval_s1_g64': dict(data='mini_eval_s1_g64', present=('pw_layer_forward', 'pw_pool_finish')),
}


@_cases(MINI_CASES)
def test_mini_pointnets_against_float64(name, hip_device):
    check_case(name, MINI_CASES[name], hip_device)


# ---- blend head ------------------------------------------------------------------------------------------
BLEND_CASES = {
    'blend_folded': dict(data='blend', present=('blend_conv_backward', 'pw_bnb_coef'), absent=('bn_relu_backward_apply',)),
    'blend_unfolded': dict(data='blend', switches={'FOLD_NORM_BWD': False},
                           present=('blend_conv_backward', 'bn_relu_backward_apply'), absent=('pw_bnb_coef',)),
    # the caller's side of the atomic form: a zero-filled table handed to the backward ...
    'blend_atomic_table': dict(data='blend', answers={'blend_backward_writes_table': False},
                               present=('blend_conv_backward', 'pw_bnb_coef')),
    # ... and the form itself (float atomics into that table), with the deterministic backward switched off
    'blend_atomic_form': dict(data='blend', atomic=True, present=('blend_conv_backward', 'pw_bnb_coef')),
    'blend_slots': dict(data='blend', slots=True, present=('blend_conv_backward', 'pw_bnb_coef'),
                        absent=('bn_relu_backward_apply',)),
}


@_cases(BLEND_CASES)
def test_blend_head_against_float64(name, hip_device):
    case = BLEND_CASES[name]
    if case.get('atomic'):
        from nesie_amd.kernels import blend_backward_form
        assert blend_backward_form(ref.H0, ref.DATA['blend']['P'], ref.DATA['blend']['m'], False) == 'atomic'
    check_case(name, case, hip_device)
    assert HipKernels.DETERMINISTIC


def test_switches_and_back_end_are_restored(hip_device):
    from nesie_amd.kernels import injected_backend
    check_case('sa2_unfolded_switch', SA_CASES['sa2_unfolded_switch'], hip_device)
    assert fused_mlp.FOLD_NORM_BWD and fused_mlp.SA1_K4 and fused_mlp.MINI_TAIL_SPARSE and fused_mlp.ENABLED
    assert injected_backend() is None and HipKernels._deferred is None
