"""The float64 restatement of the fused MLP chains (tests/_chain_ref.py) checked without a GPU:

* every seed committed in ``_chain_ref.DATA`` qualifies -- recomputed here, the table is not trusted:
  no normalised pre-activation within the decision margin of zero, no pooled group whose two
  largest values are closer than it;
* at those seeds the restatement's float32 evaluation takes the ReLU masks and arg-max of float64;
* the restatement agrees with the project's own modules evaluated module by module in float64
  (``ConvModule`` stacks and ``MiniPointNet`` under ``.double()``: their norm layers use tensor ops
  for any dtype but float32) to 1e-12 relative on outputs and 1e-10 on gradients: a referee for
  the referee, in the manner of tests/_roiaware_ref.py.

tests/test_fused_chains_fp64_gpu.py holds the device against the restatement."""
import pytest
import torch
from torch import nn

from nesie_amd import kernels
from nesie_amd.mmdet3d_ops import fused_mlp
from tests import _chain_ref as ref

SEARCHED = sorted(n for n, c in ref.DATA.items() if c.get('search', True))


@pytest.fixture(scope='module')
def evaluated():
    """name -> (qualifies, margin, float32 Result, float64 Result), each data set evaluated once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref.qualifies(name, ref.DATA[name]['seed'], second_consumer=name == 'mini_s2_g16')
        return cache[name]
    return get


@pytest.mark.parametrize('name', sorted(ref.DATA))
def test_a_seed_is_committed(name):
    assert isinstance(ref.DATA[name]['seed'], int), f'{name}: no seed qualified; shrink the shape, not the margin'


@pytest.mark.parametrize('name', SEARCHED)
def test_committed_seed_qualifies(name, evaluated):
    ok, margin, r32, r64 = evaluated(name)
    _, pool_margin = ref.margins(r32, r64)
    assert 0 < margin < 1e-4, margin        # rounding-sized: a margin that grew would hide a defect
    assert ok, f'{name}: {ref.violations(r64, margin, pool_margin)} decisions within {margin:.2e}'


@pytest.mark.parametrize('name', SEARCHED)
def test_float32_reference_takes_float64_decisions(name, evaluated):
    _, _, r32, r64 = evaluated(name)
    assert ref.same_decisions(r32, r64)
    # ... and its gradients are float64's up to rounding (a tensor whose true value is zero -- a bias
    # in front of a norm -- is measured against the case's largest gradient entry)
    scale = max(float(g.abs().max()) for g in r64.grads.values())
    for k, g64 in r64.grads.items():
        assert float((r32.grads[k].double() - g64).abs().max()) <= 1e-5 * scale, k


# ---- against the modules, module by module in float64 ---------------------------------------------------

class _Plain:
    """A back end that is not the native one: every module takes its tensor-op path."""
    name = 'plain'


@pytest.fixture
def module_by_module():
    keep = fused_mlp.ENABLED
    fused_mlp.ENABLED = False
    try:
        with kernels.use_backend(_Plain()):
            yield
    finally:
        fused_mlp.ENABLED = keep


def _close(got, want, rel, what, scale=None):
    scale = max(float(want.abs().max()), 1e-300) if scale is None else scale
    err = float((got - want).abs().max())
    assert err <= rel * scale, f'{what}: {err:.3e} against scale {scale:.3e}'


def _load(param, value):
    with torch.no_grad():
        param.copy_(value.view_as(param))


def _conv_module(cin, cout, d, l, s=None, S=1, dim=2, bias=False, norm=True):
    from nesie_amd.mmdet3d_ops.pointnet_modules import ConvModule
    m = ConvModule(cin, cout, conv_cfg=dict(type=f'Conv{dim}d'),
                   norm_cfg=dict(type=f'BN{dim}d') if norm else None,
                   act_cfg=dict(type='ReLU') if norm else None, bias=bias).double()

    def part(t):        # net s of S stacked ones
        return t if s is None else t.view(S, -1)[s] if t.dim() == 1 else t[s]
    _load(m.conv.weight, part(d[f'w{l}']).double())
    if bias:
        _load(m.conv.bias, part(d[f'b{l}']).double())
    if norm:
        _load(m.norm.weight, part(d[f'gamma{l}']).double())
        _load(m.norm.bias, part(d[f'beta{l}']).double())
    return m.train()


SA_DATA = sorted(n for n, c in ref.DATA.items() if c['family'] == 'sa' and c.get('training', True))
S1D_DATA = sorted(n for n, c in ref.DATA.items() if c['family'] == 's1d')
MINI_DATA = sorted(n for n, c in ref.DATA.items() if c['family'] == 'mini' and c.get('training', True))


@pytest.mark.parametrize('name', SA_DATA)
def test_sa_restatement_equals_the_modules(name, module_by_module):
    cfg, d = ref.DATA[name], ref.make(name)
    r64 = ref.evaluate(name, d, torch.float64)
    chans = cfg['chans']
    layers = [_conv_module(cin, cout, d, l) for l, (cin, cout) in enumerate(zip(chans, chans[1:]))]
    x = d['x'].double().requires_grad_(True)
    a = x
    for m in layers:
        a = m(a)
    out = torch.max(a, dim=-1).values
    (out * d['g_out'].double()).sum().backward()
    _close(out.detach(), r64.outs['out'], 1e-12, 'out')
    _close(x.grad, r64.grads['x'], 1e-10, 'dx')
    for l, m in enumerate(layers):
        _close(m.conv.weight.grad, r64.grads[f'w{l}'], 1e-10, f'dw{l}')
        _close(m.norm.weight.grad, r64.grads[f'gamma{l}'], 1e-10, f'dgamma{l}')
        _close(m.norm.bias.grad, r64.grads[f'beta{l}'], 1e-10, f'dbeta{l}')
        _close(m.norm.running_mean, r64.stats[l][0], 1e-12, f'running mean {l}')
        _close(m.norm.running_var, r64.stats[l][1], 1e-12, f'running variance {l}')


@pytest.mark.parametrize('name', S1D_DATA)
def test_stack1d_restatement_equals_the_modules(name, module_by_module):
    cfg, d = ref.DATA[name], ref.make(name)
    r64 = ref.evaluate(name, d, torch.float64)
    S, P = cfg['S'], cfg['P']
    x = d['x'].double().requires_grad_(True)
    g = d['g_out'].double().view(ref.B, S, -1, P)
    outs, nets = [], []
    for s in range(S):      # batch n uses weight group n % S: net s sees x[s::S]
        cin, mods = cfg['c0'], []
        for l, (cout, bias, norm) in enumerate(cfg['spec']):
            mods.append(_conv_module(cin, cout, d, l, s, S, dim=1, bias=bias, norm=norm))
            cin = cout
        a = x.view(ref.B, S, cfg['c0'], P)[:, s]
        for m in mods:
            a = m(a)
        outs.append(a)
        nets.append(mods)
    out = torch.stack(outs, 1)
    (out * g).sum().backward()
    _close(out.detach().reshape(ref.B * S, -1, P), r64.outs['out'], 1e-12, 'out')
    _close(x.grad, r64.grads['x'], 1e-10, 'dx')
    norm_index = 0
    for l, (cout, bias, norm) in enumerate(cfg['spec']):
        def stacked(pick):
            return torch.stack([pick(nets[s][l]) for s in range(S)])
        _close(stacked(lambda m: m.conv.weight.grad.flatten(1)), r64.grads[f'w{l}'], 1e-10, f'dw{l}')
        if bias and not norm:
            _close(stacked(lambda m: m.conv.bias.grad).reshape(-1), r64.grads[f'b{l}'], 1e-10, f'db{l}')
        if bias and norm:       # identically zero; the modules' tensor ops sum rounding noise around it
            assert not r64.grads[f'b{l}'].any()
            _close(stacked(lambda m: m.conv.bias.grad).reshape(-1), r64.grads[f'b{l}'], 1e-10, f'db{l}',
                   scale=max(float(v.abs().max()) for v in r64.grads.values()))
        if norm:
            _close(stacked(lambda m: m.norm.weight.grad).reshape(-1), r64.grads[f'gamma{l}'], 1e-10, f'dgamma{l}')
            _close(stacked(lambda m: m.norm.bias.grad).reshape(-1), r64.grads[f'beta{l}'], 1e-10, f'dbeta{l}')
            # (the running mean holds the bias that the values never saw)
            _close(stacked(lambda m: m.norm.running_mean).reshape(-1), r64.stats[norm_index][0], 1e-12, f'mean {l}')
            _close(stacked(lambda m: m.norm.running_var).reshape(-1), r64.stats[norm_index][1], 1e-12, f'var {l}')
            norm_index += 1


@pytest.mark.parametrize('name', MINI_DATA)
def test_mini_restatement_equals_the_modules(name, module_by_module):
    """``MiniPointNet`` carries conv biases (b3 behind the first maximum, b4 behind the last) where
    the fused functions take one row-bias vector: the restatement is composed here as
    side_pooling.fused_mini_pointnets composes the functions, bias = W [b3, b3], out + b4."""
    from nesie_amd.votenet.side_pooling import MiniPointNet
    cfg, d = ref.DATA[name], ref.make(name)
    S, G, P = cfg['S'], cfg['G'], cfg['P']
    K = P // G
    gen = torch.Generator().manual_seed(1)
    b3 = torch.randn(S, ref.HALF, generator=gen, dtype=torch.float64) * 0.5
    b4 = torch.randn(S, ref.F, generator=gen, dtype=torch.float64) * 0.5
    nets = []
    for s in range(S):
        net = MiniPointNet(259, ref.F, hide_dim=ref.H0).double().train()
        _load(net.first_conv[1].weight, d['gamma0'].view(S, -1)[s].double())
        _load(net.first_conv[1].bias, d['beta0'].view(S, -1)[s].double())
        _load(net.first_conv[3].weight, d['w3'][s].double())
        _load(net.first_conv[3].bias, b3[s])
        _load(net.second_conv[0].weight, d['w'][s].double())
        _load(net.second_conv[1].weight, d['gamma1'].view(S, -1)[s].double())
        _load(net.second_conv[1].bias, d['beta1'].view(S, -1)[s].double())
        _load(net.second_conv[3].weight, d['w4'][s].double())
        _load(net.second_conv[3].bias, b4[s])
        nets.append(net)
    g_out = d['g_out'].double()
    c0 = d['c0'].double().requires_grad_(True)
    out = torch.stack([net(conv0_out=c0[:, s].reshape(ref.B, ref.H0, K, G)) for s, net in enumerate(nets)], 1)
    (out * g_out).sum().backward()

    # the restatement, composed the same way
    t = {k: d[k].double().requires_grad_(True) for k in ('c0', 'gamma0', 'beta0', 'w3', 'w', 'gamma1', 'beta1', 'w4')}
    b3r, b4r = b3.clone().requires_grad_(True), b4.clone().requires_grad_(True)
    trace = ref.Trace()

    def bn(i):
        return d[f'rm{i}'].double(), d[f'rv{i}'].double(), ref.MOMENTUM, ref.EPS
    c, g = ref.mini_head(trace, t['c0'], bn(0), G, t['gamma0'], t['beta0'], t['w3'])
    w_g, w_l = t['w'].split(ref.HALF, dim=2)
    bias = torch.einsum('soc,sc->so', t['w'], torch.cat([b3r, b3r], 1))
    small = ref.grouped_conv(w_g, g) + bias.view(1, S, -1, 1)
    want = ref.mini_tail(trace, c, small, bn(1), G, w_l, t['gamma1'], t['beta1'], t['w4']) + b4r.view(1, S, -1, 1)
    (want * g_out).sum().backward()

    _close(out.detach(), want.detach(), 1e-12, 'out')
    _close(c0.grad, t['c0'].grad, 1e-10, 'dc0')

    def stacked(pick):
        return torch.stack([pick(n) for n in nets])
    for what, pick, key in (('dgamma0', lambda n: n.first_conv[1].weight.grad, 'gamma0'),
                            ('dbeta0', lambda n: n.first_conv[1].bias.grad, 'beta0'),
                            ('dw3', lambda n: n.first_conv[3].weight.grad.flatten(1), 'w3'),
                            ('dw', lambda n: n.second_conv[0].weight.grad.flatten(1), 'w'),
                            ('dgamma1', lambda n: n.second_conv[1].weight.grad, 'gamma1'),
                            ('dbeta1', lambda n: n.second_conv[1].bias.grad, 'beta1'),
                            ('dw4', lambda n: n.second_conv[3].weight.grad.flatten(1), 'w4')):
        _close(stacked(pick).reshape(t[key].shape), t[key].grad, 1e-10, what)
    # (b3 reaches the output through a per-channel constant in front of the second norm: its true
    # gradient is zero and both evaluations return rounding noise, measured against the largest gradient)
    _close(stacked(lambda n: n.first_conv[3].bias.grad), b3r.grad, 1e-10, 'db3',
           scale=max(float(v.grad.abs().max()) for v in t.values()))
    _close(stacked(lambda n: n.second_conv[3].bias.grad), b4r.grad, 1e-10, 'db4')
    for i, pick in enumerate((lambda n: n.first_conv[1], lambda n: n.second_conv[1])):
        _close(stacked(lambda n: pick(n).running_mean).reshape(-1), trace.stats[i][0], 1e-12, f'running mean {i}')
        _close(stacked(lambda n: pick(n).running_var).reshape(-1), trace.stats[i][1], 1e-12, f'running variance {i}')


def test_blend_restatement_equals_the_oracle(oracle_kernels):
    """The blend conv in front of ``BlendMiniHeadFn`` against the CPU oracle's restatement of the
    reference's pieces (three_interpolate per face + the xyz term as a matmul), in float32 data
    evaluated by both: float32 rounding is the only difference."""
    cfg, d = ref.DATA['blend'], ref.make('blend')
    S, G = cfg['S'], cfg['G']
    want = torch.empty(ref.B, S, ref.H0, cfg['P'])
    oracle_kernels.blend_conv_forward(d['table'], ref.H0, d['idx'], d['weight'], d['rel'], d['wx'], want, S, G,
                                      ref.H0, 0)
    got = ref.blend_conv(d['table'].double(), d['wx'].double(), d['idx'], d['weight'].double(), d['rel'].double(), S, G)
    _close(want.double(), got, 2e-6, 'blend conv')


def test_stat_partials_layout():
    c0 = ref.make('mini_s2_g16')['c0']
    part = ref.stat_partials(c0)
    S, P = 2, 64
    assert tuple(part.shape) == (S * ref.H0, ref.B * P // 64, 2)
    torch.testing.assert_close(part[:, :, 0].sum(1), c0.double().sum((0, 3)).reshape(-1).float(), rtol=1e-5, atol=1e-4)


def test_s1d_module_without_norm_is_plain(module_by_module):
    """(the helper above builds a conv without norm and without ReLU for a plain last layer)"""
    m = _conv_module(4, 3, {'w0': torch.randn(3, 4, 1), 'b0': torch.randn(3)}, 0, dim=1, bias=True, norm=False)
    assert isinstance(m.conv, nn.Conv1d) and m.norm is None and not m.with_activation
