"""Which kernels the fused MLP chains (mmdet3d_ops/fused_mlp.py) launch, in which order and over which
buffers, pinned without a GPU: ``tests/_launch_recorder.LaunchRecorder`` stands in for the HIP back
end, the autograd functions run end to end on CPU tensors, and the log of every case must equal
``tests/golden/fused_mlp_launch_trace.json`` entry for entry.  The log also holds the tuple every
``backward`` returned (None / tensor per position, and which memory a returned gradient views), so a
slip in the bookkeeping of a chain -- a gradient in the wrong position, a kernel reading the wrong
saved tensor, a slot not written -- shows here and not only as a wrong number on the device.

The fixture is this project's own record: ``python -m tests.test_fused_mlp_trace_cpu`` adds the cases
it does not hold yet from the code as it stands -- record a new case BEFORE changing the code it is to
hold -- and ``... CASE [CASE ...]`` records the named ones again (only for a change that is MEANT to
alter their launches)."""
import json
import os

import pytest
import torch

from nesie_amd import grad_slots
from nesie_amd.kernels import injected_backend, use_backend
from nesie_amd.mmdet3d_ops import fused_mlp
from tests._launch_recorder import LaunchRecorder

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fused_mlp_launch_trace.json')
_FUNCTIONS = ('SAStackFn', 'Stack1dFn', 'MiniHeadFn', 'BlendMiniHeadFn', 'MiniTailFn')
B, M = 2, 8


def _leaf(*shape, grad=True):
    return torch.zeros(*shape, requires_grad=grad)


class _Owner:
    """Stand-in for dp.FlatTrainState: one flat gradient vector with a slot per parameter."""

    def __init__(self, params):
        self.flat = torch.zeros(sum(p.numel() for p in params))
        self.views, off = [], 0
        for p in params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        grad_slots.register(self, params, self.views, [])
        grad_slots.begin(self)


def _norm_bufs(channels):
    return torch.zeros(channels), torch.ones(channels), 0.1, 1e-5


# ---- the drivers: each runs forward + backward and returns [(function, position in the tuple that
# its backward returns, the gradient slot that position must be a view of)] -----------------------------

def _sa(chans, ns, x_grad, fixed_lead=0, frozen=(), owner=False):
    x = _leaf(B, chans[0], M, ns, grad=x_grad)
    params, bufs = [], []
    for cin, cout in zip(chans, chans[1:]):
        params += [_leaf(cout, cin, 1, 1), _leaf(cout), _leaf(cout)]
        bufs.append(_norm_bufs(cout))
    for i in frozen:
        params[i].requires_grad_(False)
    state = _Owner(params) if owner else None
    fused_mlp.SAStackFn.apply(x, bufs, fixed_lead, *params).sum().backward()
    return [('SAStackFn', 3 + i, v) for i, v in enumerate(state.views)] if owner else []


def _stack1d(S, c0, spec, x_grad=True, P=128, owner=False, sliced=False):
    """``spec``: [(Cout, conv bias, norm)] per layer."""
    x = _leaf(B * S, c0, P, grad=x_grad)
    layers, tensors, registered, positions = [], [], [], []
    cin = c0
    for cout, bias, norm in spec:
        if S == 1:      # as fused_mlp.stack1d passes a single module's weight: a view of the parameter
            w = _leaf(cout, cin, 1)
            positions.append(3 + len(tensors))
            registered.append(w)
            tensors.append(w.flatten(1).unsqueeze(0))
        else:
            tensors.append(_leaf(S, cout, cin))
        if bias:
            tensors.append(_leaf(S * cout))
            if norm:    # identically zero: with a slot the backward returns None (see Stack1dFn)
                positions.append(None)
                registered.append(tensors[-1])
        if norm:
            positions += [3 + len(tensors), 4 + len(tensors)]
            tensors += [_leaf(S * cout), _leaf(S * cout)]
            registered += tensors[-2:]
        layers.append(fused_mlp.Stack1dLayer(bias, _norm_bufs(S * cout) if norm else None))
        cin = cout
    state = _Owner(registered) if owner else None
    out = fused_mlp.Stack1dFn.apply(x, tuple(layers), S, *tensors)
    if sliced:      # the consumer concatenates several chains: the gradient arrives as a channel slice
        out = torch.cat([out, torch.zeros(B * S, 5, P)], 1)
    out.sum().backward()
    return [('Stack1dFn', i, v) for i, v in zip(positions, state.views) if i is not None] if owner else []


H0, HALF, H2, F = 64, 32, 256, 128


def _mini_tail(c, g, S, G, w, gamma1, beta1, w4):
    """side_pooling.fused_mini_pointnets behind the head: the per-proposal term through a one-layer
    ``Stack1dFn``, then ``MiniTailFn``."""
    K = g.shape[-1]
    w_g, w_l = w.split(HALF, dim=2)
    small = fused_mlp.Stack1dFn.apply(g.reshape(B * S, HALF, K), (fused_mlp.Stack1dLayer(True, None),), S,
                                      w_g, _leaf(S * H2)).view(B, S, H2, K)
    return fused_mlp.MiniTailFn.apply(c, small, _norm_bufs(S * H2), G, w_l, gamma1, beta1, w4)


# where the parameters sit in the tuples that the three backwards return
_HEAD_AT = {'MiniHeadFn': 4, 'BlendMiniHeadFn': 9}         # gamma0, beta0, w3 from there on
_TAIL_AT = 5                                                # gamma1, beta1, w4 (W_l, in front, has no slot)


def _mini(S, G, second_consumer=False, owner=False, frozen=()):
    """``frozen``: which of 'w' (the weight that W_g and W_l are split from), 'w3', 'w4' need no gradient."""
    P = 64 if G == 16 else 128
    c0 = _leaf(B, S, H0, P)
    head = [_leaf(S * H0), _leaf(S * H0), _leaf(S, HALF, H0, grad='w3' not in frozen)]
    w = _leaf(S, H2, 2 * HALF, grad='w' not in frozen)
    tail = [_leaf(S * H2), _leaf(S * H2), _leaf(S, F, H2, grad='w4' not in frozen)]
    state = _Owner(head + tail) if owner else None
    c, g = fused_mlp.MiniHeadFn.apply(c0, torch.zeros(S * H0, 2, 2), _norm_bufs(S * H0), G, *head)
    loss = _mini_tail(c, g, S, G, w, *tail).sum()
    if second_consumer:     # autograd sums the two gradients of c into a tensor of its own: no mark on it
        loss = loss + c.sum()
    loss.backward()
    if not owner:
        return []
    at = [('MiniHeadFn', _HEAD_AT['MiniHeadFn'] + j) for j in range(3)] + [('MiniTailFn', _TAIL_AT + j) for j in range(3)]
    return [(f, i, v) for (f, i), v in zip(at, state.views)]


def _blend(S=2, G=16, P=64, m=16, owner=False):
    n = S * P
    head = [_leaf(S * H0), _leaf(S * H0), _leaf(S, HALF, H0)]
    state = _Owner(head) if owner else None
    c, g = fused_mlp.BlendMiniHeadFn.apply(
        _leaf(B, m, S * H0), _leaf(S, H0, 3), torch.zeros(B, n, 3, dtype=torch.int32), torch.zeros(B, n, 3),
        torch.zeros(B, n, 3), S, P, _norm_bufs(S * H0), G, *head)
    (c.sum() + g.sum()).backward()
    return [('BlendMiniHeadFn', _HEAD_AT['BlendMiniHeadFn'] + j, v) for j, v in enumerate(state.views)] if owner else []


def _sa_modules(chans):
    from nesie_amd.mmdet3d_ops.pointnet_modules import ConvModule
    return [ConvModule(cin, cout, norm_cfg=dict(type='BN2d')) for cin, cout in zip(chans, chans[1:])]


def _sa_eval(chans, ns):
    """The test path of a set-abstraction MLP: evaluation-mode norms, no autograd."""
    rec = injected_backend()
    layers = [m.eval() for m in _sa_modules(chans)]
    with torch.no_grad():
        x = torch.zeros(B, chans[0], M, ns)
        assert fused_mlp.sa_stack_eval_supported(rec, x, layers) and not fused_mlp.sa_stack_supported(rec, x, layers)
        rec.note('sa_stack_eval returned', [fused_mlp.sa_stack_eval(x, layers)])
    return []


def _mini_eval(S, G):
    """side_pooling.fused_mini_pointnets in evaluation mode: the three layer helpers called directly."""
    rec = injected_backend()
    P = 64 if G == 16 else 128
    with torch.no_grad():
        c, g, _ = fused_mlp.mini_head_kernels(rec, torch.zeros(B, S, H0, P), torch.zeros(S * H0, 4),
                                              torch.zeros(S, HALF, H0), G)
        y, _ = fused_mlp.mini_tail_first(rec, c, torch.zeros(B, S, H2, P // G), torch.zeros(S, H2, HALF), G)
        out, arg = fused_mlp.mini_tail_second(rec, y, torch.zeros(S * H2, 4), torch.zeros(S, F, H2), G)
    rec.note('evaluation returned', [c, g, y, out, arg])
    return []


def test_which_norm_layers_the_chains_accept():
    """The ``*_supported`` questions about the modules themselves (the shapes are the back end's to
    answer): native 2-D norm + ReLU behind a bias-free conv, training or evaluation mode."""
    from nesie_amd.mmdet3d_ops.norm import FusedBNReLU1d, FusedBNReLU2d
    rec = LaunchRecorder()
    x = torch.zeros(B, 4, M, 16)
    train = _sa_modules((4, 64, 128))
    assert fused_mlp.sa_stack_supported(rec, x, train) and not fused_mlp.sa_stack_eval_supported(rec, x, train)
    with torch.no_grad():
        assert not fused_mlp.sa_stack_eval_supported(rec, x, train)         # training-mode norms
        assert fused_mlp.sa_stack_eval_supported(rec, x, [m.eval() for m in _sa_modules((4, 64, 128))])
    assert not fused_mlp.sa_stack_supported(rec, x, _sa_modules((4, 64, 128))[:1])          # one layer
    assert not fused_mlp.sa_stack_supported(rec, x, _sa_modules((4, 64, 96)))              # no whole row tile
    assert not fused_mlp.sa_stack_supported(rec, x, _sa_modules((8, 64, 128)))             # another input width
    assert not fused_mlp.sa_stack_supported(rec, torch.zeros(B, 4, M, 8), train)           # nsample
    assert not fused_mlp.sa_stack_supported(LaunchRecorder({'pw_supported': False}), x, train)
    frozen_stats = _sa_modules((4, 64, 128))
    frozen_stats[1].norm.momentum = None
    assert not fused_mlp.sa_stack_supported(rec, x, frozen_stats)
    x1 = torch.zeros(B, 64, 128)
    shapes = [(64, 128), (128, 16)]
    for norm, ok in ((FusedBNReLU1d(128), True), (FusedBNReLU2d(128), True), (FusedBNReLU1d(128, relu=False), False),
                     (FusedBNReLU1d(128).eval(), False), (FusedBNReLU1d(128, affine=False), False),
                     (torch.nn.BatchNorm1d(128), False)):
        assert fused_mlp.stack1d_supported(rec, x1, shapes, [norm, None]) == ok
    assert not fused_mlp.stack1d_supported(rec, x1, shapes, [None, FusedBNReLU1d(16)])     # plain layer not last
    with torch.no_grad():
        assert not fused_mlp.stack1d_supported(rec, x1, shapes, [FusedBNReLU1d(128), None])


SA1 = (4, 64, 64, 128)
SA2 = (131, 128, 128, 256)
APPLY_PASS = {'pool_tail_supported': False, 'pw_wgrad_bn_supported': False}
# name -> (driver, its arguments, the recorder's answers, module switches)
CASES = {
    'sa1_k4_tail': (_sa, dict(chans=SA1, ns=64, x_grad=False), {}, {}),
    'sa1_stream_tail': (_sa, dict(chans=SA1, ns=64, x_grad=False), {'k4_supported': False}, {}),
    'sa1_stream_dense_pool': (_sa, dict(chans=SA1, ns=64, x_grad=False),
                              {'k4_supported': False, 'pool_tail_supported': False}, {}),
    'sa1_k4_switch_off': (_sa, dict(chans=SA1, ns=64, x_grad=False), {}, {'SA1_K4': False}),
    'sa2_apply_pass_lead0': (_sa, dict(chans=SA2, ns=32, x_grad=True, fixed_lead=0), APPLY_PASS, {}),
    'sa2_apply_pass_lead3': (_sa, dict(chans=SA2, ns=32, x_grad=True, fixed_lead=3), APPLY_PASS, {}),
    'sa2_input_grad_bmm': (_sa, dict(chans=SA2, ns=32, x_grad=True), dict(APPLY_PASS, pw_supported=False), {}),
    'sa2_folded': (_sa, dict(chans=SA2, ns=32, x_grad=True), {}, {}),
    'sa2_unfolded_switch': (_sa, dict(chans=SA2, ns=32, x_grad=True), {}, {'FOLD_NORM_BWD': False}),
    'sa_no_lead_rows': (_sa, dict(chans=(128, 128, 256), ns=32, x_grad=True), {}, {}),
    'sa_two_layers': (_sa, dict(chans=(4, 64, 128), ns=16, x_grad=False), {}, {}),
    'sa_two_layers_dense_pool': (_sa, dict(chans=(4, 64, 128), ns=16, x_grad=False),
                                 {'pool_tail_supported': False}, {}),
    'sa_frozen_middle_weight': (_sa, dict(chans=SA1, ns=64, x_grad=False, frozen=(3,)), {}, {}),
    'sa_frozen_middle_dense': (_sa, dict(chans=SA1, ns=64, x_grad=False, frozen=(3,)), APPLY_PASS, {}),
    'sa_nothing_needs_grad': (_sa, dict(chans=SA1, ns=64, x_grad=True, frozen=range(9)), {}, {}),
    'sa1_slots': (_sa, dict(chans=SA1, ns=64, x_grad=False, owner=True), {}, {}),
    'sa1_stream_slots': (_sa, dict(chans=SA1, ns=64, x_grad=False, owner=True), {'k4_supported': False}, {}),
    'sa2_slots_wgrad_paths': (_sa, dict(chans=SA2, ns=32, x_grad=True, owner=True),
                              dict(APPLY_PASS, pw_wgrad_tiled=False, pw_wgrad_supported=False), {}),
    's1d_s2_bias_norm_then_bias': (_stack1d, dict(S=2, c0=64, spec=[(128, True, True), (32, True, False)]), {}, {}),
    's1d_s1_norm_everywhere': (_stack1d, dict(S=1, c0=64, spec=[(128, False, True), (128, True, True),
                                                               (64, True, True)]), {}, {}),
    's1d_s1_unfolded': (_stack1d, dict(S=1, c0=64, spec=[(128, False, True), (128, True, True), (64, True, True)]),
                        {'pw_wgrad_bn_supported': False}, {}),
    's1d_single_bias_layer': (_stack1d, dict(S=2, c0=32, spec=[(256, True, False)], P=4), {}, {}),
    's1d_input_without_grad': (_stack1d, dict(S=1, c0=64, spec=[(128, True, True), (16, True, False)],
                                              x_grad=False), {}, {}),
    's1d_input_grad_matmul': (_stack1d, dict(S=2, c0=64, spec=[(128, True, True), (32, False, False)]),
                              {'pw_supported': False}, {}),
    's1d_sliced_gradient': (_stack1d, dict(S=1, c0=64, spec=[(128, False, True), (16, True, False)],
                                           sliced=True), {}, {}),
    's1d_slots': (_stack1d, dict(S=1, c0=64, spec=[(128, True, True), (128, False, True), (16, True, False)],
                                 owner=True), {}, {}),
    's1d_slots_last_norm': (_stack1d, dict(S=1, c0=64, spec=[(128, False, True), (64, True, True)], owner=True),
                            {'pw_wgrad_bn_supported': False}, {}),
    'mini_s2_g16': (_mini, dict(S=2, G=16), {}, {}),
    'mini_s1_g64': (_mini, dict(S=1, G=64), {}, {}),
    'mini_s2_g16_dense': (_mini, dict(S=2, G=16), {}, {'MINI_TAIL_SPARSE': False}),
    'mini_s1_g64_dense': (_mini, dict(S=1, G=64), {}, {'MINI_TAIL_SPARSE': False}),
    'mini_s2_g16_unfolded': (_mini, dict(S=2, G=16), {'pw_wgrad_bn_supported': False}, {}),
    'mini_s1_g64_unfolded': (_mini, dict(S=1, G=64), {'pw_wgrad_bn_supported': False}, {}),
    'mini_s2_g16_unmarked_dc': (_mini, dict(S=2, G=16, second_consumer=True), {}, {}),
    'mini_s2_g16_slots': (_mini, dict(S=2, G=16, owner=True), {}, {}),
    'mini_s1_g64_dense_slots': (_mini, dict(S=1, G=64, owner=True), {}, {'MINI_TAIL_SPARSE': False}),
    'mini_s2_g16_frozen_wl': (_mini, dict(S=2, G=16, frozen=('w',)), {}, {}),
    'mini_s1_g64_frozen_w4': (_mini, dict(S=1, G=64, frozen=('w4',)), {}, {}),
    'mini_s2_g16_frozen_w3': (_mini, dict(S=2, G=16, frozen=('w3',)), {}, {}),
    'sa_eval': (_sa_eval, dict(chans=SA2, ns=32), {}, {}),
    'sa_eval_ns16': (_sa_eval, dict(chans=(4, 64, 128), ns=16), {}, {}),
    'mini_eval_s2_g16': (_mini_eval, dict(S=2, G=16), {}, {}),
    'mini_eval_s1_g64': (_mini_eval, dict(S=1, G=64), {}, {}),
    'blend_folded': (_blend, {}, {}, {}),
    'blend_unfolded': (_blend, {}, {}, {'FOLD_NORM_BWD': False}),
    'blend_atomic_table': (_blend, {}, {'blend_backward_writes_table': False}, {}),
    'blend_slots': (_blend, dict(owner=True), {}, {}),
}


def run_case(name):
    """-> (log, [(returned gradient, the slot it must view)])."""
    driver, kwargs, answers, switches = CASES[name]
    rec = LaunchRecorder(answers)
    returned = {}
    real = {f: getattr(fused_mlp, f).backward for f in _FUNCTIONS}
    keep = {k: getattr(fused_mlp, k) for k in switches}

    def spy(f):
        def backward(ctx, *grads):
            out = real[f](ctx, *grads)
            returned[f] = out
            rec.note(f + '.backward returned', out)
            return out
        return staticmethod(backward)
    try:
        for f in _FUNCTIONS:
            setattr(getattr(fused_mlp, f), 'backward', spy(f))
        for k, v in switches.items():
            setattr(fused_mlp, k, v)
        with use_backend(rec):
            views = driver(**kwargs)
    finally:
        for f in _FUNCTIONS:
            setattr(getattr(fused_mlp, f), 'backward', staticmethod(real[f]))
        for k, v in keep.items():
            setattr(fused_mlp, k, v)
    return json.loads(json.dumps(rec.log)), [(returned[f][i], v) for f, i, v in views]


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_launch_trace_equals_the_record(name, recorded):
    log, views = run_case(name)
    want = recorded[name]
    for i, (got, exp) in enumerate(zip(log, want)):
        assert got == exp, f'{name}: entry {i} differs'
    assert len(log) == len(want)
    assert bool(views) == ('slots' in name)
    for grad, slot in views:
        # a parameter gradient that a kernel wrote straight into the flat gradient vector
        assert grad is not None and grad.data_ptr() == slot.data_ptr() and grad.numel() == slot.numel()
        assert grad.untyped_storage()._cdata == slot.untyped_storage()._cdata


def write_fixture(names=None):
    """Record ``names`` (default: the cases the fixture does not hold yet); every other entry is written
    back as it was read."""
    with open(FIXTURE) as fh:
        held = json.load(fh)
    lines = []
    for name in sorted(CASES):
        log = run_case(name)[0] if name not in held or name in (names or ()) else held[name]
        entries = ',\n'.join('  ' + json.dumps(e, separators=(',', ':')) for e in log)
        lines.append(f'{json.dumps(name)}: [\n{entries}\n]')
    with open(FIXTURE, 'w') as fh:
        fh.write('{\n' + ',\n'.join(lines) + '\n}\n')


if __name__ == '__main__':
    import sys
    write_fixture(sys.argv[1:])
