"""PAConv on the device: the three kernels of csrc/paconv.hip against the float64 referee
(tests/_paconv_ref.py), the autograd Function's contract, the two layers and the four
set-abstraction modules.

The value bound, no element excused: |dev - f64| <= gamma_n * S, gamma_n = n u / (1 - n u),
u = 2^-24, with n the element's own number of products, subtractions and additions and S the
referee's sum on absolute operands (tests/_paconv_ref.py; the bound of tests/test_spconv_gpu.py).
It holds for any order of the sum, fused or not.  An element with n == 0 -- an invalid pair, a
point that nobody references -- has the bound 0 and must be exactly 0.0.
"""
import functools

import pytest
import torch

from tests import _paconv_ref as R
from tests._launch_recorder import LaunchRecorder

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1, 1), (2, 37, 5, 3, 2, 7), (2, 64, 16, 16, 8, 64), (1, 130, 33, 17, 16, 65),
          (2, 256, 64, 32, 16, 128)]
PATTERNS = ['random', 'ball_padded', 'one_source', 'half_unreferenced', 'invalid', 'shared_centre']
BAD = (-1, None, 2 ** 31 + 3)      # None: N0 itself


def make_idx(pattern, B, N0, N1, K, gen):
    idx = torch.randint(0, N0, (B, N1, K), generator=gen)
    if pattern == 'ball_padded':        # a ball query's row: its hits, then the first hit again
        hits = torch.randint(1, K + 1, (B, N1, 1), generator=gen)
        idx = torch.where(torch.arange(K).view(1, 1, K) < hits, idx, idx[:, :, :1])
    elif pattern == 'one_source':       # one run of N1 * K entries
        idx[:] = N0 // 2
    elif pattern == 'half_unreferenced':
        idx = idx % max((N0 + 1) // 2, 1)
    elif pattern == 'invalid':
        for r in range(N1):
            bad = BAD[r % 3]
            bad = N0 if bad is None else bad
            if r % 2 == 0:              # at k = 0: the centre index itself is out of range
                idx[:, r, 0] = bad
            if K > 1:                   # and at some k > 0 of every row
                idx[:, r, 1 + r % (K - 1)] = BAD[(r + 1) % 3] if BAD[(r + 1) % 3] is not None else N0
    elif pattern == 'shared_centre':
        idx[:, 1::2, 0] = idx[:, 0::2, 0][:, :idx[:, 1::2].shape[1]]
    return idx


@functools.lru_cache(maxsize=None)
def case(shape, pattern, device):
    """Inputs on the device and the referee's float64 results, computed once per case."""
    B, N0, N1, K, M, O = shape
    gen = torch.Generator().manual_seed(hash((shape, PATTERNS.index(pattern))) % (2 ** 31))
    rand = lambda *s: torch.randn(*s, generator=gen).to(device)
    c = dict(points=rand(B, N0, M, O), centers=rand(B, N0, M, O), scores=rand(B, N1, K, M),
             idx=make_idx(pattern, B, N0, N1, K, gen).to(device), grad_out=rand(B, O, N1, K))
    c['fwd'] = R.forward(c['points'], c['centers'], c['scores'], c['idx'])
    c['bwd'] = R.backward(c['points'], c['centers'], c['scores'], c['idx'], c['grad_out'])
    return c


def nan_like(t):
    return torch.full_like(t, float('nan'))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_values_against_float64(hip_device, shape, pattern):
    from nesie_amd.kernels import backend_for
    B, N0, N1, K, M, O = shape
    c = case(shape, pattern, str(hip_device))
    hip = backend_for(c['points'])
    out = torch.full((B, O, N1, K), float('nan'), device=hip_device)
    hip.assign_score_withk_forward(B, N0, N1, M, K, O, c['points'], c['centers'], c['scores'], c['idx'], out)
    gp, gc, gs = nan_like(c['points']), nan_like(c['centers']), nan_like(c['scores'])
    hip.assign_score_withk_backward(B, N0, N1, M, K, O, c['grad_out'], c['points'], c['centers'],
                                    c['scores'], c['idx'], gp, gc, gs)
    label = f'{"x".join(map(str, shape))} {pattern}'
    f, b = c['fwd'], c['bwd']
    R.check(f'{label} output', out, f['out'], f['S'], f['n'])
    R.check(f'{label} grad_scores', gs, b['grad_scores'], b['S_scores'], b['n_scores'])
    R.check(f'{label} grad_points', gp, b['grad_points'], b['S_points'], b['n_points'])
    R.check(f'{label} grad_centers', gc, b['grad_centers'], b['S_centers'], b['n_centers'])
    # said once more in plain words: invalid pairs and unreferenced rows are zeros, not small numbers
    invalid = (c['idx'] < 0) | (c['idx'] >= N0)
    assert not out.permute(0, 2, 3, 1)[invalid].any() and not gs[invalid].any()
    assert not gp[b['n_points'] == 0].any() and not gc[b['n_centers'] == 0].any()
    if pattern == 'invalid' and N1 > 1:
        assert invalid[:, :, 0].any() and (K == 1 or invalid[:, :, 1:].any())
    if pattern == 'half_unreferenced' and N0 > 1:
        assert (b['n_points'][:, (N0 + 1) // 2:] == 0).all()


MID = (1, 130, 33, 17, 16, 65)
VEC = (2, 64, 16, 16, 8, 64)


def run_function(c, want=(True, True, True), idx=None):
    from nesie_amd.mmdet3d_ops.paconv import assign_score_withk
    leaves = [c[k].clone().requires_grad_(w) for k, w in zip(('scores', 'points', 'centers'), want)]
    out = assign_score_withk(leaves[0], leaves[1], leaves[2], c['idx'] if idx is None else idx, 'sum')
    if any(want):
        out.backward(c['grad_out'])
    return out.detach(), [leaf.grad for leaf in leaves]


@pytest.mark.parametrize('shape', [MID, VEC], ids=['scalar', 'vector'])
def test_needs_input_grad_and_repeat_runs_give_the_same_bits(hip_device, shape):
    from nesie_amd.kernels import HipKernels
    from nesie_amd.mmdet3d_ops.paconv import assign_score_withk
    c = case(shape, 'invalid', str(hip_device))
    out, grads = run_function(c)
    assert all(g is not None for g in grads)
    R.check('function output', out, c['fwd']['out'], c['fwd']['S'], c['fwd']['n'])
    for name, g in zip(('scores', 'points', 'centers'), grads):
        R.check(f'function grad_{name}', g, c['bwd'][f'grad_{name}'], c['bwd'][f'S_{name}'],
                c['bwd'][f'n_{name}'])
    for alone in range(3):
        want = tuple(i == alone for i in range(3))
        out1, grads1 = run_function(c, want)
        assert torch.equal(out1, out) and torch.equal(grads1[alone], grads[alone])
        assert all(g is None for i, g in enumerate(grads1) if i != alone)
    out0, grads0 = run_function(c, (False, False, False))
    assert torch.equal(out0, out) and grads0 == [None, None, None]
    assert not assign_score_withk(c['scores'], c['points'], c['centers'], c['idx']).requires_grad
    again, grads_again = run_function(c)
    assert torch.equal(again, out) and all(torch.equal(a, g) for a, g in zip(grads_again, grads))
    with HipKernels.cu_budget(232):
        budget, grads_budget = run_function(c)
    assert torch.equal(budget, out) and all(torch.equal(a, g) for a, g in zip(grads_budget, grads))
    for how in ('avg', 'max'):      # accepted, and as in the reference without effect
        assert torch.equal(assign_score_withk(c['scores'], c['points'], c['centers'], c['idx'], how), out)
    with pytest.raises(KeyError):
        assign_score_withk(c['scores'], c['points'], c['centers'], c['idx'], 'mean')


def test_int32_index_equals_int64(hip_device):
    B, N0, N1, K, M, O = MID
    c = case(MID, 'ball_padded', str(hip_device))
    idx = c['idx'].clone()
    idx[:, 0, 0], idx[:, 1, 2], idx[:, 2, 1] = -1, N0, -7
    want, want_grads = run_function(c, idx=idx)
    got, got_grads = run_function(c, idx=idx.int())
    assert torch.equal(got, want) and all(torch.equal(a, g) for a, g in zip(got_grads, want_grads))
    assert not want[:, :, 0, 0].any() and not want[:, :, 1, 2].any() and want[:, :, 1, 1].any()


def test_graph_replay_equals_eager(hip_device):
    from nesie_amd.mmdet3d_ops.paconv import assign_score_withk
    c = case(VEC, 'invalid', str(hip_device))
    eager_out, eager_grads = run_function(c)
    leaves = [c[k].clone().requires_grad_(True) for k in ('scores', 'points', 'centers')]

    def step():
        out = assign_score_withk(leaves[0], leaves[1], leaves[2], c['idx'], 'sum')
        return (out,) + torch.autograd.grad(out, leaves, c['grad_out'])

    side = torch.cuda.Stream(hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(hip_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize(hip_device)
    assert torch.equal(captured[0], eager_out)
    assert all(torch.equal(a, g) for a, g in zip(captured[1:], eager_grads))


def test_empty_problems_launch_nothing(hip_device):
    from nesie_amd import kernels
    from nesie_amd.mmdet3d_ops.paconv import assign_score_withk
    for B, N0, N1 in ((0, 5, 3), (2, 5, 0), (2, 0, 3)):
        K, M, O = 4, 2, 6
        leaf = lambda *s: torch.randn(*s, device=hip_device, requires_grad=True)
        scores, points, centers = leaf(B, N1, K, M), leaf(B, N0, M, O), leaf(B, N0, M, O)
        idx = torch.zeros(B, N1, K, dtype=torch.int64, device=hip_device)
        with kernels.use_backend(LaunchRecorder()) as rec:
            out = assign_score_withk(scores, points, centers, idx)
            out.sum().backward()
        assert rec.log == []
        assert tuple(out.shape) == (B, O, N1, K) and not out.any()
        for t in (scores, points, centers):
            assert t.grad.shape == t.shape and not t.grad.any()


# ---------------------------------------------------------------------------------------------
# layers


def layer_inputs(device, channels, seed):
    from nesie_amd.mmdet3d_ops import QueryAndGroup
    gen = torch.Generator().manual_seed(seed)
    xyz = torch.rand(2, 128, 3, generator=gen).to(device)
    feats = torch.randn(2, channels, 128, generator=gen).to(device)
    grouper = QueryAndGroup(0.4, 8, use_xyz=False, return_grouped_xyz=True, return_grouped_idx=True)
    grouped, grouped_xyz, idx = grouper(xyz, xyz[:, :16].contiguous(), feats)
    return feats, grouped, grouped_xyz, idx


def run_cuda_layer(layer, feats, grouped_xyz, idx):
    """-> the layer's output, the scores its ScoreNet produced in that very call, and the
    referee's aggregate of those scores with the device's assign_kernel_withoutk outputs."""
    from nesie_amd.mmdet3d_ops.paconv.utils import assign_kernel_withoutk
    seen = []
    hook = layer.scorenet.register_forward_hook(lambda mod, args, result: seen.append(result))
    with torch.no_grad():
        out = layer((feats, grouped_xyz, idx.long()))[0]
        point, center = assign_kernel_withoutk(feats, layer.weight_bank, layer.m)
    hook.remove()
    return out, seen[0].contiguous(), R.forward(point, center, seen[0].contiguous(), idx)


def test_layers_against_the_float64_aggregate(hip_device):
    """PAConvCUDA is held to the kernel's own bound.  PAConv reaches the same sum by another
    route -- the bank applied to cat(f_kn - f_cn, f_kn) per pair, then the blend -- so its distance
    from the aggregate of the GIVEN float32 bank outputs has two parts: its own rounding and the
    rounding already inside the given ones.  With C input channels each route is a chain of at most
    2C products and 2C additions (the bank) plus one subtraction, then M products and M additions
    (the blend); both are bounded by gamma_k * S_w with k that count and
        S_w = sum_m |s| sum_c (|f_kn| + |f_cn|) (|W_diff| + |W_self|),
    which dominates every partial sum of either route.  The bound is gamma_n * S_w with n the sum of
    the two counts."""
    from nesie_amd.mmdet3d_ops.paconv import PAConv, PAConvCUDA
    C, O, M = 4, 16, 4
    feats, grouped, grouped_xyz, idx = layer_inputs(hip_device, C, 11)
    torch.manual_seed(3)
    fast = PAConvCUDA(C, O, M, norm_cfg=None, act_cfg=None).to(hip_device).eval()
    plain = PAConv(C, O, M, norm_cfg=None, act_cfg=None).to(hip_device).eval()
    plain.load_state_dict(fast.state_dict())
    out, scores, ref = run_cuda_layer(fast, feats, grouped_xyz, idx)
    assert tuple(out.shape) == (2, O, 16, 8)
    R.check('PAConvCUDA', out, ref['out'], ref['S'], ref['n'])
    with torch.no_grad():
        out_plain = plain((grouped, grouped_xyz))[0]
    bank = fast.weight_bank.detach().double().abs().view(2 * C, M, O)
    f_abs = grouped.double().abs()                                          # (B, C, npoint, K)
    f_sum = f_abs + f_abs[..., :1]
    S_w = torch.einsum('bnkm,bcnk,cmo->bonk', scores.double().abs(), f_sum, bank[:C] + bank[C:])
    n = 2 * (4 * C + 1 + 2 * M)
    R.check('PAConv', out_plain, ref['out'], S_w, torch.full_like(S_w, n))


def test_odd_width_layer_against_the_referee(hip_device):
    from nesie_amd.mmdet3d_ops.paconv import PAConvCUDA
    feats, _, grouped_xyz, idx = layer_inputs(hip_device, 3, 12)
    torch.manual_seed(4)
    layer = PAConvCUDA(3, 10, 4, norm_cfg=None, act_cfg=None).to(hip_device).eval()
    out, _, ref = run_cuda_layer(layer, feats, grouped_xyz, idx)
    R.check('PAConvCUDA, 3 channels', out, ref['out'], ref['S'], ref['n'])
    assert out.abs().max() > 0


# ---------------------------------------------------------------------------------------------
# set-abstraction modules

SSG = dict(num_point=16, radius=0.4, num_sample=8, mlp_channels=[4, 8, 16], paconv_num_kernels=[4, 4])
MSG = dict(num_point=16, radii=[0.2, 0.4], sample_nums=[4, 8], mlp_channels=[[4, 8], [4, 8, 16]],
           paconv_num_kernels=[[4], [4, 4]])


def run_module(module, xyz, feats):
    for p in module.parameters():
        p.grad = None
    new_xyz, out, indices = module(xyz, feats)
    out.square().mean().backward()
    return new_xyz, out.detach(), indices, [p.grad.clone() for p in module.parameters()]


@pytest.mark.parametrize('kind, cfg, width', [
    ('PAConvCUDASAModule', SSG, 16), ('PAConvSAModule', SSG, 16),
    ('PAConvCUDASAModuleMSG', MSG, 24), ('PAConvSAModuleMSG', MSG, 24)])
def test_sa_modules_end_to_end(hip_device, kind, cfg, width):
    from nesie_amd.mmdet3d_ops import build_sa_module
    torch.manual_seed(7)
    module = build_sa_module(dict(type=kind, **cfg)).to(hip_device)
    xyz = torch.rand(2, 128, 3, device=hip_device)
    feats = torch.randn(2, 4, 128, device=hip_device)
    new_xyz, out, indices, grads = run_module(module, xyz, feats)
    assert tuple(new_xyz.shape) == (2, 16, 3) and tuple(out.shape) == (2, width, 16)
    assert tuple(indices.shape) == (2, 16)
    assert torch.isfinite(out).all() and out.abs().max() > 0
    names = [n for n, _ in module.named_parameters()]
    assert len(grads) == len(names) > 0
    for name, g in zip(names, grads):
        assert torch.isfinite(g).all(), name
    assert any(g.abs().max() > 0 for n, g in zip(names, grads) if n.endswith('weight_bank'))
    new_xyz2, out2, indices2, grads2 = run_module(module, xyz, feats)
    assert torch.equal(out2, out) and torch.equal(new_xyz2, new_xyz) and torch.equal(indices2, indices)
    for name, a, b in zip(names, grads2, grads):
        assert torch.equal(a, b), name
