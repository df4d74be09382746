"""PAConv without a GPU: the torch-only helpers against arrays recorded from the reference
(tests/golden/paconv.npz, written by tests/golden/make_paconv_golden.py), the float64 referee
(tests/_paconv_ref.py) against the reference's own formulation and torch autograd, the package
surface, the constructors, the state-dict keys, and the C entry points' argument checks (which
come before any launch).

The golden comparison uses the a-priori bound with u = 2^-53: an inner product of L terms is
within gamma_L * sum |a||b| of the exact value however it is ordered, so two correct float64
evaluations differ by at most twice that; on one machine the arrays are expected to be equal
bit for bit.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _paconv_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'paconv.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def within(got, want, n, S):
    assert got.dtype == torch.float64 and got.shape == want.shape
    bound = 2 * R.gamma(n, R.U64) * S
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() - bound).max())


def test_utils_equal_the_reference_recordings(golden):
    from nesie_amd.mmdet3d_ops.paconv import utils
    for i in range(4):
        a, b = golden[f'dist{i}_a'], golden[f'dist{i}_b']
        want = golden[f'dist{i}_out']
        # three squares, two additions, a root, after one subtraction per coordinate
        within(utils.calc_euclidian_dist(a, b), want, 8, want)
        assert want[0] == 0
        scores, feats = golden[f'score{i}_scores'], golden[f'score{i}_feats']
        S = torch.einsum('bnkm,bnkmo->bnko', scores.abs(), feats.abs())
        within(utils.assign_score(scores, feats), golden[f'score{i}_out'], scores.shape[-1], S)
        feats, bank, m = golden[f'kernel{i}_feats'], golden[f'kernel{i}_bank'], int(golden[f'kernel{i}_m'])
        cin = feats.shape[1]
        assert cin == 3 + i                                   # odd, even, odd, even
        point, center = utils.assign_kernel_withoutk(feats, bank, m)
        rows = feats.permute(0, 2, 1).abs()
        half = lambda w: torch.matmul(rows[:, :, :w.shape[0]], w.abs()).view(*point.shape)
        within(point, golden[f'kernel{i}_point'], cin + 1, half(bank[:cin]) + half(bank[cin:]))
        within(center, golden[f'kernel{i}_center'], cin + 1,
               half(bank[:cin]) + half(bank[cin:cin + 3]))
        if cin % 2 == 0:      # no coordinate term: the centre half is the difference half alone
            assert torch.equal(center, torch.matmul(feats.permute(0, 2, 1), bank[:cin]).view(*center.shape))
        else:
            assert not torch.equal(center, torch.matmul(feats.permute(0, 2, 1), bank[:cin]).view(*center.shape))


def test_utils_run_in_float32_too():
    from nesie_amd.mmdet3d_ops.paconv import utils
    point, center = utils.assign_kernel_withoutk(torch.randn(2, 4, 9), torch.randn(8, 3 * 5), 3)
    assert point.shape == center.shape == (2, 9, 3, 5) and point.dtype == torch.float32
    assert utils.assign_score(torch.randn(2, 3, 4, 3), torch.randn(2, 3, 4, 3, 5)).shape == (2, 3, 4, 5)
    with pytest.raises(AssertionError):
        utils.calc_euclidian_dist(torch.zeros(3, 3), torch.zeros(4, 3))


def test_referee_equals_the_reference_formulation_and_autograd():
    """With every index valid the operator is assign_score(scores, P[knn_idx] - C[knn_idx[..., 0]])
    (what PAConv computes on grouped features), and its gradients are autograd's."""
    from nesie_amd.mmdet3d_ops.paconv import utils
    gen = torch.Generator().manual_seed(5)
    B, N0, N1, K, M, O = 2, 11, 5, 4, 3, 6
    leaf = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).requires_grad_(True)
    points, centers, scores = leaf(B, N0, M, O), leaf(B, N0, M, O), leaf(B, N1, K, M)
    idx = torch.randint(0, N0, (B, N1, K), generator=gen)
    idx[0, 1] = idx[0, 0]                                     # two centres share one cn
    grad_out = torch.randn(B, O, N1, K, generator=gen, dtype=torch.float64)
    batch = torch.arange(B)
    grouped = points[batch[:, None, None], idx] - centers[batch[:, None], idx[:, :, 0]][:, :, None]
    want = utils.assign_score(scores, grouped).permute(0, 3, 1, 2)
    got = R.forward(points.detach(), centers.detach(), scores.detach(), idx)
    torch.testing.assert_close(got['out'], want.detach(), rtol=0, atol=1e-12)
    assert int(got['n'].min()) == 3 * M - 1 == int(got['n'].max())
    want.backward(grad_out)
    back = R.backward(points.detach(), centers.detach(), scores.detach(), idx, grad_out)
    torch.testing.assert_close(back['grad_scores'], scores.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(back['grad_points'], points.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(back['grad_centers'], centers.grad, rtol=0, atol=1e-12)


def test_referee_validity_rule():
    gen = torch.Generator().manual_seed(6)
    B, N0, N1, K, M, O = 1, 4, 3, 3, 2, 2
    points, centers = torch.randn(B, N0, M, O, generator=gen), torch.randn(B, N0, M, O, generator=gen)
    scores = torch.randn(B, N1, K, M, generator=gen)
    idx = torch.tensor([[[0, 1, -1], [N0, 2, 3], [1, 2 ** 31 + 3, 1]]])
    got = R.forward(points, centers, scores, idx)
    assert torch.equal(got['out'][0, :, 0, 2], torch.zeros(O, dtype=torch.float64))
    assert torch.equal(got['out'][0, :, 1, 0], torch.zeros(O, dtype=torch.float64))
    assert torch.equal(got['out'][0, :, 2, 1], torch.zeros(O, dtype=torch.float64))
    # an invalid centre index: the centre row is dropped, the neighbour's term stays
    want = torch.einsum('m,mo->o', scores[0, 1, 1].double(), points[0, 2].double())
    torch.testing.assert_close(got['out'][0, :, 1, 1], want, rtol=0, atol=1e-14)
    assert got['n'][0, 0].tolist() == [[5, 5, 0], [0, 3, 3], [5, 0, 5]]
    back = R.backward(points, centers, scores, idx, torch.randn(B, O, N1, K, generator=gen))
    assert torch.equal(back['grad_scores'][0, 0, 2], torch.zeros(M, dtype=torch.float64))
    assert back['n_points'][0, :, 0, 0].tolist() == [1, 5, 1, 1]
    assert back['n_centers'][0, :, 0, 0].tolist() == [3, 3, 0, 0]


def test_package_surface():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import build_sa_module, paconv
    from nesie_amd.mmdet3d_ops.pointnet_modules import SA_MODULES
    assert paconv.__all__ == ['assign_score_withk', 'PAConv', 'PAConvCUDA']
    for name in ('PAConvCUDA', 'PAConvSAModuleMSG', 'PAConvSAModule', 'PAConvCUDASAModule',
                 'PAConvCUDASAModuleMSG'):
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__ and isinstance(getattr(mmdet3d_ops, name), type)
    assert mmdet3d_ops.PAConvCUDA is paconv.PAConvCUDA
    with pytest.raises(NotImplementedError, match='mmdet3d_ops.paconv'):
        mmdet3d_ops.PAConv()
    for kind in ('PAConvSAModule', 'PAConvCUDASAModule'):
        built = build_sa_module(dict(type=kind, num_point=16, radius=0.4, num_sample=8,
                                     mlp_channels=[4, 8, 16], paconv_num_kernels=[4, 4]))
        assert type(built) is SA_MODULES[kind] and len(built.mlps) == 1 and len(built.mlps[0]) == 2
    for kind in ('PAConvSAModuleMSG', 'PAConvCUDASAModuleMSG'):
        built = build_sa_module(dict(type=kind, num_point=16, radii=[0.2, 0.4], sample_nums=[4, 8],
                                     mlp_channels=[[4, 8], [4, 8, 16]],
                                     paconv_num_kernels=[[4], [4, 2]]))
        assert type(built) is SA_MODULES[kind] and [len(m) for m in built.mlps] == [1, 2]
        assert built.groupers[0].return_grouped_xyz
        assert built.groupers[0].return_grouped_idx == (kind == 'PAConvCUDASAModuleMSG')


def test_constructors():
    from nesie_amd.mmdet3d_ops.paconv import PAConv, PAConvCUDA
    from nesie_amd.mmdet3d_ops.paconv.paconv import ScoreNet
    from nesie_amd.mmdet3d_ops import PAConvSAModuleMSG, PAConvCUDASAModuleMSG
    layer = PAConv(6, 10, 4)
    assert tuple(layer.weight_bank.shape) == (12, 40) and layer.kernel_mul == 2 and layer.m == 4
    assert tuple(PAConv(6, 10, 4, kernel_input='identity', weight_bank_init='xavier').weight_bank.shape) == (6, 40)
    for how, width in (('identity', 3), ('w_neighbor', 6), ('w_neighbor_dist', 7)):
        net = PAConv(6, 10, 4, scorenet_input=how).scorenet
        assert net.mlps.layer0.conv.in_channels == width
        assert net.mlps.layer3.conv.out_channels == 4 and net.mlps.layer3.conv.bias is not None
        assert net.mlps.layer3.norm is None and not net.mlps.layer3.with_activation
    assert PAConv(6, 10, 4, norm_cfg=None, act_cfg=None).bn is None
    assert PAConv(6, 10, 4, norm_cfg=None, act_cfg=None).activate is None
    assert PAConv(6, 10, 4).bn.momentum == 0.1
    assert ScoreNet([3, 8, 4], last_bn=True).mlps.layer1.norm is not None
    with pytest.raises(NotImplementedError, match='kernel_input'):
        PAConv(6, 10, 4, kernel_input='neighbor')
    with pytest.raises(NotImplementedError, match='scorenet_input'):
        PAConv(6, 10, 4, scorenet_input='dist')
    with pytest.raises(NotImplementedError, match='weight bank init'):
        PAConv(6, 10, 4, weight_bank_init='normal')
    with pytest.raises(AssertionError, match='score_norm'):
        PAConv(6, 10, 4, scorenet_cfg=dict(mlp_channels=[8], score_norm='tanh'))
    with pytest.raises(AssertionError, match='w_neighbor'):
        PAConvCUDA(6, 10, 4, kernel_input='identity')
    for cls in (PAConvSAModuleMSG, PAConvCUDASAModuleMSG):
        with pytest.raises(AssertionError):
            cls(16, [0.2], [8], [[4, 8]], paconv_num_kernels=[[4], [4]])
        with pytest.raises(AssertionError, match='weight kernels'):
            cls(16, [0.2], [8], [[4, 8, 16]], paconv_num_kernels=[[4]])
    # a caller's config is read, never written
    cfg = dict(mlp_channels=[8, 16], score_norm='sigmoid', temp_factor=2.0, last_bn=False)
    before = copy.deepcopy(cfg)
    for build in (lambda: PAConv(6, 10, 4, scorenet_cfg=cfg), lambda: PAConvCUDA(6, 10, 4, scorenet_cfg=cfg),
                  lambda: PAConvSAModuleMSG(16, [0.2], [8], [[4, 8]], [[4]], scorenet_cfg=cfg, bias=True),
                  lambda: PAConvCUDASAModuleMSG(16, [0.2], [8], [[4, 8]], [[4]], scorenet_cfg=cfg)):
        made = build()
        assert cfg == before
    assert made.mlps[0][0].scorenet.score_norm == 'sigmoid'
    # two default constructions see the same defaults (the reference grows its default list)
    assert len(PAConv(6, 10, 4).scorenet.mlps) == len(PAConv(6, 10, 4).scorenet.mlps) == 4


def _norm_keys(prefix):
    return {f'{prefix}.{leaf}' for leaf in ('weight', 'bias', 'running_mean', 'running_var',
                                             'num_batches_tracked')}


@pytest.mark.parametrize('kind, bank', [('PAConvSAModule', 'mlps.0.layer0'),
                                        ('PAConvCUDASAModule', 'mlps.0.0')])
def test_state_dict_keys(kind, bank):
    from nesie_amd.mmdet3d_ops import build_sa_module
    module = build_sa_module(dict(type=kind, num_point=16, radius=0.4, num_sample=8,
                                  mlp_channels=[4, 8], paconv_num_kernels=[4],
                                  scorenet_cfg=dict(mlp_channels=[8, 8], score_norm='softmax',
                                                    temp_factor=1.0, last_bn=False)))
    want = {f'{bank}.weight_bank'} | _norm_keys(f'{bank}.bn')
    for j in (0, 1):
        want |= {f'{bank}.scorenet.mlps.layer{j}.conv.weight'} | _norm_keys(f'{bank}.scorenet.mlps.layer{j}.bn')
    want |= {f'{bank}.scorenet.mlps.layer2.conv.weight', f'{bank}.scorenet.mlps.layer2.conv.bias'}
    assert set(module.state_dict()) == want
    assert tuple(module.state_dict()[f'{bank}.weight_bank'].shape) == (2 * (4 + 3), 4 * 8)
    # the default ScoreNet has one more hidden layer: layer3 is the bias-carrying last one
    default = build_sa_module(dict(type=kind, num_point=16, radius=0.4, num_sample=8,
                                   mlp_channels=[4, 8], paconv_num_kernels=[4]))
    assert f'{bank}.scorenet.mlps.layer3.conv.bias' in default.state_dict()
    assert f'{bank}.scorenet.mlps.layer2.bn.weight' in default.state_dict()


def test_entry_points_check_their_arguments_before_any_launch():
    from nesie_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    fwd = lambda *sizes: lib.nesie_assign_score_withk_forward(*sizes, null, null, null, null, null, null)
    bwd = lambda *sizes: lib.nesie_assign_score_withk_backward(*sizes, null, null, null, null, null, null,
                                                               null, null, null, 0, null)
    for call, name in ((fwd, 'assign_score_withk_forward'), (bwd, 'assign_score_withk_backward')):
        for sizes in ((-1, 4, 4, 2, 2, 2), (1, -4, 4, 2, 2, 2), (1, 4, -4, 2, 2, 2), (1, 4, 4, 0, 2, 2),
                      (1, 4, 4, 2, 0, 2), (1, 4, 4, 2, 2, -1)):
            assert call(*sizes) == 1, sizes
            assert name in lib.nesie_last_error().decode()
        for sizes in ((0, 4, 4, 2, 2, 2), (1, 0, 4, 2, 2, 2), (1, 4, 0, 2, 2, 2)):
            assert call(*sizes) == 0, sizes
        assert call(1, 1 << 20, 4, 2, 64, 64) == 2           # 2^32 point features
        assert name in lib.nesie_last_error().decode()
        assert call(4, 4, 1 << 20, 64, 2, 16) == 2           # 2^32 outputs
    # non-empty with null pointers: an argument error for the forward; a backward that is asked for
    # no gradient has nothing to do
    assert fwd(1, 4, 4, 2, 2, 2) == 1 and bwd(1, 4, 4, 2, 2, 2) == 0
    ws = lib.nesie_assign_score_withk_backward_workspace_bytes
    assert ws(0, 4, 4, 2, 2, 2) == 0 and ws(1, 4, 4, -2, 2, 2) == 0 and ws(1, 1 << 20, 4, 2, 64, 64) == 0
    # gT (B*N1*K*O floats) + four int arrays over the pairs + four over the centres, each padded to 16 bytes
    assert ws(2, 5, 3, 4, 2, 7) == 2 * 3 * 4 * 7 * 4 + 4 * (2 * 3 * 4 * 4) + 4 * 32
    assert lib.nesie_abi_version() == 2


def test_function_refuses_cpu_tensors_and_unknown_aggregates():
    from nesie_amd.mmdet3d_ops.paconv import assign_score_withk
    scores, feats = torch.rand(1, 3, 2, 2), torch.rand(1, 5, 2, 4)
    idx = torch.zeros(1, 3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        assign_score_withk(scores, feats, feats, idx)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        assign_score_withk(scores, feats, feats, idx, 'max')
    with pytest.raises(KeyError):
        assign_score_withk(scores, feats, feats, idx, 'mean')
