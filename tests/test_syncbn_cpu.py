"""NaiveSyncBatchNorm1d/2d without a GPU: the public surface, the local path under an injected
back end, and the torch formulation of the sync path on two gloo ranks against the float64
referee of tests/_syncbn_ref.py (BatchNorm over the concatenation of the shards)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from nesie_amd import kernels, mmdet3d_ops
from nesie_amd.mmdet3d_ops import norm as N
from tests import _syncbn_ref as R

NAMES = ('NaiveSyncBatchNorm1d', 'NaiveSyncBatchNorm2d')


def test_the_two_names_are_real_and_the_pinned_stubs_still_raise():
    for name in NAMES:
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__
        assert isinstance(getattr(mmdet3d_ops, name), type)
    assert mmdet3d_ops.NaiveSyncBatchNorm1d is N.NaiveSyncBatchNorm1d
    assert mmdet3d_ops.NaiveSyncBatchNorm2d is N.NaiveSyncBatchNorm2d
    assert issubclass(N.NaiveSyncBatchNorm1d, nn.BatchNorm1d)
    assert issubclass(N.NaiveSyncBatchNorm2d, nn.BatchNorm2d)
    # every fused chain gates on these two classes: a sync layer must not pass for one
    assert not issubclass(N.NaiveSyncBatchNorm1d, (N.FusedBNReLU1d, N.FusedBNReLU2d))
    assert not issubclass(N.NaiveSyncBatchNorm2d, (N.FusedBNReLU1d, N.FusedBNReLU2d))
    assert N.NaiveSyncBatchNorm1d(7).state_dict().keys() == nn.BatchNorm1d(7).state_dict().keys()
    assert N.NaiveSyncBatchNorm2d(7).state_dict().keys() == nn.BatchNorm2d(7).state_dict().keys()
    for name in ('assign_score_withk', 'PAConv', 'SparseBottleneck'):
        assert name in mmdet3d_ops._OUT_OF_SCOPE
        with pytest.raises(NotImplementedError):
            getattr(mmdet3d_ops, name)()


def test_constructor_signature_and_conv_module_norm_types():
    m = N.NaiveSyncBatchNorm2d(6, 1e-3, 0.2, True, True, relu=True)
    assert (m.num_features, m.eps, m.momentum, m.affine, m.track_running_stats) == (6, 1e-3, 0.2, True, True)
    assert m.fuse_relu and m.group is None and not N.NaiveSyncBatchNorm1d(6).fuse_relu
    with pytest.raises(TypeError):
        N.NaiveSyncBatchNorm1d(6, 1e-5, 0.1, True, True, True)     # relu is keyword-only
    cm = mmdet3d_ops.ConvModule(3, 8, norm_cfg=dict(type='naiveSyncBN2d'))
    assert type(cm.norm) is N.NaiveSyncBatchNorm2d and cm.act_fused and cm.norm.fuse_relu
    assert cm.state_dict().keys() == mmdet3d_ops.ConvModule(3, 8, norm_cfg=dict(type='BN2d')).state_dict().keys()
    cm = mmdet3d_ops.ConvModule(3, 8, conv_cfg=dict(type='Conv1d'), norm_cfg=dict(type='naiveSyncBN1d'),
                                act_cfg=None)
    assert type(cm.norm) is N.NaiveSyncBatchNorm1d and not cm.act_fused and not cm.norm.fuse_relu
    sa = mmdet3d_ops.PointSAModule(mlp_channels=[3, 8, 8], num_point=4, radius=0.4, num_sample=4,
                                   norm_cfg=dict(type='naiveSyncBN2d'))
    assert all(type(layer.norm) is N.NaiveSyncBatchNorm2d for layer in sa.mlps[0])


def test_the_four_entry_points_are_declared_and_refuse_invalid_sizes_before_any_launch():
    """Status 1 and a message naming the entry point; the refusal comes before any HIP call (safe
    without a GPU): a negative b, c = 0, and a null workspace where one is needed."""
    import ctypes
    from nesie_amd import _lib
    i, f, p, ll, z = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_size_t
    sig = _lib.SIGNATURES
    assert sig['nesie_syncbn_local_moments'] == (i, [i, i, ll, p, p, p, z, p])
    assert sig['nesie_syncbn_forward_apply'] == (i, [i, i, ll] + [p] * 6 + [f, f, i, p, p, p])
    assert sig['nesie_syncbn_backward_local'] == (i, [i, i, ll, p, p, p, p, f, i, p, p, p, p, z, p])
    assert sig['nesie_syncbn_backward_apply'] == (i, [i, i, ll] + [p] * 6 + [f, i, p, p])
    assert sig['nesie_syncbn_workspace_bytes'] == (z, [i, i, ll])
    lib = _lib.load()
    n, a = None, 16     # a: a non-null address that must never be read
    for b, c, ws in ((-1, 4, a), (2, 0, a), (2, 4, None)):
        calls = {
            'syncbn_local_moments': lambda: lib.nesie_syncbn_local_moments(b, c, 8, a, a, ws, 1 << 20, n),
            'syncbn_backward_local': lambda: lib.nesie_syncbn_backward_local(
                b, c, 8, a, a, a, a, 1e-5, 1, a, a, a, ws, 1 << 20, n),
        }
        if ws is not None:
            calls['syncbn_forward_apply'] = lambda: lib.nesie_syncbn_forward_apply(
                b, c, 8, a, a, a, a, a, a, 0.1, 1e-5, 1, a, a, n)
            calls['syncbn_backward_apply'] = lambda: lib.nesie_syncbn_backward_apply(
                b, c, 8, a, a, a, a, a, a, 1e-5, 1, a, n)
        for name, call in calls.items():
            assert call() == 1, (name, b, c, ws)
            assert name.encode() in lib.nesie_last_error(), name
    # a workspace that is too small is refused as well
    assert lib.nesie_syncbn_workspace_bytes(2, 4, 8) == 4 * 2 * 2 * 8
    assert lib.nesie_syncbn_workspace_bytes(70, 3, 8200) == 3 * 140 * 2 * 8
    assert lib.nesie_syncbn_local_moments(2, 4, 8, a, a, a, 8, n) == 1


def test_guards_that_need_no_process_group(oracle_kernels):
    for cls in (N.NaiveSyncBatchNorm1d, N.NaiveSyncBatchNorm2d):
        with pytest.raises(ValueError, match='momentum=None'):
            cls(4, momentum=None)
    with kernels.use_backend(oracle_kernels):
        with pytest.raises(AssertionError, match='float32'):
            N.NaiveSyncBatchNorm1d(4)(torch.zeros(2, 4, 3, dtype=torch.float64))


@pytest.mark.parametrize('dims', [1, 2])
@pytest.mark.parametrize('relu', [True, False])
def test_without_a_process_group_it_is_the_local_norm(oracle_kernels, dims, relu):
    shape = (3, 5, 17) if dims == 1 else (3, 5, 6, 4)
    (x,), (go,), gamma, beta = R.make_inputs([shape], seed=dims)
    ref = (nn.BatchNorm1d if dims == 1 else nn.BatchNorm2d)(5)
    with torch.no_grad():
        ref.weight.copy_(gamma)
        ref.bias.copy_(beta)
    mine = (N.NaiveSyncBatchNorm1d if dims == 1 else N.NaiveSyncBatchNorm2d)(5, relu=relu)
    mine.load_state_dict(ref.state_dict())
    xr, xm = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr = ref(xr)
    yr = torch.relu(yr) if relu else yr
    yr.backward(go)
    with kernels.use_backend(oracle_kernels):
        ym = mine(xm)
        ym.backward(go)
    assert torch.equal(ym, yr) and torch.equal(xm.grad, xr.grad)
    assert torch.equal(mine.weight.grad, ref.weight.grad) and torch.equal(mine.bias.grad, ref.bias.grad)
    assert torch.equal(mine.running_var, ref.running_var)       # the unbiased variance: the local path
    assert int(mine.num_batches_tracked) == 1


# ---- two gloo ranks on the CPU: the torch formulation of the sync path -------------------------
CASES = {   # name -> (class, shard shape per rank)
    'equal_1d': ('NaiveSyncBatchNorm1d', [(2, 5, 33), (2, 5, 33)]),
    'unequal_2d': ('NaiveSyncBatchNorm2d', [(3, 5, 8, 4), (1, 5, 8, 4)]),
    'one_position_per_rank': ('NaiveSyncBatchNorm1d', [(1, 4, 1), (1, 4, 1)]),
}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    import oracle
    from nesie_amd import dp
    dp.init_distributed(backend="gloo")
    out = {}
    for ci, (name, (cls, shapes)) in enumerate(CASES.items()):
        for relu in (True, False):
            xs, gos, gamma, beta = R.make_inputs(shapes, seed=10 + ci)     # the same on both ranks
            layer = getattr(N, cls)(shapes[0][1], relu=relu)
            with torch.no_grad():
                layer.weight.copy_(gamma)
                layer.bias.copy_(beta)
            x = xs[rank].clone().requires_grad_(True)
            y = layer(x)                   # a CPU tensor, no injected back end: the torch formulation
            y.backward(gos[rank])
            out[name, relu] = dict(y=y.detach(), dx=x.grad, dgamma=layer.weight.grad, dbeta=layer.bias.grad,
                                   running_mean=layer.running_mean.clone(),
                                   running_var=layer.running_var.clone(),
                                   tracked=int(layer.num_batches_tracked))
    # the guards of the sync path
    layer = N.NaiveSyncBatchNorm1d(4)
    try:
        layer(torch.zeros(0, 4, 3))
        out['empty'] = 'accepted'
    except AssertionError as e:
        out['empty'] = str(e)
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        try:
            N.NaiveSyncBatchNorm1d(4, **kw)(torch.zeros(2, 4, 3))
            out[tuple(kw)] = 'accepted'
        except RuntimeError as e:
            out[tuple(kw)] = str(e)
    # evaluation mode does no collective: rank 0 ALONE calls the layer and returns (a collective
    # would wait for rank 1 until the barrier below is all that is left to match it)
    if rank == 0:
        with kernels.use_backend(oracle.OracleKernels()):
            layer = N.NaiveSyncBatchNorm1d(4, relu=True).eval()
            x = torch.randn(2, 4, 3)
            out['eval'] = torch.equal(layer(x), torch.relu(nn.BatchNorm1d(4).eval()(x)))
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope='module')
def two_ranks(tmp_path_factory):
    out_dir = tmp_path_factory.mktemp('syncbn')
    mp.spawn(_worker, args=(2, _free_port(), str(out_dir)), nprocs=2, join=True)
    return [torch.load(out_dir / f"rank{r}.pt") for r in range(2)]


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', list(CASES))
def test_two_gloo_ranks_equal_batchnorm_over_the_concatenation(two_ranks, name, relu):
    ci = list(CASES).index(name)
    shapes = CASES[name][1]
    xs, gos, gamma, beta = R.make_inputs(shapes, seed=10 + ci)
    ref = R.Referee(xs, gamma, beta, relu=relu)
    got = [r[name, relu] for r in two_ranks]
    back = ref.backward(gos, [g['y'] for g in got])
    for i, g in enumerate(got):
        ref.check_forward(i, g['y'], name)
        ref.check_backward(i, back, g['dx'], g['dgamma'], g['dbeta'], name)
        ref.check_running(g['running_mean'], g['running_var'])      # global mean, BIASED variance
        assert g['tracked'] == 0                                    # the sync path leaves it alone
    assert torch.equal(got[0]['running_mean'], got[1]['running_mean'])
    assert torch.equal(got[0]['running_var'], got[1]['running_var'])


def test_sync_path_guards_and_eval_mode_without_a_collective(two_ranks):
    for r in two_ranks:
        assert 'empty inputs' in r['empty']
        assert 'affine=True and track_running_stats=True' in r['affine',]
        assert 'affine=True and track_running_stats=True' in r['track_running_stats',]
    assert two_ranks[0]['eval'] is True
