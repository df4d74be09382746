"""RoI-aware 3-D pooling and points_in_boxes_gpu on the device: bit-exact against the numpy referee
(tests/_roiaware_ref.py), the fixed-order backward, the module, and graph capture."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import _roiaware_ref as R
from tests.test_roiaware_cpu import random_rois

pytestmark = pytest.mark.gpu

GARBAGE_I = 0x7f7f7f7f


def _out3(out_size):
    return (out_size,) * 3 if isinstance(out_size, int) else tuple(out_size)


# name -> (N, P, C, out_size, m)
CASES = {
    'degenerate': (1, 1, 1, 1, 2),
    'tile_plus_one': (3, 257, 3, (2, 3, 5), 8),
    'overlapping': (5, 1000, 65, 4, 128),
    'overflow': (2, 300, 4, 2, 4),
    'capacity_zero': (2, 300, 4, 2, 1),
    'empty_box_ties': (4, 512, 128, 4, 16),
    'many_boxes': (70000, 64, 1, 1, 4),
    'proposals': (256, 4096, 128, 4, 128),
}
MANY_DISTINCT = 700      # 'many_boxes' repeats this many distinct boxes: the referee runs them once


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rois, pts, feat (numpy), out, m, table, idx, kept, max=(pooled, argmax), avg=...),
    computed once per session and never modified."""
    N, P, C, out_size, m = CASES[name]
    out = _out3(out_size)
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    feat = rng.standard_normal((P, C)).astype(np.float32)
    tile = 1
    if name == 'degenerate':
        rois = np.array([[0.1, -0.2, 0.0, 1.0, 2.0, 1.5, 0.3]], np.float32)
        pts = np.array([[0.2, -0.1, 0.7]], np.float32)
    elif name in ('overflow', 'capacity_zero'):
        rois = np.array([[0.0, 0.0, -0.25, 0.5, 0.5, 0.5, 0.4], [3.0, 3.0, 0.0, 1.0, 1.0, 1.0, -1.0]],
                        np.float32)
        pts = rng.uniform(-0.15, 0.15, (P, 3)).astype(np.float32)     # all inside box 0
    elif name == 'empty_box_ties':
        rois = random_rois(rng, N, centre_span=0.5)
        rois[2, :3] = (40.0, 40.0, 40.0)                               # holds no point
        pts = rng.uniform(-1.5, 1.5, (P, 3)).astype(np.float32)
        # all negative, few distinct values, and every row appears twice (points 2i and 2i + 1)
        feat = (-1.0 - rng.integers(0, 3, (P // 2, C))).astype(np.float32).repeat(2, axis=0)
    elif name == 'many_boxes':
        tile = N // MANY_DISTINCT
        rois = random_rois(rng, MANY_DISTINCT, centre_span=1.0)
        pts = rng.uniform(-2.0, 2.0, (P, 3)).astype(np.float32)
    elif name == 'proposals':
        rois = random_rois(rng, N, centre_span=3.0)
        pts = rng.uniform(-4.0, 4.0, (P, 3)).astype(np.float32)
    else:
        rois = random_rois(rng, N, centre_span=0.6)
        pts = rng.uniform(-1.6, 1.6, (P, 3)).astype(np.float32)
        if name == 'tile_plus_one':
            pts[256] = rois[1, :3] + np.array([0.0, 0.0, 0.5 * rois[1, 5]], np.float32)
    nvox = out[0] * out[1] * out[2]
    table = R.voxel_table(rois, pts, out)
    idx, kept = R.collect(table, nvox, m)
    res = dict(out=out, m=m, pts=pts, feat=feat)
    rep = lambda a: np.tile(a, (tile,) + (1,) * (a.ndim - 1)) if tile > 1 else a   # noqa: E731
    for mode in ('max', 'avg'):
        pooled, argmax = R.pool(idx, feat, mode)
        res[mode] = (rep(pooled).reshape(-1, *out, C), rep(argmax).reshape(-1, *out, C))
    res.update(rois=rep(rois), table=rep(table), kept=rep(kept), idx=rep(idx).reshape(-1, *out, m))
    assert res['rois'].shape[0] == N
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_forward(dev, c, mode, with_table=True):
    """The raw entry on garbage-filled outputs -> (pooled, argmax, idx, pts_voxel) tensors."""
    from nesie_amd.kernels import HipKernels
    rois, pts, feat = (torch.from_numpy(c[k]).to(dev) for k in ('rois', 'pts', 'feat'))
    N, P, C = rois.shape[0], pts.shape[0], feat.shape[1]
    pooled = torch.full((N, *c['out'], C), float('nan'), device=dev)
    argmax = torch.full((N, *c['out'], C), GARBAGE_I, dtype=torch.int32, device=dev)
    idx = torch.full((N, *c['out'], c['m']), GARBAGE_I, dtype=torch.int32, device=dev)
    pts_voxel = torch.full((N, P), GARBAGE_I, dtype=torch.int32, device=dev) if with_table else None
    HipKernels().roiaware_pool3d_forward(rois, pts, feat, argmax, idx, pooled,
                                         0 if mode == 'max' else 1, pts_voxel)
    return pooled, argmax, idx, pts_voxel


def _exercises_its_point(name, c):
    idx, table, kept, m = c['idx'], c['table'], c['kept'], c['m']
    counts = idx[..., 0]
    if name == 'degenerate':
        assert counts.tolist() == [[[[1]]]]
    elif name == 'tile_plus_one':
        assert kept[1, 256] >= 0                                    # the point past the first tile
        used = np.unique(table[table >= 0])
        oy, oz = c['out'][1], c['out'][2]
        # voxels that differ in x only, y only, z only are all occupied: a swapped axis would show
        assert len(np.unique(used // (oy * oz))) == 2 and len(np.unique(used // oz % oy)) == 3 \
            and len(np.unique(used % oz)) == 5
    elif name == 'overlapping':
        assert ((table >= 0).sum(0) >= 2).sum() >= 20               # points in several boxes
        assert np.abs(c['rois'][:, 6] % (math.pi / 2)).min() > 0.05   # rotated
    elif name == 'overflow':
        assert (table[0] >= 0).all() and (table[1] < 0).all()
        assert counts[0].min() == 3 and (kept[0] >= 0).sum() == 3 * 8   # 300 points, 24 kept
        # the kept ones are each voxel's first three in point order
        for v in range(8):
            assert idx.reshape(2, 8, m)[0, v, 1:].tolist() == np.nonzero(table[0] == v)[0][:3].tolist()
    elif name == 'capacity_zero':
        assert (table[0] >= 0).all() and not idx.any() and (kept < 0).all()
        assert not c['max'][0].any() and (c['max'][1] == -1).all() and not c['avg'][0].any()
    elif name == 'empty_box_ties':
        assert not counts[2].any() and counts[[0, 1, 3]].any()
        assert (c['feat'] < 0).all()
        pooled, argmax = c['max']
        flat_idx, ties = idx.reshape(-1, m), 0
        for v in np.nonzero(flat_idx[:, 0] >= 2)[0][:50]:
            rows = c['feat'][flat_idx[v, 1:1 + flat_idx[v, 0]]]
            ties += int(((rows == rows.max(0)).sum(0) >= 2).sum())
        assert ties > 100
        assert (pooled[counts > 0] < 0).all()                       # a max found among negatives
    elif name == 'many_boxes':
        assert idx.shape[0] == 70000 > 65535 and counts[65536:].any()
        assert ((table >= 0).sum(1) > 3).any() and counts.max() == 3     # and some voxel overflowed
    elif name == 'proposals':
        assert counts.max() < m - 1 and (counts > 0).sum() > 2000
        assert (table[:, 4000:] >= 0).any()                          # the last tile takes part


@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('name', list(CASES))
def test_forward_equals_the_referee(hip_device, name, mode):
    c = case(name)
    _exercises_its_point(name, c)
    pooled, argmax, idx, pts_voxel = run_forward(hip_device, c, mode)
    torch.cuda.synchronize()
    want_pooled, want_argmax = c[mode]
    assert np.array_equal(idx.cpu().numpy(), c['idx'])
    assert np.array_equal(pts_voxel.cpu().numpy(), c['kept'])
    assert np.array_equal(argmax.cpu().numpy(), want_argmax)
    assert np.array_equal(_bits(pooled.cpu().numpy()), _bits(want_pooled))


def test_forward_without_the_membership_table(hip_device):
    c = case('tile_plus_one')
    pooled, argmax, idx, _ = run_forward(hip_device, c, 'max', with_table=False)
    assert np.array_equal(idx.cpu().numpy(), c['idx'])
    assert np.array_equal(_bits(pooled.cpu().numpy()), _bits(c['max'][0]))


@pytest.mark.parametrize('empty', ['N', 'P', 'C'])
def test_an_empty_size_returns_zero_filled_outputs(hip_device, empty):
    from nesie_amd.kernels import HipKernels
    from nesie_amd.mmdet3d_ops import RoIAwarePool3d
    N, P, C = (0 if empty == s else v for s, v in (('N', 3), ('P', 40), ('C', 5)))
    c = dict(rois=random_rois(np.random.default_rng(0), N), out=(2, 2, 3), m=4,
             pts=np.random.default_rng(1).uniform(-1, 1, (P, 3)).astype(np.float32),
             feat=np.ones((P, C), np.float32))
    for mode in ('max', 'avg'):
        pooled, argmax, idx, pts_voxel = run_forward(hip_device, c, mode)
        assert tuple(pooled.shape) == (N, 2, 2, 3, C) and tuple(idx.shape) == (N, 2, 2, 3, 4)
        assert not pooled.any() and not argmax.any() and not idx.any()
        assert (pts_voxel == -1).all()
        grad_in = torch.full((P, C), float('nan'), device=hip_device)
        HipKernels().roiaware_pool3d_backward(idx, argmax, pts_voxel, torch.ones_like(pooled),
                                              grad_in, 0 if mode == 'max' else 1)
        assert not grad_in.any()
    out = RoIAwarePool3d((2, 2, 3), 4)(*(torch.from_numpy(c[k]).to(hip_device)
                                         for k in ('rois', 'pts', 'feat')))
    assert tuple(out.shape) == (N, 2, 2, 3, C) and not out.any()


def test_sizes_outside_the_kernels_range_are_refused(hip_device):
    from nesie_amd.mmdet3d_ops import RoIAwarePool3d
    rois, pts, feat = (torch.rand(2, 7, device=hip_device), torch.rand(9, 3, device=hip_device),
                       torch.rand(9, 2, device=hip_device))
    with pytest.raises(RuntimeError, match='outside 1 .. 256'):
        RoIAwarePool3d((2, 257, 2))(rois, pts, feat)
    with pytest.raises(RuntimeError, match='roiaware_pool3d'):
        RoIAwarePool3d(2, max_pts_per_voxel=0)(rois, pts, feat)


# ---- backward ------------------------------------------------------------------------------

def run_backward(dev, c, mode, fwd, grad_out):
    from nesie_amd.kernels import HipKernels
    pooled, argmax, idx, pts_voxel = fwd
    grad_in = torch.full((c['pts'].shape[0], c['feat'].shape[1]), float('nan'), device=dev)
    HipKernels().roiaware_pool3d_backward(idx, argmax, pts_voxel, grad_out, grad_in,
                                          0 if mode == 'max' else 1)
    return grad_in


def _float64_autograd(c, mode, idx, grad_out):
    """-> (grad_in, sum of |terms|, number of terms) (P,C) float64, by plain-torch autograd over a
    dense assignment built from the RETURNED pts_idx_of_voxels."""
    m = c['m']
    feat = torch.from_numpy(c['feat']).double()
    P, C = feat.shape
    slots = torch.from_numpy(idx.reshape(-1, m).astype(np.int64))
    count, members = slots[:, 0], slots[:, 1:]
    live = torch.arange(m - 1)[None, :] < count[:, None]                 # (NV, m-1)
    g = torch.from_numpy(grad_out.reshape(-1, C)).double()

    def pooled_of(x):
        rows = x[members]                                                # (NV, m-1, C)
        if mode == 'max':
            rows = torch.where(live[:, :, None], rows, torch.full_like(rows, -math.inf))
            best = rows.max(dim=1).values
            return torch.where(count[:, None] > 0, best, torch.zeros_like(best))
        rows = rows * live[:, :, None]
        return rows.sum(1) / count.clamp(min=1)[:, None]

    out = []
    for weight in (g, g.abs(), torch.ones_like(g)):
        x = feat.clone().requires_grad_(True)
        (gi,) = torch.autograd.grad((pooled_of(x) * weight).sum(), x)
        out.append(gi.numpy())
    if mode == 'avg':           # the count of terms, not the sum of their 1 / count weights
        out[2] = np.bincount(members[live].numpy(), minlength=P).astype(np.float64)[:, None] \
            * np.ones((1, C))
    return out


@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('name', ['overlapping', 'overflow'])
def test_backward_is_the_referees_ordered_sum(hip_device, name, mode):
    from nesie_amd.kernels import HipKernels
    c = case(name)
    fwd = run_forward(hip_device, c, mode)
    rng = np.random.default_rng(7)
    grad_out_np = rng.standard_normal(c[mode][0].shape).astype(np.float32)
    grad_out = torch.from_numpy(grad_out_np).to(hip_device)
    first = run_backward(hip_device, c, mode, fwd, grad_out)            # NaN-filled, overwritten
    second = run_backward(hip_device, c, mode, fwd, grad_out)
    prev = HipKernels.set_deterministic(False)
    try:
        relaxed = run_backward(hip_device, c, mode, fwd, grad_out)
    finally:
        HipKernels.set_deterministic(prev)
    assert torch.equal(first, second) and torch.equal(first, relaxed)
    got = first.cpu().numpy()
    want = R.backward(c['idx'].reshape(len(c['rois']), -1, c['m']),
                      c[mode][1].reshape(len(c['rois']), -1, got.shape[1]), grad_out_np,
                      got.shape[0], mode)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.count_nonzero(got) > 0 and np.isfinite(got).all()

    ref, mag, terms = _float64_autograd(c, mode, fwd[2].cpu().numpy(), grad_out_np)
    if name == 'overlapping':
        assert terms.max() >= 2                                         # sums of several terms
    err = np.abs(got.astype(np.float64) - ref)
    bound = (terms + 2) * 2.0 ** -24 * mag
    print(f'{name}/{mode}: max error {err.max():.3e}, bound at that element '
          f'{bound.flat[err.argmax()]:.3e}, up to {int(terms.max())} terms')
    assert np.all(err <= bound)


# ---- module --------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['max', 'avg'])
def test_module_forward_backward(hip_device, mode):
    from nesie_amd.mmdet3d_ops import RoIAwarePool3d
    c = case('overlapping')
    N, C = len(c['rois']), c['feat'].shape[1]
    rois, pts = (torch.from_numpy(c[k]).to(hip_device).requires_grad_(True) for k in ('rois', 'pts'))
    feat = torch.from_numpy(c['feat']).to(hip_device).requires_grad_(True)
    pool = RoIAwarePool3d(4, max_pts_per_voxel=c['m'], mode=mode)
    out = pool(rois, pts, feat)
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(c[mode][0]))
    # a non-contiguous grad_out
    g = torch.randn(C, N, 4, 4, 4, device=hip_device).permute(1, 2, 3, 4, 0)
    assert not g.is_contiguous()
    d_rois, d_pts, d_feat = torch.autograd.grad(out, [rois, pts, feat], g, allow_unused=True)
    assert d_rois is None and d_pts is None
    want = R.backward(c['idx'].reshape(N, -1, c['m']), c[mode][1].reshape(N, -1, C),
                      g.contiguous().cpu().numpy(), len(c['pts']), mode)
    assert np.array_equal(_bits(d_feat.cpu().numpy()), _bits(want))
    # int and tuple out_size agree
    other = RoIAwarePool3d((4, 4, 4), max_pts_per_voxel=c['m'], mode=mode)(rois, pts, feat)
    assert torch.equal(other, out)
    # .backward() accumulates into .grad as for any op
    pool(rois, pts, feat).backward(g)
    assert torch.equal(feat.grad, d_feat) and rois.grad is None and pts.grad is None


# ---- points_in_boxes_gpu -------------------------------------------------------------------

@pytest.mark.parametrize('B,M,T', [(2, 1000, 9), (1, 257, 300), (2, 50, 0)])
def test_points_in_boxes_gpu_is_the_first_hit_of_the_batch_table(hip_device, B, M, T):
    from nesie_amd.kernels import HipKernels
    from nesie_amd.mmdet3d_ops import points_in_boxes_batch, points_in_boxes_gpu
    rng = np.random.default_rng(B * 1000 + T)
    boxes = torch.from_numpy(np.stack([random_rois(rng, T, centre_span=1.5) for _ in range(B)])
                             ).to(hip_device)
    points = torch.from_numpy(rng.uniform(-2.5, 2.5, (B, M, 3)).astype(np.float32)).to(hip_device)
    got = points_in_boxes_gpu(points, boxes)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, M)
    table = points_in_boxes_batch(points, boxes).cpu().numpy()
    want = np.where(table.any(2), table.argmax(2), -1).astype(np.int32) if T else \
        np.full((B, M), -1, np.int32)
    assert np.array_equal(got.cpu().numpy(), want)
    if T:
        assert (want >= 0).sum() > M // 10 and (want < 0).any()
        assert (table.sum(2) >= 2).any()                     # "first" decides somewhere
    if T == 300:
        assert want.max() >= 256                             # a first hit past one LDS tile
    # written in full
    out = torch.full((B, M), GARBAGE_I, dtype=torch.int32, device=hip_device)
    HipKernels().points_in_boxes_gpu(boxes, points, out)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- capture -------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['max', 'avg'])
def test_forward_and_backward_replay_from_a_graph(hip_device, mode):
    """No allocation and no default-stream launch inside the entry points: forward + backward as
    one captured chain, replayed twice, gives the eager bits."""
    from nesie_amd.kernels import HipKernels
    c = case('overlapping')
    k = HipKernels()
    method = 0 if mode == 'max' else 1
    pooled, argmax, idx, pts_voxel = run_forward(hip_device, c, mode)
    grad_out = torch.randn_like(pooled)
    grad_in = run_backward(hip_device, c, mode, (pooled, argmax, idx, pts_voxel), grad_out)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (pooled, argmax, idx, pts_voxel, grad_in)]
    rois, pts, feat = (torch.from_numpy(c[n]).to(hip_device) for n in ('rois', 'pts', 'feat'))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k.roiaware_pool3d_forward(rois, pts, feat, argmax, idx, pooled, method, pts_voxel)
        k.roiaware_pool3d_backward(idx, argmax, pts_voxel, grad_out, grad_in, method)
    for _ in range(2):
        pooled.fill_(float('nan')); grad_in.fill_(float('nan'))
        argmax.fill_(GARBAGE_I); idx.fill_(GARBAGE_I); pts_voxel.fill_(GARBAGE_I)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((pooled, argmax, idx, pts_voxel, grad_in), eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
