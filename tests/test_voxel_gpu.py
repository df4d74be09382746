"""Voxel ops on the device: hard / dynamic voxelization and dynamic_scatter equal the numpy referee
(tests/_voxel_ref.py) BIT FOR BIT -- every integer output, every copied float, every reduced
float, every gradient -- and the goldens of the reference's CPU voxelizers; the modules through
autograd; run-to-run equality; graph capture; refusals before allocation.

Sizes: the sort works on tiles of 1024 keys (IX_SORT_TILE) and the scan on tiles of 1024 ints
(IX_SCAN_TILE; it scans N flags and 256 x ceil(N / 1024) digit counters), so N goes one below, at
and one above 1024, 3129 spans four tiles of the flag scan, 5000 puts the counter scan one tile
past its first (1280 counters) and 9000 gives it three (2304).  The grids need 1, 2, 3 and 4
eight-bit passes.

The scan's second level walks the tile totals 256 at a time with a carry: 262 144 flags are 256
totals (one trip, no carry), 262 145 are 257 (the carry's first use, for one element), 393 217 are
385 (a third of the elements behind the carry) and 1 048 577 points are 1025
flag tiles and 1025 sort tiles, whose 262 400 digit counters are 257 totals, so there the carry
runs inside every sort pass too.  At those sizes the referee is the vectorised form of
tests/_voxel_ref.py (tests/test_voxel_cpu.py proves it equal to the loops, bit for bit, on every
small input of this file) and the reduced features are small integers, whose fp32 sums are exact
in any order; the summation order itself is pinned by the small sizes on arbitrary floats.

Pass counts: the out-of-range key is `cells` itself, so at 2^8, 2^16 and 2^24 cells it is the only
key with a bit in the top pass; the grids and dims of the boundary tests sit one below and exactly
at those counts, and at 2^31 - 1, the largest accepted.  The key-order tests feed the sort what a
random draw never does: strictly descending keys, keys that differ only in the top byte, two
alternating cells.  The guard-band tests hand each op exactly the workspace bytes its query
returns, between two bands that must stay untouched."""
import os

import numpy as np
import pytest
import torch

from tests import _voxel_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'voxel.npz')
GARBAGE_I = -77
GRIDS = {   # name: (voxel_size, coors_range)                         grid            passes
    'tiny': ([1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0, 2.0, 1.0]),      # 2 x 2 x 1        1
    'p2': ([0.2, 0.2, 0.2], [0.0, 0.0, 0.0, 8.0, 8.0, 0.8]),        # 40 x 40 x 4      2
    'p3': ([0.0625, 0.0625, 0.0625], [-4.0, -4.0, 0.0, 4.0, 4.0, 1.0]),   # 128 x 128 x 16   3
    'lidar': ([0.05, 0.05, 0.1], [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]),    # 1408 x 1600 x 40 4
}
SIZES = (0, 1, 1023, 1024, 1025, 3129, 5000, 9000)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    """device tensor == numpy array, bit for bit, dtype and shape included"""
    got = got.detach().cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(bits(got), bits(want))


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def cloud(seed, n, c, grid, mode='mixed'):
    """(n, c) float32: half the points crowd a few cells (so cells overflow max_points), the rest
    are uniform over the range grown by a margin (so out-of-range points are interleaved)."""
    vs, cr = GRIDS[grid] if isinstance(grid, str) else grid
    rng = np.random.default_rng(seed)
    lo, hi = np.float64(cr[:3]), np.float64(cr[3:])
    pts = rng.standard_normal((n, c)).astype(np.float32)
    if mode == 'outside':
        xyz = hi + 1.0 + rng.uniform(0, 1, (n, 3))
    elif mode == 'one_cell':
        xyz = lo + (np.float64([1, 0, 0]) + rng.uniform(0.2, 0.8, (n, 3))) * np.float64(vs)
    else:
        margin = 0.1 * (hi - lo)
        xyz = lo - margin + rng.uniform(0, 1, (n, 3)) * (hi - lo + 2 * margin)
        hot = lo + rng.uniform(0, 1, (12, 3)) * (hi - lo)
        crowd = rng.random(n) < 0.5
        xyz[crowd] = hot[rng.integers(0, 12, int(crowd.sum()))] + \
            rng.uniform(-0.3, 0.3, (int(crowd.sum()), 3)) * np.float64(vs)
    pts[:, :3] = xyz.astype(np.float32)
    return pts


def run_hard(device, points, vs, cr, max_points, max_voxels, workspace=None):
    """The C entry through HipKernels with every output pre-filled with garbage."""
    from nesie_amd.kernels import HipKernels
    c = points.shape[1]
    p = dev(points, device)
    voxels = torch.full((max_voxels, max_points, c), float('nan'), device=device)
    coors = torch.full((max_voxels, 3), GARBAGE_I, dtype=torch.int32, device=device)
    num = torch.full((max_voxels,), GARBAGE_I, dtype=torch.int32, device=device)
    voxel_num = torch.full((1,), GARBAGE_I, dtype=torch.int32, device=device)
    HipKernels().hard_voxelize(p, vs, cr, voxels, coors, num, voxel_num, workspace)
    return voxels, coors, num, voxel_num


def check_voxelizers(device, points, vs, cr, max_points, max_voxels, want=None, fast=False):
    """``fast``: the vectorised referee, for sizes the serial walk cannot reach."""
    from nesie_amd.kernels import HipKernels
    from nesie_amd.mmdet3d_ops import voxelization
    if want is None:
        hard = R.hard_voxelize_fast if fast else R.hard_voxelize
        want = (R.dynamic_voxelize(points, vs, cr),
                *hard(points, vs, cr, max_points, max_voxels))
    w_dyn, w_vox, w_coors, w_num = want
    n = len(points)
    dyn = torch.full((n, 3), GARBAGE_I, dtype=torch.int32, device=device)
    HipKernels().dynamic_voxelize(dev(points, device), vs, cr, dyn)
    assert same(dyn, w_dyn)
    voxels, coors, num, voxel_num = run_hard(device, points, vs, cr, max_points, max_voxels)
    m = int(voxel_num.item())
    assert m == len(w_coors)
    assert same(coors[:m], w_coors) and same(num[:m], w_num) and same(voxels[:m], w_vox)
    # the rows at and above voxel_num are not touched
    assert (coors[m:] == GARBAGE_I).all() and (num[m:] == GARBAGE_I).all()
    assert torch.isnan(voxels[m:]).all()
    # the public function: the same rows, sliced
    got = voxelization(dev(points, device), vs, cr, max_points, max_voxels)
    assert same(got[0], w_vox) and same(got[1], w_coors) and same(got[2], w_num)
    assert same(voxelization(dev(points, device), vs, cr, -1, max_voxels), w_dyn)
    assert same(voxelization(dev(points, device), vs, cr, max_points, -1), w_dyn)
    return want


@pytest.mark.parametrize('n', SIZES)
def test_voxelizers_at_every_tile_boundary(hip_device, n):
    vs, cr = GRIDS['p2']
    points = cloud(n, n, 4, 'p2')
    _, _, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, 5, 200)
    if n >= 1023:
        assert len(w_coors) == 200 and (w_num == 5).any() and (w_num < 5).any()


@pytest.mark.parametrize('grid,c', [('tiny', 3), ('p2', 65), ('p3', 5), ('lidar', 4)])
def test_voxelizers_every_pass_count_and_channel_count(hip_device, grid, c):
    vs, cr = GRIDS[grid]
    points = cloud(17, 3000, c, grid)
    max_voxels = 8 if grid == 'tiny' else 2500        # tiny: more voxels allowed than cells exist
    _, _, w_coors, _ = check_voxelizers(hip_device, points, vs, cr, 5, max_voxels)
    assert 0 < len(w_coors) < max_voxels
    if grid == 'lidar':
        assert R.grid_size(vs, cr) == (1408, 1600, 40)


@pytest.mark.parametrize('max_points', [1, 5])
def test_all_points_in_one_cell(hip_device, max_points):
    vs, cr = GRIDS['p2']
    points = cloud(3, 1500, 4, 'p2', 'one_cell')
    _, w_vox, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, max_points, 40)
    assert w_coors.tolist() == [[0, 0, 1]] and w_num.tolist() == [max_points]
    assert np.array_equal(w_vox[0], points[:max_points])


def test_every_point_out_of_range(hip_device):
    vs, cr = GRIDS['p3']
    dyn, _, w_coors, _ = check_voxelizers(hip_device, cloud(4, 1300, 4, 'p3', 'outside'), vs, cr,
                                          5, 40)
    assert len(w_coors) == 0 and (dyn == -1).all()


def test_max_voxels_reached_mid_stream(hip_device):
    """Cells A B C with max_voxels 2: C is first seen after the cap and is dropped with all its
    points; later points of A and B are still kept."""
    vs, cr = GRIDS['p2']
    a, b, c = [0.1, 0.1, 0.1], [0.5, 0.1, 0.1], [0.1, 0.5, 0.1]
    xyz = np.float32([a, b, a, c, b, c, a, [9.0, 0.1, 0.1], b, a])
    points = np.concatenate([xyz, np.arange(10, dtype=np.float32)[:, None]], axis=1)
    _, w_vox, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, 3, 2)
    assert w_coors.tolist() == [[0, 0, 0], [0, 0, 2]] and w_num.tolist() == [3, 3]
    assert w_vox[0, :, 3].tolist() == [0, 2, 6] and w_vox[1, :, 3].tolist() == [1, 4, 8]
    # with room for it, C is the third voxel
    _, _, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, 3, 3)
    assert w_coors.tolist() == [[0, 0, 0], [0, 0, 2], [0, 2, 0]] and w_num.tolist() == [3, 3, 2]


def test_goldens_of_the_reference_cpu_programs(hip_device):
    """lo (inside), hi (outside), -0.0, NaN, inf, cell planes ... against the reference's own
    CPU output."""
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    for name in golden['names'].tolist():
        g = {k.split('/', 1)[1]: v for k, v in golden.items() if k.startswith(name + '/')}
        check_voxelizers(hip_device, g['points'], g['voxel_size'].tolist(),
                         g['coors_range'].tolist(), int(g['max_points']), int(g['max_voxels']),
                         (g['dynamic_coors'], g['voxels'], g['coors'], g['num_points_per_voxel']))


# 256, 257, 385 and 1025 tile totals of the flag scan.  At 262 145 a single element lies past the
# first 256 totals, and the cap (or an invalid key sorted last) can hide what the carry gives it;
# 393 217 puts a third of the elements there while the sort's counters still scan in one trip.
CARRY_SIZES = (262144, 262145, 393217, 1048577)


def occupied_cells(points, vs, cr):
    dyn = R.dynamic_voxelize(points, vs, cr)
    gx, gy, _ = R.grid_size(vs, cr)
    inside = dyn[dyn[:, 0] != -1].astype(np.int64)
    return len(np.unique((inside[:, 0] * gy + inside[:, 1]) * gx + inside[:, 2]))


@pytest.mark.parametrize('n', CARRY_SIZES)
def test_voxelizers_where_the_scan_carries(hip_device, n):
    """Four passes; half the points in 12 hot cells, out-of-range points interleaved; the cap on
    the voxel count (`*capped` of the scan) is reached mid-stream."""
    vs, cr = GRIDS['lidar']
    points = cloud(n, n, 4, 'lidar')
    max_voxels = 20000
    assert occupied_cells(points, vs, cr) > max_voxels
    dyn, _, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, 5, max_voxels, fast=True)
    assert len(w_coors) == max_voxels and (w_num == 5).any() and (w_num < 5).any()
    assert (dyn == -1).any()


def test_one_cell_across_257_tiles_keeps_the_lowest_indices_in_order(hip_device):
    """Every point in one cell: the voxel holds points 0 .. 4 in index order only if every pass
    kept the input order across all 257 tiles."""
    vs, cr = GRIDS['lidar']
    points = cloud(5, 262145, 4, 'lidar', 'one_cell')
    _, w_vox, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, 5, 40, fast=True)
    assert w_coors.tolist() == [[0, 0, 1]] and w_num.tolist() == [5]
    assert np.array_equal(w_vox[0], points[:5])


# name: (coors_range of a grid of voxel size 1.0)                       cells        passes
BOUNDARY_GRIDS = {
    '255': [0.0, 0.0, 0.0, 15.0, 17.0, 1.0],                          # 2^8 - 1      1
    '256': [0.0, 0.0, 0.0, 16.0, 16.0, 1.0],                          # 2^8          2
    '65535': [0.0, 0.0, 0.0, 255.0, 257.0, 1.0],                      # 2^16 - 1     2
    '65536': [0.0, 0.0, 0.0, 256.0, 256.0, 1.0],                      # 2^16         3
    '16777215': [0.0, 0.0, 0.0, 4095.0, 4097.0, 1.0],                 # 2^24 - 1     3
    '16777216': [0.0, 0.0, 0.0, 256.0, 256.0, 256.0],                 # 2^24         4
}


@pytest.mark.parametrize('cells', list(BOUNDARY_GRIDS))
def test_voxelizers_at_every_pass_boundary(hip_device, cells):
    """Grids of one cell below and exactly 2^8, 2^16, 2^24 cells: at the power of two the
    out-of-range key is the only one the top pass moves.  Points in the first and the last cell,
    some outside."""
    vs, cr = [1.0, 1.0, 1.0], BOUNDARY_GRIDS[cells]
    gx, gy, gz = R.grid_size(vs, cr)
    assert gx * gy * gz == int(cells)
    points = cloud(int(cells) % 1000, 3129, 4, (vs, cr))
    points[[0, 7, 1500], :3] = [0.5, 0.5, 0.5]
    points[[1, 9, 3128], :3] = [gx - 0.5, gy - 0.5, gz - 0.5]
    dyn, _, w_coors, _ = check_voxelizers(hip_device, points, vs, cr, 5, 2500)
    assert dyn[0].tolist() == [0, 0, 0] and dyn[1].tolist() == [gz - 1, gy - 1, gx - 1]
    assert w_coors[0].tolist() == [0, 0, 0] and w_coors[1].tolist() == [gz - 1, gy - 1, gx - 1]
    assert (dyn == -1).any() and 12 < len(w_coors) < 2500


# ---- key orders a random draw never produces -------------------------------------------------

ORDER_DIMS = (40, 1600, 1408)               # the lidar grid as (z, y, x): 90 112 000 cells, 4 passes


def ordered_keys(order, n=5000):
    cells = int(np.prod(ORDER_DIMS))
    if order == 'descending':               # strictly: every key its own cell
        keys = cells - 1 - np.arange(n, dtype=np.int64) * (cells // n)
    elif order == 'top_byte':               # the three low passes see one digit each
        keys = (np.random.default_rng(6).integers(0, (cells >> 24) + 1, n) << 24) + 1234567
    else:                                   # 'alternating': the first and the last cell
        keys = np.where(np.arange(n) % 2 == 0, 0, cells - 1).astype(np.int64)
    assert keys.min() >= 0 and keys.max() < cells
    return keys


def keys_to_coors(keys):
    _, dy, dx = ORDER_DIMS
    return np.stack([keys // (dy * dx), keys // dx % dy, keys % dx], axis=1).astype(np.int32)


@pytest.mark.parametrize('order', ['descending', 'top_byte', 'alternating'])
def test_voxelizers_on_ordered_keys(hip_device, order):
    vs, cr = GRIDS['lidar']
    coors = keys_to_coors(ordered_keys(order))
    points = np.random.default_rng(7).standard_normal((len(coors), 4)).astype(np.float32)
    centre = np.float64(cr[:3]) + (coors[:, ::-1] + 0.5) * np.float64(vs)
    points[:, :3] = centre.astype(np.float32)
    max_voxels = 3000 if order == 'descending' else 40
    dyn, w_vox, w_coors, w_num = check_voxelizers(hip_device, points, vs, cr, 5, max_voxels)
    assert np.array_equal(dyn, coors)                       # the points sit in the cells meant
    if order == 'descending':     # first appearance = input order: the first 3000 points, one each
        assert np.array_equal(w_coors, coors[:3000]) and (w_num == 1).all()
        assert np.array_equal(w_vox[:, 0], points[:3000])
    elif order == 'top_byte':
        assert len(w_coors) == 6 and (w_num == 5).all()
    else:
        assert w_coors.tolist() == [[0, 0, 0], [39, 1599, 1407]]
        assert np.array_equal(w_vox[0], points[0:10:2]) and np.array_equal(w_vox[1], points[1:10:2])


# ---- dynamic_scatter -----------------------------------------------------------------------

def scatter_case(seed, n, c, dims, invalid=0.15, ties=False, nans=False):
    rng = np.random.default_rng(seed)
    # a few hundred distinct rows at most, so voxels hold several points whatever the grid
    pool = np.stack([rng.integers(0, d, 300) for d in dims], axis=1)
    coors = pool[rng.integers(0, 300, n)].astype(np.int32)
    if invalid and n:
        bad = rng.random(n) < invalid
        coors[bad, rng.integers(0, 3, int(bad.sum()))] = -1
        over = rng.random(n) < invalid / 3
        coors[over, 2] = dims[2]                            # at the bound: invalid
    if ties:
        feats = rng.integers(-2, 3, (n, c)).astype(np.float32)
        feats[feats == 0] = -0.0
    else:
        feats = rng.standard_normal((n, c)).astype(np.float32)
    if nans and n:
        feats[rng.random((n, c)) < 0.05] = np.nan
        feats[coors[:, 0] == 0] = np.nan                    # whole voxels of NaN
    return feats, coors


def run_scatter(device, feats, coors, dims, reduce_type, workspace=None, grad_voxel=None):
    """The C entries through HipKernels, outputs pre-filled with garbage -> numpy, sliced to M."""
    from nesie_amd.kernels import HipKernels
    k = HipKernels()
    mode = {'sum': 0, 'mean': 1, 'max': 2}[reduce_type]
    n, c = feats.shape
    f, co = dev(feats, device), dev(coors, device)
    vf = torch.full((n, c), float('nan'), device=device)
    ints = [torch.full(s, GARBAGE_I, dtype=torch.int32, device=device)
            for s in ((n, 3), (n,), (n,), (1,), (n,), (n,))]
    vc, cmap, cnt, num, order, start = ints
    k.dynamic_scatter_forward(f, co, dims, mode, vf, vc, cmap, cnt, num, order, start, workspace)
    m = int(num.item())
    out = dict(m=m, voxel_feats=vf[:m], voxel_coors=vc[:m], coors_map=cmap, reduce_count=cnt[:m])
    assert torch.isnan(vf[m:]).all() and (vc[m:] == GARBAGE_I).all()
    if grad_voxel is not None and n and c:
        grad = torch.full((n, c), float('nan'), device=device)
        gv = dev(grad_voxel[:m], device) if m else torch.zeros((1, c), device=device)
        k.dynamic_scatter_backward(gv, f, vf, cmap, cnt, order, start, num, mode, grad)
        out['grad_feats'] = grad
    return out


def check_scatter(device, feats, coors, dims, reduce_type, fast=False):
    """``fast``: the vectorised referee, for sizes the loops cannot reach."""
    forward = R.scatter_forward_fast if fast else R.scatter_forward
    backward = R.scatter_backward_fast if fast else R.scatter_backward
    n, c = feats.shape
    w_out, w_vc, w_map, w_cnt = forward(feats, coors, reduce_type, dims)
    grad_voxel = np.random.default_rng(n + c).standard_normal((max(n, 1), c)).astype(np.float32)
    got = run_scatter(device, feats, coors, dims, reduce_type, grad_voxel=grad_voxel)
    assert got['m'] == len(w_vc)
    assert same(got['voxel_coors'], w_vc) and same(got['coors_map'], w_map)
    assert same(got['reduce_count'], w_cnt) and same(got['voxel_feats'], w_out)
    if 'grad_feats' in got:
        w_grad = backward(grad_voxel[:len(w_vc)], feats, w_out, w_map, w_cnt, reduce_type)
        assert same(got['grad_feats'], w_grad)
    return w_out, w_vc, w_map, w_cnt


@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
@pytest.mark.parametrize('n', SIZES)
def test_scatter_at_every_tile_boundary(hip_device, n, reduce_type):
    dims = (6, 7, 5)
    feats, coors = scatter_case(n, n, 4, dims)
    check_scatter(hip_device, feats, coors, dims, reduce_type)


@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
@pytest.mark.parametrize('dims,c', [((1, 2, 2), 3), ((4, 40, 40), 65), ((16, 128, 128), 5),
                                    ((40, 1600, 1408), 4), ((3, 3, 3), 260)])
def test_scatter_every_pass_count_and_channel_count(hip_device, dims, c, reduce_type):
    feats, coors = scatter_case(23, 700 if c == 260 else 3129, c, dims)
    check_scatter(hip_device, feats, coors, dims, reduce_type)


@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
def test_scatter_without_an_invalid_row_keeps_the_smallest_voxel(hip_device, reduce_type):
    dims = (6, 7, 5)
    feats, coors = scatter_case(31, 2000, 4, dims, invalid=0)
    _, w_vc, w_map, _ = check_scatter(hip_device, feats, coors, dims, reduce_type)
    assert (w_map >= 0).all() and (w_map == 0).any()
    assert tuple(w_vc[0]) == min(map(tuple, coors.tolist()))


@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
def test_scatter_with_only_invalid_rows(hip_device, reduce_type):
    feats, _ = scatter_case(32, 1500, 4, (6, 7, 5))
    coors = np.full((1500, 3), -1, dtype=np.int32)
    coors[::3] = [0, 7, 0]                                  # at the bound
    w_out, _, w_map, _ = check_scatter(hip_device, feats, coors, (6, 7, 5), reduce_type)
    assert len(w_out) == 0 and (w_map == -1).all()


def test_scatter_max_ties_nans_and_signed_zeros(hip_device):
    """Duplicate maxima: the lowest index takes the gradient.  NaN never wins; a voxel of NaNs
    keeps -inf and passes no gradient."""
    dims = (6, 7, 5)
    feats, coors = scatter_case(33, 3129, 5, dims, ties=True, nans=True)
    w_out, _, w_map, _ = check_scatter(hip_device, feats, coors, dims, 'max')
    assert np.isneginf(w_out).any() and not np.isnan(w_out).any()
    feats, coors = scatter_case(34, 3129, 5, dims, ties=True)
    for reduce_type in ('max', 'sum', 'mean'):
        check_scatter(hip_device, feats, coors, dims, reduce_type)


@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
def test_scatter_voxels_of_several_hundred_points(hip_device, reduce_type):
    rng = np.random.default_rng(35)
    n = 1400
    coors = np.zeros((n, 3), dtype=np.int32)
    coors[:, 2] = rng.integers(0, 3, n)                     # ~ 470 points a voxel
    coors[rng.random(n) < 0.1] = -1
    feats = rng.standard_normal((n, 6)).astype(np.float32)
    _, _, _, w_cnt = check_scatter(hip_device, feats, coors, (1, 1, 3), reduce_type)
    assert w_cnt.min() > 300


SCATTER_BOX = (4, 64, 64)


def box_scatter_case(seed, n, c, dims, span=4, box=SCATTER_BOX, invalid=0.1):
    """Coordinates from two sub-boxes of ``dims``, one in each extreme corner (so voxels hold
    several points and the keys span every byte); about ``invalid`` of the rows are invalid, a
    negative entry or one at its bound.  Features are integers in [-span, span]: every fp32 sum
    is exact whatever its order (below 2^24), and with span 1 most voxels hold their maximum more
    than once."""
    rng = np.random.default_rng(seed)
    coors = np.stack([rng.integers(0, b, n) for b in box], axis=1).astype(np.int32)
    far = rng.random(n) < 0.5
    coors[far] += np.int32(dims) - np.int32(box)
    bad = np.flatnonzero(rng.random(n) < invalid)
    col = rng.integers(0, 3, len(bad))
    coors[bad, col] = np.where(rng.random(len(bad)) < 0.7, -1, np.int32(dims)[col])
    feats = rng.integers(-span, span + 1, (n, c)).astype(np.float32)
    return feats, coors


@pytest.mark.parametrize('n,reduce_type', [(262145, 'sum'), (262145, 'mean'), (262145, 'max'),
                                           (393217, 'max'), (1048577, 'mean'), (1048577, 'max')])
def test_scatter_where_the_scan_carries(hip_device, n, reduce_type):
    """257 tile totals of the flag scan at 262 145 rows; at 1 048 577 the digit counters of every
    one of the four sort passes carry too.  max: ties in most voxels, the gradient to the lowest
    index -- where a sort that lost its stability in a later tile would show."""
    dims = (40, 1600, 1408)
    feats, coors = box_scatter_case(n % 1000, n, 4, dims, span=1 if reduce_type == 'max' else 4)
    w_out, w_vc, w_map, w_cnt = check_scatter(hip_device, feats, coors, dims, reduce_type, fast=True)
    assert 0.05 < (w_map == -1).mean() < 0.15 and w_cnt.min() >= 1 and np.median(w_cnt) >= 3
    assert w_vc[0, 0] < SCATTER_BOX[0] and w_vc[-1, 0] >= dims[0] - SCATTER_BOX[0]
    if reduce_type == 'max':
        valid = w_map >= 0
        top = (feats[valid] == w_out[w_map[valid]])[:, 0]
        tied = np.bincount(w_map[valid][top], minlength=len(w_cnt)) > 1
        assert tied.mean() > 0.5                            # most voxels hold their maximum twice


BOUNDARY_DIMS = [(1, 15, 17), (1, 16, 16), (1, 255, 257), (1, 256, 256), (1, 4095, 4097),
                 (256, 256, 256), (1, 1, 2147483647)]


@pytest.mark.parametrize('dims', BOUNDARY_DIMS)
def test_scatter_at_every_pass_boundary(hip_device, dims):
    """dims whose product is one below and exactly 2^8, 2^16, 2^24, and 2^31 - 1, the largest
    accepted: rows at cell 0 and at the last valid cell, about a tenth invalid."""
    assert int(np.prod(np.int64(dims))) in (255, 256, 65535, 65536, 16777215, 16777216, 2 ** 31 - 1)
    feats, coors = scatter_case(sum(dims) % 1000, 3129, 4, dims, invalid=0.075)
    coors[[0, 5, 2000]] = [0, 0, 0]
    coors[[1, 7, 3128]] = [d - 1 for d in dims]
    for reduce_type in ('sum', 'mean', 'max'):
        _, w_vc, w_map, _ = check_scatter(hip_device, feats, coors, dims, reduce_type)
        assert w_vc[0].tolist() == [0, 0, 0] and w_vc[-1].tolist() == [d - 1 for d in dims]
        assert 0.05 < (w_map == -1).mean() < 0.15


@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
@pytest.mark.parametrize('order', ['descending', 'top_byte', 'alternating'])
def test_scatter_on_ordered_keys(hip_device, order, reduce_type):
    coors = keys_to_coors(ordered_keys(order))
    feats, _ = scatter_case(36, len(coors), 4, ORDER_DIMS, ties=order != 'descending')
    _, w_vc, w_map, w_cnt = check_scatter(hip_device, feats, coors, ORDER_DIMS, reduce_type)
    if order == 'descending':     # voxel rows ascend: the map is the input order reversed
        assert np.array_equal(w_map, np.arange(len(coors) - 1, -1, -1)) and (w_cnt == 1).all()
    elif order == 'top_byte':
        assert len(w_vc) == 6
    else:
        assert w_map[:4].tolist() == [0, 1, 0, 1] and w_cnt.tolist() == [2500, 2500]


# ---- workspace guard bands -----------------------------------------------------------------

GUARD = 4096


class Guarded:
    """``need`` bytes of workspace between two bands of GUARD bytes, everything filled with 0xA5."""

    def __init__(self, need, device):
        self.need = need
        self.whole = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        self.workspace = self.whole[GUARD:GUARD + need]

    def bands_untouched(self):
        return bool((self.whole[:GUARD] == 0xA5).all()) and \
            bool((self.whole[GUARD + self.need:] == 0xA5).all())


def bits_equal(a, b):
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize('n', [1, 1025, 5000, 262145])
def test_hard_voxelize_stays_inside_the_workspace_it_asks_for(hip_device, n):
    from nesie_amd.kernels import HipKernels
    vs, cr = GRIDS['lidar']
    points = cloud(80 + n % 100, n, 4, 'lidar')
    _, cells = HipKernels.voxel_grid_size(vs, cr)
    guarded = Guarded(HipKernels.voxel_workspace_bytes(n, cells), hip_device)
    assert guarded.need > 0
    own = run_hard(hip_device, points, vs, cr, 5, 300)
    got = run_hard(hip_device, points, vs, cr, 5, 300, guarded.workspace)
    assert guarded.bands_untouched()
    for a, b in zip(got, own):
        assert bits_equal(a, b)


@pytest.mark.parametrize('n', [1, 1025, 5000, 262145])
def test_scatter_forward_stays_inside_the_workspace_it_asks_for(hip_device, n):
    from nesie_amd.kernels import HipKernels
    dims = (40, 1600, 1408)
    feats, coors = box_scatter_case(90 + n % 100, n, 4, dims)
    guarded = Guarded(HipKernels.voxel_workspace_bytes(n, int(np.prod(dims))), hip_device)
    assert guarded.need > 0
    own = run_scatter(hip_device, feats, coors, dims, 'mean')
    got = run_scatter(hip_device, feats, coors, dims, 'mean', guarded.workspace)
    assert guarded.bands_untouched()
    assert got['m'] == own['m'] and set(got) == set(own)
    for name in ('voxel_feats', 'voxel_coors', 'coors_map', 'reduce_count'):
        assert bits_equal(got[name], own[name])


# ---- the modules through autograd ----------------------------------------------------------

@pytest.mark.parametrize('reduce_type', ['sum', 'mean', 'max'])
def test_functional_forward_and_backward_through_autograd(hip_device, reduce_type):
    from nesie_amd.mmdet3d_ops import dynamic_scatter
    feats, coors = scatter_case(41, 3129, 7, (6, 7, 5), ties=reduce_type == 'max')
    coors[coors[:, 2] == 5, 2] = -1       # the functional's bounds come from the data itself
    w_out, w_vc, w_map, w_cnt = R.scatter_forward(feats, coors, reduce_type)
    runs = []
    for _ in range(2):
        f = dev(feats, hip_device).requires_grad_(True)
        out, vc = dynamic_scatter(f, dev(coors, hip_device), reduce_type)
        assert not vc.requires_grad and out.requires_grad
        grad_voxel = np.random.default_rng(5).standard_normal(w_out.shape).astype(np.float32)
        out.backward(dev(grad_voxel, hip_device))
        assert same(out, w_out) and same(vc, w_vc)
        assert same(f.grad, R.scatter_backward(grad_voxel, feats, w_out, w_map, w_cnt,
                                               reduce_type))
        runs.append((out.detach().clone(), f.grad.clone()))
    # two runs: bitwise equal outputs and gradients
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))


@pytest.mark.parametrize('average', [True, False])
def test_module_single_and_batched(hip_device, average):
    from nesie_amd.mmdet3d_ops import DynamicScatter, Voxelization
    vs, cr = GRIDS['p2']
    reduce_type = 'mean' if average else 'max'
    gx, gy, gz = R.grid_size(vs, cr)
    scatter = DynamicScatter(vs, cr, average)
    dynamic = Voxelization(vs, cr, -1, (-1, -1))
    clouds = [cloud(50 + b, 1500 + 100 * b, 6, 'p2') for b in range(3)]
    feats, coors4, want_f, want_c, want_g, grads = [], [], [], [], [], []
    for b, pts in enumerate(clouds):
        co = dynamic(dev(pts, hip_device))
        assert same(co, R.dynamic_voxelize(pts, vs, cr))
        co = co.cpu().numpy()
        feats.append(pts)
        coors4.append(np.concatenate([np.full((len(pts), 1), b, np.int32), co], axis=1))
        out, vc, cmap, cnt = R.scatter_forward(pts, co, reduce_type, (gz, gy, gx))
        gv = np.random.default_rng(b).standard_normal(out.shape).astype(np.float32)
        want_f.append(out)
        want_c.append(np.concatenate([np.full((len(vc), 1), b, np.int32), vc], axis=1))
        want_g.append(R.scatter_backward(gv, pts, out, cmap, cnt, reduce_type))
        grads.append(gv)
    # one scene, three columns
    f = dev(feats[0], hip_device).requires_grad_(True)
    out, vc = scatter(f, dev(coors4[0][:, 1:], hip_device))
    out.backward(dev(grads[0], hip_device))
    assert same(out, want_f[0]) and same(vc, want_c[0][:, 1:]) and same(f.grad, want_g[0])
    # the batch, four columns
    f = dev(np.concatenate(feats), hip_device).requires_grad_(True)
    out, vc = scatter(f, dev(np.concatenate(coors4), hip_device))
    out.backward(dev(np.concatenate(grads), hip_device))
    assert same(out, np.concatenate(want_f)) and same(vc, np.concatenate(want_c))
    assert same(f.grad, np.concatenate(want_g))


def test_hard_voxelization_module_and_two_runs(hip_device):
    from nesie_amd.mmdet3d_ops import Voxelization
    vs, cr = GRIDS['p3']
    points = cloud(61, 5000, 4, 'p3')
    module = Voxelization(vs, cr, 4, (150, 400))
    want_train = R.hard_voxelize(points, vs, cr, 4, 150)
    want_test = R.hard_voxelize(points, vs, cr, 4, 400)
    p = dev(points, hip_device)
    first = module(p)
    again = module(p)
    for got, other, want in zip(first, again, want_train):
        assert same(got, want) and torch.equal(got, other)
    module.eval()
    for got, want in zip(module(p), want_test):
        assert same(got, want)
    assert len(want_train[1]) == 150 and 150 < len(want_test[1]) <= 400


# ---- capture and refusals ------------------------------------------------------------------

@pytest.mark.parametrize('reduce_type', ['mean', 'max'])
def test_forward_and_backward_replay_from_a_graph(hip_device, reduce_type):
    """No allocation, no synchronisation and no default-stream launch inside the entries: hard
    voxelization and scatter forward + backward as one captured chain that shares ONE workspace,
    replayed twice over garbage, give the eager bits."""
    from nesie_amd.kernels import HipKernels
    k = HipKernels()
    mode = {'mean': 1, 'max': 2}[reduce_type]
    vs, cr = GRIDS['p3']
    dims = (16, 128, 128)
    points = cloud(71, 3129, 4, 'p3')
    feats, coors = scatter_case(72, 3129, 6, dims)
    n, c = feats.shape
    _, cells = k.voxel_grid_size(vs, cr)
    assert cells == 16 * 128 * 128
    ws = torch.empty(k.voxel_workspace_bytes(n, cells), dtype=torch.uint8, device=hip_device)
    p, f, co = dev(points, hip_device), dev(feats, hip_device), dev(coors, hip_device)
    voxels = torch.empty((200, 4, 4), device=hip_device)
    vf, grad, gv = (torch.empty((n, c), device=hip_device) for _ in range(3))
    gv.normal_()
    v_coors, vc = (torch.empty(s, dtype=torch.int32, device=hip_device) for s in ((200, 3), (n, 3)))
    v_num = torch.empty((200,), dtype=torch.int32, device=hip_device)
    cmap, cnt, order, start = (torch.empty((n,), dtype=torch.int32, device=hip_device)
                               for _ in range(4))
    voxel_num, num = (torch.empty((1,), dtype=torch.int32, device=hip_device) for _ in range(2))
    outputs = (voxels, v_coors, v_num, voxel_num, vf, vc, cmap, cnt, num, grad)

    def chain():
        k.hard_voxelize(p, vs, cr, voxels, v_coors, v_num, voxel_num, ws)
        k.dynamic_scatter_forward(f, co, dims, mode, vf, vc, cmap, cnt, num, order, start, ws)
        k.dynamic_scatter_backward(gv, f, vf, cmap, cnt, order, start, num, mode, grad)

    def clear():
        for t in outputs + (order, start):
            t.fill_(float('nan') if t.dtype == torch.float32 else GARBAGE_I)
        ws.fill_(0xAB)

    clear()
    chain()
    torch.cuda.synchronize()
    eager = [t.clone() for t in outputs]
    w_vox, w_coors, w_num = R.hard_voxelize(points, vs, cr, 4, 200)
    assert int(voxel_num.item()) == len(w_coors) == 200 and same(voxels, w_vox)
    w_out = R.scatter_forward(feats, coors, reduce_type, dims)[0]
    assert same(vf[:int(num.item())], w_out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for _ in range(2):
        clear()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outputs, eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_sizes_outside_the_supported_range_are_refused_before_allocation(hip_device):
    """Each call would need far more memory than the device has if anything were allocated
    first: the refusal must be the size error, not an out-of-memory error."""
    from nesie_amd.mmdet3d_ops import Voxelization, dynamic_scatter, voxelization
    p = torch.rand((64, 4), device=hip_device)
    coors = torch.zeros((64, 3), dtype=torch.int32, device=hip_device)
    before = torch.cuda.memory_allocated(hip_device)
    huge = [0.0, 0.0, 0.0, 2048.0, 2048.0, 512.0]            # 2048 * 2048 * 512 = 2^31 cells
    with pytest.raises(RuntimeError, match='status 2'):
        voxelization(p, [1.0, 1.0, 1.0], huge, 1000, 10 ** 9)
    with pytest.raises(RuntimeError, match='status 2'):
        voxelization(p, [1.0, 1.0, 1.0], huge, -1, -1)
    with pytest.raises(RuntimeError, match='status 2'):
        Voxelization([1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 4.0, 4.0, 0.25], 1000, 10 ** 9)(p)
    with pytest.raises(RuntimeError, match='status 2'):
        dynamic_scatter(p, coors, 'max', (2048, 2048, 512))
    assert torch.cuda.memory_allocated(hip_device) == before
    with pytest.raises(TypeError):
        dynamic_scatter(p.double(), coors, 'max')
    with pytest.raises(TypeError):
        dynamic_scatter(p, coors.long(), 'max')
    with pytest.raises(TypeError):
        dynamic_scatter(p, torch.zeros((64, 4), dtype=torch.int32, device=hip_device), 'max')
    with pytest.raises(TypeError):
        voxelization(p.half(), [1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 4.0, 4.0, 2.0], 5, 20)
    with pytest.raises(ValueError):
        dynamic_scatter(p, coors, 'min')
