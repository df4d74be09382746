"""Voxel ops, the tier that needs no GPU: the numpy referee (tests/_voxel_ref.py) against the
goldens of the reference's CPU voxelizers bit for bit, the scatter referee against torch float64,
the package surface, the refusals, the constructors and the C entries' argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from nesie_amd import _lib
from tests import _voxel_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'voxel.npz')
NAMES = ('Voxelization', 'voxelization', 'dynamic_scatter', 'DynamicScatter')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_covers_the_cases(golden):
    names = set(golden['names'].tolist())
    assert {'room_cap_midstream', 'room_more_voxels_than_cells', 'lidar_sparse', 'tiny_grid',
            'one_cell_max1', 'one_cell_max5', 'all_out_of_range', 'edges_and_specials'} <= names
    # the cap really is reached mid-stream, and really is not where it should not be
    assert len(golden['room_cap_midstream/coors']) == 200
    assert len(golden['room_more_voxels_than_cells/coors']) < 32 * 32 * 12
    assert len(golden['all_out_of_range/coors']) == 0
    assert (golden['all_out_of_range/dynamic_coors'] == -1).all()
    assert golden['one_cell_max5/num_points_per_voxel'].tolist() == [5]
    edge = golden['edges_and_specials/dynamic_coors']
    assert edge[0].tolist() == [0, 0, 0] and edge[5].tolist() == [0, 16, 16]
    # (row 3, one ulp below hi: the fp32 subtraction rounds 7.9999998 up to 8, so it is outside)
    assert (edge[[1, 2, 3, 4, 6, 7, 8, 9, 10]] == -1).all() and edge[11].tolist() == [3, 18, 17]


def test_referee_equals_the_reference_cpu_programs_bit_for_bit(golden):
    for name in golden['names'].tolist():
        g = {k.split('/', 1)[1]: v for k, v in golden.items() if k.startswith(name + '/')}
        vs, cr = g['voxel_size'].tolist(), g['coors_range'].tolist()
        dyn = R.dynamic_voxelize(g['points'], vs, cr)
        assert dyn.dtype == np.int32 and np.array_equal(dyn, g['dynamic_coors']), name
        voxels, coors, num = R.hard_voxelize(g['points'], vs, cr, int(g['max_points']),
                                             int(g['max_voxels']))
        assert np.array_equal(coors, g['coors']), name
        assert np.array_equal(num, g['num_points_per_voxel']), name
        assert voxels.shape == g['voxels'].shape, name
        assert np.array_equal(voxels.view(np.uint32), g['voxels'].view(np.uint32)), name


def test_referee_grid_rounds_halves_away_from_zero():
    assert R.grid_size([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]) == (1408, 1600, 40)
    assert R.grid_size([2.0, 2.0, 2.0], [0, 0, 0, 5, 7, 1]) == (3, 4, 1)      # 2.5, 3.5, 0.5
    lib = _lib.load()
    for vs, cr in (([2.0, 2.0, 2.0], [0, 0, 0, 5, 7, 1]), ([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]),
                   ([0.3, 0.7, 0.11], [-3.3, -1, 0.2, 9.15, 8.45, 2.95])):
        grid, cells = (ctypes.c_int * 3)(), ctypes.c_longlong()
        assert lib.nesie_voxel_grid_size((ctypes.c_float * 3)(*vs), (ctypes.c_float * 6)(*cr),
                                         grid, ctypes.byref(cells)) == 0
        assert tuple(grid) == R.grid_size(vs, cr)
        assert cells.value == grid[0] * grid[1] * grid[2]


def _scatter_case(seed, n, c, dims, invalid):
    rng = np.random.default_rng(seed)
    coors = np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.int32)
    if invalid:
        coors[rng.random(n) < 0.2, rng.integers(0, 3)] = -1
        coors[rng.integers(0, n)] = [-1, -1, -1]
    feats = rng.standard_normal((n, c)).astype(np.float32)
    return feats, coors


@pytest.mark.parametrize('invalid', [True, False])
def test_scatter_referee_against_torch_float64(invalid):
    """Voxel order and map: torch.unique(dim=0).  max: exact.  sum / mean: a voxel of t points is
    within (t + 2) * 2^-24 * sum|terms| of the float64 sum (the bound of DESIGN section 7g; the
    mean's bound is that divided by t).  Prints the worst ratio of error to bound."""
    feats, coors = _scatter_case(5, 4000, 7, (3, 5, 4), invalid)
    tc = torch.from_numpy(coors).long()
    valid = (tc >= 0).all(1)
    uniq, inverse, counts = torch.unique(tc[valid], dim=0, return_inverse=True, return_counts=True)
    m = len(uniq)
    assert not invalid or not valid.all()
    f64 = torch.from_numpy(feats).double()[valid]
    expect_map = torch.full((len(tc),), -1, dtype=torch.long)
    expect_map[valid] = inverse
    for reduce_type in ('max', 'sum', 'mean'):
        out, vc, cmap, cnt = R.scatter_forward(feats, coors, reduce_type)
        assert np.array_equal(vc, uniq.numpy()) and np.array_equal(cmap, expect_map.numpy())
        assert np.array_equal(cnt, counts.numpy()) and out.dtype == np.float32
        if reduce_type == 'max':
            ref = torch.stack([f64[inverse == v].amax(0) for v in range(m)])
            assert np.array_equal(out.astype(np.float64), ref.numpy())
            continue
        ref = torch.zeros((m, feats.shape[1]), dtype=torch.float64).index_add(0, inverse, f64)
        mag = torch.zeros((m, feats.shape[1]), dtype=torch.float64).index_add(0, inverse, f64.abs())
        t = counts.double()[:, None]
        bound = (t + 2) * 2.0 ** -24 * mag
        if reduce_type == 'mean':
            ref, bound = ref / t, bound / t
        err = (torch.from_numpy(out).double() - ref).abs()
        print(f'{reduce_type}: worst error / bound = {(err / bound).max().item():.3f}, '
              f'largest voxel {int(counts.max())} points')
        assert (err <= bound).all()


def test_scatter_referee_keeps_the_smallest_voxel_and_drops_only_invalid_rows():
    feats = np.arange(8, dtype=np.float32).reshape(4, 2)
    coors = np.int32([[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]])
    out, vc, cmap, cnt = R.scatter_forward(feats, coors, 'sum')
    assert vc.tolist() == [[0, 0, 0], [1, 0, 0]] and cmap.tolist() == [1, 0, 1, 0]
    assert out.tolist() == [[8.0, 10.0], [4.0, 6.0]] and cnt.tolist() == [2, 2]
    out, vc, cmap, cnt = R.scatter_forward(feats, np.full((4, 3), -1, np.int32), 'max')
    assert out.shape == (0, 2) and vc.shape == (0, 3) and (cmap == -1).all()
    # an entry at or above its bound is invalid too
    _, vc, cmap, _ = R.scatter_forward(feats, coors, 'sum', dims=(1, 1, 1))
    assert vc.tolist() == [[0, 0, 0]] and cmap.tolist() == [-1, 0, -1, 0]


def test_scatter_referee_backward():
    feats = np.float32([[1, 5], [3, 5], [3, np.nan], [2, np.nan], [9, 9]])
    coors = np.int32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1], [-1, 0, 0]])
    gv = np.float32([[10, 20], [30, 40]])
    out, _, cmap, cnt = R.scatter_forward(feats, coors, 'max')
    assert out[0].tolist() == [3.0, 5.0] and out[1, 0] == 2.0 and out[1, 1] == -np.inf
    g = R.scatter_backward(gv, feats, out, cmap, cnt, 'max')
    # duplicate maxima: the lowest index takes it; an all-NaN cell passes nothing
    assert g.tolist() == [[0, 20], [10, 0], [0, 0], [30, 0], [0, 0]]
    g = R.scatter_backward(gv, feats, out, cmap, cnt, 'mean')
    assert np.array_equal(g[:3], np.repeat(gv[:1] / np.float32(3), 3, 0))
    assert g[3].tolist() == [30, 40] and g[4].tolist() == [0, 0]
    g = R.scatter_backward(gv, feats, out, cmap, cnt, 'sum')
    assert g.tolist() == [[10, 20]] * 3 + [[30, 40], [0, 0]]


# ---- the vectorised referee equals the loops, on the inputs the device tests use ------------------

def identical(got, want):
    """dtype, shape and every bit of every element"""
    bits = (lambda a: a.view(np.uint32)) if want.dtype == np.float32 else (lambda a: a)
    return isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape \
        and np.array_equal(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(want)))


def _voxelizer_inputs():
    """(points, voxel_size, coors_range, max_points, max_voxels) of tests/test_voxel_gpu.py"""
    from tests import test_voxel_gpu as G
    for n in G.SIZES:
        yield (G.cloud(n, n, 4, 'p2'), *G.GRIDS['p2'], 5, 200)
    for grid, c in (('tiny', 3), ('p2', 65), ('p3', 5), ('lidar', 4)):
        yield (G.cloud(17, 3000, c, grid), *G.GRIDS[grid], 5, 8 if grid == 'tiny' else 2500)
    for max_points in (1, 5):
        yield (G.cloud(3, 1500, 4, 'p2', 'one_cell'), *G.GRIDS['p2'], max_points, 40)
    yield (G.cloud(4, 1300, 4, 'p3', 'outside'), *G.GRIDS['p3'], 5, 40)
    a, b, c = [0.1, 0.1, 0.1], [0.5, 0.1, 0.1], [0.1, 0.5, 0.1]
    xyz = np.float32([a, b, a, c, b, c, a, [9.0, 0.1, 0.1], b, a])
    midstream = np.concatenate([xyz, np.arange(10, dtype=np.float32)[:, None]], axis=1)
    for max_voxels in (2, 3):
        yield (midstream, *G.GRIDS['p2'], 3, max_voxels)
    for max_voxels in (150, 400):
        yield (G.cloud(61, 5000, 4, 'p3'), *G.GRIDS['p3'], 4, max_voxels)
    for cells, cr in G.BOUNDARY_GRIDS.items():
        yield (G.cloud(int(cells) % 1000, 3129, 4, ([1.0, 1.0, 1.0], cr)), [1.0, 1.0, 1.0], cr, 5,
               2500)
    vs, cr = G.GRIDS['lidar']
    for order in ('descending', 'top_byte', 'alternating'):
        coors = G.keys_to_coors(G.ordered_keys(order))
        points = np.zeros((len(coors), 4), dtype=np.float32)
        points[:, :3] = (np.float64(cr[:3]) + (coors[:, ::-1] + 0.5) * np.float64(vs))
        points[:, 3] = np.arange(len(coors))
        yield (points, vs, cr, 5, 3000 if order == 'descending' else 40)
    # a small slice of the carrying sizes' own cloud and cap
    yield (G.cloud(262145, 262145, 4, 'lidar')[:9000], vs, cr, 5, 1000)


def test_fast_hard_voxelizer_equals_the_walk_bit_for_bit(golden):
    cases = 0
    for points, vs, cr, max_points, max_voxels in _voxelizer_inputs():
        want = R.hard_voxelize(points, vs, cr, max_points, max_voxels)
        got = R.hard_voxelize_fast(points, vs, cr, max_points, max_voxels)
        for g, w in zip(got, want):
            assert identical(g, w), (len(points), vs, max_points, max_voxels)
        cases += 1
    assert cases == 29
    for name in golden['names'].tolist():
        g = {k.split('/', 1)[1]: v for k, v in golden.items() if k.startswith(name + '/')}
        got = R.hard_voxelize_fast(g['points'], g['voxel_size'].tolist(), g['coors_range'].tolist(),
                                   int(g['max_points']), int(g['max_voxels']))
        for a, key in zip(got, ('voxels', 'coors', 'num_points_per_voxel')):
            assert identical(a, g[key]), name


def _scatter_inputs():
    """(feats, coors, dims) of tests/test_voxel_gpu.py; dims None: the functional's own bounds"""
    from tests import test_voxel_gpu as G
    for n in G.SIZES:
        yield (*G.scatter_case(n, n, 4, (6, 7, 5)), (6, 7, 5))
    for dims, c in (((1, 2, 2), 3), ((4, 40, 40), 65), ((16, 128, 128), 5), ((40, 1600, 1408), 4),
                    ((3, 3, 3), 260)):
        yield (*G.scatter_case(23, 700 if c == 260 else 3129, c, dims), dims)
    yield (*G.scatter_case(31, 2000, 4, (6, 7, 5), invalid=0), (6, 7, 5))
    feats, _ = G.scatter_case(32, 1500, 4, (6, 7, 5))
    coors = np.full((1500, 3), -1, dtype=np.int32)
    coors[::3] = [0, 7, 0]
    yield feats, coors, (6, 7, 5)
    yield (*G.scatter_case(33, 3129, 5, (6, 7, 5), ties=True, nans=True), (6, 7, 5))
    yield (*G.scatter_case(34, 3129, 5, (6, 7, 5), ties=True), (6, 7, 5))
    rng = np.random.default_rng(35)
    coors = np.zeros((1400, 3), dtype=np.int32)
    coors[:, 2] = rng.integers(0, 3, 1400)
    coors[rng.random(1400) < 0.1] = -1
    yield rng.standard_normal((1400, 6)).astype(np.float32), coors, (1, 1, 3)
    feats, coors = G.scatter_case(41, 3129, 7, (6, 7, 5), ties=True)
    coors[coors[:, 2] == 5, 2] = -1
    yield feats, coors, None
    for dims in G.BOUNDARY_DIMS:
        yield (*G.scatter_case(sum(dims) % 1000, 3129, 4, dims, invalid=0.075), dims)
    for order in ('descending', 'top_byte', 'alternating'):
        feats, _ = G.scatter_case(36, 5000, 4, G.ORDER_DIMS, ties=order != 'descending')
        yield feats, G.keys_to_coors(G.ordered_keys(order)), G.ORDER_DIMS
    # a small slice of the carrying sizes' own generator, both feature ranges
    for span in (1, 4):
        feats, coors = G.box_scatter_case(145, 262145, 4, (40, 1600, 1408), span=span)
        coors = coors[:9000].copy()
        valid = ((coors >= 0) & (coors < np.int32([40, 1600, 1408]))).all(axis=1)
        coors[valid, 2] %= 8                                   # several points to a voxel
        yield feats[:9000], coors, (40, 1600, 1408)


def test_fast_scatter_equals_the_loops_bit_for_bit():
    cases = 0
    for feats, coors, dims in _scatter_inputs():
        n, c = feats.shape
        grad_voxel = np.random.default_rng(n + c).standard_normal((max(n, 1), c)).astype(np.float32)
        for reduce_type in ('sum', 'mean', 'max'):
            want = R.scatter_forward(feats, coors, reduce_type, dims)
            got = R.scatter_forward_fast(feats, coors, reduce_type, dims)
            for g, w in zip(got, want):
                assert identical(g, w), (n, c, dims, reduce_type)
            w_out, w_vc, w_map, w_cnt = want
            gv = grad_voxel[:len(w_vc)]
            w_grad = R.scatter_backward(gv, feats, w_out, w_map, w_cnt, reduce_type)
            g_grad = R.scatter_backward_fast(gv, feats, w_out, w_map, w_cnt, reduce_type)
            assert identical(g_grad, w_grad), (n, c, dims, reduce_type)
        cases += 1
    assert cases == 31


def test_the_four_names_are_real():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import voxel as mod
    for name in NAMES:
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__
        assert getattr(mmdet3d_ops, name) is getattr(mod, name)
    assert mmdet3d_ops.voxelization == mod._Voxelization.apply
    assert mmdet3d_ops.dynamic_scatter == mod._dynamic_scatter.apply
    # the other names keep their stubs
    with pytest.raises(NotImplementedError):
        mmdet3d_ops.assign_score_withk()
    with pytest.raises(NotImplementedError):
        mmdet3d_ops.PAConv()


def _device_op_calls():
    from nesie_amd.mmdet3d_ops import DynamicScatter, Voxelization, dynamic_scatter, voxelization
    vs, cr = [0.5, 0.5, 0.5], [0, 0, 0, 4, 4, 2]
    pts = torch.rand(16, 4)
    coors = torch.zeros(16, 3, dtype=torch.int32)
    coors4 = torch.zeros(16, 4, dtype=torch.int32)
    return (lambda: voxelization(pts, vs, cr, 5, 20),
            lambda: voxelization(pts, vs, cr, -1, -1),
            lambda: Voxelization(vs, cr, 5)(pts),
            lambda: dynamic_scatter(pts.clone().requires_grad_(True), coors, 'mean'),
            lambda: DynamicScatter(vs, cr, True)(pts, coors),
            lambda: DynamicScatter(vs, cr, False)(pts, coors4))


def test_device_ops_refuse_cpu_tensors():
    for call in _device_op_calls():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_no_cpu_fallback_behind_an_injected_back_end(oracle_kernels):
    from nesie_amd import kernels
    with kernels.use_backend(oracle_kernels):
        for call in _device_op_calls():
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                call()


def test_constructors_and_repr_match_the_reference():
    from nesie_amd.mmdet3d_ops import DynamicScatter, Voxelization
    vs, cr = [0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]
    v = Voxelization(vs, cr, 5, 16000)
    assert v.max_voxels == (16000, 16000) and v.max_num_points == 5
    assert v.grid_size.tolist() == [1408, 1600, 40] and v.grid_size.dtype == torch.int64
    assert [int(s) for s in v.pcd_shape] == [1, 1600, 1408]
    assert repr(v) == ('Voxelization(voxel_size=[0.05, 0.05, 0.1], point_cloud_range='
                       '[0, -40, -3, 70.4, 40, 1], max_num_points=5, max_voxels=(16000, 16000))')
    assert Voxelization(vs, cr, 5).max_voxels == (20000, 20000)
    assert Voxelization(vs, cr, -1, (-1, -1)).max_voxels == (-1, -1)
    assert Voxelization(vs, cr, 10, (16000, 40000)).max_voxels == (16000, 40000)
    d = DynamicScatter(vs, cr, True)
    assert (d.voxel_size, d.point_cloud_range, d.average_points) == (vs, cr, True)
    assert repr(d) == ('DynamicScatter(voxel_size=[0.05, 0.05, 0.1], point_cloud_range='
                       '[0, -40, -3, 70.4, 40, 1], average_points=True)')
    assert isinstance(d, torch.nn.Module) and list(d.parameters()) == [] and d.training


def test_entries_are_declared():
    c = ctypes
    sig = _lib.SIGNATURES
    ll, i, p = c.c_longlong, c.c_int, c.c_void_p
    assert sig['nesie_voxel_grid_size'] == (i, [p] * 4)
    assert sig['nesie_voxel_workspace_bytes'] == (i, [ll, ll, p])
    assert sig['nesie_dynamic_voxelize'] == (i, [ll, i] + [p] * 5)
    assert sig['nesie_hard_voxelize'] == (i, [ll, i] + [p] * 3 + [i, i] + [p] * 6)
    assert sig['nesie_dynamic_scatter_forward'] == (i, [ll, i] + [p] * 3 + [i] + [p] * 9)
    assert sig['nesie_dynamic_scatter_backward'] == (i, [ll, i] + [p] * 8 + [i] + [p] * 2)


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    n = None
    vs = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    cr = (ctypes.c_float * 6)(0, 0, 0, 4, 4, 2)
    out = ctypes.c_longlong()
    INVALID, UNSUPPORTED = 1, 2

    # the workspace query
    assert lib.nesie_voxel_workspace_bytes(1000, 4096, ctypes.byref(out)) == 0 and out.value > 0
    assert lib.nesie_voxel_workspace_bytes(0, 1, ctypes.byref(out)) == 0
    assert lib.nesie_voxel_workspace_bytes(-1, 4096, ctypes.byref(out)) == INVALID
    assert lib.nesie_voxel_workspace_bytes(10, 4096, n) == INVALID
    assert lib.nesie_voxel_workspace_bytes(10, 2 ** 31, ctypes.byref(out)) == UNSUPPORTED
    assert lib.nesie_voxel_workspace_bytes(10, 0, ctypes.byref(out)) == UNSUPPORTED
    assert lib.nesie_voxel_workspace_bytes(2 ** 31, 4096, ctypes.byref(out)) == UNSUPPORTED
    assert lib.nesie_voxel_workspace_bytes(10, 2 ** 31 - 1, ctypes.byref(out)) == 0
    assert b'voxel_workspace_bytes' in lib.nesie_last_error()

    # a grid of 2^31 cells or more, or an axis below one cell, before anything else is looked at
    big = (ctypes.c_float * 6)(0, 0, 0, 1024, 1024, 1024)            # 2048^3 = 2^33
    exact = (ctypes.c_float * 6)(0, 0, 0, 1024, 1024, 256)           # 2048 * 2048 * 512 = 2^31
    flat = (ctypes.c_float * 6)(0, 0, 0, 4, 4, 0.2)                  # round(0.4) = 0
    grid = (ctypes.c_int * 3)()
    for bad in (big, exact, flat):
        assert lib.nesie_voxel_grid_size(vs, bad, grid, ctypes.byref(out)) == UNSUPPORTED
        assert lib.nesie_dynamic_voxelize(10, 4, n, vs, bad, n, n) == UNSUPPORTED
        assert lib.nesie_hard_voxelize(10, 4, n, vs, bad, 5, 20, n, n, n, n, n, n) == UNSUPPORTED
    assert b'hard_voxelize' in lib.nesie_last_error()
    assert lib.nesie_voxel_grid_size(n, cr, grid, ctypes.byref(out)) == INVALID
    assert lib.nesie_voxel_grid_size(vs, cr, n, ctypes.byref(out)) == INVALID

    # the voxelizers
    one = ctypes.c_int(7)
    assert lib.nesie_dynamic_voxelize(-1, 4, n, vs, cr, n, n) == INVALID
    assert lib.nesie_dynamic_voxelize(10, -4, n, vs, cr, n, n) == INVALID
    assert lib.nesie_dynamic_voxelize(10, 4, n, n, cr, n, n) == INVALID
    assert lib.nesie_dynamic_voxelize(10, 4, n, vs, n, n, n) == INVALID
    assert lib.nesie_dynamic_voxelize(10, 4, n, vs, cr, n, n) == INVALID       # null points
    assert lib.nesie_dynamic_voxelize(10, 2, n, vs, cr, n, n) == INVALID       # no z column
    assert lib.nesie_dynamic_voxelize(0, 4, n, vs, cr, n, n) == 0
    for args in ((-1, 4, 5, 20), (10, -1, 5, 20), (10, 4, 0, 20), (10, 4, 5, 0), (10, 4, -1, 20),
                 (10, 4, 5, -1), (10, 4, 5, 20), (10, 2, 5, 20)):
        nn_, c_, mp, mv = args
        assert lib.nesie_hard_voxelize(nn_, c_, n, vs, cr, mp, mv, n, n, n, ctypes.byref(one), n,
                                       n) == INVALID, args
    assert lib.nesie_hard_voxelize(0, 4, n, vs, cr, 5, 20, n, n, n, n, n, n) == INVALID   # voxel_num

    # the scatter
    dims = (ctypes.c_int * 3)(4, 4, 2)
    huge = (ctypes.c_int * 3)(2048, 2048, 512)
    zero = (ctypes.c_int * 3)(4, 0, 2)

    def fwd(nn_, c_, d, mode, num=ctypes.byref(one)):
        return lib.nesie_dynamic_scatter_forward(nn_, c_, n, n, d, mode, n, n, n, n, num, n, n, n, n)

    assert fwd(-1, 4, dims, 0) == INVALID and fwd(10, -4, dims, 0) == INVALID
    assert fwd(10, 4, dims, 3) == INVALID and fwd(10, 4, dims, -1) == INVALID
    assert fwd(10, 4, n, 0) == INVALID and fwd(10, 4, dims, 0, n) == INVALID
    assert fwd(10, 4, dims, 2) == INVALID                                        # null tensors
    assert fwd(10, 4, huge, 0) == UNSUPPORTED and fwd(10, 4, zero, 0) == UNSUPPORTED
    assert b'dynamic_scatter_forward' in lib.nesie_last_error()

    def bwd(nn_, c_, mode):
        return lib.nesie_dynamic_scatter_backward(nn_, c_, n, n, n, n, n, n, n, n, mode, n, n)

    assert bwd(-1, 4, 0) == INVALID and bwd(10, -1, 0) == INVALID and bwd(10, 4, 5) == INVALID
    for mode in (0, 1, 2):
        assert bwd(10, 4, mode) == INVALID                                       # null tensors
        assert bwd(0, 4, mode) == 0 and bwd(10, 0, mode) == 0                    # empty: no launch
    assert b'dynamic_scatter_backward' in lib.nesie_last_error()
