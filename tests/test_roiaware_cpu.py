"""RoI-aware 3-D pooling and the single-index points-in-boxes ops, the tier that needs no GPU: the
package surface, the refusals, the C entries' status codes, ``points_in_boxes_cpu`` against the
numpy referee of the in-box test, and the pooling referee (tests/_roiaware_ref.py) against an
independent float64 brute force."""
import ctypes
import math

import numpy as np
import pytest
import torch

from nesie_amd import _lib
from tests import _np_ref, _roiaware_ref as R


def random_rois(rng, n, centre_span=2.0):
    """(n,7) float32 rotated LiDAR-frame boxes around the origin, sizes 0.6 .. 2.4."""
    rois = np.empty((n, 7), dtype=np.float32)
    rois[:, :3] = rng.uniform(-centre_span, centre_span, (n, 3))
    rois[:, 3:6] = rng.uniform(0.6, 2.4, (n, 3))
    rois[:, 6] = rng.uniform(-math.pi, math.pi, n)
    return rois


def test_the_three_names_are_real():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import roiaware_pool3d as mod
    for name in ('RoIAwarePool3d', 'points_in_boxes_gpu', 'points_in_boxes_cpu'):
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__
        assert getattr(mmdet3d_ops, name) is getattr(mod, name)
    pool = mmdet3d_ops.RoIAwarePool3d(4)
    assert (pool.out_size, pool.max_pts_per_voxel, pool.mode) == (4, 128, 0)
    assert mmdet3d_ops.RoIAwarePool3d((2, 3, 5), 16, 'avg').mode == 1
    with pytest.raises(AssertionError):
        mmdet3d_ops.RoIAwarePool3d(4, mode='sum')
    # the other names keep their stubs
    with pytest.raises(NotImplementedError):
        mmdet3d_ops.assign_score_withk()


def _device_op_calls():
    from nesie_amd.mmdet3d_ops import RoIAwarePool3d, points_in_boxes_gpu
    rois, pts, feat = torch.rand(2, 7) + 0.5, torch.rand(16, 3), torch.rand(16, 4)
    return (lambda: points_in_boxes_gpu(pts[None], rois[None]),
            lambda: RoIAwarePool3d(2)(rois, pts, feat),
            lambda: RoIAwarePool3d((2, 2, 1), 4, 'avg')(rois, pts, feat.requires_grad_(True)))


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


def test_entries_are_declared_with_the_reference_argument_order():
    c = ctypes
    sig = _lib.SIGNATURES
    assert sig['nesie_points_in_boxes_gpu'] == (c.c_int, [c.c_int] * 3 + [c.c_void_p] * 4)
    assert sig['nesie_roiaware_pool3d_sizes'] == (c.c_int, [c.c_int] * 7 + [c.c_void_p])
    assert sig['nesie_roiaware_pool3d_forward'] == (
        c.c_int, [c.c_int] * 7 + [c.c_void_p] * 7 + [c.c_int, c.c_void_p])
    assert sig['nesie_roiaware_pool3d_backward'] == (
        c.c_int, [c.c_int] * 7 + [c.c_void_p] * 5 + [c.c_int, c.c_void_p])


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    n = None

    def fwd(N, P, C, m, ox, oy, oz, method=0):
        return lib.nesie_roiaware_pool3d_forward(N, P, C, m, ox, oy, oz, n, n, n, n, n, n, n,
                                                 method, n)

    def bwd(N, P, ox, oy, oz, C, m, method=0):
        return lib.nesie_roiaware_pool3d_backward(N, P, ox, oy, oz, C, m, n, n, n, n, n, method, n)

    # negative sizes, m < 1, an unknown pool method: NESIE_ERR_INVALID_ARG
    for args in ((-1, 8, 4, 8, 2, 2, 2), (2, -8, 4, 8, 2, 2, 2), (2, 8, -4, 8, 2, 2, 2),
                 (2, 8, 4, 0, 2, 2, 2), (2, 8, 4, -3, 2, 2, 2)):
        assert fwd(*args) == 1, args
        assert b'roiaware_pool3d_forward' in lib.nesie_last_error()
    assert fwd(2, 8, 4, 8, 2, 2, 2, method=2) == 1
    for args in ((-1, 8, 2, 2, 2, 4, 8), (2, -8, 2, 2, 2, 4, 8), (2, 8, 2, 2, 2, -4, 8),
                 (2, 8, 2, 2, 2, 4, 0)):
        assert bwd(*args) == 1, args
        assert b'roiaware_pool3d_backward' in lib.nesie_last_error()
    assert bwd(2, 8, 2, 2, 2, 4, 8, method=-1) == 1
    # out_* outside 1 .. 256: NESIE_ERR_UNSUPPORTED
    for out in ((0, 2, 2), (2, 257, 2), (2, 2, -1), (300, 300, 300)):
        assert fwd(2, 8, 4, 8, *out) == 2, out
        assert b'roiaware_pool3d_forward' in lib.nesie_last_error()
        assert bwd(2, 8, *out, 4, 8) == 2, out
    assert fwd(2, 8, 4, 8, 256, 1, 256) == 1          # in range: now the null pointers count
    # empty problems succeed without touching the device
    for args in ((0, 8, 4, 8, 2, 2, 2), (2, 0, 4, 8, 2, 2, 2), (2, 8, 0, 8, 2, 2, 2)):
        assert fwd(*args) == 0, args
    for args in ((0, 8, 2, 2, 2, 4, 8), (2, 0, 2, 2, 2, 4, 8), (2, 8, 2, 2, 2, 0, 8)):
        assert bwd(*args) == 0, args
    # null pointers for a problem that is not empty are an argument error, not a crash
    assert fwd(2, 8, 4, 8, 2, 2, 2) == 1 and bwd(2, 8, 2, 2, 2, 4, 8) == 1

    # the size query: same refusals, and the three element counts
    out = (ctypes.c_longlong * 3)()
    assert lib.nesie_roiaware_pool3d_sizes(3, 10, 5, 2, 3, 4, 7, ctypes.addressof(out)) == 0
    assert list(out) == [3 * 24 * 7, 3 * 24 * 5, 30]
    assert lib.nesie_roiaware_pool3d_sizes(70000, 64, 128, 256, 256, 256, 128,
                                           ctypes.addressof(out)) == 0
    assert out[0] == 70000 * 256 ** 3 * 128                # no 32-bit overflow
    assert lib.nesie_roiaware_pool3d_sizes(3, 10, 5, 2, 3, 4, 7, None) == 1
    assert lib.nesie_roiaware_pool3d_sizes(3, 10, 5, 2, 3, 4, 0, ctypes.addressof(out)) == 1
    assert lib.nesie_roiaware_pool3d_sizes(3, 10, 5, 2, 3, 257, 7, ctypes.addressof(out)) == 2
    assert b'roiaware_pool3d_sizes' in lib.nesie_last_error()

    # points_in_boxes_gpu
    for args in ((-1, 3, 8), (1, -3, 8), (1, 3, -8)):
        assert lib.nesie_points_in_boxes_gpu(*args, n, n, n, n) == 1, args
        assert b'points_in_boxes_gpu' in lib.nesie_last_error()
    assert lib.nesie_points_in_boxes_gpu(0, 3, 8, n, n, n, n) == 0
    assert lib.nesie_points_in_boxes_gpu(2, 3, 0, n, n, n, n) == 0
    assert lib.nesie_points_in_boxes_gpu(1, 3, 8, n, n, n, n) == 1
    assert lib.nesie_points_in_boxes_gpu(1, 0, 8, n, n, n, n) == 1   # T = 0 still writes -1: needs out


def _points_on_faces(rois, rng, per_box=24):
    """Points placed exactly (as far as fp32 goes) on the faces of each box, plus its corners'
    neighbourhood: the cases where strict / inclusive comparisons decide."""
    out = []
    for cx, cy, cz, w, l, h, rz in rois.astype(np.float64):
        a = rz + math.pi / 2
        u = rng.uniform(-0.5, 0.5, (per_box, 3))
        face = rng.integers(0, 6, per_box)
        u[face == 0, 0], u[face == 1, 0] = 0.5, -0.5
        u[face == 2, 1], u[face == 3, 1] = 0.5, -0.5
        u[face == 4, 2], u[face == 5, 2] = 0.5, -0.5
        lx, ly, lz = u[:, 0] * l, u[:, 1] * w, u[:, 2] * h + h / 2
        # local = R(a) shift  ->  shift = R(a)^T local
        sx = lx * math.cos(a) + ly * math.sin(a)
        sy = -lx * math.sin(a) + ly * math.cos(a)
        out.append(np.stack([cx + sx, cy + sy, cz + lz], 1))
    return np.concatenate(out).astype(np.float32)


def test_points_in_boxes_cpu_equals_the_referee():
    from nesie_amd.mmdet3d_ops import points_in_boxes_cpu
    rng = np.random.default_rng(5)
    rois = random_rois(rng, 12)
    rois[0, 6], rois[1, 6] = 0.0, -math.pi / 2           # axis-aligned: faces hit exactly
    rois[0, :6] = (0.5, -0.25, 0.0, 1.0, 2.0, 0.5)
    rois[1, :6] = (-1.0, 1.0, -0.5, 0.5, 1.5, 1.0)
    pts = np.concatenate([rng.uniform(-3, 3, (1500, 3)).astype(np.float32),
                          _points_on_faces(rois, rng)])
    # exact face hits of the axis-aligned box 0 (rz = 0: local x = -shift_y, local y = shift_x)
    exact = np.array([[0.5 + 0.5, -0.25, 0.25], [0.5 - 0.5, -0.25, 0.25], [0.5, -0.25 + 1.0, 0.25],
                      [0.5, -0.25, 0.5], [0.5, -0.25, 0.0], [0.5, -0.25, 0.5000001]], np.float32)
    pts = np.concatenate([pts, exact])
    want = _np_ref.points_in_boxes(rois, pts).T
    got = points_in_boxes_cpu(torch.from_numpy(pts), torch.from_numpy(rois))
    assert got.dtype == torch.int32 and tuple(got.shape) == (12, len(pts))
    assert np.array_equal(got.numpy(), want)
    assert 200 < want.sum() < want.size // 2
    # z is inclusive, x / y strict: the top and bottom face centres are in, the side faces out
    tail = want[0, -6:]
    assert tail.tolist() == [0, 0, 0, 1, 1, 0]
    # the pooling referee restates the same test: its mask is this one
    for n in range(len(rois)):
        assert np.array_equal(R.local_coords(rois[n], pts)[0], want[n].astype(bool))
    assert tuple(points_in_boxes_cpu(torch.zeros(0, 3), torch.from_numpy(rois)).shape) == (12, 0)


def _brute_force(rois, pts, out):
    """Independent float64 assignment: the point in the box's frame as projections on the box's
    axes, the voxel as floor(out * (fraction along the axis)).  -> (voxel (N,P) or -1, near (N,P)
    bool = within 1e-4 x extent of a box face or a voxel plane)."""
    rois, pts = rois.astype(np.float64), pts.astype(np.float64)
    N, P = len(rois), len(pts)
    vox = np.full((N, P), -1, dtype=np.int64)
    near = np.zeros((N, P), dtype=bool)
    for n, (cx, cy, cz, w, l, h, rz) in enumerate(rois):
        a = rz + math.pi / 2
        ax, ay = np.array([math.cos(a), -math.sin(a)]), np.array([math.sin(a), math.cos(a)])
        d = pts[:, :2] - np.array([cx, cy])
        frac = np.stack([d @ ax / l + 0.5, d @ ay / w + 0.5, (pts[:, 2] - cz) / h], 1)   # 0 .. 1 inside
        scaled = frac * np.array(out)
        cell = np.floor(scaled).astype(np.int64)
        inside = np.all((frac > 0) & (frac < 1), axis=1)
        # a voxel plane (the faces are planes 0 and out) within 1e-4 x extent: 1e-4 * out in `scaled`
        near[n] = np.any(np.abs(scaled - np.round(scaled)) < 1e-4 * np.array(out), axis=1) & \
            np.all((frac > -1e-3) & (frac < 1 + 1e-3), axis=1)
        cell = np.clip(cell, 0, np.array(out) - 1)
        vox[n] = np.where(inside, (cell[:, 0] * out[1] + cell[:, 1]) * out[2] + cell[:, 2], -1)
    return vox, near


@pytest.mark.parametrize('out,m', [((4, 4, 4), 128), ((2, 3, 5), 6)])
def test_referee_against_a_float64_brute_force(out, m):
    rng = np.random.default_rng(11)
    rois = random_rois(rng, 6, centre_span=1.0)
    pts = rng.uniform(-2.5, 2.5, (3000, 3)).astype(np.float32)
    feat = rng.standard_normal((3000, 5)).astype(np.float32)
    vox, near = _brute_force(rois, pts, out)
    res = {mode: R.forward(rois, pts, feat, out, m, mode) for mode in ('max', 'avg')}
    table = res['max']['table']
    compared = (vox >= 0) & ~near
    share = near.sum() / max((near | (vox >= 0)).sum(), 1)
    print(f'compared {compared.sum()} inside points, left out {near.sum()} ({share:.3%})')
    assert share < 0.01
    assert compared.sum() >= 200
    assert np.array_equal(table[~near], vox[~near])
    # collection and pooling, restated set-wise on the referee's own table: a voxel's kept points
    # are its m - 1 smallest indices; max / first index of the max; float64 mean
    nvox = out[0] * out[1] * out[2]
    idx = res['max']['pts_idx_of_voxels'].reshape(len(rois), nvox, m)
    assert np.array_equal(idx, res['avg']['pts_idx_of_voxels'].reshape(idx.shape))
    overflowed = 0
    for n in range(len(rois)):
        for v in range(nvox):
            members = np.nonzero(table[n] == v)[0]
            keep = members[:m - 1]
            overflowed += len(members) > m - 1
            assert idx[n, v, 0] == len(keep)
            assert idx[n, v, 1:1 + len(keep)].tolist() == keep.tolist()
            assert not idx[n, v, 1 + len(keep):].any()
            assert np.array_equal(np.nonzero(res['max']['kept'][n] == v)[0], keep)
            pooled_max = res['max']['pooled'].reshape(len(rois), nvox, -1)[n, v]
            arg = res['max']['argmax'].reshape(len(rois), nvox, -1)[n, v]
            pooled_avg = res['avg']['pooled'].reshape(len(rois), nvox, -1)[n, v]
            if len(keep) == 0:
                assert not pooled_max.any() and not pooled_avg.any() and (arg == -1).all()
                continue
            assert np.array_equal(pooled_max, feat[keep].max(0))
            assert np.array_equal(arg, keep[feat[keep].argmax(0)])
            mean = feat[keep].astype(np.float64).mean(0)
            bound = (len(keep) + 1) * 2.0 ** -24 * np.abs(feat[keep]).astype(np.float64).mean(0)
            assert np.all(np.abs(pooled_avg - mean) <= bound)
    assert (overflowed > 0) == (m == 6)
    assert not res['avg']['argmax'].any()

    # backward: the referee's ordered fp32 sums against a float64 scatter of the same terms
    grad_out = rng.standard_normal(res['max']['pooled'].shape).astype(np.float32)
    g = grad_out.reshape(len(rois), nvox, -1).astype(np.float64)
    for mode in ('max', 'avg'):
        got = R.grad_in(res[mode], grad_out, len(pts), mode)
        want = np.zeros(got.shape)
        mag = np.zeros(got.shape)
        terms = np.zeros(got.shape)
        for n in range(len(rois)):
            for v in range(nvox):
                keep = idx[n, v, 1:1 + idx[n, v, 0]]
                if mode == 'avg':
                    want[keep] += g[n, v] / max(len(keep), 1)
                    mag[keep] += np.abs(g[n, v]) / max(len(keep), 1)
                    terms[keep] += 1
                else:
                    arg = res['max']['argmax'].reshape(len(rois), nvox, -1)[n, v]
                    ok = arg >= 0
                    np.add.at(want, (arg[ok], np.arange(len(arg))[ok]), g[n, v][ok])
                    np.add.at(mag, (arg[ok], np.arange(len(arg))[ok]), np.abs(g[n, v][ok]))
                    np.add.at(terms, (arg[ok], np.arange(len(arg))[ok]), 1)
        assert terms.max() >= 2          # overlapping boxes: some point gathers from several
        assert np.all(np.abs(got - want) <= (terms + 2) * 2.0 ** -24 * mag)
