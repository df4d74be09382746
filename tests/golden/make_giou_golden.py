#!/usr/bin/env python
"""Generate tests/golden/giou3d.npz from the REFERENCE's own enclosing-box losses.

Runs where the reference tree is (NESIE_REFERENCE, default /root/reference), on the CPU; it is not a
test.  The reference's ``min_enclosing_box.py``, ``oriented_iou_loss.py``, ``box_intersection_2d.py``
and ``cuda_op/cuda_ext.py`` are loaded by path under their dotted names, unmodified, as
make_golden.py loads the package, with two accommodations:
  * ``sort_vertices`` (the CUDA extension behind ``sort_v``) is the CPU oracle's restatement;
  * ``numpy.int``, which numpy 2 removed and ``min_enclosing_box.py`` still spells, is ``int``.

Per input mode (tests/_giou_ref.py MODES) the file holds the inputs and, for cal_giou_3d and
cal_diou_3d with the "smallest" and the "aligned" enclosing box, in float32 and in float64: loss,
iou and the autograd gradient of loss.sum() w.r.t. box3d1; plus the winning candidate of
``smallest_bounding_box(verbose=True)`` with the area of the best two candidates (float64).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("NESIE_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from tests import _giou_ref  # noqa: E402

SEEDS = dict(overlap=11, disjoint=12, yaw0=13, small_yaw=14, inside=15, identical=16, sizes=17)


def _boxes(rng, n, lo=0.4, hi=2.0):
    return np.concatenate([rng.random((n, 3)) * 2, lo + rng.random((n, 3)) * (hi - lo),
                           (rng.random((n, 1)) - 0.5) * np.pi], -1)


def make_inputs(mode):
    """-> (pred, target), float32 (n, 7): x, y, z, dx, dy, dz, yaw."""
    rng = np.random.default_rng(SEEDS[mode])
    n = 8 if mode == 'identical' else 64
    b = _boxes(rng, n)
    a = b.copy()
    if mode == 'overlap':                 # random yaw on both, centres close
        a[:, :3] += (rng.random((n, 3)) - 0.5) * 0.6
        a[:, 3:6] *= 0.7 + rng.random((n, 3)) * 0.6
        a[:, 6] = (rng.random(n) - 0.5) * np.pi
    elif mode == 'disjoint':              # centre distance > sum of the BEV half diagonals
        a[:, 3:6] = 0.4 + rng.random((n, 3)) * 1.6
        a[:, 6] = (rng.random(n) - 0.5) * np.pi
        reach = 0.5 * (np.hypot(a[:, 3], a[:, 4]) + np.hypot(b[:, 3], b[:, 4]))
        phi = rng.random(n) * 2 * np.pi
        dist = reach * (1.05 + rng.random(n))
        a[:, 0] = b[:, 0] + dist * np.cos(phi)
        a[:, 1] = b[:, 1] + dist * np.sin(phi)
        a[:, 2] = b[:, 2] + (rng.random(n) - 0.5) * 1.0
    elif mode == 'yaw0':                  # the ScanNet case: both axis-aligned
        b[:, 6] = 0
        a[:, :3] += (rng.random((n, 3)) - 0.5) * 0.8
        a[:, 3:6] *= 0.7 + rng.random((n, 3)) * 0.6
        a[:, 6] = 0
    elif mode == 'small_yaw':             # axis-aligned target, |yaw| < 0.05 on the prediction
        b[:, 6] = 0
        a[:, :3] += (rng.random((n, 3)) - 0.5) * 0.8
        a[:, 3:6] *= 0.7 + rng.random((n, 3)) * 0.6
        a[:, 6] = (rng.random(n) - 0.5) * 0.098
    elif mode == 'inside':                # the prediction strictly inside the target
        side = np.minimum(b[:, 3], b[:, 4])[:, None]       # (its circumscribed circle fits)
        a[:, 3:5] = side * (0.2 + rng.random((n, 2)) * 0.25)
        a[:, 5] = b[:, 5] * (0.2 + rng.random(n) * 0.25)
        a[:, :2] += (rng.random((n, 2)) - 0.5) * 0.1 * side
        a[:, 2] += (rng.random(n) - 0.5) * 0.1 * b[:, 5]
        a[:, 6] = (rng.random(n) - 0.5) * np.pi
    elif mode == 'identical':
        pass
    elif mode == 'sizes':                 # 0.05 m .. 5 m, log-uniform
        b[:, 3:6] = np.exp(rng.uniform(np.log(0.05), np.log(5.0), (n, 3)))
        a[:, 3:6] = np.exp(rng.uniform(np.log(0.05), np.log(5.0), (n, 3)))
        a[:, :3] = b[:, :3] + (rng.random((n, 3)) - 0.5) * 0.5 * (a[:, 3:6] + b[:, 3:6])
        a[:, 6] = (rng.random(n) - 0.5) * np.pi
    else:
        raise KeyError(mode)
    return (torch.from_numpy(a.astype(np.float32)).contiguous(),
            torch.from_numpy(b.astype(np.float32)).contiguous())


def load_reference():
    np.int = int                              # min_enclosing_box.py:53-54

    def sort_vertices_forward(vertices, mask, num_valid):
        v = vertices.float().contiguous()
        idx = torch.empty(v.shape[0], v.shape[1], 9, dtype=torch.int32)
        oracle.OracleKernels().sort_vertices_forward(v, mask.contiguous(),
                                                     num_valid.contiguous(), idx)
        return idx
    ext = types.ModuleType('sort_vertices')
    ext.sort_vertices_forward = sort_vertices_forward
    sys.modules['sort_vertices'] = ext
    r = os.path.join(REF, 'mmdet3d')
    for name, path in (('mmdet3d', r), ('mmdet3d.ops', os.path.join(r, 'ops')),
                       ('mmdet3d.ops.rotated_iou', os.path.join(r, 'ops', 'rotated_iou')),
                       ('mmdet3d.ops.rotated_iou.cuda_op',
                        os.path.join(r, 'ops', 'rotated_iou', 'cuda_op'))):
        shell = types.ModuleType(name)        # path-only shells: no __init__.py is executed
        shell.__path__ = [path]
        sys.modules[name] = shell
    return (importlib.import_module('mmdet3d.ops.rotated_iou.oriented_iou_loss'),
            importlib.import_module('mmdet3d.ops.rotated_iou.min_enclosing_box'))


def main():
    oi, meb = load_reference()
    fns = dict(giou=oi.cal_giou_3d, diou=oi.cal_diou_3d)
    out = {}
    for mode in _giou_ref.MODES:
        a, b = make_inputs(mode)
        out[f'{mode}/box1'], out[f'{mode}/box2'] = a.numpy(), b.numpy()
        for dtype, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
            for kind, fn in fns.items():
                for enc in _giou_ref.ENCLOSING:
                    p = a[None].to(dtype).requires_grad_(True)
                    loss, iou = fn(p, b[None].to(dtype), enc)
                    (grad,) = torch.autograd.grad(loss.sum(), p)
                    key = f'{mode}/{kind}/{enc}/{tag}'
                    out[f'{key}/loss'] = loss.detach()[0].numpy()
                    out[f'{key}/iou'] = iou.detach()[0].numpy()
                    out[f'{key}/grad'] = grad[0].numpy()
        # the winner of the brute force, and how far the runner-up is, in float64
        with torch.no_grad():
            _, c1, c2, _, _ = oi.cal_iou_3d(a[None].double(), b[None].double(), verbose=True)
            corners = torch.cat([c1, c2], dim=-2)
            _, _, _, idx = meb.smallest_bounding_box(corners, verbose=True)
            lines, points, _, _ = meb.gather_lines_points(corners)
            area = meb.point_line_projection_range(lines, points) \
                * meb.point_line_distance_range(lines, points)
            area = area + 1e8 * (area == 0).double()
        out[f'{mode}/winner'] = idx[0].numpy().astype(np.int32)
        out[f'{mode}/best_two'] = torch.sort(area[0], dim=-1)[0][:, :2].numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'giou3d.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
