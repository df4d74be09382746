#!/usr/bin/env python
"""Generate tests/golden/aa_iou3d.npz from the REFERENCE's own axis-aligned overlaps.

Runs where the reference tree is (NESIE_REFERENCE, default /root/reference), on the CPU; it is not a
test.  The reference's ``core/bbox/iou_calculators/iou3d_calculator.py`` is loaded by path under its
dotted name, unmodified; the three imports at its top that the axis-aligned calculator never touches
(``mmdet.core.bbox.bbox_overlaps``, mmdet's ``IOU_CALCULATORS`` registry, ``..structures``) are
stand-ins: a registry whose ``register_module()`` returns the class, and two names that raise.

Per case (tests/_aa_iou.py CASES) the file holds the inputs (float32 corner boxes) and, for mode
'iou' and 'giou', for the aligned and the matrix form, in float32 and in float64:
  out            the reference's result,
  grad1, grad2   autograd's gradient of (out * gout).sum() w.r.t. bboxes1 and bboxes2,
with gout all ones for the aligned form (the gradients are then the per-pair Jacobians) and the
recorded ``<case>/gout`` (m, n) for the matrix form.  The 'matrix' case (b = 2, 37 x 53) has the
matrix form only.
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

from tests import _aa_iou  # noqa: E402

SEEDS = dict(overlap=21, disjoint=22, inside=23, identical=24, touching=25, tiny=26, matrix=27)


def _corners(centre, size):
    return np.concatenate([centre - size / 2, centre + size / 2], -1).astype(np.float32)


def make_inputs(case):
    """-> (bboxes1, bboxes2) float32 corner boxes, (n, 6) or, for 'matrix', (2, 37, 6) / (2, 53, 6)."""
    rng = np.random.default_rng(SEEDS[case])
    n = _aa_iou.COUNT[case]
    if case == 'matrix':        # a room's worth of boxes: some overlap, most do not
        def scene(count):
            return _corners(rng.random((2, count, 3)) * 3.0, 0.3 + rng.random((2, count, 3)) * 1.5)
        return scene(37), scene(53)
    c2, s2 = rng.random((n, 3)) * 2, 0.4 + rng.random((n, 3)) * 1.6
    if case == 'overlap':
        c1 = c2 + (rng.random((n, 3)) - 0.5) * 0.6
        s1 = s2 * (0.7 + rng.random((n, 3)) * 0.6)
    elif case == 'disjoint':    # apart along a random axis, by more than the half sizes
        s1 = 0.4 + rng.random((n, 3)) * 1.6
        c1 = c2 + (rng.random((n, 3)) - 0.5) * 0.6
        axis = rng.integers(0, 3, n)
        gap = 0.5 * (s1 + s2)[np.arange(n), axis] * (1.05 + rng.random(n))
        c1[np.arange(n), axis] = c2[np.arange(n), axis] + gap * rng.choice([-1.0, 1.0], n)
    elif case == 'inside':      # the first box strictly inside the second
        s1 = s2 * (0.2 + rng.random((n, 3)) * 0.25)
        c1 = c2 + (rng.random((n, 3)) - 0.5) * 0.1 * s2
    elif case == 'identical':
        c1, s1 = c2, s2
    elif case == 'tiny':        # volumes of about 1e-9: the union is below eps = 1e-6
        s2 = 1e-3 * (0.5 + rng.random((n, 3)))
        s1 = s2 * (0.7 + rng.random((n, 3)) * 0.6)
        c1 = c2 + (rng.random((n, 3)) - 0.5) * 0.5e-3
    elif case == 'touching':
        c1 = c2 + (rng.random((n, 3)) - 0.5) * 0.6
        s1 = s2 * (0.7 + rng.random((n, 3)) * 0.6)
    else:
        raise KeyError(case)
    a, b = _corners(c1, s1), _corners(c2, s2)
    if case == 'touching':      # flush on one face, in float32 bits; pairs 6 and 7 also share y
        for i in range(n):
            axis, side = i % 3, (i // 3) % 2
            size = a[i, 3 + axis] - a[i, axis]
            if side == 0:       # the first box ends where the second begins
                a[i, 3 + axis] = b[i, axis]
                a[i, axis] = b[i, axis] - size
            else:
                a[i, axis] = b[i, 3 + axis]
                a[i, 3 + axis] = b[i, 3 + axis] + size
            if i >= 6:
                other = (axis + 1) % 3
                a[i, other], a[i, 3 + other] = b[i, other], b[i, 3 + other]
    return a, b


def load_reference():
    def refuse(*args, **kwargs):
        raise RuntimeError('not part of the axis-aligned calculator')

    class Registry:
        def register_module(self):
            return lambda cls: cls

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    module('mmdet').__path__ = []
    module('mmdet.core').__path__ = []
    module('mmdet.core.bbox', bbox_overlaps=refuse).__path__ = []
    module('mmdet.core.bbox.iou_calculators').__path__ = []
    module('mmdet.core.bbox.iou_calculators.builder', IOU_CALCULATORS=Registry())
    r = os.path.join(REF, 'mmdet3d')
    for name, path in (('mmdet3d', r), ('mmdet3d.core', os.path.join(r, 'core')),
                       ('mmdet3d.core.bbox', os.path.join(r, 'core', 'bbox')),
                       ('mmdet3d.core.bbox.iou_calculators',
                        os.path.join(r, 'core', 'bbox', 'iou_calculators'))):
        module(name).__path__ = [path]        # path-only shells: no __init__.py is executed
    module('mmdet3d.core.bbox.structures', get_box_type=refuse)
    return importlib.import_module('mmdet3d.core.bbox.iou_calculators.iou3d_calculator')


def main():
    ref = load_reference()
    calculator = ref.AxisAlignedBboxOverlaps3D()
    out = {}
    for case in _aa_iou.CASES:
        a, b = (torch.from_numpy(x) for x in make_inputs(case))
        out[f'{case}/box1'], out[f'{case}/box2'] = a.numpy(), b.numpy()
        rng = np.random.default_rng(SEEDS[case] + 100)
        gout = torch.from_numpy(
            rng.uniform(-1.0, 2.0, a.shape[:-1] + b.shape[-2:-1]).astype(np.float32))
        out[f'{case}/gout'] = gout.numpy()
        for form in _aa_iou.FORMS:
            if form == 'aligned' and case == 'matrix':
                continue
            for mode in _aa_iou.MODES:
                for dtype, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
                    p = a.to(dtype).requires_grad_(True)
                    q = b.to(dtype).requires_grad_(True)
                    res = calculator(p, q, mode, is_aligned=form == 'aligned')
                    w = torch.ones_like(res) if form == 'aligned' else gout.to(dtype)
                    g1, g2 = torch.autograd.grad((res * w).sum(), (p, q))
                    key = f'{case}/{mode}/{form}/{tag}'
                    out[f'{key}/out'] = res.detach().numpy()
                    out[f'{key}/grad1'], out[f'{key}/grad2'] = g1.numpy(), g2.numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'aa_iou3d.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
