"""Shared by the axis-aligned IoU tests and tests/golden/make_aa_iou_golden.py: the cases of
tests/golden/aa_iou3d.npz and the error bound taken from the reference's own float32 error."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'aa_iou3d.npz')
PAIRED = ('overlap', 'disjoint', 'inside', 'identical', 'touching', 'tiny')
CASES = PAIRED + ('matrix',)
COUNT = dict(overlap=64, disjoint=64, inside=16, identical=8, touching=8, tiny=8, matrix=None)
TIES = ('identical', 'touching')      # a max / min / clamp sits exactly on its kink
MODES = ('iou', 'giou')
FORMS = ('aligned', 'matrix')
FLOOR = 4 * 2.0 ** -24

_golden = None


def golden():
    """The fixture, loaded once; nobody writes to it."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def forms_of(case):
    return ('matrix',) if case == 'matrix' else FORMS


def bound(case, mode, form, what):
    """What a float32 implementation may be away from the float64 result of ``what`` ('out',
    'grad1', 'grad2') on this case: 4 x the largest |reference float32 - float64| + 4 x 2^-24, the
    gradients' scaled by the largest float64 gradient entry of the case.  The factor 4 allows for
    FMA contraction and another division sequence, the floor covers cases where the reference's
    float32 is exact."""
    z = golden()
    key = f'{case}/{mode}/{form}'
    f32, f64 = z[f'{key}/f32/{what}'].astype(np.float64), z[f'{key}/f64/{what}']
    ref_err = float(np.abs(f32 - f64).max())
    if what == 'out':
        return 4 * ref_err + FLOOR, ref_err
    scale = max(float(np.abs(z[f'{key}/f64/grad1']).max()), float(np.abs(z[f'{key}/f64/grad2']).max()))
    return 4 * ref_err + FLOOR * scale, ref_err
