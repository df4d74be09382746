#!/usr/bin/env python
"""Generate tests/golden/lovasz.npz from the REFERENCE's own mmdet3d/models/losses/lovasz_loss.py.

    NESIE_REFERENCE=/path/to/reference python tests/golden/make_lovasz_golden.py

The reference file is loaded from its path at generation time (nothing of it is copied here); the two
names it imports from mmdet (``mmdet.models.builder.LOSSES``, ``mmdet.models.losses.utils.
weighted_loss``) are stubbed, as make_golden.py does for the other losses.  For every case the file
records the float32 inputs and the reference's float32 loss and d loss / d probas (autograd through
its torch.sort / cumsum / dot chain, on the CPU).  The reference only runs in float32, so these
vectors carry the cancellation of its ``jaccard[i] - jaccard[i - 1]``: an absolute error of about one
ulp of 1 in each gradient entry of a class, divided by the number of averaged classes.

The probabilities are the softmax (sigmoid for the 3-D case) of 3 * randn logits: tie-free, so the
gradient does not depend on how torch.sort orders equal errors.  The script asserts that.

Measured when the committed file was made (the float64 referee tests/_lovasz_ref.py against these
vectors; the script prints the figures):
    max |loss - referee|              6.68e-08  (relative to the loss: 7.72e-08)
    max |gradient element - referee|  7.36e-08  (the sigmoid case: one averaged class, so a whole
                                                 ulp of 1 reaches the entry)
tests/test_lovasz_cpu.py bounds both absolutely at 4x these maxima: 2.7e-07 and 3.0e-07.
"""
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NESIE_REFERENCE")
sys.path.insert(0, os.path.dirname(HERE))

# name, shape of probas, classes, per_image, ignore, labels drawn from
CASES = [
    ("present_4d", (2, 5, 10, 15), 'present', False, None, range(5)),
    ("all_absent_class_4d", (2, 5, 10, 15), 'all', False, None, (0, 1, 3, 4)),
    ("present_per_image_4d", (3, 4, 8, 10), 'present', True, None, range(4)),
    ("list_ignore_4d", (2, 6, 12, 10), [1, 3, 4], False, 255, range(6)),
    ("present_ignore_per_image_5d", (2, 4, 3, 6, 8), 'present', True, 3, range(4)),
    ("present_ignore_5d_2000x20", (1, 20, 5, 20, 20), 'present', False, 255, range(20)),
    ("all_ignore_per_image_4d", (2, 3, 9, 11), 'all', True, 7, range(3)),
    ("sigmoid_3d", (2, 10, 10), [1], False, None, (0, 1)),
]


def load_reference():
    if not REF:
        raise SystemExit("set NESIE_REFERENCE to a checkout of the reference")
    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    for name, attrs in (("mmdet", {}), ("mmdet.models", {}),
                        ("mmdet.models.builder", {"LOSSES": _Registry()}),
                        ("mmdet.models.losses", {}),
                        ("mmdet.models.losses.utils", {"weighted_loss": lambda f: f})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    path = os.path.join(REF, "mmdet3d", "models", "losses", "lovasz_loss.py")
    spec = importlib.util.spec_from_file_location("reference_lovasz_loss", path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the reference compares a string with `is`
        spec.loader.exec_module(mod)
    return mod


def draw(rng, name, shape, ignore, pool):
    logits = torch.from_numpy((3.0 * rng.randn(*shape)).astype(np.float32))
    probas = torch.sigmoid(logits) if len(shape) == 3 else torch.softmax(logits, dim=1)
    lshape = shape[:1] + shape[(1 if len(shape) == 3 else 2):]
    labels = np.asarray(list(pool))[rng.randint(0, len(pool), size=lshape)].astype(np.int64)
    if name == "present_per_image_4d":
        labels[1][labels[1] == 2] = 0            # image 1 lacks class 2
    if ignore is not None:
        labels[rng.rand(*lshape) < 0.2] = ignore
    return probas.clone(), labels


def tie_free(p3, l2, ignore):
    """Inside a class no valid background point shares its error with another valid point
    (foreground points of equal error are neighbours with the same g = 1 / U)."""
    valid = (l2 != ignore).reshape(-1) if ignore is not None else np.ones(l2.size, bool)
    for k in range(p3.shape[1]):
        fg = (l2 == k).reshape(-1)[valid]
        e = np.abs(fg.astype(np.float32) - p3[:, k].reshape(-1)[valid])
        _, inverse, counts = np.unique(e, return_inverse=True, return_counts=True)
        if np.any((counts[inverse] > 1) & ~fg):
            return False
    return True


def main():
    import _lovasz_ref as referee
    ref = load_reference()
    rng = np.random.RandomState(20)
    out, meta = {}, []
    worst_loss = worst_rel = worst_grad = 0.0
    for name, shape, classes, per_image, ignore, pool in CASES:
        b, c = (shape[0], 1) if len(shape) == 3 else shape[:2]
        while True:                              # drawn again until tie-free (same stream of draws)
            probas, labels = draw(rng, name, shape, ignore, pool)
            p = probas.numpy()
            p3, l2 = p.reshape(b, c, -1), labels.reshape(b, -1)
            if c == 1:                           # the sigmoid form: foreground = the listed label
                l2 = np.where(l2 == classes[0], 0, -1)
            if tie_free(p3, l2, ignore):
                break
        probas.requires_grad_(True)
        # the literal: the reference tests `classes is 'present'`
        arg = 'present' if classes == 'present' else classes
        loss = ref.lovasz_softmax(probas, torch.from_numpy(labels), arg, per_image, ignore)
        assert loss.dtype == torch.float32
        loss.backward()
        loss = loss.detach()
        want, want_grad = referee.lovasz(p3, l2, [0] if c == 1 else classes, per_image, ignore)
        got, got_grad = float(loss), probas.grad.numpy().reshape(b, c, -1)
        worst_loss = max(worst_loss, abs(got - want))
        worst_rel = max(worst_rel, abs(got - want) / abs(want))
        worst_grad = max(worst_grad, float(np.abs(got_grad - want_grad).max()))
        out[name + "_probas"] = p
        out[name + "_labels"] = labels
        out[name + "_loss"] = np.float32(got)
        out[name + "_grad"] = probas.grad.numpy()
        meta.append(dict(name=name, classes=classes, per_image=per_image, ignore=ignore))
    out["cases"] = np.asarray(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "lovasz.npz"), **out)
    print(f"max |loss - referee| {worst_loss:.3g} (relative {worst_rel:.3g}), "
          f"max |gradient element - referee| {worst_grad:.3g}")


if __name__ == "__main__":
    main()
