"""Float64 numpy referee of the Lovasz-Softmax loss and its gradient, shared by
test_lovasz_cpu.py and test_lovasz_gpu.py.

The errors e = |fg - p| are formed in float32 exactly as the kernel forms them, so the permutation
(e descending, equal errors by ascending point index, +inf and NaN first, void points last) is
determined exactly; everything after the sort is float64.  Two independent forms of the Lovasz
gradient g are kept: ``closed`` (from the integer counts, no subtraction of nearby numbers) and
``cumulative`` (the paper's 1 - I / U, differenced in float64)."""
import numpy as np


def g_closed(fg_sorted):
    fg = np.asarray(fg_sorted, dtype=bool)
    n = fg.size
    big_g = int(fg.sum())
    cf = np.cumsum(fg.astype(np.int64))
    at = np.arange(1, n + 1, dtype=np.int64)
    union = (big_g + (at - cf)).astype(np.float64)
    inter = (big_g - cf).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        bg = np.where(union > 1, inter / (union * (union - 1)), 1.0)
    return np.where(fg, 1.0 / union, bg)


def g_cumulative(fg_sorted):
    fg = np.asarray(fg_sorted, dtype=bool)
    gts = float(fg.sum())
    inter = gts - np.cumsum(fg.astype(np.float64))
    union = gts + np.cumsum((~fg).astype(np.float64))
    jaccard = 1.0 - inter / union
    out = jaccard.copy()
    out[1:] = jaccard[1:] - jaccard[:-1]
    return out


def segment(p, labels, c, ignore=None, form=g_closed):
    """One segment: p (L,) float32 probabilities of class c, labels (L,) -> (loss, d loss / d p (L,),
    G), float64.  A void point has gradient 0."""
    p = np.asarray(p, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    void = labels == ignore if ignore is not None else np.zeros(labels.shape, dtype=bool)
    fg = (labels == c) & ~void
    e = np.abs(fg.astype(np.float32) - p)
    assert e.dtype == np.float32
    with np.errstate(invalid='ignore'):
        key = np.where(np.isfinite(e), -e.astype(np.float64), -np.inf)
    key = np.where(void, np.inf, key)
    perm = np.argsort(key, kind='stable')
    valid = int((~void).sum())
    perm_v = perm[:valid]                       # the void points are behind every valid one
    grad = np.zeros(p.shape, dtype=np.float64)
    if valid == 0:
        return 0.0, grad, 0
    g = form(fg[perm_v])
    loss = float(np.sum(e[perm_v].astype(np.float64) * g))
    grad[perm_v] = np.where(fg[perm_v], -g, g)
    return loss, grad, int(fg.sum())


def lovasz(probas, labels, classes='present', per_image=False, ignore=None, form=g_closed):
    """probas (B, C, S) float32, labels (B, S) -> (loss float64, d loss / d probas (B, C, S) float64)."""
    probas = np.asarray(probas, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    b, c, s = probas.shape
    if not per_image:
        probas = probas.transpose(1, 0, 2).reshape(1, c, b * s)
        labels = labels.reshape(1, b * s)
    images = probas.shape[0]
    grad = np.zeros(probas.shape, dtype=np.float64)
    total = 0.0
    for im in range(images):
        losses, grads, counts = [], [], []
        for k in range(c):
            l, g, big_g = segment(probas[im, k], labels[im], k, ignore, form)
            losses.append(l); grads.append(g); counts.append(big_g)
        if classes == 'all':
            weight = [1] * c
        elif classes == 'present':
            weight = [1 if n > 0 else 0 for n in counts]
        else:
            weight = [list(classes).count(k) for k in range(c)]
        n = sum(weight)
        if n == 0:
            continue
        for k in range(c):
            if weight[k]:
                total += weight[k] * losses[k] / n / images
                grad[im, k] = grads[k] * (weight[k] / n / images)
    if not per_image:
        grad = grad.reshape(c, b, s).transpose(1, 0, 2)
    return total, grad
