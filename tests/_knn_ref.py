"""numpy referee for the kNN index op, written from the rule in include/nesie_ops.h
(``nesie_knn_wrapper``): all float32 squared distances of a centre in the selected distance form
(``_np_ref.sqdist``, switch ``_np_ref.FORM``), a stable lexicographic sort by (distance, point
index), the first k, and (index 0, distance 1e10) in the slots no point reaches."""
import numpy as np

from tests import _np_ref

PAD_DIST = np.float32(1e10)


def knn(new_xyz, xyz, k):
    """(M, 3), (N, 3) -> idx (M, k) int32, dist2 (M, k) float32."""
    m, n = new_xyz.shape[0], xyz.shape[0]
    idx = np.zeros((m, k), dtype=np.int32)
    dist2 = np.full((m, k), PAD_DIST, dtype=np.float32)
    if n == 0:
        return idx, dist2
    d = _np_ref.sqdist(new_xyz[:, None, :], xyz[None, :, :])          # (M, N) float32
    # a stable sort by distance keeps equal distances in ascending point index
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    have = order.shape[1]
    idx[:, :have] = order
    dist2[:, :have] = np.take_along_axis(d, order, axis=1)
    return idx, dist2


def knn_batch(new_xyz, xyz, k):
    """(B, M, 3), (B, N, 3) -> idx, dist2 (B, M, k)."""
    pairs = [knn(c, p, k) for c, p in zip(new_xyz, xyz)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
