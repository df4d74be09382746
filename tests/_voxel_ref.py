"""Plain numpy referee of the voxel ops' pinned semantics (include/nesie_ops.h,
``nesie_hard_voxelize`` / ``nesie_dynamic_scatter_forward``), restated from the reference's lines:
the serial walk of voxelization_cpu.cpp:20-96 for the voxelizers, and for the scatter the
lexicographic unique rows of scatter_points_cuda.cu:202-210, fixed-order fp32 sums and the
lowest-index arg-max of :136-160.  Written for clarity, not speed."""
import numpy as np

F32 = np.float32


def grid_size(voxel_size, coors_range):
    """(grid_x, grid_y, grid_z): roundf((hi - lo) / vs) in fp32, halves away from zero."""
    vs = np.asarray(voxel_size, dtype=F32)
    cr = np.asarray(coors_range, dtype=F32)
    q64 = ((cr[3:] - cr[:3]) / vs).astype(np.float64)   # the fp32 quotient; + 0.5 is exact in double
    r = np.where(q64 >= 0, np.floor(q64 + 0.5), np.ceil(q64 - 0.5))
    return tuple(int(v) for v in r)


def dynamic_voxelize(points, voxel_size, coors_range):
    """points (N, C>=3) float32 -> coors (N, 3) int32: (c_z, c_y, c_x), (-1, -1, -1) out of range."""
    points = np.asarray(points, dtype=F32)
    vs = np.asarray(voxel_size, dtype=F32)
    lo = np.asarray(coors_range, dtype=F32)[:3]
    grid = np.asarray(grid_size(voxel_size, coors_range), dtype=np.float64)
    with np.errstate(all='ignore'):
        q = (points[:, :3] - lo[None, :]) / vs[None, :]        # fp32: one subtraction, one division
        f = np.floor(q).astype(np.float64)
    ok = (np.isfinite(q) & (f >= 0) & (f < grid[None, :])).all(axis=1)
    cell = np.where(ok[:, None], f, -1.0).astype(np.int32)
    return np.ascontiguousarray(cell[:, ::-1])


def hard_voxelize(points, voxel_size, coors_range, max_points, max_voxels):
    """The serial walk -> voxels (M, max_points, C), coors (M, 3), num_points_per_voxel (M)."""
    points = np.asarray(points, dtype=F32)
    n, c = points.shape
    cell = dynamic_voxelize(points, voxel_size, coors_range)
    voxels = np.zeros((max_voxels, max_points, c), dtype=F32)
    coors = np.zeros((max_voxels, 3), dtype=np.int32)
    num = np.zeros((max_voxels,), dtype=np.int32)
    seen = {}
    voxel_num = 0
    for i in range(n):
        if cell[i, 0] == -1:
            continue
        key = (int(cell[i, 0]), int(cell[i, 1]), int(cell[i, 2]))
        v = seen.get(key, -1)
        if v == -1:
            if voxel_num >= max_voxels:
                continue
            v = voxel_num
            voxel_num += 1
            seen[key] = v
            coors[v] = cell[i]
        if num[v] < max_points:
            voxels[v, num[v]] = points[i]
            num[v] += 1
    return voxels[:voxel_num], coors[:voxel_num], num[:voxel_num]


def scatter_forward(feats, coors, reduce_type, dims=None):
    """feats (N, C) float32, coors (N, 3) int32 -> voxel_feats (M, C), voxel_coors (M, 3),
    coors_map (N), reduce_count (M).  A row is invalid if an entry is negative or >= dims."""
    feats = np.asarray(feats, dtype=F32)
    coors = np.asarray(coors, dtype=np.int32)
    n, c = feats.shape
    valid = (coors >= 0).all(axis=1)
    if dims is not None:
        valid &= (coors < np.asarray(dims, dtype=np.int64)[None, :]).all(axis=1)
    rows = sorted({tuple(int(x) for x in coors[i]) for i in range(n) if valid[i]})
    ordinal = {r: v for v, r in enumerate(rows)}
    m = len(rows)
    voxel_coors = np.asarray(rows, dtype=np.int32).reshape(m, 3)
    coors_map = np.full((n,), -1, dtype=np.int32)
    count = np.zeros((m,), dtype=np.int32)
    out = np.full((m, c), -np.inf if reduce_type == 'max' else 0.0, dtype=F32)
    with np.errstate(all='ignore'):
        for i in range(n):                                    # ascending point index
            if not valid[i]:
                continue
            v = ordinal[tuple(int(x) for x in coors[i])]
            coors_map[i] = v
            count[v] += 1
            if reduce_type == 'max':
                out[v] = np.where(feats[i] > out[v], feats[i], out[v])   # a NaN never wins
            else:
                out[v] = out[v] + feats[i]                    # fp32 running sum
        if reduce_type == 'mean':
            out = out / count.astype(F32)[:, None]
    return out, voxel_coors, coors_map, count


def scatter_backward(grad_voxel, feats, voxel_feats, coors_map, count, reduce_type):
    """-> grad_feats (N, C) float32, zeros for invalid rows."""
    feats = np.asarray(feats, dtype=F32)
    grad_voxel = np.asarray(grad_voxel, dtype=F32)
    n, c = feats.shape
    grad = np.zeros((n, c), dtype=F32)
    taken = np.zeros(voxel_feats.shape, dtype=bool)
    with np.errstate(all='ignore'):
        for i in range(n):                                    # ascending: the lowest index wins
            v = coors_map[i]
            if v < 0:
                continue
            if reduce_type == 'sum':
                grad[i] = grad_voxel[v]
            elif reduce_type == 'mean':
                grad[i] = grad_voxel[v] / F32(count[v])
            else:
                take = (feats[i] == voxel_feats[v]) & ~taken[v]
                grad[i] = np.where(take, grad_voxel[v], F32(0))
                taken[v] |= take
    return grad


# ---- the same outputs in vectorised numpy: for sizes the loops above cannot reach.  The CPU tests
# assert that each form equals its loop bit for bit on every input the device tests use at small
# sizes; that equality is their licence to stand as referee at the large ones.

def _segments(group):
    """group (V,) ints, 0 .. m - 1 -> order (V,) = the stable argsort of group (so every group's
    members are contiguous, in ascending position), starts (m + 1,), rank (V,) = a member's place
    inside its group in the order of `order`."""
    order = np.argsort(group, kind='stable')
    m = int(group.max()) + 1 if len(group) else 0
    starts = np.zeros((m + 1,), dtype=np.int64)
    np.cumsum(np.bincount(group, minlength=m), out=starts[1:])
    rank = np.arange(len(group), dtype=np.int64) - starts[group[order]]
    return order, starts, rank


def hard_voxelize_fast(points, voxel_size, coors_range, max_points, max_voxels):
    """hard_voxelize without the walk: a cell's voxel is the ordinal of its first appearance
    (np.unique's first index, ranked), a point's slot its rank inside the cell."""
    points = np.asarray(points, dtype=F32)
    n, c = points.shape
    cell = dynamic_voxelize(points, voxel_size, coors_range)
    gx, gy, _ = grid_size(voxel_size, coors_range)
    inside = np.flatnonzero(cell[:, 0] != -1)
    c64 = cell[inside].astype(np.int64)
    key = (c64[:, 0] * gy + c64[:, 1]) * gx + c64[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    ordinal = np.empty((len(first),), dtype=np.int64)
    ordinal[np.argsort(first, kind='stable')] = np.arange(len(first))
    order, _, rank = _segments(inverse)
    voxel = ordinal[inverse[order]]
    keep = (voxel < max_voxels) & (rank < max_points)
    m = min(len(first), max_voxels)
    voxels = np.zeros((m, max_points, c), dtype=F32)
    voxels[voxel[keep], rank[keep]] = points[inside[order[keep]]]
    coors = np.zeros((m, 3), dtype=np.int32)
    head = ordinal < max_voxels
    coors[ordinal[head]] = cell[inside[first[head]]]
    num = np.zeros((m,), dtype=np.int32)
    count = np.bincount(inverse, minlength=len(first))
    num[ordinal[head]] = np.minimum(count[head], max_points)
    return voxels, coors, num


def scatter_forward_fast(feats, coors, reduce_type, dims=None):
    """scatter_forward with the running sum / maximum taken in rounds: round r adds every voxel's
    r-th point (ascending point index), so each voxel sees its terms in the loop's order."""
    feats = np.asarray(feats, dtype=F32)
    coors = np.asarray(coors, dtype=np.int32)
    n, c = feats.shape
    valid = (coors >= 0).all(axis=1)
    if dims is not None:
        valid &= (coors < np.asarray(dims, dtype=np.int64)[None, :]).all(axis=1)
    rows = np.flatnonzero(valid)
    c64 = coors[rows].astype(np.int64)
    span = c64.max(axis=0) + 1 if len(rows) else np.ones((3,), dtype=np.int64)
    key = (c64[:, 0] * span[1] + c64[:, 1]) * span[2] + c64[:, 2]    # lexicographic, below 2^63
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    m = len(first)
    voxel_coors = coors[rows[first]].reshape(m, 3)
    coors_map = np.full((n,), -1, dtype=np.int32)
    coors_map[rows] = inverse
    count = np.bincount(inverse, minlength=m).astype(np.int32)
    out = np.full((m, c), -np.inf if reduce_type == 'max' else 0.0, dtype=F32)
    order, _, rank = _segments(inverse)
    by_rank, rounds, _ = _segments(rank)
    with np.errstate(all='ignore'):
        for r in range(len(rounds) - 1):
            sel = order[by_rank[rounds[r]:rounds[r + 1]]]             # one point of each voxel
            v, f = inverse[sel], feats[rows[sel]]
            if reduce_type == 'max':
                out[v] = np.where(f > out[v], f, out[v])
            else:
                out[v] = out[v] + f
        if reduce_type == 'mean':
            out = out / count.astype(F32)[:, None]
    return out, voxel_coors, coors_map, count


def scatter_backward_fast(grad_voxel, feats, voxel_feats, coors_map, count, reduce_type):
    feats = np.asarray(feats, dtype=F32)
    grad_voxel = np.asarray(grad_voxel, dtype=F32)
    n, c = feats.shape
    grad = np.zeros((n, c), dtype=F32)
    rows = np.flatnonzero(coors_map >= 0)
    v = coors_map[rows].astype(np.int64)
    if not len(rows):
        return grad
    with np.errstate(all='ignore'):
        if reduce_type == 'sum':
            grad[rows] = grad_voxel[v]
        elif reduce_type == 'mean':
            grad[rows] = grad_voxel[v] / count[v].astype(F32)[:, None]
        else:
            equal = feats[rows] == voxel_feats[v]
            order, starts, _ = _segments(v)          # every voxel below len(count) has a point
            assert (starts[1:] > starts[:-1]).all()
            cand = np.where(equal[order], rows[order][:, None], n)
            lowest = np.minimum.reduceat(cand, starts[:-1], axis=0)   # (M, C): who takes it
            take = equal & (lowest[v] == rows[:, None])
            grad[rows] = np.where(take, grad_voxel[v], F32(0))
    return grad
