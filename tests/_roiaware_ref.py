"""Numpy referee of RoI-aware 3-D pooling (include/nesie_ops.h, nesie_roiaware_pool3d_forward).

Written from the reference's lines (mmdet3d/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu),
not from the kernels: generate_pts_mask_for_box3d :45-91, the serial walk of
collect_inside_pts_for_box3d :93-127, roiaware_maxpool3d :129-187, roiaware_avgpool3d :189-226 and
the two backward kernels :277-341 (their atomic adds replaced by the pinned ascending
(box, voxel) order).  The in-box test is _np_ref.points_in_boxes' arithmetic, restated here only
because the voxel rule needs the local coordinates it does not return; test_roiaware_cpu.py pins
the two masks to each other.

There is no golden file: the reference's implementation is CUDA-only and cannot run on the
machines this project is built on, so there is no reference program to record from.
"""
import math

import numpy as np

from tests._np_ref import f32

f64 = np.float64


def local_coords(box, pts):
    """One LiDAR-frame box (7,), pts (P,3) -> (inside (P,) bool, local_x, local_y (P,) float32):
    check_pt_in_box3d :27-44 in the canonical mixed f32 / f64 form of _np_ref.points_in_boxes."""
    cx, cy, cz, w, l, h, rz = [f32(v) for v in box]
    czm = f32(f64(cz) + f64(h) / 2.0)
    rot = f32(f64(rz) + math.pi / 2)
    cosa, sina = f32(math.cos(float(rot))), f32(math.sin(float(rot)))
    x, y, z = (pts[:, i].astype(f32) for i in range(3))
    zin = ~(np.abs((z - czm).astype(f32)).astype(f64) > f64(h) / 2.0)
    sx, sy = (x - cx).astype(f32), (y - cy).astype(f32)
    lx = ((sx * cosa).astype(f32) + (sy * f32(-sina)).astype(f32)).astype(f32)
    ly = ((sx * sina).astype(f32) + (sy * cosa).astype(f32)).astype(f32)
    hl, hw = f64(l) / 2.0, f64(w) / 2.0
    inside = zin & (lx.astype(f64) > -hl) & (lx.astype(f64) < hl) & \
        (ly.astype(f64) > -hw) & (ly.astype(f64) < hw)
    return inside, lx, ly


def _out3(out_size):
    return (out_size,) * 3 if isinstance(out_size, int) else tuple(out_size)


def voxel_table(rois, pts, out_size):
    """(N,P) int32: the flat voxel (x_idx * oy + y_idx) * oz + z_idx of every inside point, -1
    outside (:65-78; fp32 throughout, IEEE division, truncation, clamp into [0, out - 1])."""
    ox, oy, oz = _out3(out_size)
    rois, pts = np.asarray(rois, dtype=f32), np.asarray(pts, dtype=f32)
    table = np.full((rois.shape[0], pts.shape[0]), -1, dtype=np.int32)
    for n, box in enumerate(rois):
        inside, lx, ly = local_coords(box, pts)
        w, l, h = f32(box[3]), f32(box[4]), f32(box[5])
        x_res, y_res, z_res = f32(l / f32(ox)), f32(w / f32(oy)), f32(h / f32(oz))
        sel = np.nonzero(inside)[0]
        lz = (pts[sel, 2] - f32(box[2])).astype(f32)
        xi = np.trunc(((lx[sel] + f32(l / f32(2))).astype(f32) / x_res).astype(f32)).astype(np.int64)
        yi = np.trunc(((ly[sel] + f32(w / f32(2))).astype(f32) / y_res).astype(f32)).astype(np.int64)
        zi = np.trunc((lz / z_res).astype(f32)).astype(np.int64)
        xi, yi, zi = np.clip(xi, 0, ox - 1), np.clip(yi, 0, oy - 1), np.clip(zi, 0, oz - 1)
        table[n, sel] = ((xi * oy + yi) * oz + zi).astype(np.int32)
    return table


def collect(table, nvox, m):
    """The serial walk :93-127 -> (pts_idx_of_voxels (N, nvox, m) int32, kept (N,P) int32 = the
    voxel a point is KEPT in, else -1)."""
    N, P = table.shape
    idx = np.zeros((N, nvox, m), dtype=np.int32)
    kept = np.full((N, P), -1, dtype=np.int32)
    for n in range(N):
        for k in np.nonzero(table[n] != -1)[0]:
            v = table[n, k]
            cnt = idx[n, v, 0]
            if cnt < m - 1:
                idx[n, v, cnt + 1] = k
                idx[n, v, 0] += 1
                kept[n, k] = v
    return idx, kept


def pool(idx, feat, mode):
    """(pooled (N, nvox, C) float32, argmax (N, nvox, C) int32) from the slot lists: 'max' :129-187
    (strict > from -inf in slot order; 0 / -1 where nothing was taken), 'avg' :189-226 (fp32 running
    sum in slot order over the count; argmax stays 0, the reference's zero fill)."""
    feat = np.asarray(feat, dtype=f32)
    N, nvox, _ = idx.shape
    C = feat.shape[1]
    pooled = np.zeros((N, nvox, C), dtype=f32)
    argmax = np.zeros((N, nvox, C), dtype=np.int32)
    if mode == 'max':
        argmax[:] = -1
    for n, v in zip(*np.nonzero(idx[:, :, 0])):
        total = idx[n, v, 0]
        if mode == 'max':
            best = np.full(C, -np.inf, dtype=f32)
            arg = np.full(C, -1, dtype=np.int32)
            for k in range(1, total + 1):
                row = feat[idx[n, v, k]]
                take = row > best
                best[take] = row[take]
                arg[take] = idx[n, v, k]
            pooled[n, v] = np.where(arg != -1, best, f32(0))
            argmax[n, v] = arg
        else:
            s = np.zeros(C, dtype=f32)
            for k in range(1, total + 1):
                s = (s + feat[idx[n, v, k]]).astype(f32)
            pooled[n, v] = (s / f32(total)).astype(f32)
    return pooled, argmax


def backward(idx, argmax, grad_out, num_pts, mode):
    """grad_in (P,C) float32: every element the fp32 sum of its contributions in ascending
    (box, voxel) order (:277-341 with the atomicAdd given that order); avg rounds
    grad_out * (1 / max(count, 1)) to fp32 before the add."""
    N, nvox, _ = idx.shape
    grad_out = np.asarray(grad_out, dtype=f32).reshape(N, nvox, -1)
    C = grad_out.shape[2]
    grad_in = np.zeros((num_pts, C), dtype=f32)
    chan = np.arange(C)
    for n in range(N):
        for v in range(nvox):
            g = grad_out[n, v]
            if mode == 'max':
                arg = argmax[n, v]
                ok = arg != -1
                grad_in[arg[ok], chan[ok]] = (grad_in[arg[ok], chan[ok]] + g[ok]).astype(f32)
            else:
                total = idx[n, v, 0]
                scale = f32(f32(1) / max(f32(total), f32(1)))
                term = (g * scale).astype(f32)
                for k in range(1, total + 1):
                    p = idx[n, v, k]
                    grad_in[p] = (grad_in[p] + term).astype(f32)
    return grad_in


def forward(rois, pts, feat, out_size, m, mode):
    """-> dict(pts_idx_of_voxels (N,ox,oy,oz,m), argmax, pooled (N,ox,oy,oz,C), kept (N,P),
    table (N,P) = the voxel before the capacity rule)."""
    ox, oy, oz = _out3(out_size)
    table = voxel_table(rois, pts, out_size)
    idx, kept = collect(table, ox * oy * oz, m)
    pooled, argmax = pool(idx, feat, mode)
    N, C = table.shape[0], np.asarray(feat).shape[1]
    return dict(pts_idx_of_voxels=idx.reshape(N, ox, oy, oz, m),
                argmax=argmax.reshape(N, ox, oy, oz, C), pooled=pooled.reshape(N, ox, oy, oz, C),
                kept=kept, table=table)


def grad_in(res, grad_out, num_pts, mode):
    """``backward`` on a ``forward`` result."""
    idx = res['pts_idx_of_voxels']
    N, m = idx.shape[0], idx.shape[-1]
    C = res['argmax'].shape[-1]
    return backward(idx.reshape(N, -1, m), res['argmax'].reshape(N, -1, C), grad_out, num_pts, mode)
