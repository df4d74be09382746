"""The voxel ops at two sizes: this project's own scene (40 000 points in an 8 x 8 x 3 m room,
0.05 m voxels: a 160 x 160 x 60 grid) and a LiDAR-sized synthetic cloud (300 000 points, a
1408 x 1600 x 40 grid, max_points 5, max_voxels 150 000).  C = 4 for the voxelizers, C = 64 for
the scatter, whose coordinates are the dynamic voxelizer's.  HIP events around ``--calls``
back-to-back calls, ``--repeats`` windows after ``--warmup`` untimed ones, forward and
forward + backward alternating; prints the median, the min and the max per call, the counts and
the bytes each op must move (computed from the shapes and the counts, not measured).  Needs a HIP
device; reads nothing but this repository.
usage: python tools/voxel_bench.py [--calls 10] [--repeats 15]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nesie_amd.kernels import backend_for  # noqa: E402

SIZES = {
    'room': dict(points=40000, voxel_size=[0.05, 0.05, 0.05],
                 coors_range=[0.0, 0.0, 0.0, 8.0, 8.0, 3.0], max_points=5, max_voxels=40000),
    'lidar': dict(points=300000, voxel_size=[0.05, 0.05, 0.1],
                  coors_range=[0.0, -40.0, -3.0, 70.4, 40.0, 1.0], max_points=5,
                  max_voxels=150000),
}
C_VOXELIZE, C_SCATTER = 4, 64


def cloud(cfg, seed, dev):
    """Three quarters of the points on a few hundred surfaces' worth of cells (several points a
    voxel, as a scan gives), the rest uniform; 2 % outside the range."""
    g = torch.Generator().manual_seed(seed)
    n = cfg['points']
    lo = torch.tensor(cfg['coors_range'][:3])
    span = torch.tensor(cfg['coors_range'][3:]) - lo
    xyz = torch.rand(n, 3, generator=g)
    dense = torch.rand(n, generator=g) < 0.75
    xyz[dense, 2] = (xyz[dense, 2] * 8).floor() / 8 + 0.001      # horizontal sheets ...
    xyz[dense, :2] = xyz[dense, :2] ** 3                         # ... denser towards one corner
    xyz = lo + xyz * span
    out = torch.rand(n, generator=g) < 0.02
    xyz[out] += span
    pts = torch.cat([xyz, torch.rand(n, C_VOXELIZE - 3, generator=g)], 1)
    return pts.to(dev), torch.randn(n, C_SCATTER, generator=g).to(dev)


def window(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls             # us per call


def measure(fns, args):
    times = {name: [] for name in fns}
    for it in range(args.warmup + args.repeats):
        for name, fn in fns.items():                    # alternating
            t = window(fn, args.calls)
            if it >= args.warmup:
                times[name].append(t)
    return {name + '_us': dict(median=round(statistics.median(ts), 1), min=round(min(ts), 1),
                               max=round(max(ts), 1)) for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('voxel_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    for size, cfg in SIZES.items():
        pts, feats = cloud(cfg, 7, dev)
        hip = backend_for(pts)
        n, vs, cr = cfg['points'], cfg['voxel_size'], cfg['coors_range']
        mp, mv = cfg['max_points'], cfg['max_voxels']
        (gx, gy, gz), cells = hip.voxel_grid_size(vs, cr)
        passes = (cells.bit_length() + 7) // 8
        ws = torch.empty(hip.voxel_workspace_bytes(n, cells), dtype=torch.uint8, device=dev)
        sort_bytes = 8 * n + passes * 20 * n             # keys + indices out; count, read, write
        scan_bytes = 16 * n

        # ---- the voxelizers
        i32 = dict(dtype=torch.int32, device=dev)
        dyn = torch.empty((n, 3), **i32)
        voxels = torch.empty((mv, mp, C_VOXELIZE), device=dev)
        coors, num, voxel_num = (torch.empty(s, **i32) for s in ((mv, 3), (mv,), (1,)))
        fns = {
            'dynamic_voxelize': lambda: hip.dynamic_voxelize(pts, vs, cr, dyn),
            'hard_voxelize': lambda: hip.hard_voxelize(pts, vs, cr, voxels, coors, num,
                                                       voxel_num, ws),
        }
        row = dict(size=size, points=n, grid=[gx, gy, gz], sort_passes=passes, c=C_VOXELIZE)
        row.update(measure(fns, args))
        m = int(voxel_num.item())
        kept = int(num[:m].sum())
        row.update(voxels=m, kept_points=kept, in_range=int((dyn[:, 0] >= 0).sum()),
                   algorithmic_bytes_dynamic_voxelize=n * (12 + 12),
                   algorithmic_bytes_hard_voxelize=(
                       n * C_VOXELIZE * 4 + sort_bytes + 12 * n + scan_bytes + 8 * n
                       + kept * C_VOXELIZE * 4 + m * (mp * C_VOXELIZE * 4 + 16)))
        print(json.dumps(row))

        # ---- the scatter
        dims = (gz, gy, gx)
        vf, grad, gv = (torch.empty((n, C_SCATTER), device=dev) for _ in range(3))
        gv.normal_()
        vc = torch.empty((n, 3), **i32)
        cmap, cnt, order, start = (torch.empty((n,), **i32) for _ in range(4))
        nv = torch.empty((1,), **i32)
        for reduce_type, mode in (('max', 2), ('mean', 1)):
            def fwd():
                hip.dynamic_scatter_forward(feats, dyn, dims, mode, vf, vc, cmap, cnt, nv, order,
                                            start, ws)

            def fwd_bwd():
                fwd()
                hip.dynamic_scatter_backward(gv, feats, vf, cmap, cnt, order, start, nv, mode, grad)

            row = dict(size=size, points=n, grid=[gx, gy, gz], sort_passes=passes, c=C_SCATTER,
                       reduce=reduce_type)
            row.update(measure({'forward': fwd, 'forward+backward': fwd_bwd}, args))
            m = int(nv.item())
            valid = int((cmap >= 0).sum())
            row.update(voxels=m, valid_points=valid, largest_voxel=int(cnt[:m].max()),
                       algorithmic_bytes_forward=(
                           12 * n + sort_bytes + 8 * n + scan_bytes + 12 * n + m * 28
                           + valid * C_SCATTER * 4 + 4 * n + m * (C_SCATTER * 4 + 4)),
                       algorithmic_bytes_backward=(
                           n * C_SCATTER * 4 + 4 * n + m * C_SCATTER * 4
                           + (valid * C_SCATTER * 4 + m * C_SCATTER * 4 if mode == 2 else 0)))
            print(json.dumps(row))


if __name__ == '__main__':
    main()
