"""RoI-aware 3-D pooling at this project's own shape: one scene, 256 proposals, out_size 4,
C = 128, points = the 1 024 seeds and the 40 000 input points; forward alone and forward +
backward, max and avg.  HIP events around ``--calls`` back-to-back calls (one call is far below
a millisecond for the seeds), ``--repeats`` windows after ``--warmup`` untimed ones; prints the
median, the min and the max per call, the kept memberships and the bytes the three kernels must
move (computed from the shapes and the counts, not measured).  Needs a HIP device; reads nothing
but this repository.  usage: python tools/roiaware_bench.py [--calls 20] [--repeats 15]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nesie_amd.kernels import backend_for  # noqa: E402

N, OUT, C, M = 256, 4, 128, 128


def scene(points, seed, dev):
    """A room of 8 x 8 x 3 m: uniform points, proposals of 0.4 .. 2.2 m with any yaw."""
    g = torch.Generator().manual_seed(seed)
    span = torch.tensor([8.0, 8.0, 3.0])
    pts = torch.rand(points, 3, generator=g) * span
    rois = torch.cat([torch.rand(N, 3, generator=g) * (span - torch.tensor([0.0, 0.0, 1.5])),
                      0.4 + torch.rand(N, 3, generator=g) * 1.8,
                      (torch.rand(N, 1, generator=g) - 0.5) * 2 * math.pi], 1)
    feat = torch.randn(points, C, generator=g)
    return rois.to(dev), pts.to(dev), feat.to(dev)


def window(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls             # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('roiaware_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    for points in (1024, 40000):
        rois, pts, feat = scene(points, points, dev)
        hip = backend_for(feat)
        pooled = feat.new_empty(N, OUT, OUT, OUT, C)
        argmax = torch.empty(N, OUT, OUT, OUT, C, dtype=torch.int32, device=dev)
        idx = torch.empty(N, OUT, OUT, OUT, M, dtype=torch.int32, device=dev)
        pts_voxel = torch.empty(N, points, dtype=torch.int32, device=dev)
        grad_out, grad_in = torch.randn_like(pooled), torch.empty_like(feat)
        for mode, method in (('max', 0), ('avg', 1)):
            def fwd():
                hip.roiaware_pool3d_forward(rois, pts, feat, argmax, idx, pooled, method, pts_voxel)

            def fwd_bwd():
                fwd()
                hip.roiaware_pool3d_backward(idx, argmax, pts_voxel, grad_out, grad_in, method)

            times = {'forward': [], 'forward+backward': []}
            for it in range(args.warmup + args.repeats):
                for name, fn in (('forward', fwd), ('forward+backward', fwd_bwd)):   # alternating
                    t = window(fn, args.calls)
                    if it >= args.warmup:
                        times[name].append(t)
            kept = int((pts_voxel >= 0).sum())
            # collect: points once per box + both int tables; pool: kept rows + outputs;
            # backward: the table + one grad_out (and argmax) row per membership + grad_in
            bytes_fwd = N * points * (12 + 4) + idx.numel() * 4 + kept * C * 4 + pooled.numel() * 8
            bytes_bwd = N * points * 4 + kept * C * (8 if method == 0 else 4) + grad_in.numel() * 4
            row = dict(points=points, mode=mode, kept_memberships=kept,
                       algorithmic_bytes_forward=bytes_fwd, algorithmic_bytes_backward=bytes_bwd)
            for name, ts in times.items():
                row[name + '_us'] = dict(median=round(statistics.median(ts), 1),
                                         min=round(min(ts), 1), max=round(max(ts), 1))
            print(json.dumps(row))


if __name__ == '__main__':
    main()
