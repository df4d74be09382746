"""nesie_iou3d_forward against nesie_giou3d_forward (GIoU, "smallest", with Jacobian): HIP events
around ONE call, the two kernels alternating in the same process, median of 20 after 5 warm-ups,
at n = 2 048 (8 scenes x 256 proposals) and n = 4 096.  usage: python tools/giou_bench.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nesie_amd.kernels import backend_for

dev = torch.device('cuda:0')


def boxes(n, seed):
    g = torch.Generator().manual_seed(seed)
    target = torch.cat([torch.rand(n, 3, generator=g) * 2, 0.4 + torch.rand(n, 3, generator=g) * 1.6,
                        (torch.rand(n, 1, generator=g) - 0.5) * 3.14159], 1)
    pred = target.clone()
    pred[:, :3] += (torch.rand(n, 3, generator=g) - 0.5) * 0.8
    pred[:, 3:6] *= 0.7 + torch.rand(n, 3, generator=g) * 0.6
    pred[:, 6] += (torch.rand(n, generator=g) - 0.5)
    target[::2, 6] = 0                               # half the targets axis-aligned, as ScanNet's
    return pred.to(dev).contiguous(), target.to(dev).contiguous()


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3                   # us


for n in (2048, 4096):
    a, b = boxes(n, n)
    hip = backend_for(a)
    iou, loss, jac = a.new_empty(n), a.new_empty(n), a.new_empty(n, 7)
    calls = dict(iou3d=lambda: hip.iou3d_forward(a, b, iou, jac),
                 giou3d=lambda: hip.giou3d_forward(a, b, 0, 0, loss, iou, jac))
    times = {k: [] for k in calls}
    for it in range(25):
        for k, fn in calls.items():
            t = once(fn)
            if it >= 5:
                times[k].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'n = {n}: iou3d_forward {med["iou3d"]:.1f} us (min {min(times["iou3d"]):.1f}), '
          f'giou3d_forward {med["giou3d"]:.1f} us (min {min(times["giou3d"]):.1f}), '
          f'ratio {med["giou3d"] / med["iou3d"]:.2f}')
