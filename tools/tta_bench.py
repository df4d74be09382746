"""Test-time augmentation timing at the full config: ``aug_test`` with 4 views (identity,
horizontal, vertical, both flips) of one 40 000-point scene -- one batched forward plus the
device merge -- against 4 calls of ``simple_test`` (one per view, what the reference's
aug_test runs before its merge), and the BEV NMS launch sequence alone (nms_gpu /
nms_normal_gpu) at n = 1 024 / 4 096 / 8 192.  Times are host clocks around work that ends in
a device synchronise, median of the timed repeats.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nesie_amd.mmdet3d_ops import nms_gpu, nms_normal_gpu
from nesie_amd.scenes import make_batch
from nesie_amd.tta import tta_views
from nesie_amd.votenet import build_nesie_votenet


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 3)


def nms_boxes(n, seed):
    g = torch.Generator().manual_seed(seed)
    side = (n * 0.4) ** 0.5 + 1.0            # each box meets a few others
    c = torch.rand(n, 2, generator=g) * side
    h = 0.2 + torch.rand(n, 2, generator=g) * 0.8
    yaw = (torch.rand(n, 1, generator=g) - 0.5) * 6.3
    return torch.cat([c - h / 2, c + h / 2, yaw], 1), torch.rand(n, generator=g)


def main(reps=20):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = build_nesie_votenet().to(dev).eval()
    pts, _, _ = make_batch(11, 1, num_points=40000)
    views, metas = tta_views(pts[0].to(dev), flips=((False, False), (True, False),
                                                     (False, True), (True, True)))
    res = dict(what='tta_bench', views=4, num_points=40000, reps=reps)
    res['aug_test_ms'] = timed(lambda: model.aug_test(views, metas), reps)
    res['simple_test_x4_ms'] = timed(
        lambda: [model.simple_test(v, m) for v, m in zip(views, metas)], reps)
    res['merged_boxes'] = int(model.aug_test(views, metas)[0]['scores_3d'].shape[0])
    for n in (1024, 4096, 8192):
        b, s = nms_boxes(n, n)
        b, s = b.to(dev), s.to(dev)
        res[f'nms_gpu_{n}_ms'] = timed(lambda: nms_gpu(b, s, 0.25), reps)
        res[f'nms_normal_gpu_{n}_ms'] = timed(lambda: nms_normal_gpu(b, s, 0.25), reps)
        res[f'nms_gpu_{n}_kept'] = int(nms_gpu(b, s, 0.25).shape[0])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
