"""``lovasz_softmax`` ('present', 20 % void labels) at two sizes: 8 x 40 000 points x 20 classes, a
batch of full indoor scenes through a PointNet++ decoder, and 1 x 40 000 x 20, one scene.  Forward
and forward + backward on the HIP kernels (``csrc/lovasz.hip``: the forward call produces the
gradient, the backward is one multiplication), each beside the yardstick on the same device: the
same closed form and tie rule in torch ops (``lovasz_softmax_torch``: one batched stable sort,
cumsum and scatter over all classes -- already far fewer launches than the reference's per-class
chains).  ``--per-image`` measures the per-image segmentation instead.

HIP events around ``--calls`` back-to-back calls, ``--repeats`` windows after ``--warmup`` untimed
ones, the two variants alternating inside every repeat; prints the median, min and max per call and
the peak device memory one call of each side allocates beyond its inputs.  A first measurement:
nothing passes or fails on it.  Needs a HIP device; reads nothing but this repository.
usage: python tools/lovasz_bench.py [--calls 10] [--repeats 10] [--only 8x20x40000] [--per-image]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nesie_amd.mmdet3d_ops import lovasz as LV  # noqa: E402

SHAPES = [(8, 20, 40000), (1, 20, 40000)]
VOID = 255


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


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--only', default=None, help='one size, e.g. 8x20x40000')
    ap.add_argument('--per-image', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lovasz_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    for b, c, s in SHAPES:
        if args.only and args.only != f'{b}x{c}x{s}':
            continue
        gen = torch.Generator().manual_seed(b + c + s)
        x = torch.softmax(torch.randn(b, c, s, generator=gen) * 3, dim=1).to(dev).requires_grad_(True)
        t = torch.randint(0, c, (b, s), generator=gen)
        t[torch.rand(b, s, generator=gen) < 0.2] = VOID
        t = t.to(dev)
        mode = LV.CLASS_MODES['present']
        upstream = torch.ones((), device=dev)

        ours = lambda: LV.lovasz_softmax_op(x, t, 'present', args.per_image, VOID)
        ref = lambda: LV.lovasz_softmax_torch(x, t, args.per_image, VOID, mode)[0]
        ours_bwd = lambda: torch.autograd.grad(ours(), x)[0]

        def ref_bwd():
            loss, grad = LV.lovasz_softmax_torch(x, t, args.per_image, VOID, mode)
            return grad * upstream

        g_ours, g_ref = ours_bwd(), ref_bwd()
        row = dict(images=b, classes=c, points=s, per_image=args.per_image, entries=b * c * s,
                   max_abs_grad_diff_to_yardstick=float((g_ours - g_ref).abs().max()))
        del g_ours, g_ref
        with torch.no_grad():
            row.update(rel_diff_to_yardstick=float(((ours() - ref()) / ref()).abs()))
            row.update(measure({'forward': ours, 'yardstick_forward': ref}, args))
        row.update(measure({'forward+backward': ours_bwd, 'yardstick_forward+backward': ref_bwd}, args))
        row.update(peak_bytes_forward_backward=peak_bytes(ours_bwd),
                   yardstick_peak_bytes_forward_backward=peak_bytes(ref_bwd),
                   workspace_bytes=LV.backend_for(x).lovasz_softmax_workspace_bytes(b, c, s))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
