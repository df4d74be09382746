"""``FocalLoss`` (mean-reduced, one weight per row) at four sizes: (2048, 2) and (2048, 18), the
objectness and semantic terms of the indoor head at B = 8, K = 256; (844 800, 3), a 200 x 176 x 6
anchor grid at B = 4; (2 500 000, 10).  Forward and forward + backward of the module on the HIP
kernels, each beside the yardstick on the same device: the same stable formulas in torch ops
(``py_sigmoid_focal_loss``, what the module runs for every other dtype), backward by autograd.

HIP events around ``--calls`` back-to-back calls, ``--repeats`` windows after ``--warmup`` untimed
ones, the two variants alternating inside every repeat; prints the median, min and max per call and
the bytes each direction must move at the least (logits in, 8 B of label and 4 B of weight per row;
the backward reads the logits again and writes the gradient).  After the timings, one row per size
with the number of device kernels each side launches, counted by the profiler (null where the
profiler does not report device activity).  A first measurement: nothing passes or fails on it.
Needs a HIP device; reads nothing but this repository.
usage: python tools/focal_bench.py [--calls 20] [--repeats 10] [--only 2048x18]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nesie_amd.votenet.losses import FocalLoss, py_sigmoid_focal_loss  # noqa: E402

SHAPES = [(2048, 2), (2048, 18), (844800, 3), (2500000, 10)]
GAMMA, ALPHA = 2.0, 0.25


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


def device_kernels(fn):
    """Kernels one call of ``fn`` puts on the device, or None when the profiler sees none."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    count = sum(1 for e in prof.events()
                if getattr(e, 'device_type', None) == torch.autograd.DeviceType.CUDA
                and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    return count or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, help='one size, e.g. 2048x18')
    ap.add_argument('--no-launch-count', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('focal_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    module = FocalLoss(gamma=GAMMA, alpha=ALPHA, reduction='mean')
    cases = {}
    for n, c in SHAPES:
        if args.only and args.only != f'{n}x{c}':
            continue
        gen = torch.Generator().manual_seed(n + c)
        x = (torch.randn(n, c, generator=gen) * 3).to(dev).requires_grad_(True)
        t = torch.randint(0, c + 1, (n,), generator=gen).to(dev)
        w = torch.rand(n, generator=gen).to(dev)
        onehot = t.view(-1, 1) == torch.arange(c, device=dev)

        ours = lambda x=x, t=t, w=w: module(x, t, w)
        ref = lambda x=x, w=w, onehot=onehot: py_sigmoid_focal_loss(x, onehot, w, GAMMA, ALPHA, 'mean')
        ours_bwd = lambda ours=ours, x=x: torch.autograd.grad(ours(), x)
        ref_bwd = lambda ref=ref, x=x: torch.autograd.grad(ref(), x)
        cases[(n, c)] = (ours, ref, ours_bwd, ref_bwd)

        row = dict(n=n, c=c, gamma=GAMMA, alpha=ALPHA,
                   max_abs_grad_diff_to_yardstick=float((ours_bwd()[0] - ref_bwd()[0]).abs().max()))
        with torch.no_grad():
            row.update(rel_diff_to_yardstick=float(((ours() - ref()) / ref()).abs()))
            row.update(measure({'forward': ours, 'yardstick_forward': ref}, args))
        row.update(measure({'forward+backward': ours_bwd, 'yardstick_forward+backward': ref_bwd}, args))
        fwd_bytes = 4 * n * c + 12 * n
        row.update(min_bytes_forward=fwd_bytes, min_bytes_forward_backward=2 * fwd_bytes + 4 * n * c)
        print(json.dumps(row), flush=True)
    if args.no_launch_count:
        return
    for (n, c), (ours, ref, ours_bwd, ref_bwd) in cases.items():
        row = dict(n=n, c=c)
        with torch.no_grad():
            row.update(kernels_forward=device_kernels(ours), yardstick_kernels_forward=device_kernels(ref))
        row.update(kernels_forward_backward=device_kernels(ours_bwd),
                   yardstick_kernels_forward_backward=device_kernels(ref_bwd))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
