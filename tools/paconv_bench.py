"""``assign_score_withk`` at the four set-abstraction levels of the PAConv SSG backbone: npoint
1024 / 256 / 64 / 16 centres among 4096 / 1024 / 256 / 64 points, K = 32 neighbours, M = 16 bank
kernels, output widths 32 .. 512 (``--batch`` scenes, 8 by default).  Forward and forward +
backward (all three gradients) of the op, each beside the yardstick on the same device: the
reference's own non-kernel formulation in torch ops -- gather the transformed features of every
pair, subtract the centre's, then ``assign_score`` (the algorithm ``PAConv`` runs), backward by
autograd.  The yardstick has to form the (B, npoint, K, M, O) operand the op exists to avoid, so
both sides' peak memory above the inputs is reported too.

HIP events around ``--calls`` back-to-back calls, ``--repeats`` windows after ``--warmup`` untimed
ones, the two variants alternating inside every repeat; prints the median, min and max per call,
the bytes each direction must move at the least (every operand once; the gathered rows once per
pair when nothing is reused on chip) and the FLOPs.  A first measurement: nothing passes or fails
on it.  Needs a HIP device; reads nothing but this repository.
usage: python tools/paconv_bench.py [--batch 8] [--calls 5] [--repeats 10] [--only sa1]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nesie_amd.mmdet3d_ops.paconv import assign_score_withk  # noqa: E402
from nesie_amd.mmdet3d_ops.paconv.utils import assign_score  # noqa: E402

K, M = 32, 16
# level: (points N0, centres N1, output widths of the level's layers)
LEVELS = {
    'sa1': (4096, 1024, (32, 64)),
    'sa2': (1024, 256, (64, 128)),
    'sa3': (256, 64, (128, 256)),
    'sa4': (64, 16, (256, 512)),
}


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


def peak_above_inputs(fn):
    """MiB the call allocates at its peak on top of what is live before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    result = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del result
    return round((peak - before) / 2 ** 20, 1)


def neighbourhoods(b, n0, n1, gen):
    """(B, N1, K) int64: every row starts with its centre, then K - 1 points of a window of 4 K
    consecutive indices around it (neighbours of a spatially sorted cloud are near in index, and
    each point is referenced about K * N1 / N0 times)."""
    centre = torch.sort(torch.randperm(n0, generator=gen)[:n1])[0].view(1, n1, 1).expand(b, n1, 1)
    near = torch.randint(-2 * K, 2 * K, (b, n1, K - 1), generator=gen)
    return torch.cat([centre, (centre + near).clamp_(0, n0 - 1)], dim=2).contiguous()


def yardstick(scores, points, centers, idx):
    """(B, O, N1, K) the way the reference's PAConv gets there: group, subtract, assign_score."""
    b = points.shape[0]
    batch = torch.arange(b, device=points.device)
    grouped = points[batch[:, None, None], idx] - centers[batch[:, None], idx[:, :, 0]][:, :, None]
    return assign_score(scores, grouped).permute(0, 3, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, help='one level of ' + ', '.join(LEVELS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('paconv_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    b = args.batch
    for name, (n0, n1, widths) in LEVELS.items():
        if args.only and name != args.only:
            continue
        for o in widths:
            gen = torch.Generator().manual_seed(n0 + o)
            leaf = lambda *s: torch.randn(*s, generator=gen).to(dev).requires_grad_(True)
            points, centers = leaf(b, n0, M, o), leaf(b, n0, M, o)
            scores = torch.softmax(torch.randn(b, n1, K, M, generator=gen), -1).to(dev).requires_grad_(True)
            idx = neighbourhoods(b, n0, n1, gen).to(dev)
            g_out = torch.randn(b, o, n1, K, generator=gen).to(dev)
            leaves = (scores, points, centers)

            ours = lambda: assign_score_withk(scores, points, centers, idx, 'sum')
            ref = lambda: yardstick(scores, points, centers, idx)
            ours_bwd = lambda: torch.autograd.grad(ours(), leaves, g_out)
            ref_bwd = lambda: torch.autograd.grad(ref(), leaves, g_out)

            with torch.no_grad():
                worst = float((ours() - ref()).abs().max())
            row = dict(level=name, batch=b, n0=n0, n1=n1, k=K, m=M, o=o,
                       max_abs_diff_to_yardstick=worst)
            with torch.no_grad():
                row.update(measure({'forward': ours, 'yardstick_forward': ref}, args))
                row.update(peak_mib_forward=peak_above_inputs(ours),
                           yardstick_peak_mib_forward=peak_above_inputs(ref))
            row.update(measure({'forward+backward': ours_bwd,
                                'yardstick_forward+backward': ref_bwd}, args))
            row.update(peak_mib_backward=peak_above_inputs(ours_bwd),
                       yardstick_peak_mib_backward=peak_above_inputs(ref_bwd))
            pairs = b * n1 * K
            table = 4 * b * n0 * M * o                     # one of points / centers, bytes
            row.update(
                pairs=pairs,
                flops_forward=3 * pairs * M * o,           # a subtraction and an fma per (pair, m, o)
                flops_backward=(3 + 2 + 2) * pairs * M * o,
                # every operand once: both tables, scores, indices in; the output out
                algorithmic_bytes_forward=2 * table + 4 * pairs * M + 8 * pairs + 4 * pairs * o,
                # what the gather reads when no row is reused on chip: one table row per pair and
                # one centre row per centre
                gathered_bytes_forward=4 * (pairs + b * n1) * M * o,
                # grad_out, scores, both tables in; three gradients out
                algorithmic_bytes_backward=4 * pairs * o + 4 * pairs * M + 2 * table
                + 2 * table + 4 * pairs * M,
                intermediate_mib_avoided=round(4 * pairs * M * o / 2 ** 20, 1))
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
