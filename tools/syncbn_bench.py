"""Per-layer cost of the synchronised norm on one GPU.

For each shape: forward and forward + backward time of
  local   FusedBNReLU{1,2}d, the per-rank norm (3 + 5 tensor passes);
  sync    NaiveSyncBatchNorm{1,2}d(relu=True) under a forced one-rank process group
          (NESIE_FORCE_PG=1: the real all-reduces, 3C and 2C doubles, over RCCL);
  kernels the four nesie_syncbn_* entry points in sequence with no collective between them.
Device events around ITERS calls after WARMUP, the three variants alternating within every
round, the median round reported.  One JSON line per shape.

    python tools/syncbn_bench.py [--iters 20] [--rounds 7]
"""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(8, 64, 2048, 64), (8, 128, 1024, 32), (8, 256, 256)]


def timed(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3      # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    os.environ['NESIE_FORCE_PG'] = '1'
    if 'MASTER_PORT' not in os.environ:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            os.environ['MASTER_PORT'] = str(s.getsockname()[1])
    import torch
    import torch.distributed as dist
    from nesie_amd import dp
    from nesie_amd.kernels import HipKernels
    from nesie_amd.mmdet3d_ops import norm as N
    if not torch.cuda.is_available():
        raise SystemExit('syncbn_bench needs a HIP device: a time taken elsewhere says nothing')
    dp.init_distributed()
    assert dist.is_initialized() and dist.get_world_size() == 1
    dev, hip = torch.device('cuda:0'), HipKernels()
    for shape in SHAPES:
        c, two_d = shape[1], len(shape) == 4
        x = (torch.randn(shape, device=dev) * 2 + 3).requires_grad_(True)
        go = torch.randn(shape, device=dev)
        local = (N.FusedBNReLU2d if two_d else N.FusedBNReLU1d)(c, relu=True).to(dev)
        sync = (N.NaiveSyncBatchNorm2d if two_d else N.NaiveSyncBatchNorm1d)(c, relu=True).to(dev)
        xd = x.detach()
        y, dx, coef = torch.empty_like(xd), torch.empty_like(xd), torch.empty(c, 4, device=dev)
        moments = torch.empty(c, 3, dtype=torch.float64, device=dev)
        sums = torch.empty(c, 2, dtype=torch.float64, device=dev)
        dgamma, dbeta = torch.empty(c, device=dev), torch.empty(c, device=dev)

        def kernels_fwd():
            hip.syncbn_local_moments(xd, moments)
            hip.syncbn_forward_apply(xd, moments, sync.weight, sync.bias, sync.running_mean,
                                     sync.running_var, sync.momentum, sync.eps, True, y, coef)

        def kernels_fwd_bwd():
            kernels_fwd()
            hip.syncbn_backward_local(go, xd, coef, moments, sync.eps, True, sums, dgamma, dbeta)
            hip.syncbn_backward_apply(go, xd, coef, sync.weight, sums, moments, sync.eps, True, dx)

        def module_fwd(layer):
            with torch.no_grad():
                layer(xd)

        def module_fwd_bwd(layer):
            x.grad = None
            layer(x).backward(go)

        variants = {
            'local_fwd': lambda: module_fwd(local), 'sync_fwd': lambda: module_fwd(sync),
            'kernels_fwd': kernels_fwd,
            'local_fwd_bwd': lambda: module_fwd_bwd(local), 'sync_fwd_bwd': lambda: module_fwd_bwd(sync),
            'kernels_fwd_bwd': kernels_fwd_bwd,
        }
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.iters))
        numel = x.numel()
        res = dict(shape=list(shape), tensor_mb=round(numel * 4 / 2 ** 20, 1), unit='us per call',
                   iters=args.iters, rounds=args.rounds)
        for k, v in times.items():
            res[k] = round(statistics.median(v), 1)
            res[k + '_spread'] = [round(min(v), 1), round(max(v), 1)]
        # bytes the passes must move: 3 tensor passes forward, 3 + 5 forward + backward
        res['kernels_fwd_tb_s'] = round(3 * numel * 4 / res['kernels_fwd'] / 1e6, 2)
        res['kernels_fwd_bwd_tb_s'] = round(8 * numel * 4 / res['kernels_fwd_bwd'] / 1e6, 2)
        print(json.dumps(res), flush=True)
        del x, go, y, dx, xd
        torch.cuda.empty_cache()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
