"""Sparse 3-D convolution at the sizes a voxel detector runs: a LiDAR-sized grid
(41 x 1600 x 1408, 60 000 and 120 000 active voxels; submanifold 16->16, 32->32, 64->64, 128->128
and stride-2 16->32, 32->64, all 3 x 3 x 3) and this project's room (60 x 160 x 160, 40 000 active
voxels).  Per layer: the rulebook build (both phases and the one host read), forward, and
forward + backward (input and weight gradient), each beside the yardstick on the same device: the
reference's algorithm restated in torch ops -- per tap ``index_select``, ``mm``, ``index_add_``,
backward by autograd -- fed from pair lists that sit on the device before the clock starts (they
are read off this build's own tables, which tests/test_spconv_gpu.py proves equal to the brute-force
referee's).  HIP events around ``--calls`` back-to-back calls, ``--repeats`` windows after
``--warmup`` untimed ones, the variants alternating inside every repeat; prints the median, min and
max per call, the pair count, the FLOPs (2 * pairs * Cin * Cout) and the bytes each must move
(computed from the shapes and the counts, not measured).  Needs a HIP device; reads nothing but
this repository.
usage: python tools/spconv_bench.py [--calls 5] [--repeats 10] [--only lidar60k] [--order shuffled]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nesie_amd.mmdet3d_ops import spconv  # noqa: E402
from nesie_amd.mmdet3d_ops.spconv import ops  # noqa: E402

SUBM = [(16, 16), (32, 32), (64, 64), (128, 128)]
DOWN = [(16, 32), (32, 64)]
WORKLOADS = {
    'lidar60k': dict(shape=[41, 1600, 1408], voxels=60000, subm=SUBM, down=DOWN),
    'lidar120k': dict(shape=[41, 1600, 1408], voxels=120000, subm=SUBM, down=DOWN),
    'room40k': dict(shape=[60, 160, 160], voxels=40000, subm=[(16, 16), (64, 64)],
                    down=[(16, 32)]),
}


def active_sites(shape, n, seed, order):
    """n distinct (0, z, y, x) rows as a scan leaves them: horizontal sheets and vertical walls a
    voxel thick inside a square of side sqrt(n / 5), denser towards one corner, so that a
    3 x 3 x 3 stencil meets about five sites.  ``order``: 'sorted' = lexicographic, the order
    DynamicScatter and a regular sparse conv emit; 'shuffled' = no locality between rows."""
    g = torch.Generator().manual_seed(seed)
    d, h, w = shape
    side = min(h, w, int((n / 5) ** 0.5))
    rows = torch.zeros(0, 3, dtype=torch.long)
    while len(rows) < n:
        m = 2 * n
        y = (torch.rand(m, generator=g) ** 1.5 * side).long()
        x = (torch.rand(m, generator=g) ** 1.5 * side).long()
        z = torch.randint(0, d, (m,), generator=g)
        sheet = torch.rand(m, generator=g) < 0.6
        z[sheet] = (z[sheet] // 8) * 8 % d                       # floors
        wall = ~sheet
        x[wall] = (x[wall] // 16) * 16                           # walls
        rows = torch.unique(torch.cat([rows, torch.stack([z, y, x], 1)]), dim=0)
    rows = rows[torch.randperm(len(rows), generator=g)[:n]]
    if order == 'sorted':
        rows = torch.unique(rows, dim=0)
    return torch.cat([torch.zeros(n, 1, dtype=torch.long), rows], 1).int()


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


def pair_lists(nbr):
    """Per tap (input rows, output rows) int64 on the device, from the gather table."""
    out = []
    for k in range(nbr.shape[1]):
        o = torch.nonzero(nbr[:, k] >= 0).flatten()
        out.append((nbr[o, k].long(), o))
    return out


def yardstick(feats, weight, pairs, m):
    """The reference's gather - GEMM - scatter-add per tap, in torch ops."""
    w = weight.reshape(len(pairs), weight.shape[-2], weight.shape[-1])
    out = feats.new_zeros((m, w.shape[2]))
    for k, (i, o) in enumerate(pairs):
        if len(i):
            out.index_add_(0, o, feats.index_select(0, i) @ w[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--order', default='sorted', choices=['sorted', 'shuffled'],
                    help='row order of the input sites')
    ap.add_argument('--only', default=None, help='one workload of ' + ', '.join(WORKLOADS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spconv_bench needs a HIP device: a CPU run measures nothing')
    dev = torch.device('cuda:0')
    for name, cfg in WORKLOADS.items():
        if args.only and name != args.only:
            continue
        shape, n = cfg['shape'], cfg['voxels']
        idx = active_sites(shape, n, 7, args.order).to(dev)
        for subm, pairs_of in ((True, cfg['subm']), (False, cfg['down'])):
            geo = dict(ksize=3, stride=1 if subm else 2, padding=1, subm=subm)
            build = measure({'rulebook': lambda: ops.get_indice_pairs(idx, 1, shape, **geo)}, args)
            outids, rules, pair_num = ops.get_indice_pairs(idx, 1, shape, **geo)
            m, kvol, total = int(outids.shape[0]), rules.kvol, int(pair_num.sum())
            lists = pair_lists(rules.nbr)
            entry = (outids, idx, rules, pair_num, shape)
            # the sort moves (key, index) pairs: count, read, write per 8-bit pass
            cells_in = shape[0] * shape[1] * shape[2]
            passes = (cells_in.bit_length() + 7) // 8
            sorted_elems = n if subm else n + n * kvol
            print(json.dumps(dict(
                workload=name, order=args.order, layer='subm3' if subm else 'conv3s2', voxels=n,
                out_voxels=m, pairs=total, pairs_per_output=round(total / max(m, 1), 2), **build,
                algorithmic_bytes_rulebook=16 * n + passes * 20 * sorted_elems
                + 4 * kvol * (n + m) + 16 * m)))
            for cin, cout in pairs_of:
                torch.manual_seed(1)
                cls = spconv.SubMConv3d if subm else spconv.SparseConv3d
                layer = cls(cin, cout, 3, 1 if subm else 2, 1, bias=False, indice_key='k').to(dev)
                feats = torch.randn(n, cin, device=dev, requires_grad=True)
                g_out = torch.randn(m, cout, device=dev)

                def ours():
                    x = spconv.SparseConvTensor(feats, idx, shape, 1)
                    x.indice_dict['k'] = entry
                    return layer(x).features

                def ours_bwd():
                    return torch.autograd.grad(ours(), (feats, layer.weight), g_out)

                def ref():
                    return yardstick(feats, layer.weight, lists, m)

                def ref_bwd():
                    return torch.autograd.grad(ref(), (feats, layer.weight), g_out)

                with torch.no_grad():
                    worst = float((ours() - ref()).abs().max())
                row = dict(workload=name, layer='subm3' if subm else 'conv3s2', cin=cin, cout=cout,
                           voxels=n, out_voxels=m, pairs=total, max_abs_diff_to_yardstick=worst)
                with torch.no_grad():
                    row.update(measure({'forward': ours, 'yardstick_forward': ref}, args))
                row.update(measure({'forward+backward': ours_bwd,
                                    'yardstick_forward+backward': ref_bwd}, args))
                w_bytes = 4 * kvol * cin * cout
                row.update(
                    flops_forward=2 * total * cin * cout,
                    flops_backward=4 * total * cin * cout,
                    # each operand once: features in, rows out, weight, table
                    algorithmic_bytes_forward=4 * (n * cin + m * cout) + w_bytes + 4 * m * kvol,
                    # dIn: dOut in, dIn out, weight, nbr_t; dW: features and dOut in, dW out, nbr
                    algorithmic_bytes_backward=4 * (m * cout + n * cin) + w_bytes + 4 * n * kvol
                    + 4 * (n * cin + m * cout) + w_bytes + 4 * m * kvol,
                    # what the gather itself reads when no row is reused on chip
                    gathered_bytes_forward=4 * total * cin)
                print(json.dumps(row))


if __name__ == '__main__':
    main()
