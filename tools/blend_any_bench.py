"""nesie_blend_conv_backward_any against nesie_blend_conv_backward_staged: HIP events around ONE
call (workspace allocation and index build included), the two entries alternating in the same
process, median of 20 after 5 warm-ups.  Cases: the reference side-face shape (b = 8, c = 256,
m = 1024, n = 512 * 6 * 16) with the taps of nesie_grid_taps on a scenes.make_batch scene; the same
shape with 70 % of the taps on 3 seeds; a SAQE-like shape (c = 128, n = 200 * 6 * 27) that only the
general entry serves.  Every case runs in a child process under its own time limit; the first
failure ends the run.
usage: python tools/blend_any_bench.py            (all cases)
       python tools/blend_any_bench.py CASE       (one case, in this process)"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ('side', 'side_skewed', 'saqe')
LIMIT = 120      # seconds per case


def face_grid(g, planes):
    """Box-frame multipliers of the six face groups of a g^3 grid (SidePooling._register_grid_tables)."""
    import torch
    step = torch.linspace(-1, 1, g)
    full = torch.stack([step.view(g, 1, 1).expand(g, g, g), step.view(1, g, 1).expand(g, g, g),
                        step.view(1, 1, g).expand(g, g, g)], -1).reshape(-1, 3)
    left = [i // g * g * g + i % g for i in range(g * g)]
    right = [i + g * (g - 1) for i in left]
    face_idx = (list(range(0, g * g)) + list(range(g ** 3 - g * g, g ** 3))
                + list(range(g - 1, g ** 3, g)) + list(range(0, g ** 3, g)) + left + right)
    side = full[torch.tensor(face_idx)]
    if not planes:
        return side.contiguous(), torch.zeros_like(side)
    g2 = g * g
    axes = torch.zeros(6, 3)
    for f, a in enumerate((0, 0, 2, 2, 1, 1)):
        axes[f, a] = 0.1
    side = side.view(6, g2, 3)
    pl = axes.view(6, 1, 3).expand(6, g2, 3)
    return (torch.cat([side, side, side], 1).reshape(-1, 3).contiguous(),
            torch.cat([-pl, torch.zeros_like(pl), pl], 1).reshape(-1, 3).contiguous())


def run(case):
    import torch
    from nesie_amd import kernels
    from nesie_amd.scenes import make_batch
    dev = torch.device('cuda:0')
    hip = kernels.backend_for(torch.empty(1, device=dev))
    B, m = 8, 1024
    c, K, g, planes = (128, 200, 3, True) if case == 'saqe' else (256, 512, 4, False)
    segs, G = 6, g * g * (3 if planes else 1)
    n = K * segs * G
    gen = torch.Generator().manual_seed(0)
    pts = make_batch(11, B, num_points=8192)[0][:, :, :3]
    known = pts[:, torch.randperm(pts.shape[1], generator=gen)[:m]].contiguous().to(dev)
    centre = known[:, torch.randperm(m, generator=gen)[:K]].contiguous()
    size = (0.4 + 1.6 * torch.rand(B, K, 3, generator=gen)).to(dev)
    heading = ((torch.rand(B, K, generator=gen) - 0.5) * 6.28318).to(dev)
    mult, plane = face_grid(g, planes)
    idx, w, rel = hip.grid_taps(centre, size, heading, mult.to(dev), plane.to(dev), known)
    assert tuple(idx.shape) == (B, n, 3)
    if case == 'side_skewed':
        hot = torch.randint(0, 3, (B, n, 3), generator=gen, dtype=torch.int32).to(dev)
        idx = torch.where(torch.rand(B, n, 3, generator=gen).to(dev) < 0.7, hot, idx).contiguous()
    dy = torch.randn(B, segs, c, K * G, generator=gen).to(dev)
    d_table = torch.empty(B, m, segs * c, device=dev)
    d_wx = torch.empty(segs, c, 3, device=dev)
    calls = dict(any=lambda: hip.blend_conv_backward_any(dy, c, idx, w, rel, d_table, d_wx, segs, G))
    if kernels.blend_backward_form(c, n // segs, m, True) == 'staged':
        prev = hip.set_deterministic(True)
        calls['staged'] = lambda: hip.blend_conv_backward(dy, c, idx, w, rel, d_table, d_wx, segs, G)

    def once(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3                   # us

    times = {k: [] for k in calls}
    for it in range(25):
        for k, fn in calls.items():
            t = once(fn)
            if it >= 5:
                times[k].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    taps = torch.bincount(idx[0].long().flatten(), minlength=m)
    line = (f'{case}: b={B} c={c} m={m} n={n} (max taps on one seed {int(taps.max())}): '
            f'any {med["any"]:.1f} us (min {min(times["any"]):.1f})')
    if 'staged' in med:
        line += (f', staged {med["staged"]:.1f} us (min {min(times["staged"]):.1f}), '
                 f'ratio any/staged {med["any"] / med["staged"]:.2f}')
    print(line, flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for case in CASES:
            r = subprocess.run(['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__), case])
            if r.returncode != 0:
                sys.exit(f'{case}: exit status {r.returncode}; stopping')
