"""The blend forward restated in float32 torch on the CPU, rounding by rounding as the HIP tile
kernel does it (nesie_amd/csrc/interpolate.hip, blend_fwd_kernel):

  v = (w0 * a0 + w1 * a1) + w2 * a2            every product rounded on its own (separate mul / add)
  v = ((v + x0 * r0) + x1 * r1) + x2 * r2      with wx
  per (channel, 64-query tile): for each 16-query quarter, from 0 with q ascending, s += v and
  ss += v * v; the quarters combine as (0 + 1) + (2 + 3).

Separate elementwise torch ops round once each, and torch never contracts across two ops, so the
result is what the kernel must give bit for bit."""
import torch


def make_case(k, segs, g, c, m, b, seed, with_wx=True, pitch=None, seg_off=None, edge_taps=True):
    """Seeded inputs on the CPU.  edge_taps: some taps are -1 and m (the kernels clamp them)."""
    gen = torch.Generator().manual_seed(seed)
    n = k * segs * g
    seg_off = c if seg_off is None else seg_off
    pitch = ((segs - 1) * seg_off + c) if pitch is None else pitch
    idx = torch.randint(0, m, (b, n, 3), generator=gen, dtype=torch.int32)
    if edge_taps:
        where = torch.rand(b, n, 3, generator=gen)
        idx[where < 0.05] = -1
        idx[where > 0.95] = m
    w = torch.rand(b, n, 3, generator=gen)
    w = (w / w.sum(-1, keepdim=True)).contiguous()
    table = torch.randn(b, m, pitch, generator=gen)
    rel = torch.randn(b, n, 3, generator=gen) if with_wx else None
    wx = torch.randn(segs, c, 3, generator=gen) if with_wx else None
    return dict(k=k, segs=segs, g=g, c=c, m=m, b=b, n=n, pitch=pitch, seg_off=seg_off, idx=idx,
                weight=w, table=table, rel=rel, wx=wx)


def blend_forward_ref(case):
    """-> out (B, segs, c, K * g) float32."""
    b, k, segs, g, c, m = (case[x] for x in ('b', 'k', 'segs', 'g', 'c', 'm'))
    per_seg = k * g
    j = case['idx'].long().clamp(0, m - 1).view(b, k, segs, g, 3)
    w = case['weight'].view(b, k, segs, g, 3)
    out = torch.empty(b, segs, c, per_seg)
    for s in range(segs):
        T = case['table'][:, :, s * case['seg_off']:s * case['seg_off'] + c]      # (b, m, c)
        js, ws = j[:, :, s].reshape(b, per_seg, 3), w[:, :, s].reshape(b, per_seg, 3)
        a = [torch.gather(T, 1, js[:, :, t, None].expand(-1, -1, c)) for t in range(3)]
        p = [ws[:, :, t, None] * a[t] for t in range(3)]
        v = (p[0] + p[1]) + p[2]
        if case['wx'] is not None:
            r = case['rel'].view(b, k, segs, g, 3)[:, :, s].reshape(b, per_seg, 3)
            x = case['wx'][s]                                                      # (c, 3)
            for d in range(3):
                v = v + x[None, None, :, d] * r[:, :, d, None]
        out[:, s] = v.transpose(1, 2)
    return out


def blend_stats_ref(out):
    """out (B, segs, c, per_seg) -> partial (segs * c, B * per_seg / 64, 2): bn.hip's slot layout,
    slot = b * (per_seg / 64) + tile."""
    b, segs, c, per_seg = out.shape
    tiles = per_seg // 64
    v = out.view(b, segs, c, tiles, 4, 16)
    s = torch.zeros(b, segs, c, tiles, 4)
    q = torch.zeros(b, segs, c, tiles, 4)
    for i in range(16):
        s = s + v[..., i]
        q = q + v[..., i] * v[..., i]
    s = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    q = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    both = torch.stack([s, q], -1)                                    # (b, segs, c, tiles, 2)
    return both.permute(1, 2, 0, 3, 4).reshape(segs * c, b * tiles, 2).contiguous()
