"""Float64 referee of PAConv's ``assign_score_withk`` (include/nesie_ops.h states the operator).
Shares no code with the package: explicit gathers, ``einsum`` and ``index_add_`` in torch float64
on whatever device the inputs live on.

Besides the values it returns, per output element, ``S`` = the same expression on absolute
operands and ``n`` = the element's own number of products, subtractions and additions, so that a
test can hold a float32 result to the a-priori bound  |got - f64| <= gamma_n * S,
gamma_n = n u / (1 - n u)  (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: any
order of the sum, fused or not, stays inside it).  An element with n == 0 must be exactly zero.
"""
import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n, u=U32):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * u / (1.0 - n * u)


def _gathered(points, centers, knn_idx):
    """-> valid (B,N1,K) bool, centre_valid (B,N1) bool, kn, cn (clamped, int64),
    P[kn] (B,N1,K,M,O) and C[cn] (B,N1,M,O), the latter zero where the centre index is invalid."""
    B, N0 = points.shape[:2]
    idx = knn_idx.long()
    valid = (idx >= 0) & (idx < N0)
    kn = torch.where(valid, idx, torch.zeros_like(idx))
    cn, cvalid = kn[:, :, 0], valid[:, :, 0]
    batch = torch.arange(B, device=points.device)
    gp = points.double()[batch[:, None, None], kn]
    gc = centers.double()[batch[:, None], cn] * cvalid[:, :, None, None]
    return valid, cvalid, kn, cn, gp, gc


def forward(points, centers, scores, knn_idx):
    """-> dict(out (B,O,N1,K) float64, S, n)."""
    M = points.shape[2]
    valid, cvalid, _, _, gp, gc = _gathered(points, centers, knn_idx)
    mask = valid[..., None, None].double()
    diff = (gp - gc[:, :, None]) * mask
    mag = (gp.abs() + gc.abs()[:, :, None]) * mask
    s = scores.double()
    out = torch.einsum('bnkm,bnkmo->bonk', s, diff)
    S = torch.einsum('bnkm,bnkmo->bonk', s.abs(), mag)
    # per m: a product, a subtraction where there is a centre row, and all but the first an addition
    n = valid * (M * (2 + cvalid[:, :, None].long()) - 1)
    return dict(out=out, S=S, n=n[:, None].expand_as(out))


def backward(points, centers, scores, knn_idx, grad_out):
    """-> dict of grad_scores (B,N1,K,M), grad_points, grad_centers (B,N0,M,O) in float64, each
    with its S_* and n_*."""
    B, N0, M, O = points.shape
    valid, cvalid, kn, cn, gp, gc = _gathered(points, centers, knn_idx)
    mask = valid[..., None, None].double()
    diff = (gp - gc[:, :, None]) * mask
    mag = (gp.abs() + gc.abs()[:, :, None]) * mask
    s = scores.double()
    g = grad_out.double().permute(0, 2, 3, 1)                      # (B, N1, K, O)
    res = dict(grad_scores=torch.einsum('bnkmo,bnko->bnkm', diff, g),
               S_scores=torch.einsum('bnkmo,bnko->bnkm', mag, g.abs()))
    n_scores = valid * (O * (2 + cvalid[:, :, None].long()) - 1)
    res['n_scores'] = n_scores[..., None].expand_as(res['grad_scores'])

    prod = torch.einsum('bnkm,bnko->bnkmo', s, g) * mask           # every pair's contribution
    mag_prod = torch.einsum('bnkm,bnko->bnkmo', s.abs(), g.abs()) * mask
    zeros = lambda: torch.zeros(B, N0, M, O, dtype=torch.float64, device=points.device)
    count = lambda: torch.zeros(B, N0, dtype=torch.long, device=points.device)
    gpts, S_pts, L_pts = zeros(), zeros(), count()
    gctr, S_ctr, L_ctr = zeros(), zeros(), count()
    per_centre = valid.sum(-1) * cvalid                            # pairs that reach the centre row
    cmask = cvalid[:, :, None, None].double()
    for b in range(B):
        flat = kn[b].reshape(-1)
        gpts[b].index_add_(0, flat, prod[b].reshape(-1, M, O))
        S_pts[b].index_add_(0, flat, mag_prod[b].reshape(-1, M, O))
        L_pts[b].index_add_(0, flat, valid[b].reshape(-1).long())
        gctr[b].index_add_(0, cn[b], -(prod[b].sum(1) * cmask[b]))
        S_ctr[b].index_add_(0, cn[b], mag_prod[b].sum(1) * cmask[b])
        L_ctr[b].index_add_(0, cn[b], per_centre[b])
    ops = lambda L: (2 * L - 1).clamp_(min=0)[:, :, None, None].expand(B, N0, M, O)
    res.update(grad_points=gpts, S_points=S_pts, n_points=ops(L_pts),
               grad_centers=gctr, S_centers=S_ctr, n_centers=ops(L_ctr))
    return res


def check(label, got, want, S, n, u=U32):
    """Assert |got - want| <= gamma_n * S for EVERY element; -> the worst fraction of the bound
    used (0 where the bound is 0 and met).  Prints the fraction before it asserts."""
    got = got.double()
    assert got.shape == want.shape, (label, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), f'{label}: non-finite values'
    err = (got - want).abs()
    bound = gamma(n, u).to(err.device) * S
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(frac.max()) if frac.numel() else 0.0
    print(f'{label}: worst fraction of the bound {worst:.4f} over {err.numel()} elements')
    over = err > bound
    assert not over.any(), (f'{label}: {int(over.sum())} of {err.numel()} elements over the bound, '
                            f'worst error {float(err[over].max()):.3e}, fraction {worst:.3f}')
    return worst
