"""Referee of the sparse convolution tests.  It shares no code with the package.

* ``rulebook``: brute force in Python -- a dict from site to row, the candidate output sites
  collected in a set and sorted -- giving out_indices, nbr, nbr_t and pair_num as
  ``include/nesie_ops.h`` pins them.
* ``Dense``: the layer as a DENSE convolution in torch on the CPU (``conv3d`` /
  ``conv_transpose3d`` of the densified input with the permuted weight, read back at the output
  rows), in float64 for the truth and in float32 for the referee's own rounding error; gradients
  by autograd through that dense form.  The same form on |operands| gives S, the sum of
  |a| * |b| over an element's products, that the a-priori error bound scales with.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(n):
    """(n + 1) u / (1 - (n + 1) u): the a-priori relative bound of an fp32 sum of n products in
    any order, fused or not (Higham, Accuracy and Stability, section 3.1)."""
    n = np.asarray(n, dtype=np.float64)
    return (n + 1) * U / (1 - (n + 1) * U)


def triple(v):
    return [int(e) for e in v] if isinstance(v, (list, tuple)) else [int(v)] * 3


def geometry(shape, ksize, stride, padding, subm):
    """-> ksize, stride, padding as the layer applies them, and the output shape."""
    ksize, stride, padding = triple(ksize), triple(stride), triple(padding)
    if subm:
        stride, padding = [1, 1, 1], [k // 2 for k in ksize]
        return ksize, stride, padding, list(shape)
    out = [(shape[a] + 2 * padding[a] - (ksize[a] - 1) - 1) // stride[a] + 1 for a in range(3)]
    return ksize, stride, padding, out


def rulebook(indices, batch_size, shape, ksize, stride, padding, subm):
    """indices (N, 4) int rows (b, z, y, x), pairwise distinct and inside the grid ->
    out_indices (M, 4) int32, nbr (M, K) int32, nbr_t (N, K) int32, pair_num (K) int32."""
    ksize, stride, padding, out_shape = geometry(shape, ksize, stride, padding, subm)
    rows = [tuple(int(v) for v in r) for r in np.asarray(indices)]
    site_row = {r: i for i, r in enumerate(rows)}
    assert len(site_row) == len(rows), 'the referee takes distinct rows'
    taps = [(kz, ky, kx) for kz in range(ksize[0]) for ky in range(ksize[1])
            for kx in range(ksize[2])]
    if subm:
        outs = rows
    else:
        cand = set()
        for (b, *c) in rows:
            for t in taps:
                v = [c[a] + padding[a] - t[a] for a in range(3)]
                if all(v[a] >= 0 and v[a] % stride[a] == 0 and v[a] // stride[a] < out_shape[a]
                       for a in range(3)):
                    cand.add((b, v[0] // stride[0], v[1] // stride[1], v[2] // stride[2]))
        outs = sorted(cand)
    nbr = np.full((len(outs), len(taps)), -1, np.int32)
    nbr_t = np.full((len(rows), len(taps)), -1, np.int32)
    for o, (b, *c) in enumerate(outs):
        for k, t in enumerate(taps):
            i = site_row.get((b, *(c[a] * stride[a] - padding[a] + t[a] for a in range(3))))
            if i is not None:
                nbr[o, k] = i
                assert nbr_t[i, k] == -1
                nbr_t[i, k] = o
    out_indices = np.asarray(outs, np.int32).reshape(len(outs), 4)
    return out_indices, nbr, nbr_t, (nbr >= 0).sum(0).astype(np.int32)


def rulebook_fast(indices, batch_size, shape, ksize, stride, padding, subm):
    """``rulebook`` in vectorised numpy, for site counts the dict form cannot reach: sites and
    candidate outputs as flat int64 keys, np.unique for the output rows, searchsorted for the
    gather table.  The CPU tests assert that it equals ``rulebook`` exactly."""
    ksize, stride, padding, out_shape = geometry(shape, ksize, stride, padding, subm)
    rows = np.asarray(indices).astype(np.int64).reshape(-1, 4)
    n = len(rows)
    dims_in, dims_out = np.int64(shape), np.int64(out_shape)
    st, pd = np.int64(stride), np.int64(padding)

    def flat(b, c, dims):
        return ((b * dims[0] + c[..., 0]) * dims[1] + c[..., 1]) * dims[2] + c[..., 2]

    site_key = flat(rows[:, 0], rows[:, 1:], dims_in)
    by_key = np.argsort(site_key, kind='stable')
    sorted_key = site_key[by_key]
    assert (sorted_key[1:] != sorted_key[:-1]).all(), 'the referee takes distinct rows'
    taps = np.int64([(kz, ky, kx) for kz in range(ksize[0]) for ky in range(ksize[1])
                     for kx in range(ksize[2])])
    if subm:
        outs = rows
    else:
        v = rows[:, None, 1:] + pd[None, None, :] - taps[None, :, :]            # (N, K, 3)
        ok = ((v >= 0) & (v % st == 0) & (v // st < dims_out)).all(axis=2)
        cand = np.unique(flat(rows[:, None, 0], v // st, dims_out)[ok])
        outs = np.empty((len(cand), 4), dtype=np.int64)
        rest = cand
        for a in (2, 1, 0):
            rest, outs[:, 1 + a] = np.divmod(rest, dims_out[a])
        outs[:, 0] = rest
    m = len(outs)
    site = outs[:, None, 1:] * st[None, None, :] - pd[None, None, :] + taps[None, :, :]   # (M, K, 3)
    inside = ((site >= 0) & (site < dims_in)).all(axis=2)
    want = flat(outs[:, None, 0], site, dims_in)
    at = np.minimum(np.searchsorted(sorted_key, want), max(n - 1, 0))
    hit = inside & (sorted_key[at] == want) if n else np.zeros(want.shape, dtype=bool)
    nbr = np.where(hit, by_key[at] if n else 0, -1).astype(np.int32).reshape(m, len(taps))
    nbr_t = np.full((n, len(taps)), -1, np.int32)
    o, k = np.nonzero(nbr >= 0)
    nbr_t[nbr[o, k], k] = o
    assert len(o) == int((nbr_t >= 0).sum())
    out_indices = outs.astype(np.int32).reshape(m, 4)
    return out_indices, nbr, nbr_t, (nbr >= 0).sum(0).astype(np.int32)


def pair_lists(nbr):
    """The reference's pair lists from the gather table: per tap (input rows, output rows)."""
    out = []
    for k in range(nbr.shape[1]):
        o = np.nonzero(nbr[:, k] >= 0)[0]
        out.append((nbr[o, k].astype(np.int64), o.astype(np.int64)))
    return out


def densify(features, indices, batch_size, shape):
    idx = torch.tensor(np.asarray(indices), dtype=torch.long)
    dense = features.new_zeros((batch_size, features.shape[1], *shape))
    dense[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = features
    return dense


def read_rows(dense, indices):
    idx = torch.tensor(np.asarray(indices), dtype=torch.long)
    return dense[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


def dense_conv(features, indices, batch_size, shape, weight, stride, padding, subm):
    """The dense (B, Cout, Do, Ho, Wo) result of the layer: cross-correlation, weight
    (kz, ky, kx, Cin, Cout)."""
    ksize, stride, padding, _ = geometry(shape, list(weight.shape[:3]), stride, padding, subm)
    dense = densify(features, indices, batch_size, shape)
    return F.conv3d(dense, weight.permute(4, 3, 0, 1, 2), None, stride, padding)


def dense_inverse(features, out_indices, batch_size, shape, weight, stride, padding):
    """The inverse of a regular conv (shape, stride, padding are that conv's): features sit at its
    output sites; -> dense (B, Cout', D, H, W) on its input grid."""
    ksize, stride, padding, out_shape = geometry(shape, list(weight.shape[:3]), stride, padding,
                                                 False)
    dense = densify(features, out_indices, batch_size, out_shape)
    extra = [shape[a] - ((out_shape[a] - 1) * stride[a] - 2 * padding[a] + ksize[a])
             for a in range(3)]
    return F.conv_transpose3d(dense, weight.permute(3, 4, 0, 1, 2), None, stride, padding, extra)


class Dense:
    """One layer application and its gradients by the dense form, in ``dtype``.

    kind 'conv' / 'subm': features at ``indices`` -> rows at ``out_indices``;
    kind 'inverse': features at ``out_indices`` (the partner's outputs) -> rows at ``indices``.
    Attributes: out, and after ``backward(grad_out)``: d_features, d_weight, d_bias."""

    def __init__(self, kind, features, weight, bias, indices, out_indices, batch_size, shape,
                 stride, padding, dtype=torch.float64, absolute=False):
        prep = (lambda t: t.detach().to(dtype).abs()) if absolute else \
            (lambda t: t.detach().to(dtype))
        self.absolute = absolute
        self.features = prep(features).requires_grad_(True)
        self.weight = prep(weight).requires_grad_(True)
        self.bias = None if bias is None else prep(bias).requires_grad_(True)
        if kind == 'inverse':
            dense = dense_inverse(self.features, out_indices, batch_size, shape, self.weight,
                                  stride, padding)
            self.dense, rows = dense, indices
        else:
            dense = dense_conv(self.features, indices, batch_size, shape, self.weight, stride,
                               padding, kind == 'subm')
            self.dense, rows = dense, out_indices
        self.rows = rows
        self.out = read_rows(dense, rows)
        if self.bias is not None:
            self.out = self.out + self.bias
        self.dtype = dtype

    def backward(self, grad_out):
        g = grad_out.detach().to(self.dtype)
        g = g.abs() if self.absolute else g
        wrt = [self.features, self.weight] + ([] if self.bias is None else [self.bias])
        grads = torch.autograd.grad(self.out, wrt, g)
        self.d_features, self.d_weight = grads[0], grads[1]
        self.d_bias = None if self.bias is None else grads[2]
        return self


def off_support_max(dense, rows):
    """max |dense| over the sites that are not in ``rows`` (0 for a regular conv: every reachable
    site is an output row)."""
    mask = torch.ones_like(dense[:, 0], dtype=torch.bool)
    idx = torch.tensor(np.asarray(rows), dtype=torch.long)
    mask[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = False
    picked = dense.permute(0, 2, 3, 4, 1)[mask]
    return float(picked.abs().max()) if picked.numel() else 0.0


def sparse_by_tables(features, weight, table):
    """out[r] = sum_k features[table[r, k]] . W[k] in the dtype of the operands, on the CPU."""
    kvol = table.shape[1]
    w = weight.reshape(kvol, weight.shape[-2], weight.shape[-1])
    out = features.new_zeros((table.shape[0], w.shape[2]))
    for k in range(kvol):
        r = np.nonzero(table[:, k] >= 0)[0]
        if r.size:
            out[torch.as_tensor(r)] += features[torch.as_tensor(table[r, k].astype(np.int64))] @ w[k]
    return out


def random_sites(rng, n, batch_size, shape, faces=True, empty_batch=None):
    """n distinct rows (b, z, y, x) in shuffled order; with ``faces`` the corners of the grid are
    among them (every face holds a site, so padded taps get dropped); ``empty_batch``: a sample
    that gets no site."""
    d, h, w = shape
    cells = batch_size * d * h * w
    batches = [b for b in range(batch_size) if b != empty_batch]
    chosen = set()
    if faces and n >= 2:
        chosen.add((batches[0], 0, 0, 0))
        chosen.add((batches[-1], d - 1, h - 1, w - 1))
    assert n <= len(batches) * d * h * w
    while len(chosen) < n:
        need = n - len(chosen)
        flat = rng.integers(0, cells, size=2 * need + 8)
        for f in flat:
            b, r = divmod(int(f), d * h * w)
            if b == empty_batch:
                continue
            z, r = divmod(r, h * w)
            y, x = divmod(r, w)
            chosen.add((b, z, y, x))
            if len(chosen) == n:
                break
    rows = np.asarray(sorted(chosen), np.int32).reshape(-1, 4)
    return rows[rng.permutation(len(rows))] if len(rows) else rows
