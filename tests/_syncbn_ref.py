"""The float64 referee of the synchronised norm: BatchNorm (+ ReLU) over the CONCATENATION of all
ranks' shards, forward and closed-form backward, and the bounds the sync tests hold it to.

The running variance takes the biased variance (reference mmdet3d/ops/norm.py:68-71).  The ReLU
mask is taken from the fp32 output under test (tests/test_kernels_gpu.py::
test_fused_bn_relu_matches_aten says why the mask must be shared).  A shard's dgamma / dbeta are
sums over that shard only: the flat-gradient all-reduce averages them afterwards."""
import torch

OFFSET_CHANNEL = 1


def make_inputs(shapes, seed):
    """One fp32 (x, grad_out) pair per shard shape (same C): x = randn * 2 + 3, with channel
    OFFSET_CHANNEL replaced by randn * 0.5 + 50 -- an offset channel, where unshifted fp32 sums
    would cancel; gamma in [0.5, 1.5), beta ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    c = shapes[0][1]
    xs, gos = [], []
    for shape in shapes:
        x = torch.randn(shape, generator=g) * 2.0 + 3.0
        x[:, OFFSET_CHANNEL] = torch.randn(x[:, OFFSET_CHANNEL].shape, generator=g) * 0.5 + 50.0
        xs.append(x)
        gos.append(torch.randn(shape, generator=g))
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g)
    return xs, gos, gamma, beta


def _cv(v, x):
    return v.view(1, -1, *([1] * (x.dim() - 2)))


class Referee:
    """Forward over the concatenated shards at construction; ``backward(gos, ys)`` afterwards."""

    def __init__(self, xs, gamma, beta, eps=1e-5, momentum=0.1, relu=True,
                 running_mean=None, running_var=None):
        self.xs = [x.double() for x in xs]
        whole = torch.cat(self.xs, dim=0)
        c = whole.shape[1]
        self.dims = [0] + list(range(2, whole.dim()))
        self.n = whole.numel() // c
        self.relu = relu
        self.gamma, self.beta = gamma.double(), beta.double()
        self.mean = whole.mean(self.dims)
        self.var = whole.var(self.dims, unbiased=False)          # biased
        self.invstd = 1.0 / torch.sqrt(self.var + eps)
        self.scale = self.gamma * self.invstd
        self.shift = self.beta - self.mean * self.scale
        self.pre = [x * _cv(self.scale, x) + _cv(self.shift, x) for x in self.xs]
        self.ys = [p.clamp_min(0.0) if relu else p for p in self.pre]
        rm = torch.zeros(c, dtype=torch.float64) if running_mean is None else running_mean.double()
        rv = torch.ones(c, dtype=torch.float64) if running_var is None else running_var.double()
        self.running_mean = (1.0 - momentum) * rm + momentum * self.mean
        self.running_var = (1.0 - momentum) * rv + momentum * self.var
        self.xhat = [(x - _cv(self.mean, x)) * _cv(self.invstd, x) for x in self.xs]

    def backward(self, gos, ys):
        """-> (dx per shard, dgamma per shard, dbeta per shard); ys: the fp32 outputs under test."""
        gs = [go.double() * (y.double() > 0) if self.relu else go.double() for go, y in zip(gos, ys)]
        dbeta = [g.sum(self.dims) for g in gs]
        dgamma = [(g * xh).sum(self.dims) for g, xh in zip(gs, self.xhat)]
        k1, k2 = sum(dbeta) / self.n, sum(dgamma) / self.n
        dx = [_cv(self.scale, g) * (g - _cv(k1, g) - xh * _cv(k2, g)) for g, xh in zip(gs, self.xhat)]
        return dx, dgamma, dbeta

    # ---- the bounds ----------------------------------------------------------------------------
    def check_forward(self, i, y, what=''):
        """|y - y64| <= 1e-5 |y64 - beta| + 2^-22 (|x scale| + |beta - mean scale|): the project's
        rtol for fp32 statistics, plus the rounding of the two fp32 coefficients and of the two fp32
        operations of the apply."""
        x, y64 = self.xs[i], self.ys[i]
        bound = 1e-5 * (y64 - _cv(self.beta, x)).abs() + \
            2.0 ** -22 * ((x * _cv(self.scale, x)).abs() + _cv(self.shift, x).abs())
        err = (y.double() - y64).abs()
        worst = (err / bound).max().item()
        print(f'{what} shard {i}: forward max err {err.max().item():.3e}, worst err/bound {worst:.3f}')
        assert worst <= 1.0, (what, i, worst)

    def check_backward(self, i, ref, dx, dgamma, dbeta, what=''):
        """test_fused_bn_relu_matches_aten's tolerances: dx within 1e-4 of the largest |dx|,
        dgamma / dbeta rtol 1e-4, atol 1e-4; at the offset channel atol is scaled by max |xhat|."""
        dx64, dgamma64, dbeta64 = (r[i] for r in ref)
        c = dx64.shape[1]
        scale = max(max(d.abs().max().item() for d in ref[0]), 1e-3)
        xmax = max(xh[:, OFFSET_CHANNEL].abs().max().item() for xh in self.xhat)
        atol = torch.full((c,), 1e-4, dtype=torch.float64)
        atol[OFFSET_CHANNEL] *= xmax
        err = (dx.double() - dx64).abs().amax(self.dims)
        print(f'{what} shard {i}: dx max err {err.max().item():.3e} (scale {scale:.3e}), '
              f'dgamma {(dgamma.double() - dgamma64).abs().max().item():.3e}, '
              f'dbeta {(dbeta.double() - dbeta64).abs().max().item():.3e}')
        assert (err <= atol * scale).all(), (what, i, err, scale)
        for got, want in ((dgamma, dgamma64), (dbeta, dbeta64)):
            assert ((got.double() - want).abs() <= atol + 1e-4 * want.abs()).all(), (what, i, got, want)

    def check_running(self, running_mean, running_var):
        torch.testing.assert_close(running_mean.double(), self.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(running_var.double(), self.running_var, rtol=1e-5, atol=1e-6)
