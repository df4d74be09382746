"""Training-mode BatchNorm with the following ReLU fused, on the native kernels.

The reference builds conv -> BN -> ReLU from mmcv ``ConvModule`` and from
``nn.BatchNorm{1,2}d`` + ``nn.ReLU`` (point_sa_module.py:277-289,
side_pooling_module.py:55-78, 346-358); these classes ARE ``nn.BatchNorm{1,2}d`` (same
parameters, buffers and state-dict keys) whose training forward runs
``nesie_bn_relu_forward`` (3 streaming passes) instead of batch_norm + relu (5), and whose
backward runs ``nesie_bn_relu_backward`` (5 passes instead of 10).  In evaluation mode (no
autograd) the running statistics are folded into one scale / bias pair per channel and the layer
is a single read + write pass (``nesie_affine_relu_forward``); with autograd enabled, and on the
injected CPU back end, evaluation uses the ATen path.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function

from ..kernels import backend_for


_counter_sink = None


class deferred_bn_counters:
    """Within this context the fused norms queue their ``num_batches_tracked += 1`` (a
    one-element launch per layer, ~50 per VoteNet step) and the exit applies them all with
    one multi-tensor add.  Same buffer values after the block."""

    def __enter__(self):
        global _counter_sink
        self.prev, _counter_sink = _counter_sink, []
        return self

    def __exit__(self, *exc):
        global _counter_sink
        queued, _counter_sink = _counter_sink, self.prev
        if queued and exc[0] is None:
            seen = {}
            for t in queued:  # a layer called twice in the block counts twice
                seen.setdefault(id(t), [t, 0])[1] += 1
            torch._foreach_add_([t for t, _ in seen.values()], [n for _, n in seen.values()])
        return False


def count_batch(counter):
    """``num_batches_tracked += 1`` (queued inside ``deferred_bn_counters``)."""
    if _counter_sink is not None:
        _counter_sink.append(counter)
    else:
        counter.add_(1)


class BNReLUTrain(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu,
                row_bias=None, pre_partial=None):
        """pre_partial (C, nslice, 2): unshifted (sum, sum of squares) partials of x left by its
        producer; the statistics pass over x is then skipped."""
        x = x.contiguous()
        if row_bias is not None:
            row_bias = row_bias.contiguous()
        c = x.shape[1]
        y = torch.empty_like(x)
        save_mean = x.new_empty(c)
        save_invstd = x.new_empty(c)
        fwd_coef = x.new_empty(c, 4)  # scale, bias, mean, invstd as the forward applied them
        backend_for(x).bn_relu_forward(x, weight, bias, running_mean, running_var, momentum,
                                       eps, relu, y, save_mean, save_invstd, fwd_coef,
                                       row_bias=row_bias, pre_partial=pre_partial)
        ctx.relu = relu
        ctx.has_row_bias = row_bias is not None
        saved = (x, y, weight, bias, save_mean, save_invstd, fwd_coef)
        ctx.save_for_backward(*(saved + ((row_bias,) if ctx.has_row_bias else ())))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, bias, save_mean, save_invstd, fwd_coef = ctx.saved_tensors[:7]
        row_bias = ctx.saved_tensors[7] if ctx.has_row_bias else None
        # a per-channel row_bias is a conv bias folded into the norm: the mean subtraction removes
        # it, its gradient is identically zero and is returned as a zero tensor (a summation of dx,
        # as the unfused graph does, returns rounding noise around that zero; a None would make a
        # per-parameter optimiser skip the bias -- no weight decay on it)
        d_row_bias = torch.empty_like(row_bias) if ctx.has_row_bias and row_bias.dim() != 1 else None
        d_chan_bias = torch.zeros_like(row_bias) if ctx.has_row_bias and row_bias.dim() == 1 else None
        dy = dy.contiguous()
        c = x.shape[1]
        dx = torch.empty_like(x)
        dgamma, dbeta = x.new_empty(c), x.new_empty(c)
        backend_for(dy).bn_relu_backward(dy, x, y, weight, bias, save_mean, save_invstd, fwd_coef,
                                         ctx.relu, dx, dgamma, dbeta, row_bias=row_bias,
                                         d_row_bias=d_row_bias)
        return dx, dgamma, dbeta, None, None, None, None, None, \
            (d_row_bias if d_chan_bias is None else d_chan_bias), None


class BNReLUMaxPoolTrain(Function):
    """x (B, C, M, ns) -> max_ns relu(bn(x)) (B, C, M): the tail of a set-abstraction MLP
    (ConvModule's BN2d + ReLU, then F.max_pool2d([1, ns]): point_sa_module.py:277-289,
    136-158) without materialising the normalised tensor, forward or backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps):
        x = x.contiguous()
        b, c, m, _ = x.shape
        pooled = x.new_empty(b, c, m)
        argmax = torch.empty(b, c, m, dtype=torch.uint8, device=x.device)
        save_mean, save_invstd = x.new_empty(c), x.new_empty(c)
        fwd_coef = x.new_empty(c, 4)
        backend_for(x).bn_relu_maxpool_forward(x, weight, bias, running_mean, running_var,
                                               momentum, eps, pooled, argmax, save_mean,
                                               save_invstd, fwd_coef)
        ctx.save_for_backward(x, pooled, argmax, weight, save_invstd, fwd_coef)
        ctx.mark_non_differentiable(argmax)
        return pooled

    @staticmethod
    def backward(ctx, g):
        x, pooled, argmax, weight, save_invstd, fwd_coef = ctx.saved_tensors
        c = x.shape[1]
        dx = torch.empty_like(x)
        dgamma, dbeta = x.new_empty(c), x.new_empty(c)
        backend_for(x).bn_relu_maxpool_backward(g.contiguous(), argmax, x, pooled, weight,
                                                save_invstd, fwd_coef, dx, dgamma, dbeta)
        return dx, dgamma, dbeta, None, None, None, None


def eval_coefficients(weight, bias, running_mean, running_var, eps):
    """(C,4) = (scale, bias, 0, 0) of an evaluation-mode BatchNorm: scale = gamma / sqrt(var +
    eps), bias = beta - mean * scale."""
    scale = torch.rsqrt(running_var + eps)
    if weight is not None:
        scale = scale * weight
    shift = -running_mean * scale
    if bias is not None:
        shift = shift + bias
    zero = torch.zeros_like(scale)
    return torch.stack([scale, shift, zero, zero], dim=1).contiguous()


def stacked_eval_coef(layers):
    """(S*C, 4) evaluation coefficients of S same-width norm layers stacked along the channel
    axis: every layer's launch fills its own slice (no concatenation)."""
    if len(layers) == 1:
        return layers[0].eval_coef()
    c = layers[0].num_features
    table = layers[0].running_mean.new_empty(len(layers) * c, 4)
    for i, l in enumerate(layers):
        l.eval_coef(out=table[i * c:(i + 1) * c])
    return table


def affine_relu_eval(x, coef, relu, row_bias=None):
    x = x.contiguous()
    y = torch.empty_like(x)
    backend_for(x).affine_relu_forward(x, coef, relu, y,
                                       None if row_bias is None else row_bias.contiguous())
    return y


class _FusedBNReLU:
    """Mixin over nn.BatchNorm{1,2}d: ``relu=True`` folds the activation into the norm."""

    def _init_fused(self, relu):
        self.fuse_relu = bool(relu)

    def forward(self, x, row_bias=None, pre_partial=None, chan_bias=None):
        """``row_bias`` (B, C, K), optional: normalise ``x + row_bias[..., None]`` for
        ``x`` (B, C, K, G) without materialising the sum (G a power of two in 4..256).
        ``pre_partial`` (C, nslice, 2), optional: (sum, sum of squares) partials of x left by
        its producer (native training path only; ignored otherwise).
        ``chan_bias`` (C), optional: the bias of the convolution that produced ``x``: normalise
        ``x + chan_bias`` with the sum formed in registers (same rounding as the separate add)."""
        backend = backend_for(x)  # raises for CPU tensors without an injected back end
        native = (backend.name == 'hip' and self.training and x.dtype == torch.float32
                  and self.affine and self.track_running_stats and self.momentum is not None)
        native_eval = self._native_eval(x, backend)
        if chan_bias is not None:
            assert row_bias is None and pre_partial is None
            if native or native_eval:
                row_bias = chan_bias
            else:
                x = x + chan_bias.view(1, -1, *([1] * (x.dim() - 2)))
        elif row_bias is not None:
            g = x.shape[-1]
            if not ((native or native_eval) and x.dim() == 4 and 4 <= g <= 256 and g & (g - 1) == 0):
                x, row_bias = x + row_bias.unsqueeze(-1), None
        if native_eval:
            return affine_relu_eval(x, self.eval_coef(), self.fuse_relu, row_bias)
        if native:
            if _counter_sink is not None:
                _counter_sink.append(self.num_batches_tracked)
            else:
                self.num_batches_tracked.add_(1)
            return BNReLUTrain.apply(x, self.weight, self.bias, self.running_mean,
                                     self.running_var, self.momentum, self.eps, self.fuse_relu,
                                     row_bias, pre_partial if row_bias is None else None)
        y = super().forward(x)
        return F.relu(y) if self.fuse_relu else y


    def eval_coef(self, out=None):
        """(C,4) = (scale, shift, 0, 0) of this layer in evaluation mode, recomputed on every call
        by one native launch (``nesie_bn_eval_coef``).  NOT cached: the running statistics are
        written by the training kernels through raw pointers, the parameters through the flat
        optimiser vector and the EMA swap through ``.data`` copies -- none of which moves a
        tensor version counter, so a cache keyed on them served stale coefficients in any
        train -> eval -> train -> eval loop and across ``EMATeacher.swap``.  ``out`` (C,4),
        optional: a slice of a stacked table to fill in place."""
        c = self.num_features
        coef = self.running_mean.new_empty(c, 4) if out is None else out
        with torch.no_grad():
            backend_for(self.running_mean).bn_eval_coef(
                None if self.weight is None else self.weight.detach(),
                None if self.bias is None else self.bias.detach(),
                self.running_mean, self.running_var, self.eps, coef)
        return coef

    def _native_eval(self, x, backend):
        return (backend.name == 'hip' and not self.training and self.track_running_stats
                and self.running_mean is not None and x.dtype == torch.float32
                and not torch.is_grad_enabled())

    def forward_max_pool(self, x):
        """relu(bn(x)) followed by the max over the last axis of x (B, C, M, ns) -> (B, C, M),
        in one fused pass when the native training path applies; else the two-step form."""
        backend = backend_for(x)
        ns = x.shape[-1]
        native = (backend.name == 'hip' and self.training and x.dtype == torch.float32
                  and self.affine and self.track_running_stats and self.momentum is not None
                  and self.fuse_relu and x.dim() == 4 and 4 <= ns <= 64 and ns & (ns - 1) == 0)
        if (self._native_eval(x, backend) and self.fuse_relu and x.dim() == 4
                and 4 <= ns <= 64 and ns & (ns - 1) == 0):
            x = x.contiguous()
            pooled = x.new_empty(x.shape[:3])
            argmax = torch.empty(x.shape[:3], dtype=torch.uint8, device=x.device)
            backend.affine_relu_maxpool_forward(x, self.eval_coef(), pooled, argmax)
            return pooled
        if not native:
            from .pool import group_max_pool
            return group_max_pool(self.forward(x))
        if _counter_sink is not None:
            _counter_sink.append(self.num_batches_tracked)
        else:
            self.num_batches_tracked.add_(1)
        return BNReLUMaxPoolTrain.apply(x, self.weight, self.bias, self.running_mean,
                                        self.running_var, self.momentum, self.eps)


class FusedBNReLU1d(_FusedBNReLU, nn.BatchNorm1d):
    def __init__(self, num_features, relu=True, **kw):
        nn.BatchNorm1d.__init__(self, num_features, **kw)
        self._init_fused(relu)


class FusedBNReLU2d(_FusedBNReLU, nn.BatchNorm2d):
    def __init__(self, num_features, relu=True, **kw):
        nn.BatchNorm2d.__init__(self, num_features, **kw)
        self._init_fused(relu)


# ---- synchronised batch statistics (reference mmdet3d/ops/norm.py:27-133) ----------------------
def _sync_group_active(group):
    """A process group is up and either spans several ranks or ``dp.force_process_group()`` asks
    for the real collectives on one rank."""
    import torch.distributed as dist
    from ..dp import force_process_group
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or force_process_group()


def _channel_view(v, x):
    return v.view(1, -1, *([1] * (x.dim() - 2)))


class SyncBNReLUTrain(Function):
    """Training BatchNorm (+ ReLU) over the batches of ALL ranks of ``group``: local raw moments
    (C, 3) float64 -> all-reduce(SUM) -> apply; backward: local (sum g, sum g xhat) (C, 2) float64
    -> all-reduce(SUM) -> apply.  Two collectives per layer per step.  On a ``hip`` tensor the four
    steps are the ``nesie_syncbn_*`` kernels; on any other tensor (CPU ranks under gloo, an
    injected back end) the same mathematics in torch ops.  x and fwd_coef are saved, y is not.
    dgamma / dbeta are the LOCAL sums: the flat-gradient all-reduce averages them afterwards."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, group):
        import torch.distributed as dist
        x = x.contiguous()
        c = x.shape[1]
        native = x.is_cuda and backend_for(x).name == 'hip'
        moments = torch.empty(c, 3, dtype=torch.float64, device=x.device)
        fwd_coef = x.new_empty(c, 4)  # scale, bias, mean, invstd as the forward applied them
        if native:
            backend = backend_for(x)
            y = torch.empty_like(x)
            backend.syncbn_local_moments(x, moments)
            dist.all_reduce(moments, op=dist.ReduceOp.SUM, group=group)
            backend.syncbn_forward_apply(x, moments, weight, bias, running_mean, running_var,
                                         momentum, eps, relu, y, fwd_coef)
        else:
            xd = x.double().reshape(x.shape[0], c, -1)
            moments[:, 0] = xd.shape[0] * xd.shape[2]
            moments[:, 1] = xd.sum(dim=(0, 2))
            moments[:, 2] = (xd * xd).sum(dim=(0, 2))
            dist.all_reduce(moments, op=dist.ReduceOp.SUM, group=group)
            n = moments[:, 0]
            mean = moments[:, 1] / n
            var = (moments[:, 2] / n - mean * mean).clamp_min(0.0)
            invstd = 1.0 / torch.sqrt(var + eps)
            g = weight.detach().double()
            fwd_coef[:, 0] = g * invstd
            fwd_coef[:, 1] = bias.detach().double() - mean * g * invstd
            fwd_coef[:, 2] = mean
            fwd_coef[:, 3] = invstd
            # the BIASED variance, as the reference (norm.py:68-71)
            running_mean.copy_((1.0 - momentum) * running_mean.double() + momentum * mean)
            running_var.copy_((1.0 - momentum) * running_var.double() + momentum * var)
            y = x * _channel_view(fwd_coef[:, 0], x) + _channel_view(fwd_coef[:, 1], x)
            if relu:
                y = y.clamp_min_(0.0)
        ctx.relu, ctx.group, ctx.native, ctx.eps = relu, group, native, eps
        ctx.save_for_backward(x, weight, fwd_coef, moments)
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        x, weight, fwd_coef, moments = ctx.saved_tensors
        dy = dy.contiguous()
        c = x.shape[1]
        sums = torch.empty(c, 2, dtype=torch.float64, device=x.device)
        if ctx.native:
            backend = backend_for(x)
            dx = torch.empty_like(x)
            dgamma, dbeta = x.new_empty(c), x.new_empty(c)
            backend.syncbn_backward_local(dy, x, fwd_coef, moments, ctx.eps, ctx.relu, sums,
                                          dgamma, dbeta)
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=ctx.group)
            backend.syncbn_backward_apply(dy, x, fwd_coef, weight, sums, moments, ctx.eps,
                                          ctx.relu, dx)
        else:
            # the mask in the forward's fp32 operations; xhat and the closed form in double (with few
            # positions per channel the form cancels completely), dx rounded once
            scale, shift = _channel_view(fwd_coef[:, 0], x), _channel_view(fwd_coef[:, 1], x)
            g = (dy * (x * scale + shift > 0) if ctx.relu else dy).double()
            n = moments[:, 0]
            mean = moments[:, 1] / n
            var = (moments[:, 2] / n - mean * mean).clamp_min(0.0)
            invstd = 1.0 / torch.sqrt(var + ctx.eps)
            xhat = (x.double() - _channel_view(mean, x)) * _channel_view(invstd, x)
            axes = [0] + list(range(2, x.dim()))
            sums[:, 0] = g.sum(dim=axes)
            sums[:, 1] = (g * xhat).sum(dim=axes)
            dbeta, dgamma = sums[:, 0].float(), sums[:, 1].float()
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=ctx.group)
            a = weight.detach().double() * invstd
            k1, k2 = sums[:, 0] / n, sums[:, 1] / n
            dx = (_channel_view(a, x) * (g - _channel_view(k1, x) - xhat * _channel_view(k2, x))).float()
        return dx, dgamma, dbeta, None, None, None, None, None, None


class _NaiveSyncBN(_FusedBNReLU):
    """Mixin over nn.BatchNorm{1,2}d: batch statistics over every rank of ``group`` while
    training under an initialised process group (world size > 1, or
    ``dp.force_process_group()``); otherwise -- evaluation, one rank, no group -- the fused local
    norm.  NOT a ``FusedBNReLU{1,2}d``: every fused chain gates on those two classes, and a chain
    would normalise with local statistics.

    One deliberate difference from the reference: it averages the per-rank means with equal weight
    per rank, which is the global batch statistic only when every rank holds the same number of
    positions.  Here the count travels in the moments, so the result always equals BatchNorm over
    the concatenated batch; with equal shards the two agree.  As in the reference the running
    variance takes the biased variance and ``num_batches_tracked`` is not touched on the sync
    path."""

    def _init_sync(self, relu, group):
        if self.momentum is None:
            raise ValueError(f'{type(self).__name__}: momentum=None (a cumulative moving average) '
                             'is not supported; give a float momentum')
        self._init_fused(relu)
        self.group = group

    def forward(self, x):
        assert x.dtype == torch.float32, f'input should be in float32 type, got {x.dtype}'
        if not (self.training and _sync_group_active(self.group)):
            return _FusedBNReLU.forward(self, x)
        assert x.numel() > 0, 'SyncBN does not support empty inputs'
        if not (self.affine and self.track_running_stats):
            raise RuntimeError(f'{type(self).__name__}: the synchronised path needs affine=True and '
                               'track_running_stats=True')
        if x.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{type(self).__name__}: the synchronised path cannot be captured in '
                               'a graph (its all-reduce is not captured); keep plain BN in a '
                               'graphed step')
        self._check_input_dim(x)
        return SyncBNReLUTrain.apply(x, self.weight, self.bias, self.running_mean,
                                     self.running_var, self.momentum, self.eps, self.fuse_relu,
                                     self.group)


class NaiveSyncBatchNorm1d(_NaiveSyncBN, nn.BatchNorm1d):
    """``nn.BatchNorm1d`` (same parameters, buffers, state-dict keys) with cross-rank batch
    statistics; norm type ``naiveSyncBN1d``.  See ``_NaiveSyncBN``."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True,
                 track_running_stats=True, *, relu=False, group=None):
        nn.BatchNorm1d.__init__(self, num_features, eps, momentum, affine, track_running_stats)
        self._init_sync(relu, group)


class NaiveSyncBatchNorm2d(_NaiveSyncBN, nn.BatchNorm2d):
    """``nn.BatchNorm2d`` with cross-rank batch statistics; norm type ``naiveSyncBN2d``."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True,
                 track_running_stats=True, *, relu=False, group=None):
        nn.BatchNorm2d.__init__(self, num_features, eps, momentum, affine, track_running_stats)
        self._init_sync(relu, group)
