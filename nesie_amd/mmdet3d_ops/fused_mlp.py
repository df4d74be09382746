"""conv -> BN -> ReLU chains of the grouped per-seed MLPs on the native layer kernel.

The reference evaluates a shared MLP op by op -- mmcv ``ConvModule(Conv2d 1x1, BN2d, ReLU)`` three
times, then ``F.max_pool2d([1, nsample])`` (point_sa_module.py:277-289, 136-158).  Here a layer is
ONE launch of ``nesie_pw_layer_forward``: the previous layer's folded BatchNorm + ReLU is applied
to the operand on its way to the matrix cores, the layer's own batch statistics (and, for the
last layer, the max / min over the neighbourhood) leave from the accumulators, and the normalised
activations are never written.  Per layer the forward moves its tensor through HBM twice (read
the previous raw conv output, write this one) instead of five times.

The backward is hand-written too: per layer ONE input-gradient launch (the same layer kernel on
the transposed weight view, ``nesie_pw_dgrad_bn_reduce``: its epilogue also leaves the two sums of
the BatchNorm backward), one weight-gradient launch on the matrix cores with the activation
recomputed on load (``nesie_pw_wgrad``), and the BatchNorm + ReLU apply pass from the RAW conv
output and the saved (scale, bias, mean, invstd) (``nesie_bn_relu_backward_apply``; the mask is
re-derived with the same fused multiply-add the forward's operand load used).

Same function as the module-by-module path (which stays the CPU checker's and serves shapes the
kernels are not built for); differences are fp32 summation order and fma-vs-mul/add rounding.

How the host side is laid out: the three chain functions (``SAStackFn``, ``Stack1dFn``, ``MiniTailFn``)
describe their layers once as ``_Layer`` records (``_chain_layout``: which of the function's tensors is
a layer's weight, bias, scale, shift -- the same positions address the gradient slots and the
returned gradients, behind however many arguments the function has in front of them), store and
fetch their state through ``_save_chain`` / ``_saved_chain``, and share ONE walk back through the
layers (``_chain_backward``); what differs between them -- how the top of the chain is entered, SA1's
rebuilt first activation, the coordinate rows of the input gradient, the zero bias gradient --
stays in the ``backward``s.  Particular to the MiniPointNet tail: the row bias that joins its first
layer's output (its gradient leaves from that layer's norm backward, ``rb_group``), its two ways in
at the top (the max-pool's entries, or the expanded dense gradient), and W_l, a split view that
gets no slot.  The two head functions (``MiniHeadFn``, ``BlendMiniHeadFn``) are a norm without a conv
in front of one conv, not a chain: they share ``_mini_head_backward`` / ``_first_norm_apply`` and name
their three parameters' positions once (``_GAMMA0, _BETA0, _W3``).  A layer that leaves through a max
over groups of positions is ``_pooled_layer`` everywhere.  Which launches each function issues, in
which order and over which buffers is pinned without a GPU by tests/test_fused_mlp_trace_cpu.py.
"""

from collections import namedtuple

import torch
from torch.autograd import Function

from .. import grad_slots
from ..kernels import backend_for


# Tests flip this to obtain the module-by-module evaluation of the same network on the device.
ENABLED = True
# Plain constants like ENABLED, not settings: tests flip them to compare the same model both ways.
# SA1_K4: SA1's first activation (4 -> 64 over 10^6 positions, 268 MB) is rebuilt from the 17 MB input
# wherever it is an operand instead of being stored (include/nesie_ops.h, round 5).
# FOLD_NORM_BWD: the BatchNorm + ReLU backward's apply pass runs inside the weight gradient instead
# of as its own launch (nesie_bn_relu_backward_apply) in front of it.
SA1_K4 = True
FOLD_NORM_BWD = True

# Ownership hand-over of a freshly allocated gradient buffer between MiniTailFn.backward and
# MiniHeadFn.backward: the producer marks the TENSOR OBJECT (an attribute, not its address -- an
# address outlives the tensor in the caching allocator and could be handed to an unrelated gradient
# later); whatever autograd builds from it for a second consumer is a new object without the mark.
_OWNED_MARK = '_nesie_fresh_grad'


def _dst(slot, like, *shape):
    """Where a backward kernel writes a parameter gradient: the parameter's slot of the flat
    gradient vector (``grad_slots.take`` in the forward) or a fresh tensor."""
    return slot.view(*shape) if slot is not None else like.new_empty(*shape)


def _into(slot, g):
    """A gradient that some other op produced, moved into the slot that was taken for it."""
    if slot is None or g is None:
        return g
    slot.view(g.shape).copy_(g)
    return slot.view(g.shape)


def _wgrad(backend, dy, x, x_coef, ng=1, slot=None):
    """dW (ng, Cout, Cin) = sum over n % ng == g of dy[n] @ act(x[n])^T; act = relu(scale * x +
    bias) when x_coef (ng * Cin, 4).  ``slot``: the weight's gradient slot (written in place)."""
    nb, co, p = dy.shape
    ci = x.shape[1]
    # wide products over few positions run tiled; the rest natively while one workgroup's accumulators
    # hold the whole product (wider layers as column blocks were slower than a transposed copy + rocBLAS)
    if backend.pw_wgrad_tiled(nb, ng, co, ci, p) or (
            backend.pw_wgrad_supported(co, ci, p) and (ci <= 320 if co <= 128 else ci <= 128)):
        dw = _dst(slot, dy, ng, co, ci)
        # (a slot of the flat gradient vector is read by nobody before the optimiser: its reduction
        # may wait for the one batched launch at FlatTrainState.collect())
        backend.pw_wgrad(dy, x, dw, ng=ng, x_coef=x_coef, x_relu=True, final=slot is not None)
        return dw
    if ng == 1 and ci <= 8 and backend.conv_wgrad_supported(co, ci):
        dw = _dst(slot, dy, co, ci)
        backend.conv_wgrad(dy, x, dw, x_coef=x_coef, x_relu=x_coef is not None)
        return dw.view(1, co, ci)
    return _into(slot, _wgrad_aten(backend, dy, x, x_coef, ng))


def _wgrad_aten(backend, dy, x, x_coef, ng):
    nb, co, p = dy.shape
    ci = x.shape[1]
    out = []
    for g in range(ng):      # shapes outside the native kernels (short rows, wide layers)
        dyg, xg = dy[g::ng], x[g::ng]
        cg = None if x_coef is None else x_coef[g * ci:(g + 1) * ci].contiguous()
        if ci <= 8 and backend.conv_wgrad_supported(co, ci):
            dw = dy.new_empty(co, ci)
            backend.conv_wgrad(dyg, xg, dw, x_coef=cg, x_relu=cg is not None)
            out.append(dw)
            continue
        a, d = xg.contiguous(), dyg.contiguous()
        if cg is not None:
            a2 = torch.empty_like(a)
            backend.affine_relu_forward(a, cg, True, a2)
            a = a2
        b = d.shape[0]
        if p <= 2048 and b > 1:
            out.append(torch.mm(d.transpose(0, 1).reshape(co, b * p), a.transpose(0, 1).reshape(ci, b * p).t()))
        else:
            out.append(torch.bmm(d, a.transpose(1, 2)).sum(0))
    return out[0].unsqueeze(0) if ng == 1 else torch.stack(out)


def _norm_backward_wgrad(backend, da, z, gamma, coef, part, src, src_coef, need_w, ng=1, need_dz=True,
                         slots=(None, None, None), rb_group=None):
    """The backward of relu(bn(z)) given da (its gradient) and the reduction partials the
    input-gradient launch left, and the weight gradient dz . act(src)^T of the conv that produced z:
    -> (dz, dw | None, dgamma, dbeta).  One launch where the layer kernel's weight gradient serves
    the shape (``nesie_pw_wgrad_bn_backward``: dz is formed on the operand load and written over
    da), the apply pass + ``_wgrad`` otherwise.  ``need_dz`` False (the layer's input needs no
    gradient) and a skinny input (Cin <= 8, the first layer of SA1): ``nesie_conv_wgrad_bn`` forms
    dz on its load and never writes it -> dz None.  ``slots`` = gradient slots of (weight, gamma,
    beta): the kernels write there.  ``rb_group`` = G: the forward added a row bias per group of G
    positions to z (the MiniPointNet tail); its gradient (nb, co, p / G) leaves from the launch that forms
    dz and is returned as a fifth value (the one-launch form serves G = 16 and 64, adding into zeros at 64)."""
    nb, co, p = da.shape
    ci = src.shape[1]
    s_w, s_g, s_b = slots
    dgamma, dbeta = _dst(s_g, da, ng * co), _dst(s_b, da, ng * co)
    fold = FOLD_NORM_BWD and need_w and rb_group in (None, 16, 64) and backend.pw_wgrad_bn_supported(co, ci, p)
    d_rb, out = None, (dgamma, dbeta)
    if rb_group:
        d_rb = (da.new_zeros if fold and rb_group == 64 else da.new_empty)(nb, co, p // rb_group)
        out += (d_rb,)
    if fold:
        dw = _dst(s_w, da, ng, co, ci)
        backend.pw_wgrad_bn_backward(da, z, coef, gamma, part, src, da, dw, dgamma, dbeta, ng=ng, x_coef=src_coef,
                                     d_row_bias=d_rb, group=rb_group or 0, final=s_w is not None)
        return (da, dw) + out
    if (FOLD_NORM_BWD and need_w and not need_dz and not rb_group and ng == 1 and ci <= 8
            and backend.conv_wgrad_supported(co, ci)):
        bnb = backend.pw_bnb_coef(part, coef, gamma, float(nb) * float(p), dgamma, dbeta)
        dw = _dst(s_w, da, co, ci)
        backend.conv_wgrad(da, src, dw, x_coef=src_coef, x_relu=src_coef is not None, bn_z=z, bnb=bnb)
        return None, dw.view(1, co, ci), dgamma, dbeta
    dz = torch.empty_like(da)
    b = nb // ng
    backend.bn_relu_backward_apply(da.view(b, ng * co, p), z.view(b, ng * co, p), gamma, None, coef, part,
                                   dz.view(b, ng * co, p), dgamma, dbeta,
                                   d_row_bias=d_rb.view(b, ng * co, -1) if rb_group else None, group=rb_group)
    dw = _wgrad(backend, dz, src, src_coef, ng=ng, slot=s_w) if need_w else None
    return (dz, dw) + out


def _take_slots(ctx, first_index, tensors):
    """Gradient slots of ``tensors`` = the arguments of ``ctx``'s forward from ``first_index`` on (negative:
    counted from the back; None entries are passed over) -- only for those whose gradient a backward
    will be asked for."""
    return [grad_slots.take(t) if ctx.needs_input_grad[first_index + j] else None for j, t in enumerate(tensors)]


def _returned(ctx, inputs, params):
    """What a backward returns: the gradients of its leading ``inputs``, None for every argument
    between them and the trailing ``params``, then theirs."""
    return tuple(inputs) + (None,) * (len(ctx.needs_input_grad) - len(inputs) - len(params)) + tuple(params)


def _pool_group(G):
    return 16 if G == 16 else 32


def _pooled_layer(backend, src, w, ng, in_coef, group, y=None, stat_part=None, norm_coef=None, zstar=False):
    """A layer whose output leaves as its maximum over groups of ``group`` positions: src (..., Cin, P),
    w (ng, Cout, Cin) -> (pooled (..., Cout, P / group), arg-max uint8, raw extremum | None) of
    W . relu(in_coef src), through relu(norm(.)) when ``norm_coef`` is given.  The layer launch
    leaves partial extrema (the minima too under a norm: its scale may be negative), the finishing
    launch the rest.  ``norm_coef()`` runs BETWEEN the two and returns the norm's folded
    coefficients (training: the statistics in ``stat_part`` are finalised there).  ``y``: the dense
    output as well; ``zstar``: return the raw extremum behind every pooled value.  Leading axes
    (scene, net) are one batch axis to the kernels."""
    *lead, cin, P = src.shape
    src = src.flatten(0, -3)
    cout = w.shape[1]
    pg = _pool_group(group)
    normed = norm_coef is not None

    def buf(n, dtype=src.dtype, batch=src.shape[:1]):
        return torch.empty(*batch, cout, n, dtype=dtype, device=src.device)
    pool_out = (buf(P // pg), buf(P // pg) if normed else None,
                buf(P // pg, torch.uint8), buf(P // pg, torch.uint8) if normed else None)
    backend.pw_layer_forward(src, w, ng=ng, in_coef=in_coef, in_relu=True, y=y, stat_part=stat_part,
                             pool_group=pg, pool_min=normed, pool_out=pool_out)
    coef = norm_coef() if normed else None
    pooled, argmax = buf(P // group, batch=lead), buf(P // group, torch.uint8, lead)
    raw = buf(P // group, batch=lead) if zstar else None
    backend.pw_pool_finish(ng, P, group, pg, pool_out, coef, normed, pooled.flatten(0, -3), argmax.flatten(0, -3),
                           zstar=raw)
    return pooled, argmax, raw


# ---- a chain's layers: one record per layer, one walk back through them ------------------------------

class Stack1dLayer:
    """Static description of one layer: ``bias`` (the conv has one), ``bn`` = None or
    (running_mean, running_var, momentum, eps) (-> conv, BatchNorm, ReLU)."""

    def __init__(self, bias, bn):
        self.bias, self.bn = bool(bias), bn


# One layer of a chain function (SAStackFn, Stack1dFn, MiniTailFn).  ``iw, ib, ig, ibeta``: where its
# weight, conv bias, norm scale and shift sit among the function's trailing tensors (None = the layer
# has none) -- which is also where their gradients sit in what the backward returns behind the
# ``ctx.lead`` entries of its leading arguments, and their slots in ``ctx.slots``; ``bn`` = the norm's
# (running_mean, running_var, momentum, eps) or None.  The positions are static and live on ``ctx``;
# ``w, b, gamma, beta`` are filled in by ``_bind`` from the forward's arguments or from the saved tensors.
_Layer = namedtuple('_Layer', 'bn iw ib ig ibeta w b gamma beta', defaults=(None,) * 4)


def _chain_layout(layers):
    """[Stack1dLayer] -> [_Layer] without tensors: per layer W, then the bias if the conv has one,
    then gamma, beta if it has a norm."""
    chain, pos = [], 0
    for lay in layers:
        ib = pos + 1 if lay.bias else None
        ig = pos + 1 + lay.bias if lay.bn is not None else None
        chain.append(_Layer(lay.bn, pos, ib, ig, None if ig is None else ig + 1))
        pos += 1 + lay.bias + (0 if lay.bn is None else 2)
    return chain


def _bind(chain, tensors):
    def at(i):
        return None if i is None else tensors[i]
    return [lay._replace(w=at(lay.iw), b=at(lay.ib), gamma=at(lay.ig), beta=at(lay.ibeta)) for lay in chain]


def _save_chain(ctx, chain, head, ys, coefs, tensors, no_slot=()):
    """What a chain's backward needs: ``head`` (the input and whatever else the function keeps), per
    layer the raw conv output and the folded norm coefficients (None where there is none), the
    layers' tensors -- the LAST arguments of the function's forward; ``ctx.lead`` counts the ones in
    front of them -- and the gradient slots of the tensors whose gradient a kernel (or a fill)
    writes: weights, norm scales / shifts, and the identically-zero bias in front of a norm (a plain
    conv's bias gradient is a reduction of its own: nothing to gain there).  ``no_slot``: positions
    among ``tensors`` whose gradient is somebody else's to place."""
    skip = {lay.ib for lay in chain if lay.bn is None} | set(no_slot)
    ctx.lead = len(ctx.needs_input_grad) - len(tensors)
    ctx.slots = _take_slots(ctx, ctx.lead, [None if i in skip else t for i, t in enumerate(tensors)])
    ctx.chain, ctx.n_head = chain, len(head)
    ctx.save_for_backward(*head, *ys, *coefs, *tensors)


def _saved_chain(ctx):
    """-> (head, ys, coefs, the layers bound to the saved tensors) as ``_save_chain`` stored them."""
    sv, h, L = ctx.saved_tensors, ctx.n_head, len(ctx.chain)
    return sv[:h], sv[h:h + L], sv[h + L:h + 2 * L], _bind(ctx.chain, sv[h + 2 * L:])


def _transposed(w):
    """The (ng, Cin, Cout) view of a layer's weight that the input-gradient product reads:
    w (S, Cout, Cin) of a 1-D chain, or a conv weight (Cout, Cin, 1, 1)."""
    return w.transpose(1, 2) if w.dim() == 3 else w.flatten(1).t().unsqueeze(0)


def _chain_backward(backend, ctx, lays, x, ys, coefs, grads, top, dz, pending=None, ng=1, input_grad=None,
                    bottom=0, rb_group=None):
    """The walk from layer ``top`` down through a chain: per layer the norm backward and the weight
    gradient, then the input-gradient launch that also leaves the reduction of the next norm
    backward.  It is entered with ``dz`` = the gradient of layer ``top``'s raw output, or with
    ``pending`` = (da, part): the gradient of its ACTIVATION and the reduction partials of its norm
    backward, not applied yet.  Parameter gradients go into ``grads`` at the layers' positions (written
    into ``ctx.slots`` where there are any).  At layer 0 it returns ``input_grad(dz, layer)``; without
    an ``input_grad`` nobody reads the first layer's dz and it may never be written.  ``bottom`` > 0:
    the walk ends in front of layer ``bottom - 1`` and returns that layer's pending.  ``rb_group`` = G:
    layer 0's forward added a row bias per group of G positions; its gradient is ``input_grad``'s
    third argument."""
    need, slots = ctx.needs_input_grad[ctx.lead:], ctx.slots
    d_rb = ()
    for l in range(top, bottom - 1, -1):
        lay = lays[l]
        src, src_coef = (x, None) if l == 0 else (ys[l - 1], coefs[l - 1])
        if pending is not None:     # norm backward of this layer, with its weight gradient
            dz, dw, grads[lay.ig], grads[lay.ibeta], *d_rb = _norm_backward_wgrad(
                backend, pending[0], ys[l], lay.gamma, coefs[l], pending[1], src, src_coef, need[lay.iw], ng=ng,
                need_dz=l > 0 or input_grad is not None, slots=(slots[lay.iw], slots[lay.ig], slots[lay.ibeta]),
                rb_group=None if l else rb_group)
            if dw is not None:
                grads[lay.iw] = dw.view(lay.w.shape)
        elif need[lay.iw]:
            grads[lay.iw] = _wgrad(backend, dz, src, src_coef, ng=ng, slot=slots[lay.iw]).view(lay.w.shape)
        if l == 0:
            return None if input_grad is None else input_grad(dz, lay, *d_rb)
        # gradient of the previous layer's activation (+ the reduction of its norm backward)
        da = dz.new_empty(dz.shape[0], src.shape[1], dz.shape[2])
        part = backend.pw_dgrad_bn_reduce(dz, _transposed(lay.w), src, src_coef, da, ng=ng)
        pending = (da, part)
    return pending


class SAStackFn(Function):
    """x (B, C0, M, ns) -> max_ns relu(bn_L(conv_L(... relu(bn_1(conv_1(x)))))) (B, C_L, M).
    ``fixed_lead`` = number of leading input channels that are inputs of the step (grouped
    coordinates of the backbone levels: nothing consumes their gradient).  It must be 0 when the
    coordinates were computed by the network (vote aggregation groups the predicted votes)."""

    @staticmethod
    def forward(ctx, x, bufs, fixed_lead, *params):
        backend = backend_for(x)
        x = x.contiguous()
        B, c0, M, ns = x.shape
        P = M * ns
        chain = _chain_layout([Stack1dLayer(False, bn) for bn in bufs])      # no bias, always a norm
        lays = _bind(chain, params)
        L = len(lays)
        x3 = x.view(B, c0, P)
        ys, coefs = [], []
        coef = k4_mom = None
        need = ctx.needs_input_grad
        k4_ok = getattr(backend, 'k4_supported', None)
        # (need[3:9]: the parameters of the first two layers -- all of them or nothing at all)
        ctx.k4 = bool(SA1_K4 and L >= 3 and k4_ok is not None and not need[0]
                      and (all(need[3:9]) or not any(need))
                      and k4_ok(c0, lays[0].w.shape[0], lays[1].w.shape[0], P))
        w0c = lays[0].w.reshape(lays[0].w.shape[0], c0) if ctx.k4 else None
        for l, lay in enumerate(lays):
            gamma, beta = lay.gamma, lay.beta
            rm, rv, momentum, eps = lay.bn
            cout, cin = lay.w.shape[0], lay.w.shape[1]
            w2 = lay.w.reshape(1, cout, cin)
            src = x3 if l == 0 else ys[-1]
            last = l == L - 1
            # the pooled last layer without its dense pre-pool tensor (csrc/pool_tail.hip): the forward
            # keeps (pooled, arg-max, raw extremum) only, the backward goes through
            # dZ = sparse + alpha + beta Z; the dense form serves the shapes pool_tail_supported refuses
            tail = bool(last and l > 0 and backend.pool_tail_supported(cin, cout, P, ns))
            # (tail: the raw output is never written; k4: nor is the first layer's)
            y = None if (tail or (ctx.k4 and l == 0)) else x.new_empty(B, cout, P)
            new_coef = x.new_empty(cout, 4)
            if ctx.k4 and l == 1:
                part = x.new_empty(1, backend.pw_stat_slots(B, 1, cin, cout, P), cout, 4)
                backend.pw_layer_forward_k4(x3, w0c, w2[0], coef, y, part)
                backend.pw_stats_finalize(part, gamma, beta, rm, rv, momentum, eps, new_coef)
            elif ctx.k4 and l == 0:
                k4_mom = backend.k4_moments(x3)
                backend.k4_stat_finalize(k4_mom, w0c, gamma, beta, rm, rv, momentum, eps, float(B) * float(P), new_coef)
            elif l == 0 and cin <= 8 and not last:
                part = x.new_empty(backend.mlp_stream_parts(B, P), cout, 2)
                backend.mlp_stream_forward(src, w2[0].contiguous(), y, part)
                backend.mlp_stat_finalize(part, B * P, gamma, beta, rm, rv, momentum, eps, new_coef)
            else:
                part = x.new_empty(1, backend.pw_stat_slots(B, 1, cin, cout, P), cout, 4)

                def finalize():
                    backend.pw_stats_finalize(part, gamma, beta, rm, rv, momentum, eps, new_coef)
                    return new_coef
                if last:
                    pooled, argmax, raw = _pooled_layer(backend, src, w2, 1, coef, ns, y=y, stat_part=part,
                                                        norm_coef=finalize, zstar=tail)
                    if tail:
                        y = raw             # the raw extremum behind every pooled value
                else:
                    backend.pw_layer_forward(src, w2, in_coef=coef, in_relu=True, y=y, stat_part=part)
                    finalize()
            coef = new_coef
            ys.append(y)
            coefs.append(coef)
        ctx.tail = tail
        ctx.ns, ctx.fixed_lead = ns, int(fixed_lead)
        _save_chain(ctx, chain, (x3, pooled, argmax, k4_mom), ys, coefs, params)
        ctx.mark_non_differentiable(argmax)
        return pooled

    @staticmethod
    def backward(ctx, g):
        (x3, pooled, argmax, k4_mom), ys, coefs, lays = _saved_chain(ctx)
        ns, slots, need = ctx.ns, ctx.slots, ctx.needs_input_grad
        backend = backend_for(g)
        B, c0, P = x3.shape
        M = P // ns
        grads = [None] * len(slots)
        last, yl = lays[-1], ys[-1]
        cl = yl.shape[1]
        dgamma, dbeta = _dst(slots[last.ig], g, cl), _dst(slots[last.ibeta], g, cl)
        grads[last.ig], grads[last.ibeta] = dgamma, dbeta
        dy = pending = None
        top = len(lays) - 1
        if ctx.tail:
            # last layer without its dense tensors: yl is the raw extremum per (channel, group)
            wl = last.w
            need_w = need[ctx.lead + last.iw]
            dwl = _dst(slots[last.iw], g, cl, wl.shape[1]) if need_w else None
            pending = backend.pool_tail_backward(g.contiguous(), pooled, yl, argmax, coefs[-1], last.gamma,
                                                 wl.reshape(cl, wl.shape[1]), ys[-2], coefs[-2], ns,
                                                 dgamma, dbeta, dw=dwl)
            if need_w:
                grads[last.iw] = dwl.view_as(wl)
            top -= 1
        else:
            # last layer: BatchNorm + ReLU + max backward into the dense raw-output gradient
            dy = torch.empty_like(yl)
            backend.bn_relu_maxpool_backward(g.contiguous(), argmax, yl.view(B, cl, M, ns), pooled, last.gamma,
                                             None, coefs[-1], dy.view(B, cl, M, ns), dgamma, dbeta)

        def input_grad(dy, lay):
            # the layer kernel serves up to 256 output rows: the (at most 3) coordinate
            # rows in front are a separate skinny product, or zero when nobody reads them
            cout = lay.w.shape[0]
            w2 = lay.w.reshape(cout, c0)
            lead = 3 if c0 in (131, 259) else 0
            dx = dy.new_empty(B, c0, P)
            if backend.pw_supported(cout, c0 - lead, P):
                backend.pw_layer_forward(dy, w2[:, lead:].t().unsqueeze(0), y=dx[:, lead:])
                if lead and ctx.fixed_lead >= lead:
                    dx[:, :lead].zero_()
                elif lead:
                    torch.bmm(w2[:, :lead].t().unsqueeze(0).expand(B, -1, -1), dy,
                              out=dx[:, :lead])
            else:
                dx = torch.bmm(w2.t().unsqueeze(0).expand(B, -1, -1), dy)
            return dx.view(B, c0, M, ns)
        out = _chain_backward(backend, ctx, lays, x3, ys, coefs, grads, top, dy, pending,
                              input_grad=input_grad if need[0] else None, bottom=2 if ctx.k4 else 0)
        if not ctx.k4:
            return _returned(ctx, (out,), grads)
        # second layer over the rebuilt first activation: its fused norm backward + weight
        # gradient and ONLY the reductions of its input gradient -- they determine the
        # first layer's norm backward and weight gradient (nesie_k4_first_layer_wgrad) --
        # as one launch: the layer's dZ never leaves the chip
        da, part = out
        first, second = lays[:2]
        cout, cin = second.w.shape[0], second.w.shape[1]
        w0c = first.w.reshape(first.w.shape[0], c0)
        dgamma, dbeta = _dst(slots[second.ig], g, cout), _dst(slots[second.ibeta], g, cout)
        dw = _dst(slots[second.iw], g, 1, cout, cin)
        part, g_part = backend.pw_wgrad_bn_backward_k4_fused(
            da, ys[1], coefs[1], second.gamma, part, x3, w0c, coefs[0], second.w.reshape(cout, cin), dw,
            dgamma, dbeta, final=slots[second.iw] is not None)
        grads[second.iw], grads[second.ig], grads[second.ibeta] = dw.view_as(second.w), dgamma, dbeta
        dgamma0, dbeta0 = _dst(slots[first.ig], g, cin), _dst(slots[first.ibeta], g, cin)
        bnb = backend.pw_bnb_coef(part, coefs[0], first.gamma, float(B) * float(P), dgamma0, dbeta0)
        dw0 = _dst(slots[first.iw], g, cin, c0)
        backend.k4_first_layer_wgrad(k4_mom, w0c, bnb, g_part, dw0)
        grads[first.iw], grads[first.ig], grads[first.ibeta] = dw0.view_as(first.w), dgamma0, dbeta0
        return _returned(ctx, (), grads)


def _pooled_tail_whole(cin, cout):
    """True when a pooled last layer cin -> cout is a whole number of row tiles: the pooling
    epilogues of the layer kernel are built for whole row tiles only (pwconv.hip pw_geometry: 64
    rows for <= 64 channels over <= 128 inputs, else 128; pwconv_fwd.h GOW).  Any other width (a
    32-channel level, say) goes module by module."""
    return cout % 128 == 0 or (cout == 64 and cin <= 128)


def _native_norm(norm, training, only_2d=False):
    """True for the native norm layer with its ReLU folded in, in the asked mode: training = batch
    statistics, an affine transform and running statistics to update; evaluation = running
    statistics to apply."""
    from .norm import FusedBNReLU1d, FusedBNReLU2d
    if not (isinstance(norm, FusedBNReLU2d if only_2d else (FusedBNReLU1d, FusedBNReLU2d))
            and norm.fuse_relu and norm.track_running_stats):
        return False
    if training:
        return bool(norm.training and norm.affine and norm.momentum is not None)
    return not norm.training and norm.running_mean is not None


def _sa_layer_ok(layer, cin, training):
    """A bias-free 1x1 conv from ``cin`` channels with a native 2-D norm + ReLU behind it."""
    return (_native_norm(getattr(layer, 'norm', None), training, only_2d=True) and layer.act_fused
            and layer.conv.bias is None and layer.conv.in_channels == cin)


def sa_stack_supported(backend, x, layers):
    """True when ``SAStackFn`` serves this shared MLP: native training BatchNorm behind bias-free
    1x1 convs, fp32, nsample in {16, 32, 64}, every layer inside the built tiles."""
    if not ENABLED or backend.name != 'hip' or x.dtype != torch.float32 or x.dim() != 4 \
            or len(layers) < 2:
        return False
    B, c0, M, ns = x.shape
    if ns not in (16, 32, 64):
        return False
    P = M * ns
    cin = c0
    for i, layer in enumerate(layers):
        if not _sa_layer_ok(layer, cin, training=True):
            return False
        cout = layer.conv.out_channels
        first_stream = i == 0 and cin <= 8 and len(layers) > 1
        if not first_stream and not backend.pw_supported(cin, cout, P):
            return False
        if i > 0 and not backend.pw_supported(cout, cin, P):   # input-gradient product
            return False
        if i == len(layers) - 1 and not _pooled_tail_whole(cin, cout):
            return False
        cin = cout
    return True


def sa_stack_eval_supported(backend, x, layers):
    """True when ``sa_stack_eval`` serves this shared MLP: evaluation-mode norms with running
    statistics, no autograd, shapes inside the built tiles."""
    if not ENABLED or backend.name != 'hip' or x.dtype != torch.float32 or x.dim() != 4 \
            or len(layers) < 2 or torch.is_grad_enabled():
        return False
    B, cin, M, ns = x.shape
    if ns not in (16, 32, 64):
        return False
    for layer in layers:
        if not (_sa_layer_ok(layer, cin, training=False)
                and backend.pw_supported(cin, layer.conv.out_channels, M * ns)):
            return False
        if layer is layers[-1] and not _pooled_tail_whole(cin, layer.conv.out_channels):
            return False
        cin = layer.conv.out_channels
    return True


def sa_stack_eval(x, layers):
    """Evaluation-mode shared MLP + max pooling on the layer kernel: every layer's folded running
    statistics are the next layer's operand transform, the last layer leaves through the pooled
    tail (test path, ``simple_test``: conv + scale/bias pass + pooling pass per layer otherwise)."""
    backend = backend_for(x)
    x = x.contiguous()
    B, c0, M, ns = x.shape
    P = M * ns
    src, coef = x.view(B, c0, P), None
    for layer in layers[:-1]:
        cout, cin = layer.conv.out_channels, layer.conv.in_channels
        y = x.new_empty(B, cout, P)
        backend.pw_layer_forward(src, layer.conv.weight.reshape(1, cout, cin), in_coef=coef, in_relu=True, y=y)
        src, coef = y, layer.norm.eval_coef()
    layer = layers[-1]
    cout, cin = layer.conv.out_channels, layer.conv.in_channels
    part = x.new_empty(1, backend.pw_stat_slots(B, 1, cin, cout, P), cout, 4)
    return _pooled_layer(backend, src, layer.conv.weight.reshape(1, cout, cin), 1, coef, ns,
                         y=x.new_empty(B, cout, P), stat_part=part, norm_coef=layer.norm.eval_coef)[0]


def sa_stack(x, layers, fixed_lead=0):
    """Shared MLP + max pooling of a set-abstraction module through ``SAStackFn``;
    ``fixed_lead`` = leading channels of x whose gradient nobody consumes (see SAStackFn)."""
    from . import norm as _norm
    params, bufs = [], []
    for layer in layers:
        n = layer.norm
        params += [layer.conv.weight, n.weight, n.bias]
        bufs.append((n.running_mean, n.running_var, n.momentum, n.eps))
        _norm.count_batch(n.num_batches_tracked)
    return SAStackFn.apply(x, bufs, fixed_lead, *params)


class StackGroups(Function):
    """Several groups of S same-shaped tensors -> one stacked (S, ...) tensor per group, all
    filled by ONE multi-tensor copy (a ``torch.stack`` per group is a launch per group).  The
    gradient of a stacked tensor goes back as S views."""

    @staticmethod
    def forward(ctx, sizes, *tensors):
        outs, dst, off = [], [], 0
        for n in sizes:
            group = tensors[off:off + n]
            o = group[0].new_empty(n, *group[0].shape)
            outs.append(o)
            dst += list(o.unbind(0))
            off += n
        torch._foreach_copy_(dst, list(tensors))
        ctx.sizes = sizes
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        out = [None]
        for n, g in zip(ctx.sizes, grads):
            out += [None] * n if g is None else list(g.unbind(0))
        return tuple(out)


class CatRows(Function):
    """Same-width 2-D tensors (rows_i, C) -> their row concatenation (sum rows_i, C) filled by one
    multi-tensor copy; the gradient goes back as row slices.  1-D tensors concatenate likewise."""

    @staticmethod
    def forward(ctx, *tensors):
        rows = [t.shape[0] for t in tensors]
        out = tensors[0].new_empty(sum(rows), *tensors[0].shape[1:])
        torch._foreach_copy_(list(out.split(rows, 0)), [t.detach() for t in tensors])
        ctx.rows = rows
        return out

    @staticmethod
    def backward(ctx, g):
        return tuple(g.split(ctx.rows, 0))


def stack_groups(groups):
    """[[t_0 .. t_{S-1}], ...] -> [stacked (S, ...) per group]; S = 1 needs no copy at all, and
    neither does a group whose members sit side by side in the flat parameter vector
    (``grad_slots.stacked``: a view, with the group's gradient slot attached); the rest share one
    multi-tensor copy."""
    if len(groups[0]) == 1:
        return [g[0].unsqueeze(0) for g in groups]
    out = [grad_slots.stacked(g) for g in groups]
    rest = [i for i, o in enumerate(out) if o is None]
    if rest:
        flat = [t for i in rest for t in groups[i]]
        for i, o in zip(rest, StackGroups.apply(tuple(len(groups[i]) for i in rest), *flat)):
            out[i] = o
    return out


# ---- MiniPointNet (side_pooling_module.py:343-370) -------------------------------------------
# f = conv3(relu(bn0(c0))); g = max_G f; y = relu(bn1(W_g (g + b3) + W_l f + ...)); out = max_G conv4(y)
# split at the two places where small per-proposal tensors leave the big ones (g, and the
# per-proposal term `small` built from it with ordinary torch ops):
#   MiniHeadFn : c0 -> (f without its bias, max_G of it)
#   MiniTailFn : (f, small) -> max_G conv4(relu(bn1(W_l f + small)))

def mini_head_kernels(backend, c0, coef0, w3, G):
    """c0 (B,S,H0,P) raw, coef0 (S*H0,4) -> c = W3 . relu(coef0 c0) (B,S,half,P), its max over
    groups of G positions g (B,S,half,P/G) and the arg-max."""
    B, S, H0, P = c0.shape
    half = w3.shape[1]
    c = c0.new_empty(B, S, half, P)
    g, arg, _ = _pooled_layer(backend, c0, w3, S, coef0, G, y=c.view(B * S, half, P))
    return c, g, arg


def mini_tail_first(backend, c, small, wl, G):
    """y = W_l c + small (row bias per group of G positions) (B,S,H2,P) + its statistics partials."""
    B, S, half, P = c.shape
    H2 = wl.shape[1]
    y = c.new_empty(B, S, H2, P)
    part = c.new_empty(S, backend.pw_stat_slots(B * S, S, half, H2, P), H2, 4)
    backend.pw_layer_forward(c.view(B * S, half, P), wl, ng=S, row_bias=small.view(B * S, H2, -1),
                             rb_group=G, y=y.view(B * S, H2, P), stat_part=part)
    return y, part


def mini_tail_second(backend, y, coef1, w4, G):
    """max over groups of G positions of W4 . relu(coef1 y) -> (B,S,F,P/G) and the arg-max."""
    return _pooled_layer(backend, y, w4, y.shape[1], coef1, G)[:2]


def _mini_head_forward(backend, c0, c0_part, bufs, G, gamma0, beta0, w3):
    """-> (c, g, arg, coef0): the first norm's statistics from the producer's partials, then
    ``mini_head_kernels``."""
    B, S, H0, P = c0.shape
    rm, rv, momentum, eps = bufs
    coef0 = c0.new_empty(S * H0, 4)
    backend.mlp_stat_finalize(c0_part, B * P, gamma0, beta0, rm, rv, momentum, eps, coef0,
                              channel_major=True)
    c, g, arg = mini_head_kernels(backend, c0, coef0, w3, G)
    return c, g, arg, coef0


# MiniHeadFn and BlendMiniHeadFn take different inputs and END in the same three parameters: where these
# sit in ``needs_input_grad``, in ``ctx.slots`` and in the returned gradients is counted from the back.
# (The norm without a conv in front of W3 is no ``_Layer``: the two heads share the helpers below.)
_GAMMA0, _BETA0, _W3 = -3, -2, -1


def _mini_head_backward(backend, ctx, dc, dg, c0, coef0, arg, gamma0, w3):
    """-> (da0 (B*S, H0, P) = gradient of relu(bn0(c0)), reduction partials, where the first norm's
    backward writes dgamma and dbeta, dw3)."""
    B, S, H0, P = c0.shape
    G = ctx.G
    half = w3.shape[1]
    # (MiniTailFn.backward hands over a buffer it has just allocated and marks the tensor object:
    # that one is ours to write into; anything else is copied first)
    owned = dc is None or (dc.is_contiguous() and dc._base is None and getattr(dc, _OWNED_MARK, False))
    if dc is None:
        dc = c0.new_zeros(B, S, half, P)
    if dg is not None:
        # the pooled gradient joins the dense one at the arg-max -- in a buffer of our OWN:
        # autograd does not hand a backward ownership of its incoming gradients (the same
        # tensor may be another consumer's gradient, a hook's or a retained one)
        if not owned:
            dc = dc.clone(memory_format=torch.contiguous_format)
        dcv = dc.view(B, S, half, P // G, G)
        backend.group_max_pool_backward_add(dg.contiguous(), arg, dcv)
    else:
        dc = dc.contiguous()
    x0 = c0.view(B * S, H0, P)
    dcf = dc.view(B * S, half, P)
    dw3 = None
    if ctx.needs_input_grad[_W3]:
        # per-net weight gradient: the S nets are the S strided batch subsets
        dw3 = _wgrad(backend, dcf, x0, coef0, ng=S, slot=ctx.slots[_W3])
    da0 = c0.new_empty(B * S, H0, P)
    part = backend.pw_dgrad_bn_reduce(dcf, w3.transpose(1, 2), x0, coef0, da0, ng=S)
    return da0, part, _dst(ctx.slots[_GAMMA0], c0, S * H0), _dst(ctx.slots[_BETA0], c0, S * H0), dw3


def _first_norm_apply(backend, da0, part, c0, coef0, gamma0, dgamma, dbeta):
    """The first norm's backward as its own apply pass: (da0, part) of ``_mini_head_backward`` -> the
    gradient of c0; writes dgamma, dbeta."""
    B, S, H0, P = c0.shape
    dc0 = torch.empty_like(c0)
    backend.bn_relu_backward_apply(da0.view(B, S * H0, P), c0.view(B, S * H0, P), gamma0, None, coef0, part,
                                   dc0.view(B, S * H0, P), dgamma, dbeta)
    return dc0


class MiniHeadFn(Function):
    """c0 (B, S, H0, K*G) raw first-conv outputs of S stacked nets (+ their (sum, sum^2)
    partials) -> c = W3 . relu(bn0(c0)) (B, S, half, K*G) and g = max_G c (B, S, half, K)."""

    @staticmethod
    def forward(ctx, c0, c0_part, bufs, G, gamma0, beta0, w3):
        backend = backend_for(c0)
        c0 = c0.contiguous()
        c, g, arg, coef0 = _mini_head_forward(backend, c0, c0_part, bufs, G, gamma0, beta0, w3)
        ctx.G = G
        ctx.slots = _take_slots(ctx, _GAMMA0, (gamma0, beta0, w3))
        ctx.save_for_backward(c0, coef0, arg, gamma0, beta0, w3)
        ctx.mark_non_differentiable(arg)
        return c, g

    @staticmethod
    def backward(ctx, dc, dg):
        c0, coef0, arg, gamma0, beta0, w3 = ctx.saved_tensors
        backend = backend_for(c0)
        da0, part, dgamma, dbeta, dw3 = _mini_head_backward(backend, ctx, dc, dg, c0, coef0, arg, gamma0, w3)
        dc0 = _first_norm_apply(backend, da0, part, c0, coef0, gamma0, dgamma, dbeta)
        return _returned(ctx, (dc0,), (dgamma, dbeta, dw3))


class BlendMiniHeadFn(Function):
    """``interpolate.BlendConv`` (the first 1x1 conv of S MiniPointNets through the 3-NN blend,
    side_pooling_module.py:226-243, 346-349) and ``MiniHeadFn`` as ONE autograd node:
    (table (B, M, S*H0), wx (S, H0, 3)) -> (c, g) as MiniHeadFn.

    The first norm's backward is applied by the blend backward on its tile load
    (``nesie_blend_conv_backward_bn``): no apply pass, no dZ tensor.  That needs the blend
    backward to see the gradient of the NORMALISED activation together with (c0, reduction
    coefficients) -- state that must not travel through autograd as if it were a gradient (a
    second consumer of c0, a hook or ``retain_grad`` would silently turn it into garbage).  Inside
    one node c0 and da0 are locals: nothing else can consume, hook or accumulate into them."""

    @staticmethod
    def forward(ctx, table, wx, idx, weight, rel, segs, seg_len, bufs, G, gamma0, beta0, w3):
        backend = backend_for(table)
        table, wx = table.contiguous(), wx.contiguous()
        b, m, pitch = table.shape
        h = pitch // segs
        n = idx.shape[1]
        c0 = table.new_empty(b, segs, h, n // segs)
        c0_part = table.new_empty(segs * h, b * (n // segs // 64), 2)
        backend.blend_conv_forward(table, h, idx, weight, rel, wx, c0, segs, seg_len, h, 0,
                                   stat_partial=c0_part)
        c, g, arg, coef0 = _mini_head_forward(backend, c0, c0_part, bufs, G, gamma0, beta0, w3)
        ctx.G, ctx.dims = G, (segs, seg_len, b, m, pitch, h)
        ctx.slots = _take_slots(ctx, _GAMMA0, (gamma0, beta0, w3))
        ctx.save_for_backward(c0, coef0, arg, gamma0, w3, idx, weight, rel)
        ctx.mark_non_differentiable(arg)
        return c, g

    @staticmethod
    def backward(ctx, dc, dg):
        c0, coef0, arg, gamma0, w3, idx, weight, rel = ctx.saved_tensors
        segs, seg_len, b, m, pitch, h = ctx.dims
        backend = backend_for(c0)
        B, S, H0, P = c0.shape
        da0, part, dgamma, dbeta, dw3 = _mini_head_backward(backend, ctx, dc, dg, c0, coef0, arg, gamma0, w3)
        # (the staged backward writes every row; the atomic form adds into zeros)
        d_table = (c0.new_empty if backend.blend_backward_writes_table(h, idx.shape[1], segs, m) else c0.new_zeros)(b, m, pitch)
        d_wx = c0.new_empty(segs, h, 3)          # (written, not accumulated)
        if FOLD_NORM_BWD:
            bnb = backend.pw_bnb_coef(part, coef0, gamma0, float(B) * float(P), dgamma, dbeta)
            backend.blend_conv_backward(da0.view(B, S, H0, P), h, idx, weight, rel, d_table, d_wx,
                                        segs, seg_len, bn_z=c0, bnb=bnb)
        else:       # A/B switch: the separate apply pass
            dc0 = _first_norm_apply(backend, da0, part, c0, coef0, gamma0, dgamma, dbeta)
            backend.blend_conv_backward(dc0, h, idx, weight, rel, d_table, d_wx, segs, seg_len)
        return _returned(ctx, (d_table, d_wx), (dgamma, dbeta, dw3))


def blend_mini_head_supported(backend, table, idx, segs):
    """The blend forward leaves statistics partials (what ``BlendMiniHeadFn`` needs) for stacked
    channel counts that are multiples of 64 over whole 64-query tiles."""
    h, n = table.shape[2] // segs, idx.shape[1]
    return backend.name == 'hip' and h % 64 == 0 and (n // segs) % 64 == 0


class MiniTailFn(Function):
    """c (B, S, half, K*G), small (B, S, H2, K), W_l (S, H2, half), bn1, W4 (S, F, H2) ->
    max_G W4 . relu(bn1(W_l c + small)) (B, S, F, K); the (B, S, F, K*G) tensor is never written."""

    @staticmethod
    def forward(ctx, c, small, bufs, G, wl, gamma1, beta1, w4):
        backend = backend_for(c)
        c, small = c.contiguous(), small.contiguous()
        B, S, half, P = c.shape
        H2 = wl.shape[1]
        rm, rv, momentum, eps = bufs
        y, part = mini_tail_first(backend, c, small, wl, G)
        coef1 = c.new_empty(S * H2, 4)
        backend.pw_stats_finalize(part, gamma1, beta1, rm, rv, momentum, eps, coef1)
        out, arg = mini_tail_second(backend, y, coef1, w4, G)
        # two layers: W_l with the norm (the row bias ``small`` joins its output), W4 without one, pooled
        # directly (no raw output).  W_l is half of a split: autograd's concatenation places its gradient.
        chain = _chain_layout([Stack1dLayer(False, bufs), Stack1dLayer(False, None)])
        ctx.G = G
        _save_chain(ctx, chain, (c, arg), (y.view(B * S, H2, P), None), (coef1, None), (wl, gamma1, beta1, w4),
                    no_slot=(chain[0].iw,))
        ctx.mark_non_differentiable(arg)
        return out

    @staticmethod
    def backward(ctx, dout):
        (c, arg), ys, coefs, lays = _saved_chain(ctx)
        backend = backend_for(c)
        B, S, half, P = c.shape
        G, top = ctx.G, lays[-1]
        F, H2 = top.w.shape[1:]
        grads = [None] * len(ctx.slots)
        enter, dz, pending = len(lays) - 1, None, None
        if mini_tail_sparse_supported(backend, F, H2, G, P):
            # No norm and no ReLU between conv4 and the max: the gradient of its output is ONE non-zero
            # per (channel, group) -- kept as entries (value, position); the dense (B S, F, P) tensor
            # is never formed.  The input gradient builds its operand rows from them (bit for bit the
            # dense launch's result), the weight gradient is a sparse product on the vector ALUs that
            # leaves the dense launch's partials (bit for bit its dW4, deferred reduction included).
            ent = backend.pool_tail_pack(dout.contiguous().view(B * S, F, P // G), arg.view(B * S, F, P // G))
            if ctx.needs_input_grad[ctx.lead + top.iw]:
                slot = ctx.slots[top.iw]
                grads[top.iw] = _dst(slot, c, S, F, H2)
                backend.pw_wgrad_sparse(ent, G, ys[0], grads[top.iw], ng=S, x_coef=coefs[0], final=slot is not None)
            da = c.new_empty(B * S, H2, P)
            part = backend.pw_dgrad_bn_reduce_sparse(ent, G, _transposed(top.w), ys[0], coefs[0], da, ng=S)
            enter, pending = enter - 1, (da, part)      # the top layer is done: on with the norm backward below it
        else:
            # gradient of the last conv's output: the pooled gradient at the arg-max, zero elsewhere
            dz = c.new_empty(B, S, F, P // G, G)
            backend.group_max_pool_backward(dout.contiguous(), arg, dz)
            dz = dz.view(B * S, F, P)

        def input_grad(dy, lay, dsmall):
            dc = torch.empty_like(c)
            backend.pw_layer_forward(dy, _transposed(lay.w), ng=S, y=dc.view(B * S, half, P))
            setattr(dc, _OWNED_MARK, True)      # nobody else holds this gradient buffer
            return dc, dsmall.view(B, S, H2, -1)
        inputs = _chain_backward(backend, ctx, lays, c.view(B * S, half, P), ys, coefs, grads, enter, dz, pending,
                                 ng=S, input_grad=input_grad, rb_group=G)
        return _returned(ctx, inputs, grads)


# Tests flip this to obtain the dense backward of the MiniPointNet tail on the same inputs.
MINI_TAIL_SPARSE = True


def mini_tail_sparse_supported(backend, F, H2, G, P):
    """The MiniPointNet tail's backward runs from the max-pool's entries (no dense gradient of conv4's
    output) at the built shape: F = 128, H2 = 256, G in {16, 64}, whole 64-position tiles."""
    return (MINI_TAIL_SPARSE and backend.name == 'hip' and F == 128 and H2 == 256 and G in (16, 64)
            and P % 64 == 0 and backend.pw_wgrad_sparse_supported(F, H2, P, G))


def mini_pointnets_fused_supported(backend, c0, c0_part, G):
    if not ENABLED or backend.name != 'hip' or c0.dtype != torch.float32 or c0_part is None \
            or G not in (16, 64):
        return False
    B, S, H0, P = c0.shape[0], c0.shape[1], c0.shape[2], c0.shape[3] * c0.shape[4]
    return (c0_part.numel() > 0 and backend.pw_supported(H0, H0 // 2, P)
            and backend.pw_supported(H0 // 2, H0, P))


# ---- 1-D per-seed / per-proposal stacks ----------------------------------------------------------
# VoteModule (vote_module.py:65-74, 85-147), the prediction head's trunk and its three output
# convolutions (reliable_conv_bbox_module.py:112-141, 144-177), the feature-propagation MLPs
# (point_fp_module.py:31-37) and the quality head's score heads (side_pooling_module.py:55-78, 318):
# chains of Conv1d(1x1) [-> BatchNorm1d -> ReLU] over (B, C, P) with P = 256 .. 1024.  The reference
# runs them op by op; here a chain is ONE autograd function on the layer kernel, like the
# set-abstraction stacks: per layer one forward launch (previous norm + ReLU folded into the operand
# load, this layer's statistics from the accumulators), and in the backward one input-gradient
# launch with the norm reduction, one weight-gradient launch and one norm apply pass.

class SplitXyzFeat(Function):
    """w (S, H, 3 + C) -- the stacked first-conv weights of S MiniPointNets, whose input is
    cat[rel_xyz (3), blended features (C)] (side_pooling_module.py:226-243, 346-349) -> (w_xyz (S, H, 3)
    contiguous, w_feat (S * H, C) as a strided VIEW).  Two plain slices cost autograd two zero-filled
    (S, H, 3 + C) tensors, two slice copies and an addition on the way back; here the two gradients
    are written side by side with ONE concatenation, straight into the weight's slot of the flat
    gradient vector when there is one."""

    @staticmethod
    def forward(ctx, w):
        S, H, K = w.shape
        ctx.dims = (S, H, K)
        ctx.slot = grad_slots.take(w) if ctx.needs_input_grad[0] else None
        return w[:, :, :3].contiguous(), w[:, :, 3:].reshape(S * H, K - 3)

    @staticmethod
    def backward(ctx, d_xyz, d_feat):
        S, H, K = ctx.dims
        like = d_xyz if d_xyz is not None else d_feat
        if d_xyz is None:
            d_xyz = like.new_zeros(S, H, 3)
        if d_feat is None:
            d_feat = like.new_zeros(S * H, K - 3)
        out = ctx.slot.view(S, H, K) if ctx.slot is not None else like.new_empty(S, H, K)
        torch.cat([d_xyz.view(S, H, 3), d_feat.view(S, H, K - 3)], dim=2, out=out)
        return out


class AddChannelBias(Function):
    """x (B, S, F, K) + bias (S, F) broadcast over batch and positions (the conv bias a max-pool
    commutes with, added after pooling: side_pooling_module.py:357, 361-368).  The backward hands the
    gradient through untouched and sums the bias gradient with one native launch per call
    (``channel_sum``) instead of autograd's sum-to-size reduction."""

    @staticmethod
    def forward(ctx, x, bias):
        ctx.dims = tuple(x.shape)
        return x + bias.view(1, bias.shape[0], -1, 1)

    @staticmethod
    def backward(ctx, g):
        B, S, F, K = ctx.dims
        db = None
        if ctx.needs_input_grad[1]:
            backend = backend_for(g)
            if hasattr(backend, 'channel_sum'):
                # (scene, net) runs over the batch axis of a (B * S, F, K) view; a channel slice of a
                # wider gradient (the cat in front of the score heads) keeps a uniform stride there
                if g.stride(3) == 1 and g.stride(2) == K and g.stride(0) == S * g.stride(1):
                    gv = g.as_strided((B * S, F, K), (g.stride(1), K, 1))
                else:
                    gv = g.contiguous().view(B * S, F, K)
                db = backend.channel_sum(gv, ng=S).view(S, F)
            else:
                db = g.sum((0, 3))
        return g, db


class Stack1dFn(Function):
    """x (NB, C0, P), batch n uses weight group n % S.  Layers l = 0 .. L-1:
    y_l = W_l . a_{l-1} (+ bias_l), a_l = relu(bn_l(y_l)) for a layer with a norm, a_l = y_l
    without.  Returns a_{L-1}.  Tensors after ``layers``: per layer W (S, Cout, Cin), then bias
    (S * Cout) if the conv has one, then gamma, beta (S * Cout) if it has a norm.

    A conv bias in FRONT of a norm is never added: the mean subtraction removes it from every
    normalised value; the running mean gets it (``pw_stats_finalize(chan_bias=)``) and its
    gradient -- identically zero -- is returned as a zero tensor, as ATen does (a None would make a
    per-parameter optimiser skip the parameter: no weight decay on it, "unused parameter" under
    DDP)."""

    @staticmethod
    def forward(ctx, x, layers, S, *tensors):
        backend = backend_for(x)
        x = x.contiguous()
        NB, c0, P = x.shape
        chain = _chain_layout(layers)
        src, coef = x, None
        ys, coefs = [], []
        for lay in _bind(chain, tensors):
            w, b = lay.w, None if lay.b is None else lay.b.detach().contiguous()
            cout = w.shape[1]
            y = x.new_empty(NB, cout, P)
            if lay.bn is not None:
                rm, rv, momentum, eps = lay.bn
                part = x.new_empty(S, backend.pw_stat_slots(NB, S, w.shape[2], cout, P), cout, 4)
                backend.pw_layer_forward(src, w, ng=S, in_coef=coef, in_relu=True, y=y, stat_part=part)
                coef = x.new_empty(S * cout, 4)
                backend.pw_stats_finalize(part, lay.gamma, lay.beta, rm, rv, momentum, eps, coef, chan_bias=b)
            else:
                backend.pw_layer_forward(src, w, ng=S, in_coef=coef, in_relu=True, y=y, bias=b)
                coef = None
            ys.append(y)
            coefs.append(coef)
            src = y
        out = ys[-1]
        if chain[-1].bn is not None:      # the last activation is somebody's input: materialise it
            cl = out.shape[1]
            act = torch.empty_like(out)
            backend.affine_relu_forward(out.view(NB // S, S * cl, P), coefs[-1], True,
                                        act.view(NB // S, S * cl, P))
            out = act
        ctx.S = S
        _save_chain(ctx, chain, (x,), ys, coefs, tensors)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,), ys, coefs, lays = _saved_chain(ctx)
        S, slots, need = ctx.S, ctx.slots, ctx.needs_input_grad
        backend = backend_for(dout)
        NB, c0, P = x.shape
        B = NB // S
        grads = [None] * len(slots)
        last = lays[-1]
        # a channel slice of a wider gradient (the outputs of several chains concatenated by their
        # consumer) is batch-strided: the layer kernels take a batch stride, no copy needed
        if not (S == 1 and last.bn is None and dout.stride(2) == 1 and dout.stride(1) == P):
            dout = dout.contiguous()
        # gradient of the last layer's RAW output
        cl = ys[-1].shape[1]
        if last.bn is not None:
            dz = torch.empty_like(ys[-1])
            dgamma, dbeta = _dst(slots[last.ig], dout, S * cl), _dst(slots[last.ibeta], dout, S * cl)
            backend.bn_relu_backward(dout.view(B, S * cl, P), ys[-1].view(B, S * cl, P), None, last.gamma,
                                     last.beta, None, None, coefs[-1], True, dz.view(B, S * cl, P), dgamma, dbeta)
            grads[last.ig], grads[last.ibeta] = dgamma, dbeta
        else:
            dz = dout
            if last.b is not None and need[ctx.lead + last.ib]:
                # (one workgroup per channel in a fixed order: ATen's two-axis reduction took 13 - 18 us)
                grads[last.ib] = backend.channel_sum(dz if S == 1 else dz.view(B, S * cl, P))

        def input_grad(dz, lay):
            if not need[0]:
                return None
            cout, cin = lay.w.shape[1], lay.w.shape[2]
            if not backend.pw_supported(cout, cin, P):
                return torch.matmul(lay.w.transpose(1, 2).unsqueeze(0), dz.view(B, S, cout, P)).view(NB, cin, P)
            dx = dz.new_empty(NB, cin, P)
            backend.pw_layer_forward(dz, lay.w.transpose(1, 2), ng=S, y=dx)
            return dx
        dx = _chain_backward(backend, ctx, lays, x, ys, coefs, grads, len(lays) - 1, dz, ng=S, input_grad=input_grad)
        for lay in lays:
            if lay.bn is not None and lay.b is not None and need[ctx.lead + lay.ib]:
                # the bias in front of a norm: gradient identically zero.
                # With a slot in the flat gradient vector the answer is None: FlatTrainState.collect()
                # zero-fills every parameter that got no gradient (one multi-tensor fill for all of
                # them), so whatever an earlier step, another path or a loaded vector left in the slot
                # is overwritten in every step.  Without a flat state: a zero tensor, as ATen returns
                # (a None would make a per-parameter optimiser skip the parameter).
                grads[lay.ib] = None if slots[lay.ib] is not None else torch.zeros_like(lay.b)
        return _returned(ctx, (dx,), grads)


def stack1d_supported(backend, x, shapes, norms, S=1):
    """True when ``Stack1dFn`` serves the chain: ``shapes`` = [(Cin, Cout), ...], ``norms`` = the
    norm layer (or None) behind each conv; native training BatchNorm1d/2d with a folded ReLU,
    fp32, every forward and input-gradient product inside the built tiles, only the LAST layer
    may come without a norm."""
    if not ENABLED or backend.name != 'hip' or x.dtype != torch.float32 or not torch.is_grad_enabled():
        return False
    P = x.shape[-1] if x.dim() == 3 else x.numel() // (x.shape[0] * x.shape[1])
    for i, ((cin, cout), norm) in enumerate(zip(shapes, norms)):
        if norm is None:
            if i != len(shapes) - 1:
                return False
        elif not _native_norm(norm, training=True):
            return False
        if not backend.pw_supported(cin, cout, P):
            return False
        if i > 0 and not backend.pw_supported(cout, cin, P):
            return False
    return True


def stack1d(x, convs, norms, S=1, weights=None, biases=None, gammas=None, betas=None, stats=None):
    """Run a conv / norm chain through ``Stack1dFn``.  ``convs`` / ``norms``: one module (or, for
    S > 1, a list of S structurally identical modules) per layer; norms[i] None = plain conv.
    ``weights`` etc.: pre-stacked tensors for S > 1 (see side_pooling.batched_heads)."""
    from . import norm as _norm
    layers, tensors = [], []
    for i, (conv, norm) in enumerate(zip(convs, norms)):
        first_conv = conv[0] if isinstance(conv, (list, tuple)) else conv
        first_norm = norm[0] if isinstance(norm, (list, tuple)) else norm
        w = weights[i] if weights is not None else first_conv.weight.flatten(1).unsqueeze(0)
        tensors.append(w)
        has_bias = first_conv.bias is not None
        if has_bias:
            tensors.append(biases[i] if biases is not None else first_conv.bias)
        bn = None
        if first_norm is not None:
            tensors += [gammas[i] if gammas is not None else first_norm.weight,
                        betas[i] if betas is not None else first_norm.bias]
            rm, rv = stats[i] if stats is not None else (first_norm.running_mean, first_norm.running_var)
            bn = (rm, rv, first_norm.momentum, first_norm.eps)
            for n in (norm if isinstance(norm, (list, tuple)) else [norm]):
                _norm.count_batch(n.num_batches_tracked)
        layers.append(Stack1dLayer(has_bias, bn))
    return Stack1dFn.apply(x, tuple(layers), S, *tensors)
