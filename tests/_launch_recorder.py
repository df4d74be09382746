"""A back end for ``kernels.use_backend`` that launches nothing and writes down what it was asked to
launch: the host side of the fused MLP chains (``mmdet3d_ops/fused_mlp.py``) then runs end to end
on CPU tensors, and which kernels a chain issues, in which order and over which buffers becomes a
list that a test can compare.

A call is logged as [method, positional arguments, keyword arguments], bound to the signature of
the ``kernels.HipKernels`` method of that name with its defaults filled in.  A tensor is logged as
{"T": [storage, offset, shape, strides, dtype]} with ``storage`` numbered in order of first
appearance in the log, so two arguments that share memory (a gradient slot and the view a kernel
writes, ``dz`` written over ``da``) show the same number.  Every tensor seen is kept alive: an
address is never reused for another buffer while a case runs."""
import inspect

import torch

from nesie_amd.kernels import HipKernels

# the questions a caller asks before it picks a route: answered from the case's table, yes by default
_QUESTIONS = ('pw_wgrad_tiled', 'blend_backward_writes_table')
STAT_SLOTS = 2          # pw_stat_slots
STREAM_PARTS = 3        # mlp_stream_parts


class LaunchRecorder:
    name = 'hip'

    def __init__(self, answers=None):
        """``answers``: {question: bool or callable(*args) -> bool}, e.g. {'k4_supported': False}."""
        self.answers = dict(answers or {})
        self.log = []
        self._storages = {}
        self._keep = []

    # ---- description of an argument ------------------------------------------------------------
    def describe(self, v):
        if torch.is_tensor(v):
            self._keep.append(v)
            key = v.untyped_storage()._cdata
            number = self._storages.setdefault(key, len(self._storages))
            return {'T': [number, v.storage_offset(), list(v.shape), list(v.stride()),
                          str(v.dtype).replace('torch.', '')]}
        if isinstance(v, (tuple, list)):
            return [self.describe(e) for e in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f'cannot log an argument of type {type(v).__name__}')

    def note(self, what, values):
        """An entry that is no kernel call (the tuple a backward returned)."""
        self.log.append([what, self.describe(values), {}])

    def _new(self, like, *shape, dtype=torch.float32):
        t = torch.zeros(*shape, dtype=dtype, device=like.device)
        self._keep.append(t)
        return t

    # ---- the back end --------------------------------------------------------------------------
    def pw_stat_slots(self, nb, ng, k, cout, p):
        return STAT_SLOTS

    def mlp_stream_parts(self, b, p):
        return STREAM_PARTS

    def __getattr__(self, method):
        if method.startswith('_'):
            raise AttributeError(method)
        if method.endswith('_supported') or method in _QUESTIONS:
            def ask(*args):
                answer = self.answers.get(method, True)
                return bool(answer(*args)) if callable(answer) else bool(answer)
            return ask

        signature = inspect.signature(getattr(HipKernels, method))     # unknown method: AttributeError
        takes_self = next(iter(signature.parameters), None) == 'self'

        def call(*args, **kwargs):
            # bound to the real method's signature (a misspelt keyword fails here as it would on the
            # device) with the defaults filled in: the log does not depend on how a caller spells a call
            bound = signature.bind(*((None,) if takes_self else ()), *args, **kwargs)
            bound.apply_defaults()
            args, kwargs = bound.args[1:] if takes_self else bound.args, bound.kwargs
            self.log.append([method, self.describe(args), {k: self.describe(kwargs[k]) for k in sorted(kwargs)}])
            result = getattr(self, '_result_' + method, None)
            return None if result is None else result(*args, **kwargs)
        return call

    # ---- results that the callers use (shapes as kernels.HipKernels returns them) ---------------
    def _result_pw_dgrad_bn_reduce(self, dy, w, z, z_coef, da, ng=1):
        return self._new(dy, ng * w.shape[1], STAT_SLOTS, 2)

    def _result_pw_dgrad_bn_reduce_sparse(self, ent, ns, w, z, z_coef, da, ng=1):
        return self._new(z, ng * z.shape[1], STAT_SLOTS, 2)

    def _result_pw_bnb_coef(self, part, z_coef, gamma, count, dgamma, dbeta):
        return self._new(part, part.shape[0], 8)

    def _result_channel_sum(self, x, out=None, ng=1):
        return out if out is not None else self._new(x, ng * x.shape[1])

    def _result_pool_tail_backward(self, g, pooled, zstar, argmax, coef, gamma, w, z_prev, coef_prev, ns,
                                   dgamma, dbeta, dw=None):
        nb, k, p = z_prev.shape
        return self._new(g, nb, k, p), self._new(g, k, STAT_SLOTS, 2)

    def _result_pool_tail_pack(self, g, argmax, pooled=None):
        nb, c, m = g.shape
        return self._new(g, nb, m, c, 2)

    def _result_pw_wgrad_bn_backward_k4_fused(self, da, z, z_coef, gamma, part, x4, w0, x_coef, w, dw, dgamma,
                                              dbeta, final=False):
        return self._new(da, 64, STAT_SLOTS, 2), self._new(da, 64, STAT_SLOTS, 4)

    def _result_k4_moments(self, x4):
        return self._new(x4, 2, 20, dtype=torch.float64)
