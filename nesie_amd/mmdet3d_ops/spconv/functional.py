"""The feature products of the sparse layers as autograd Functions (the role of
``mmdet3d/ops/spconv/functional.py``).  All of them are one operation, the gather-GEMM
``out[r] = sum_k src[table[r, k]] . W[k]`` (``nesie_spconv_gather_gemm``), with the table and the
weight's orientation chosen per product; the weight gradient is ``nesie_spconv_wgrad``.  No float
atomics anywhere: outputs and gradients are bit-identical from run to run."""
import torch
from torch.autograd import Function

from ..roiaware_pool3d import _hip_backend


def _features_2d(name, features, filters):
    if features.dtype != torch.float32 or filters.dtype != torch.float32:
        raise NotImplementedError(f'{name}: float32 only, got features {features.dtype} and '
                                  f'filters {filters.dtype} (fp16 is not built)')
    if features.dim() != 2 or filters.dim() != 5 or filters.shape[3] != features.shape[1]:
        raise TypeError(f'{name}: expected features (N, Cin) and filters (kz, ky, kx, Cin, Cout), '
                        f'got {tuple(features.shape)} and {tuple(filters.shape)}')


class _GatherConv(Function):

    @staticmethod
    def forward(ctx, features, filters, table, table_t):
        """features (S, Cin), filters (kz, ky, kx, Cin, Cout), table (R, K) rows of ``features``
        or -1, table_t (S, K) its transpose (rows of the output or -1) -> (R, Cout)."""
        backend = _hip_backend('sparse convolution', features)
        features, filters = features.contiguous(), filters.contiguous()
        rows, cout = int(table.shape[0]), int(filters.shape[4])
        assert table_t.shape[0] == features.shape[0] and table.shape[1] == table_t.shape[1]
        assert table.shape[1] == filters.shape[0] * filters.shape[1] * filters.shape[2]
        ctx.save_for_backward(features, filters, table, table_t)
        if rows == 0 or features.shape[0] == 0:
            return features.new_zeros((rows, cout))
        out = features.new_empty((rows, cout))                           # written in full
        backend.spconv_gather_gemm(features, filters, table, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        features, filters, table, table_t = ctx.saved_tensors
        need_in, need_w = ctx.needs_input_grad[:2]
        grad_in = grad_w = None
        empty = table.shape[0] == 0 or features.shape[0] == 0
        if empty:
            grad_in = torch.zeros_like(features) if need_in else None
            grad_w = torch.zeros_like(filters) if need_w else None
            return grad_in, grad_w, None, None
        backend = _hip_backend('sparse convolution', features)
        grad_out = grad_out.contiguous()
        if need_in:
            grad_in = torch.empty_like(features)                         # written in full
            backend.spconv_gather_gemm(grad_out, filters, table_t, grad_in, weight_transposed=True)
        if need_w:
            grad_w = torch.empty_like(filters)                           # written in full
            backend.spconv_wgrad(features, grad_out, table, grad_w)
        return grad_in, grad_w, None, None


def indice_conv(features, filters, rules, pair_num, num_activate_out):
    """A regular sparse conv: features (N, Cin) -> (M, Cout) through ``rules.nbr``."""
    _features_2d('indice_conv', features, filters)
    assert rules.nbr.shape[0] == num_activate_out
    return _GatherConv.apply(features, filters, rules.nbr, rules.nbr_t)


def indice_subm_conv(features, filters, rules, pair_num, num_activate_out):
    """A submanifold conv: the output rows are the input rows."""
    _features_2d('indice_subm_conv', features, filters)
    assert rules.nbr.shape[0] == num_activate_out
    return _GatherConv.apply(features, filters, rules.nbr, rules.nbr_t)


def indice_inverse_conv(features, filters, rules, pair_num, num_activate_out):
    """The inverse of the conv that built ``rules``: features (M, Cin') at that conv's output
    sites -> (N, Cout') at its input sites, through ``rules.nbr_t``."""
    _features_2d('indice_inverse_conv', features, filters)
    assert rules.nbr_t.shape[0] == num_activate_out
    return _GatherConv.apply(features, filters, rules.nbr_t, rules.nbr)
