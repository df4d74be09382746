"""kNN grouping, the tier that needs no GPU: the C entry's prototype and argument checks, the
package surface, the constructors of QueryAndGroup / the SA modules, and ``uniform_resample``."""
import ctypes

import pytest
import torch

from nesie_amd import _lib


def test_entry_is_declared_with_the_reference_argument_order():
    c = ctypes
    assert _lib.SIGNATURES["nesie_knn_wrapper"] == (c.c_int, [c.c_int] * 4 + [c.c_void_p] * 5)


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    for args in ((1, 5, 4, 0), (-1, 5, 4, 3), (1, -5, 4, 3), (1, 5, -4, 3), (1, 5, 4, -2)):
        assert lib.nesie_knn_wrapper(*args, None, None, None, None, None) == 1, args
        assert b"knn_wrapper" in lib.nesie_last_error()
    assert lib.nesie_knn_wrapper(1, 5, 4, 129, None, None, None, None, None) == 2
    assert b"knn_wrapper" in lib.nesie_last_error()
    # empty problems succeed without touching the device
    assert lib.nesie_knn_wrapper(0, 5, 4, 3, None, None, None, None, None) == 0
    assert lib.nesie_knn_wrapper(2, 5, 0, 3, None, None, None, None, None) == 0
    # null pointers for a problem that is not empty are an argument error, not a crash
    assert lib.nesie_knn_wrapper(1, 5, 4, 3, None, None, None, None, None) == 1
    assert lib.nesie_knn_wrapper(1, 0, 4, 3, None, None, None, None, None) == 1


def test_knn_is_the_real_op():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import knn
    from nesie_amd.mmdet3d_ops.knn import KNN
    assert 'knn' not in mmdet3d_ops._OUT_OF_SCOPE and 'knn' in mmdet3d_ops._HOT
    assert 'knn' in mmdet3d_ops.__all__
    assert knn == KNN.apply
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn(4, torch.rand(1, 32, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn(4, torch.rand(1, 3, 32), torch.rand(1, 3, 8), True)
    with pytest.raises(AssertionError):
        knn(0, torch.rand(1, 32, 3))
    with pytest.raises(AssertionError):
        knn(4, torch.rand(1, 3, 32).transpose(1, 2))      # not contiguous
    # the other names keep their stubs
    with pytest.raises(NotImplementedError):
        mmdet3d_ops.assign_score_withk()


def test_constructors():
    from nesie_amd.mmdet3d_ops import (PointSAModule, PointSAModuleMSG, QueryAndGroup,
                                       build_sa_module)
    from nesie_amd.mmdet3d_ops.group_points import sample_query_group_supported
    g = QueryAndGroup(None, 16)
    assert g.max_radius is None and g.sample_num == 16
    with pytest.raises(AssertionError, match="normalize"):
        QueryAndGroup(None, 16, normalize_xyz=True)
    u = QueryAndGroup(0.2, 16, uniform_sample=True)
    assert u.uniform_sample and u.generator is None
    QueryAndGroup(0.2, 16, uniform_sample=True, return_unique_cnt=True)
    with pytest.raises(AssertionError):
        QueryAndGroup(0.2, 16, return_unique_cnt=True)
    sa = PointSAModule(num_point=64, radius=None, num_sample=16, mlp_channels=[8, 16, 16, 32])
    assert sa.groupers[0].max_radius is None
    msg = PointSAModuleMSG(num_point=64, radii=[None, 0.4], sample_nums=[8, 16],
                           mlp_channels=[[8, 16], [8, 16]])
    assert [g.max_radius for g in msg.groupers] == [None, 0.4]
    built = build_sa_module(dict(type='PointSAModule', num_point=64, radius=None, num_sample=16,
                                 mlp_channels=[8, 16, 16, 32]))
    assert built.groupers[0].max_radius is None
    with pytest.raises(AssertionError, match="dilated_group"):
        PointSAModuleMSG(num_point=64, radii=[None, 0.4], sample_nums=[8, 16],
                         mlp_channels=[[8, 16], [8, 16]], dilated_group=True)
    # the fused sample + group node is the ball query's only
    x = torch.rand(1, 32, 3, requires_grad=True)
    assert sample_query_group_supported(x, torch.rand(1, 4, 32), g) is False


def _check_rows(idx, out, cnt):
    """Every deterministic property of uniform_resample's rows."""
    ns = idx.shape[-1]
    assert out.shape == idx.shape and out.dtype == idx.dtype
    assert cnt.shape == idx.shape[:-1] and cnt.dtype == torch.float32
    for row_in, row_out, c in zip(idx.reshape(-1, ns), out.reshape(-1, ns), cnt.reshape(-1)):
        distinct = torch.unique(row_in)                    # sorted
        count = distinct.numel()
        assert float(c) == count
        assert torch.equal(row_out[:count], distinct)
        assert torch.isin(row_out[count:], distinct).all()


def test_uniform_resample_rows():
    from nesie_amd.mmdet3d_ops.group_points import uniform_resample
    equal = torch.full((1, 1, 8), 5, dtype=torch.int32)
    out, cnt = uniform_resample(equal)
    assert torch.equal(out, equal) and cnt.tolist() == [[1.0]]

    distinct = torch.tensor([[[7, 3, 9, 1, 0, 12, 4, 2]]], dtype=torch.int32)
    out, cnt = uniform_resample(distinct)
    assert out.tolist() == [[[0, 1, 2, 3, 4, 7, 9, 12]]] and cnt.tolist() == [[8.0]]   # sorted, no draws

    mixed = torch.tensor([[[4, 4, 2, 9, 2, 4, 4, 4]]], dtype=torch.int32)
    out, cnt = uniform_resample(mixed)
    assert out[0, 0, :3].tolist() == [2, 4, 9] and cnt.tolist() == [[3.0]]
    _check_rows(mixed, out, cnt)

    g = torch.Generator().manual_seed(3)
    batch = torch.randint(0, 6, (2, 3, 8), generator=g, dtype=torch.int32)
    batch[1, 2] = torch.arange(8, dtype=torch.int32).flip(0)        # a full row inside the batch
    a, cnt_a = uniform_resample(batch, torch.Generator().manual_seed(11))
    b, cnt_b = uniform_resample(batch, torch.Generator().manual_seed(11))
    _check_rows(batch, a, cnt_a)
    assert torch.equal(a, b) and torch.equal(cnt_a, cnt_b)
    assert a[1, 2].tolist() == list(range(8)) and cnt_a[1, 2] == 8
    # the draws do depend on the stream: 2 * 3 * 8 slots, most of them draws
    others = [uniform_resample(batch, torch.Generator().manual_seed(s))[0] for s in (12, 13, 14)]
    assert any(not torch.equal(a, o) for o in others)
    # long indices pass through with their dtype
    out, _ = uniform_resample(mixed.long())
    assert out.dtype == torch.int64
