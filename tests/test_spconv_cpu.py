"""Sparse convolution, the tier that needs no GPU: the referee (tests/_spconv_ref.py) against
torch's dense convolutions, the package surface, the constructors' refusals, the layers' refusal
of CPU tensors and the C entries' argument checks."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

from nesie_amd import _lib
from nesie_amd.mmdet3d_ops import spconv
from tests import _spconv_ref as R

# (kernel, stride, padding, subm): the five geometries of the issue and a 1 x 1 x 1
GEOMETRIES = [
    ((3, 3, 3), 1, 1, True),
    ((3, 3, 3), 1, 0, False),
    ((3, 3, 3), 2, 1, False),
    ((3, 1, 1), (2, 1, 1), 0, False),
    ((2, 2, 2), 2, 0, False),
    ((1, 3, 3), 1, 0, True),
    ((1, 1, 1), 1, 0, False),
]
SHAPE, BATCH = (7, 6, 9), 2


def _case(seed, n=90, cin=3, cout=4, ksize=(3, 3, 3)):
    rng = np.random.default_rng(seed)
    idx = R.random_sites(rng, n, BATCH, SHAPE)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(n, cin, generator=g, dtype=torch.float64)
    weight = torch.randn(*ksize, cin, cout, generator=g, dtype=torch.float64)
    return idx, feats, weight


@pytest.mark.parametrize('ksize,stride,padding,subm', GEOMETRIES)
def test_referee_tables_reproduce_the_dense_convolution(ksize, stride, padding, subm):
    idx, feats, weight = _case(1, ksize=ksize)
    outids, nbr, nbr_t, pair_num = R.rulebook(idx, BATCH, SHAPE, ksize, stride, padding, subm)
    dense = R.dense_conv(feats, idx, BATCH, SHAPE, weight, stride, padding, subm)
    _, _, _, out_shape = R.geometry(SHAPE, ksize, stride, padding, subm)
    # the output-size formula is torch's
    assert list(dense.shape[2:]) == out_shape
    by_tables = R.sparse_by_tables(feats, weight, nbr)
    assert torch.allclose(by_tables, R.read_rows(dense, outids), rtol=0, atol=1e-12)
    if not subm:
        # a regular conv's output rows are ALL reachable sites: the dense result is zero elsewhere
        assert R.off_support_max(dense, outids) == 0.0
        assert [tuple(r) for r in outids] == sorted(tuple(r) for r in outids)
    else:
        assert np.array_equal(outids, idx)
    # nbr_t is nbr transposed, pair_num its column counts
    o, k = np.nonzero(nbr >= 0)
    assert np.array_equal(nbr_t[nbr[o, k], k], o) and (nbr_t >= 0).sum() == len(o)
    assert np.array_equal(pair_num, (nbr_t >= 0).sum(0))
    # the swapped-table / transposed-weight form is autograd's input gradient
    g_out = torch.randn(by_tables.shape, generator=torch.Generator().manual_seed(5),
                        dtype=torch.float64)
    ref = R.Dense('subm' if subm else 'conv', feats, weight, None, idx, outids, BATCH, SHAPE,
                  stride, padding).backward(g_out)
    d_in = R.sparse_by_tables(g_out, weight.transpose(-1, -2), nbr_t)
    assert torch.allclose(d_in, ref.d_features, rtol=0, atol=1e-12)


@pytest.mark.parametrize('ksize,stride,padding', [((3, 3, 3), 2, 1), ((2, 2, 2), 2, 0),
                                                  ((3, 1, 1), (2, 1, 1), 0)])
def test_referee_inverse_is_conv_transpose_at_the_original_sites(ksize, stride, padding):
    idx, _, _ = _case(2, ksize=ksize)
    outids, nbr, nbr_t, _ = R.rulebook(idx, BATCH, SHAPE, ksize, stride, padding, False)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(len(outids), 4, generator=g, dtype=torch.float64)
    weight = torch.randn(*ksize, 4, 3, generator=g, dtype=torch.float64)
    dense = R.dense_inverse(feats, outids, BATCH, SHAPE, weight, stride, padding)
    assert list(dense.shape[2:]) == list(SHAPE)
    by_tables = R.sparse_by_tables(feats, weight, nbr_t)
    assert torch.allclose(by_tables, R.read_rows(dense, idx), rtol=0, atol=1e-12)


def _identical(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def test_vectorised_rulebook_equals_the_brute_force_exactly():
    """On the inputs of tests/test_spconv_gpu.py: every (grid, n) of TABLE_CASES under every
    geometry, and a small draw from the box of the carrying sizes; then this file's geometries,
    a stride-1 conv without padding and a 1 x 1 x 1 among them."""
    from tests import test_spconv_gpu as G
    cases = 0
    for grid, n in G.TABLE_CASES + [('box40', 4000), ('box64', 4000)]:
        batch, shape, _, _ = G.GRIDS[grid]
        rows = G.sites(11, grid, n)
        for ksize, stride, padding, subm in G.GEOMETRIES.values():
            want = R.rulebook(rows, batch, shape, ksize, stride, padding, subm)
            got = R.rulebook_fast(rows, batch, shape, ksize, stride, padding, subm)
            for g, w in zip(got, want):
                assert _identical(g, w), (grid, n, ksize, stride, padding, subm)
            cases += 1
    assert cases == 50
    idx, _, _ = _case(1)
    for ksize, stride, padding, subm in GEOMETRIES:
        want = R.rulebook(idx, BATCH, SHAPE, ksize, stride, padding, subm)
        got = R.rulebook_fast(idx, BATCH, SHAPE, ksize, stride, padding, subm)
        for g, w in zip(got, want):
            assert _identical(g, w), (ksize, stride, padding, subm)


def test_output_size_formulas_equal_torch():
    from nesie_amd.mmdet3d_ops.spconv import ops
    for ksize, stride, padding, subm in GEOMETRIES:
        if subm:
            continue
        k, s, p = R.triple(ksize), R.triple(stride), R.triple(padding)
        out = ops.get_conv_output_size(list(SHAPE), k, s, p, [1, 1, 1])
        want = nn.functional.conv3d(torch.zeros(1, 1, *SHAPE), torch.zeros(1, 1, *k), None, s, p)
        assert out == list(want.shape[2:])
        back = ops.get_deconv_output_size(out, k, s, p, [1, 1, 1], [0, 0, 0])
        want = nn.functional.conv_transpose3d(torch.zeros(1, 1, *out), torch.zeros(1, 1, *k), None,
                                              s, p)
        assert back == list(want.shape[2:])


def test_package_surface():
    from nesie_amd import mmdet3d_ops
    from nesie_amd.mmdet3d_ops import sparse_block
    want = ['SparseConv2d', 'SparseConv3d', 'SubMConv2d', 'SubMConv3d', 'SparseConvTranspose2d',
            'SparseConvTranspose3d', 'SparseInverseConv2d', 'SparseInverseConv3d', 'SparseModule',
            'SparseSequential', 'SparseMaxPool2d', 'SparseMaxPool3d', 'SparseConvTensor',
            'scatter_nd']
    assert spconv.__all__ == want
    for name in want:
        assert getattr(spconv, name) is not None
    for name in ('make_sparse_convmodule', 'SparseBasicBlock'):
        assert name in mmdet3d_ops._HOT and name not in mmdet3d_ops._OUT_OF_SCOPE
        assert name in mmdet3d_ops.__all__
        assert getattr(mmdet3d_ops, name) is getattr(sparse_block, name)
    for name in ('assign_score_withk', 'PAConv', 'SparseBottleneck'):
        assert name in mmdet3d_ops._OUT_OF_SCOPE
        with pytest.raises(NotImplementedError):
            getattr(mmdet3d_ops, name)()


def test_tensor_dense_scatter_nd_and_sequential_on_the_cpu():
    idx, feats, _ = _case(4, n=20)
    feats = feats.float()
    x = spconv.SparseConvTensor(feats, torch.from_numpy(idx), list(SHAPE), BATCH)
    assert x.grid is None and x.indice_dict == {} and x.find_indice_pair('a') is None
    assert x.find_indice_pair(None) is None and x.spatial_size == np.prod(SHAPE)
    assert x.sparity == 20 / np.prod(SHAPE) / BATCH
    dense = x.dense()
    assert tuple(dense.shape) == (BATCH, 3, *SHAPE)
    assert torch.equal(dense, R.densify(feats, idx, BATCH, SHAPE))
    assert torch.equal(x.dense(channels_first=False), dense.permute(0, 2, 3, 4, 1))
    assert dense.abs().sum() == feats.abs().sum()
    got = spconv.scatter_nd(torch.tensor([[0, 1], [2, 0]]), torch.tensor([[1., 2.], [3., 4.]]),
                            [3, 2, 2])
    assert got[0, 1].tolist() == [1, 2] and got[2, 0].tolist() == [3, 4] and got.sum() == 10
    # positional, OrderedDict and keyword construction; dense modules act on .features
    from nesie_amd.mmdet3d_ops.spconv.modules import RemoveGrid, ToDense
    lin = nn.Linear(3, 5)
    seq = spconv.SparseSequential(lin, nn.ReLU())
    assert len(seq) == 2 and seq[0] is lin and seq[-1] is seq[1]
    with pytest.raises(IndexError):
        seq[2]
    out = seq(x)
    assert out is x and torch.equal(x.features, torch.relu(lin(feats)))
    named = spconv.SparseSequential(OrderedDict([('a', nn.ReLU()), ('b', ToDense())]))
    assert list(named._modules) == ['a', 'b'] and tuple(named(x).shape) == (BATCH, 5, *SHAPE)
    assert named.sparity_dict == {'b': x.sparity}
    kw = spconv.SparseSequential(nn.ReLU(), tail=RemoveGrid())
    assert list(kw._modules) == ['0', 'tail']
    kw.add(nn.ReLU())
    kw.add(nn.ReLU(), 'last')
    assert list(kw._modules) == ['0', 'tail', '2', 'last']
    with pytest.raises(ValueError):
        spconv.SparseSequential(nn.ReLU(), **{'0': nn.ReLU()})
    x.grid = torch.zeros(1)
    assert kw(x).grid is None
    # no rows: a dense module is skipped
    empty = spconv.SparseConvTensor(torch.zeros(0, 3), torch.zeros(0, 4, dtype=torch.int32),
                                    list(SHAPE), BATCH)
    assert spconv.SparseSequential(nn.Linear(3, 5))(empty).features.shape == (0, 3)
    with pytest.raises(NotImplementedError):
        seq.fused()
    assert isinstance(seq, spconv.SparseModule)


def test_constructors_refuse_what_is_not_built():
    for name in ('SparseConv2d', 'SubMConv2d', 'SparseConvTranspose2d', 'SparseConvTranspose3d',
                 'SparseInverseConv2d', 'SparseMaxPool2d', 'SparseMaxPool3d'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(spconv, name)(4, 4, 3)
    from nesie_amd.mmdet3d_ops.spconv.conv import SparseConvolution
    for kw in (dict(dilation=2), dict(groups=2), dict(dilation=(1, 2, 1))):
        for cls in (spconv.SubMConv3d, spconv.SparseConv3d):
            with pytest.raises(NotImplementedError):
                cls(4, 4, 3, **kw)
    for kw in (dict(fused_bn=True), dict(transposed=True), dict(ndim=2)):
        args = dict(ndim=3, in_channels=4, out_channels=4)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            SparseConvolution(**args)
    with pytest.raises(ValueError, match='indice_key'):
        spconv.SparseInverseConv3d(4, 4, 3, None)
    with pytest.raises(TypeError):
        spconv.SparseInverseConv3d(4, 4, 3)
    # an inverse conv whose partner never ran, or ran with another kernel
    idx, feats, _ = _case(6, n=10)
    x = spconv.SparseConvTensor(feats.float(), torch.from_numpy(idx), list(SHAPE), BATCH)
    with pytest.raises(ValueError, match='ran before'):
        spconv.SparseInverseConv3d(3, 4, 3, 'd')(x)
    from nesie_amd.mmdet3d_ops.spconv.ops import Rules
    table = torch.zeros(10, 8, dtype=torch.int32)
    x.indice_dict['d'] = (x.indices, x.indices, Rules(table, table), None, list(SHAPE))
    with pytest.raises(ValueError, match='kernel size'):
        spconv.SparseInverseConv3d(3, 4, 3, 'd')(x)
    from nesie_amd.mmdet3d_ops import make_sparse_convmodule
    with pytest.raises(NotImplementedError):
        make_sparse_convmodule(4, 4, 3, 'k', conv_type='SparseConv2d')
    with pytest.raises(NotImplementedError):
        make_sparse_convmodule(4, 4, 3, 'k', norm_cfg=dict(type='GN', num_groups=2))


def test_layer_attributes_and_initialisation():
    torch.manual_seed(0)
    conv = spconv.SparseConv3d(5, 16, (3, 1, 1), stride=(2, 1, 1), padding=0, indice_key='k')
    assert tuple(conv.weight.shape) == (3, 1, 1, 5, 16) and tuple(conv.bias.shape) == (16,)
    assert (conv.ndim, conv.in_channels, conv.out_channels) == (3, 5, 16)
    assert conv.kernel_size == [3, 1, 1] and conv.stride == [2, 1, 1] and conv.padding == [0, 0, 0]
    assert conv.dilation == [1, 1, 1] and conv.output_padding == [0, 0, 0] and conv.groups == 1
    assert not (conv.subm or conv.inverse or conv.transposed or conv.fused_bn or conv.conv1x1)
    assert conv.indice_key == 'k'
    # as the reference: kaiming_uniform_(a = sqrt(5)) sees the (kz, ky, kx, Cin, Cout) tensor with
    # torch's own fan rule (size(1) x the rest = 1 * 1 * 5 * 16), the bias the HWIO fan-in Cin * taps
    w, b = conv.weight.detach().abs(), conv.bias.detach().abs()
    assert 0.8 / np.sqrt(80) < float(w.max()) <= 1 / np.sqrt(80) + 1e-7
    assert float(b.max()) <= 1 / np.sqrt(5 * 3) + 1e-7
    sub = spconv.SubMConv3d(4, 8, 3, bias=False)
    assert sub.subm and sub.bias is None and list(sub.state_dict()) == ['weight']
    inv = spconv.SparseInverseConv3d(8, 4, 3, 'k', bias=False)
    assert inv.inverse and not inv.subm and inv.indice_key == 'k'
    assert spconv.SubMConv3d(4, 8, 1).conv1x1
    from nesie_amd.mmdet3d_ops import SparseBasicBlock, make_sparse_convmodule
    m = make_sparse_convmodule(4, 16, 3, 'subm1', stride=2, padding=1, conv_type='SparseConv3d',
                               norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01))
    assert isinstance(m, spconv.SparseSequential) and len(m) == 3
    assert isinstance(m[0], spconv.SparseConv3d) and m[0].bias is None and m[0].stride == [2, 2, 2]
    assert m[0].indice_key == 'subm1' and m[0].padding == [1, 1, 1]
    assert isinstance(m[1], nn.BatchNorm1d) and m[1].eps == 1e-3 and m[1].momentum == 0.01
    assert isinstance(m[2], nn.ReLU)
    m = make_sparse_convmodule(4, 4, 3, 'k', order=('act', 'conv'))
    assert isinstance(m[0], nn.ReLU) and isinstance(m[1], spconv.SubMConv3d) and len(m) == 2
    block = SparseBasicBlock(16, 16, conv_cfg=dict(type='SubMConv3d', indice_key='b'),
                             norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01))
    keys = set(block.state_dict())
    assert {'conv1.weight', 'conv2.weight', 'bn1.weight', 'bn1.bias', 'bn1.running_mean',
            'bn1.running_var', 'bn2.weight', 'bn2.bias'} <= keys
    assert not any(k.startswith('downsample') or k.endswith('conv1.bias') for k in keys)
    assert block.norm1 is block.bn1 and block.norm2 is block.bn2 and block.conv1.subm
    assert block.conv1.indice_key == 'b' and isinstance(block, spconv.SparseModule)


def test_layers_refuse_cpu_tensors():
    idx, feats, _ = _case(7, n=12)
    feats = feats.float()

    def x():
        return spconv.SparseConvTensor(feats, torch.from_numpy(idx), list(SHAPE), BATCH)

    from nesie_amd.mmdet3d_ops import SparseBasicBlock, make_sparse_convmodule
    from nesie_amd.mmdet3d_ops.spconv import functional as Fsp
    from nesie_amd.mmdet3d_ops.spconv import ops
    table = torch.zeros(12, 27, dtype=torch.int32)
    calls = (lambda: spconv.SubMConv3d(3, 4, 3)(x()),
             lambda: spconv.SparseConv3d(3, 4, 3, 2, 1)(x()),
             lambda: spconv.SubMConv3d(3, 4, 1)(x()),
             lambda: make_sparse_convmodule(3, 4, 3, 'k')(x()),
             lambda: SparseBasicBlock(3, 3)(x()),
             lambda: ops.get_indice_pairs(torch.from_numpy(idx), BATCH, SHAPE, 3, 1, 1),
             lambda: Fsp.indice_conv(feats, torch.zeros(3, 3, 3, 3, 4), ops.Rules(table, table),
                                     None, 12))
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_entries_are_declared():
    c = ctypes
    sig = _lib.SIGNATURES
    ll, i, p = c.c_longlong, c.c_int, c.c_void_p
    assert sig['nesie_spconv_rules_workspace_bytes'] == (i, [ll, i, i, p])
    assert sig['nesie_spconv_out_shape'] == (i, [p] * 4 + [i, i, p, p])
    assert sig['nesie_spconv_out_sites'] == (i, [ll, p, i] + [p] * 4 + [i] + [p] * 7)
    assert sig['nesie_spconv_gather_table'] == (i, [ll, p, ll, p, p, i] + [p] * 4 + [i] + [p] * 3)
    assert sig['nesie_spconv_gather_gemm'] == (i, [ll, ll, i, i, i, p, p, i, p, p, p])
    assert sig['nesie_spconv_wgrad_workspace_bytes'] == (i, [ll, i, i, i, p])
    assert sig['nesie_spconv_wgrad'] == (i, [ll, ll, i, i, i] + [p] * 6)
    lib = _lib.load()
    for name in sig:
        if name.startswith('nesie_spconv'):
            assert hasattr(lib, name)


def test_argument_checks_come_before_any_device_call():
    lib = _lib.load()
    n = None
    INVALID, UNSUPPORTED = 1, 2
    out = ctypes.c_longlong()
    tri = lambda a, b, c: (ctypes.c_int * 3)(a, b, c)                      # noqa: E731
    shape, k3, one, zero = tri(41, 1600, 1408), tri(3, 3, 3), tri(1, 1, 1), tri(0, 0, 0)

    # workspace queries: monotone in n, refusals
    sizes = []
    for nn_ in (0, 1, 1023, 1024, 1025, 5000, 60000):
        assert lib.nesie_spconv_rules_workspace_bytes(nn_, 27, 0, ctypes.byref(out)) == 0
        sizes.append(out.value)
    assert sizes == sorted(sizes) and sizes[0] >= 0 and sizes[-1] > sizes[1]
    assert lib.nesie_spconv_rules_workspace_bytes(5000, 27, 1, ctypes.byref(out)) == 0
    assert 0 < out.value < sizes[5]                                        # subm sorts n, not n * K
    assert lib.nesie_spconv_rules_workspace_bytes(-1, 27, 0, ctypes.byref(out)) == INVALID
    assert b'spconv_rules_workspace_bytes' in lib.nesie_last_error()
    assert lib.nesie_spconv_rules_workspace_bytes(10, 0, 0, ctypes.byref(out)) == INVALID
    assert lib.nesie_spconv_rules_workspace_bytes(10, 27, 0, n) == INVALID
    assert lib.nesie_spconv_rules_workspace_bytes(2 ** 31 // 27 + 1, 27, 0,
                                                  ctypes.byref(out)) == UNSUPPORTED
    sizes = []
    for rows in (0, 1, 512, 513, 5000, 10 ** 6):
        assert lib.nesie_spconv_wgrad_workspace_bytes(rows, 27, 16, 32, ctypes.byref(out)) == 0
        sizes.append(out.value)
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[3] == 2 * sizes[2]
    assert lib.nesie_spconv_wgrad_workspace_bytes(-1, 27, 16, 32, ctypes.byref(out)) == INVALID
    assert lib.nesie_spconv_wgrad_workspace_bytes(10, 27, 0, 32, ctypes.byref(out)) == INVALID
    assert b'spconv_wgrad_workspace_bytes' in lib.nesie_last_error()

    # the output grid
    oshape = (ctypes.c_int * 3)()
    assert lib.nesie_spconv_out_shape(shape, k3, tri(2, 2, 2), one, 0, 23, oshape,
                                      ctypes.byref(out)) == 0
    assert list(oshape) == [21, 800, 704] and out.value == 23 * 21 * 800 * 704
    assert lib.nesie_spconv_out_shape(shape, k3, tri(2, 2, 2), zero, 1, 2, oshape,
                                      ctypes.byref(out)) == 0
    assert list(oshape) == [41, 1600, 1408]                                # subm: the input grid
    # 41 x 1600 x 1408 fits up to batch 23; 2^31 cells exactly is refused
    assert lib.nesie_spconv_out_shape(shape, k3, one, one, 1, 24, oshape,
                                      ctypes.byref(out)) == UNSUPPORTED
    exact = tri(2048, 2048, 512)
    assert lib.nesie_spconv_out_shape(exact, k3, one, one, 1, 1, oshape,
                                      ctypes.byref(out)) == UNSUPPORTED
    assert lib.nesie_spconv_out_shape(tri(2, 2, 2), k3, one, zero, 0, 1, oshape,
                                      ctypes.byref(out)) == UNSUPPORTED     # no output site
    assert lib.nesie_spconv_out_shape(shape, tri(9, 9, 9), one, one, 0, 1, oshape,
                                      ctypes.byref(out)) == UNSUPPORTED     # 729 taps
    assert lib.nesie_spconv_out_shape(shape, k3, zero, one, 0, 1, oshape,
                                      ctypes.byref(out)) == INVALID
    assert lib.nesie_spconv_out_shape(shape, k3, one, tri(0, -1, 0), 0, 1, oshape,
                                      ctypes.byref(out)) == INVALID
    assert lib.nesie_spconv_out_shape(shape, k3, one, one, 0, 0, oshape,
                                      ctypes.byref(out)) == INVALID
    assert lib.nesie_spconv_out_shape(n, k3, one, one, 0, 1, oshape, ctypes.byref(out)) == INVALID

    # phase 1
    def sites(nn_, sh=shape, batch=2, subm=0):
        return lib.nesie_spconv_out_sites(nn_, n, batch, sh, k3, one, one, subm, n, n, n, n, n, n, n)

    assert sites(-1) == INVALID
    assert b'spconv_out_sites' in lib.nesie_last_error()
    assert sites(0) == 0 and sites(0, subm=1) == 0
    assert sites(10) == INVALID                                            # null tensors
    assert sites(0, exact, 1) == UNSUPPORTED and sites(10, shape, 24, 1) == UNSUPPORTED
    assert sites(2 ** 31 // 27 + 1) == UNSUPPORTED

    # phase 2
    def table(m, nn_, sh=shape):
        return lib.nesie_spconv_gather_table(m, n, nn_, n, n, 2, sh, k3, one, one, 0, n, n, n)

    assert table(-1, 10) == INVALID and table(10, -1) == INVALID
    assert b'spconv_gather_table' in lib.nesie_last_error()
    assert table(0, 10) == 0 and table(0, 0) == 0
    assert table(10, 10) == INVALID and table(10, 10, exact) == UNSUPPORTED

    # the feature products
    def gemm(rows, src_rows, kvol=27, cs=4, cd=16):
        return lib.nesie_spconv_gather_gemm(rows, src_rows, kvol, cs, cd, n, n, 0, n, n, n)

    assert gemm(-1, 10) == INVALID and gemm(10, -1) == INVALID and gemm(10, 10, 0) == INVALID
    assert gemm(10, 10, 27, 0) == INVALID and gemm(10, 10, 27, 4, 0) == INVALID
    assert b'spconv_gather_gemm' in lib.nesie_last_error()
    assert gemm(0, 10) == 0 and gemm(0, 0) == 0
    assert gemm(10, 10) == INVALID                                         # null tensors

    def wgrad(rows, src_rows, kvol=27, ci=4, co=16):
        return lib.nesie_spconv_wgrad(rows, src_rows, kvol, ci, co, n, n, n, n, n, n)

    assert wgrad(-1, 10) == INVALID and wgrad(10, -1) == INVALID and wgrad(10, 10, 0) == INVALID
    assert b'spconv_wgrad' in lib.nesie_last_error()
    assert wgrad(0, 10) == 0 and wgrad(10, 0) == 0
    assert wgrad(10, 10) == INVALID                                        # null tensors
    assert lib.nesie_abi_version() == 2
