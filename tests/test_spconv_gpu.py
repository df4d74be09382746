"""Sparse convolution on the device: the rulebook equals the brute-force referee exactly, the three
layers' outputs and gradients sit inside the a-priori fp32 bound of their float64 dense form, runs
are bit-identical, the rulebook is cached, forward + backward replay from a graph, and the voxel
ops feed it end to end (tests/_spconv_ref.py is the referee).

Constants the sizes are chosen around: the sort works on tiles of 1024 keys and the scan on tiles
of 1024 ints (N one below, at and one above 1024; N * K = 5000 * 27 crosses 132 scan tiles; the
scan's second level takes the tile totals 256 at a time with a carry, which 9710 * 27 candidates
reach for the flag scan and 38 837 * 27 for the digit counters of the candidate sort); the
gather-GEMM owns 128 output rows per workgroup (SG_TM) and stages 32 source channels a step
(SG_KC), with 32 / 64 / 128 destination channels per workgroup; the weight gradient cuts the rows
into ceil(rows / 512) chunks (SW_CHUNK_ROWS, at most 16) and walks them 32 at a time.

The value bound, no element excused: |dev - f64| <= gamma_n * S with S the sum of |a| * |b| over
the element's products (the dense form on absolute operands, float64) and
gamma_n = (n + 1) u / (1 - (n + 1) u), u = 2^-24, n the element's number of products: the
standard a-priori bound of an fp32 sum of products in any order.  The observed dev_err / ref_err
(ref_err = the float32 dense form's own error) is printed before each assertion."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import _spconv_ref as R
from tests._launch_recorder import LaunchRecorder

pytestmark = pytest.mark.gpu

GARBAGE = -77
# (kernel, stride, padding, subm)
GEOMETRIES = {
    'subm333': ((3, 3, 3), 1, 1, True),
    'conv333s2p1': ((3, 3, 3), 2, 1, False),
    'conv311s211': ((3, 1, 1), (2, 1, 1), 0, False),
    'conv222s2': ((2, 2, 2), 2, 0, False),
    'subm133': ((1, 3, 3), 1, 0, True),
}
# name: (batch, grid, box the sites are drawn from, empty sample)      cells          passes
GRIDS = {
    'p1': (1, (3, 4, 5), (3, 4, 5), None),                           # 60              1
    'p2': (2, (9, 10, 11), (9, 10, 11), None),                       # 1980            2
    'p3': (3, (16, 64, 64), (16, 20, 20), 1),                        # 196608          3
    'lidar': (2, (41, 1600, 1408), (12, 14, 16), None),              # 184729600       4
    'box40': (2, (41, 1600, 1408), (40, 40, 40), None),              # 184729600       4
    'box64': (2, (41, 1600, 1408), (40, 64, 64), None),              # 184729600       4
}
TABLE_CASES = [('p1', 0), ('p1', 1), ('p1', 37), ('p2', 1023), ('p2', 1024), ('p2', 1025),
               ('p3', 5000), ('lidar', 3000)]


def sites(seed, grid, n):
    """n distinct shuffled rows: drawn from a box (so that neighbours exist in a sparse grid), the
    last sample's box pushed into the far corner; both extreme corners of the grid are sites."""
    batch, shape, box, empty = GRIDS[grid]
    rng = np.random.default_rng(seed)
    rows = R.random_sites(rng, n, batch, box, faces=True, empty_batch=empty)
    if len(rows):
        last = max(b for b in range(batch) if b != empty)
        shift = np.int32([0] + [shape[a] - box[a] for a in range(3)])
        if batch > 1:
            rows[rows[:, 0] == last] += shift
    return rows


def dev(a, device):
    return torch.from_numpy(np.array(a, order='C')).to(device)     # a copy: `a` may be read-only


def same(got, want):
    got = got.detach().cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def build_rules(device, rows, batch, shape, geometry, workspace=None):
    """Both phases through HipKernels with every output pre-filled with garbage."""
    from nesie_amd.kernels import HipKernels
    k = HipKernels()
    ksize, stride, padding, subm = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    ksize, stride, padding = R.triple(ksize), R.triple(stride), R.triple(padding)
    kvol, n = int(np.prod(ksize)), len(rows)
    idx = dev(rows, device)
    full = lambda *s: torch.full(s, GARBAGE, dtype=torch.int32, device=device)   # noqa: E731
    _, cells = k.spconv_out_shape(shape, ksize, stride, padding, subm, batch)
    sk, sr, nbr_t, counts = full(n), full(n), full(n, kvol), full(2)
    worst = None if subm else full(min(n * kvol, cells), 4)
    k.spconv_out_sites(idx, batch, shape, ksize, stride, padding, subm, sk, sr, nbr_t, worst, counts,
                       workspace)
    m, bad = counts.tolist()
    outids = idx if subm else worst[:m].clone()
    if not subm:
        assert bool((worst[m:] == GARBAGE).all())                    # rows at and above M untouched
    nbr, pair_num = full(m, kvol), full(kvol)
    k.spconv_gather_table(outids, sk, sr, batch, shape, ksize, stride, padding, subm, nbr, pair_num)
    return dict(m=m, bad=bad, outids=outids, nbr=nbr, nbr_t=nbr_t, pair_num=pair_num, sk=sk, sr=sr)


# ---- tables ------------------------------------------------------------------------------------

def check_tables(hip_device, geometry, grid, n, rulebook):
    """Both phases against ``rulebook`` (the brute-force referee or its vectorised form): every
    table, the sorted keys and rows, the counts; built twice, the same bits."""
    batch, shape, _, _ = GRIDS[grid]
    rows = sites(11, grid, n)
    ksize, stride, padding, subm = GEOMETRIES[geometry]
    if n == 0:
        from nesie_amd.mmdet3d_ops.spconv import ops
        outids, rules, pair_num = ops.get_indice_pairs(dev(rows, hip_device), batch, shape, ksize,
                                                       stride, padding, subm=subm)
        kvol = int(np.prod(ksize))
        assert tuple(outids.shape) == (0, 4) and tuple(rules.nbr.shape) == (0, kvol)
        assert tuple(rules.nbr_t.shape) == (0, kvol) and pair_num.tolist() == [0] * kvol
        return
    w_out, w_nbr, w_nbr_t, w_pairs = rulebook(rows, batch, shape, ksize, stride, padding, subm)
    got = build_rules(hip_device, rows, batch, shape, geometry)
    assert got['bad'] == 0 and got['m'] == len(w_out)
    assert same(got['outids'], w_out)
    assert same(got['nbr'], w_nbr) and same(got['nbr_t'], w_nbr_t)
    assert same(got['pair_num'], w_pairs)
    if n > 100:
        assert int(w_pairs.sum()) >= n // 2                         # the case has pairs
    # the sorted keys and their rows
    d, h, w = shape
    keys = ((rows[:, 0].astype(np.int64) * d + rows[:, 1]) * h + rows[:, 2]) * w + rows[:, 3]
    order = np.argsort(keys, kind='stable')
    assert same(got['sk'], keys[order].astype(np.int32)) and same(got['sr'], order.astype(np.int32))
    # built twice: the same bits
    again = build_rules(hip_device, rows, batch, shape, geometry)
    for name in ('outids', 'nbr', 'nbr_t', 'pair_num'):
        assert torch.equal(got[name], again[name])
    return got


@pytest.mark.parametrize('grid,n', TABLE_CASES)
@pytest.mark.parametrize('geometry', list(GEOMETRIES))
def test_tables_equal_the_brute_force_referee(hip_device, geometry, grid, n):
    check_tables(hip_device, geometry, grid, n, R.rulebook)


@pytest.mark.parametrize('n', [9710, 38837])
def test_tables_where_the_scan_carries(hip_device, n):
    """conv333s2p1 on the (41, 1600, 1408) grid: 9710 sites are 262 170 candidates, 257 tile totals
    of the candidate flag scan; 38 837 sites are 1 048 599 candidates, 1025 sort tiles, whose
    262 400 digit counters carry inside each of the second sort's four passes too.  The referee is
    the vectorised rulebook, which tests/test_spconv_cpu.py proves equal to the brute force."""
    threshold = {9710: 262144, 38837: 1048576}[n]
    assert (n - 1) * 27 <= threshold < n * 27                       # the smallest n past it
    got = check_tables(hip_device, 'conv333s2p1', 'box40', n, R.rulebook_fast)
    assert got['m'] > 8000


def test_tables_where_the_carry_reaches_valid_candidates(hip_device):
    """With stride 2 about one candidate in eight is an output site, and the others sort last: at
    the two sizes above every position behind the scan's carry holds an out-of-range key, whose
    scan value nothing reads, so there the carry shows in the output count alone.  84 000 sites
    give more than 262 144 valid candidates: output rows and nbr_t entries come from behind it."""
    got = check_tables(hip_device, 'conv333s2p1', 'box64', 84000, R.rulebook_fast)
    assert int(got['pair_num'].sum()) > 262144 + 10000


@pytest.mark.parametrize('n', [1, 1025, 5000, 9710])
@pytest.mark.parametrize('geometry', ['subm333', 'conv333s2p1'])
def test_out_sites_stays_inside_the_workspace_it_asks_for(hip_device, geometry, n):
    """Exactly the bytes the query returns, between two bands of 4096 bytes of 0xA5 that must stay
    as they are; the regular conv carves that scratch twice, for n and then for n * K (9710 sites:
    the candidate scan carries).  Every output equals the run that allocated its own workspace."""
    from nesie_amd.kernels import HipKernels
    guard = 4096
    batch, shape, _, _ = GRIDS['box40']
    rows = sites(14, 'box40', n)
    subm = GEOMETRIES[geometry][3]
    need = HipKernels.spconv_rules_workspace_bytes(n, 27, subm)
    assert need > 0
    whole = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=hip_device)
    own = build_rules(hip_device, rows, batch, shape, geometry)
    got = build_rules(hip_device, rows, batch, shape, geometry, whole[guard:guard + need])
    assert bool((whole[:guard] == 0xA5).all()) and bool((whole[guard + need:] == 0xA5).all())
    assert (got['m'], got['bad']) == (own['m'], own['bad']) and got['bad'] == 0
    for name in ('outids', 'nbr', 'nbr_t', 'pair_num', 'sk', 'sr'):
        assert torch.equal(got[name], own[name])


@pytest.mark.parametrize('geometry', ['subm333', 'conv333s2p1'])
def test_output_order_and_input_order(hip_device, geometry):
    batch, shape, _, _ = GRIDS['p2']
    rows = sites(12, 'p2', 700)
    perm = np.random.default_rng(3).permutation(len(rows))
    a = build_rules(hip_device, rows, batch, shape, geometry)
    b = build_rules(hip_device, rows[perm], batch, shape, geometry)
    subm = GEOMETRIES[geometry][3]
    inv = np.argsort(perm)
    if subm:      # the output rows ARE the input rows, in their order
        assert same(a['outids'], rows) and same(b['outids'], rows[perm])
        nbr_a = a['nbr'].cpu().numpy()
        want = np.where(nbr_a[perm] >= 0, inv[np.maximum(nbr_a[perm], 0)], -1).astype(np.int32)
        assert same(b['nbr'], want)
    else:         # ascending key order whatever the input order
        assert torch.equal(a['outids'], b['outids'])
        out = a['outids'].cpu().numpy()
        assert [tuple(r) for r in out] == sorted(tuple(r) for r in out)
        nbr_a = a['nbr'].cpu().numpy()
        want = np.where(nbr_a >= 0, inv[np.maximum(nbr_a, 0)], -1).astype(np.int32)
        assert same(b['nbr'], want)
        assert torch.equal(a['nbr_t'][dev(perm, hip_device)], b['nbr_t'])


class Recording(LaunchRecorder):
    """Logs a call as LaunchRecorder does, then makes it on the device."""

    def __init__(self):
        super().__init__()
        from nesie_amd.kernels import HipKernels
        self._real = HipKernels()

    def __getattr__(self, method):
        if method.startswith('_'):
            raise AttributeError(method)
        log = LaunchRecorder.__getattr__(self, method)
        real = getattr(self._real, method)

        def call(*args, **kwargs):
            log(*args, **kwargs)
            return real(*args, **kwargs)
        return call

    def names(self):
        return [entry[0] for entry in self.log]


@pytest.mark.parametrize('what', ['outside', 'negative', 'batch', 'duplicate'])
@pytest.mark.parametrize('subm', [True, False])
def test_offending_rows_raise_before_any_feature_kernel(hip_device, what, subm):
    from nesie_amd import kernels
    from nesie_amd.mmdet3d_ops import spconv
    batch, shape, _, _ = GRIDS['p2']
    rows = sites(13, 'p2', 300)
    if what == 'outside':
        rows[250] = [1, 3, shape[1], 2]
    elif what == 'negative':
        rows[250] = [0, 3, 4, -1]
    elif what == 'batch':
        rows[250] = [batch, 3, 4, 2]
    else:
        rows[250] = rows[17]             # of equal rows the one of lowest index stays
    x = spconv.SparseConvTensor(torch.randn(300, 4, device=hip_device), dev(rows, hip_device),
                                list(shape), batch)
    layer = (spconv.SubMConv3d(4, 8, 3) if subm else spconv.SparseConv3d(4, 8, 3, 2, 1))
    layer = layer.to(hip_device)
    rec = Recording()
    with kernels.use_backend(rec):
        with pytest.raises(ValueError, match='1 of 300 rows'):
            layer(x)
    assert 'spconv_out_sites' in rec.names()
    assert not any(n in ('spconv_gather_gemm', 'spconv_wgrad', 'spconv_gather_table')
                   for n in rec.names())
    # an offending row takes part in no pair; the others keep theirs
    got = build_rules(hip_device, rows, batch, shape, ((3, 3, 3), 2, 1, subm))
    assert got['bad'] == 1
    assert bool((got['nbr_t'][250] == -1).all()) and not bool((got['nbr'] == 250).any())
    keep = np.ones(300, bool)
    keep[250] = False
    _, w_nbr, w_nbr_t, _ = R.rulebook(rows[keep], batch, shape, 3, 2, 1, subm)
    renum = np.flatnonzero(keep).astype(np.int32)
    if subm:
        want_t = np.where(w_nbr_t >= 0, renum[np.maximum(w_nbr_t, 0)], -1).astype(np.int32)
    else:
        want_t = w_nbr_t
    assert same(got['nbr_t'][dev(renum.astype(np.int64), hip_device)], want_t)


# ---- values ------------------------------------------------------------------------------------

VAL_BATCH, VAL_SHAPE = 2, (8, 9, 10)
LAYERS = {   # kind: (kernel, stride, padding)
    'subm': ((3, 3, 3), 1, 1),
    'conv': ((3, 3, 3), 2, 1),
    'inverse': ((3, 3, 3), 2, 1),
}
_sites_cache = {}


def value_sites(n, kind):
    """rows, the referee's rulebook for them: computed once per (n, geometry), never changed."""
    key = (n, kind == 'subm')
    if key not in _sites_cache:
        rows = R.random_sites(np.random.default_rng(100 + n), n, VAL_BATCH, VAL_SHAPE)
        ksize, stride, padding = LAYERS[kind]
        book = R.rulebook(rows, VAL_BATCH, VAL_SHAPE, ksize, stride, padding, kind == 'subm')
        for a in (rows,) + book:
            a.setflags(write=False)
        _sites_cache[key] = (rows, book)
    return _sites_cache[key]


def check(name, got, f64, f32, s_abs, n_products):
    """|got - f64| <= gamma_n * S for every element; prints dev_err / ref_err first."""
    got = got.detach().double().cpu()
    err = (got - f64).abs()
    ref = (f32.double() - f64).abs()
    bound = torch.as_tensor(R.gamma(n_products)) * s_abs
    ratio = float(err.max() / ref.max()) if float(ref.max()) > 0 else float('nan')
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{name}: dev_err {float(err.max()):.3e} ref_err {float(ref.max()):.3e} '
          f'dev_err/ref_err {ratio:.3f} max err/bound {worst:.3f}')
    assert got.shape == f64.shape
    assert bool((err <= bound).all()), f'{name}: {int((err > bound).sum())} elements past the bound'


def run_layer(device, kind, cin, cout, n, seed=0, bias=True):
    """-> the device layer's (out, d_features, d_weight, d_bias, out_indices) and the inputs."""
    from nesie_amd.mmdet3d_ops import spconv
    rows, (w_out, w_nbr, w_nbr_t, w_pairs) = value_sites(n, kind)
    ksize, stride, padding = LAYERS[kind]
    g = torch.Generator().manual_seed(seed + 7 * cin + cout)
    torch.manual_seed(seed)
    if kind == 'subm':
        layer = spconv.SubMConv3d(cin, cout, ksize, bias=bias, indice_key='k')
    elif kind == 'conv':
        layer = spconv.SparseConv3d(cin, cout, ksize, stride, padding, bias=bias, indice_key='k')
    else:
        layer = spconv.SparseInverseConv3d(cin, cout, ksize, 'k', bias=bias)
    layer = layer.to(device)
    src_rows = len(w_out) if kind == 'inverse' else n
    feats = torch.randn(src_rows, cin, generator=g)
    d_feats = feats.to(device).requires_grad_(True)
    if kind == 'inverse':
        # the partner conv builds the rulebook; the inverse layer then reads it from the cache
        partner = spconv.SparseConv3d(3, 2, ksize, stride, padding, indice_key='k').to(device)
        x0 = spconv.SparseConvTensor(torch.zeros(n, 3, device=device), dev(rows, device),
                                     list(VAL_SHAPE), VAL_BATCH)
        mid = partner(x0)
        assert same(mid.indices, w_out)
        x = spconv.SparseConvTensor(d_feats, mid.indices, mid.spatial_shape, VAL_BATCH)
        x.indice_dict = mid.indice_dict
    else:
        x = spconv.SparseConvTensor(d_feats, dev(rows, device), list(VAL_SHAPE), VAL_BATCH)
    y = layer(x)
    g_out = torch.randn(y.features.shape, generator=g)
    wrt = [d_feats, layer.weight] + ([layer.bias] if bias else [])
    grads = torch.autograd.grad(y.features, wrt, g_out.to(device))
    return dict(layer=layer, y=y, grads=grads, feats=feats, g_out=g_out, rows=rows, w_out=w_out,
                w_nbr=w_nbr, w_nbr_t=w_nbr_t, w_pairs=w_pairs, x=x)


def check_layer(tag, r, kind, cin, cout):
    layer, y = r['layer'], r['y']
    ksize, stride, padding = LAYERS[kind]
    weight = layer.weight.detach().cpu()
    bias = None if layer.bias is None else layer.bias.detach().cpu()
    args = (kind, r['feats'], weight, bias, r['rows'], r['w_out'], VAL_BATCH, list(VAL_SHAPE),
            stride, padding)
    f64 = R.Dense(*args).backward(r['g_out'])
    f32 = R.Dense(*args, dtype=torch.float32).backward(r['g_out'])
    mag = R.Dense(*args, absolute=True).backward(r['g_out'])
    # which table gathers for the output, which for the input gradient
    fwd, bwd = (r['w_nbr_t'], r['w_nbr']) if kind == 'inverse' else (r['w_nbr'], r['w_nbr_t'])
    want_ids = r['rows'] if kind == 'inverse' else r['w_out']
    assert same(y.indices, want_ids)
    assert list(y.spatial_shape) == (list(VAL_SHAPE) if kind != 'conv' else
                                     R.geometry(VAL_SHAPE, ksize, stride, padding, False)[3])
    n_out = (fwd >= 0).sum(1, keepdims=True) * cin + (bias is not None)
    check(f'{tag} out', y.features, f64.out.detach(), f32.out.detach(), mag.out.detach(), n_out)
    n_in = (bwd >= 0).sum(1, keepdims=True) * cout
    check(f'{tag} d_features', r['grads'][0], f64.d_features, f32.d_features, mag.d_features, n_in)
    n_w = (fwd >= 0).sum(0).reshape(*weight.shape[:3], 1, 1)
    check(f'{tag} d_weight', r['grads'][1], f64.d_weight, f32.d_weight, mag.d_weight, n_w)
    if bias is not None:
        check(f'{tag} d_bias', r['grads'][2], f64.d_bias, f32.d_bias, mag.d_bias, fwd.shape[0])


@pytest.mark.parametrize('cin,cout', [(1, 1), (4, 16), (5, 16), (16, 16), (33, 7), (64, 64)])
@pytest.mark.parametrize('kind', list(LAYERS))
def test_values_against_float64(hip_device, kind, cin, cout):
    check_layer(f'{kind} {cin}->{cout} n=129', run_layer(hip_device, kind, cin, cout, 129), kind,
                cin, cout)


def test_values_against_float64_128_channels(hip_device):
    check_layer('subm 128->128 n=129', run_layer(hip_device, 'subm', 128, 128, 129), 'subm', 128,
                128)


@pytest.mark.parametrize('kind,cin,cout,n', [
    ('subm', 4, 16, 127), ('subm', 4, 16, 128), ('subm', 4, 16, 512), ('subm', 4, 16, 513),
    ('subm', 5, 16, 513), ('conv', 16, 16, 600), ('inverse', 16, 5, 600), ('subm', 16, 33, 1100),
    ('conv', 4, 16, 1), ('subm', 4, 16, 1)])
def test_values_across_row_tiles_and_chunks(hip_device, kind, cin, cout, n):
    """Rows one below, at and one above the 128-row tile; 512 / 513 and 1100 rows put the weight
    gradient in 1, 2 and 3 chunks (a regular conv of 600 sites has its own M: whatever it is, the
    bound holds); a single site."""
    check_layer(f'{kind} {cin}->{cout} n={n}', run_layer(hip_device, kind, cin, cout, n, bias=False),
                kind, cin, cout)


def test_conv1x1_is_a_matmul_and_empty_tensors_give_zeros(hip_device):
    from nesie_amd.mmdet3d_ops import spconv
    rows, _ = value_sites(129, 'subm')
    feats = torch.randn(129, 8, device=hip_device)
    x = spconv.SparseConvTensor(feats, dev(rows, hip_device), list(VAL_SHAPE), VAL_BATCH)
    layer = spconv.SubMConv3d(8, 4, 1).to(hip_device)
    y = layer(x)
    assert torch.equal(y.features, feats @ layer.weight.view(8, 4) + layer.bias)
    assert y.indices is x.indices and x.indice_dict == {}
    empty = spconv.SparseConvTensor(torch.zeros(0, 8, device=hip_device, requires_grad=True),
                                    torch.zeros(0, 4, dtype=torch.int32, device=hip_device),
                                    list(VAL_SHAPE), VAL_BATCH)
    for layer in (spconv.SubMConv3d(8, 4, 3, bias=False), spconv.SparseConv3d(8, 4, 3, 2, 1, bias=False)):
        layer = layer.to(hip_device)
        y = layer(empty)
        assert tuple(y.features.shape) == (0, 4) and tuple(y.indices.shape) == (0, 4)
        gi, gw = torch.autograd.grad(y.features.sum(), (empty.features, layer.weight))
        assert tuple(gi.shape) == (0, 8) and gw.shape == layer.weight.shape
        assert float(gw.abs().max()) == 0.0


# ---- determinism, cache, capture ---------------------------------------------------------------

@pytest.mark.parametrize('kind,cin,cout', [('subm', 16, 16), ('conv', 5, 16), ('inverse', 64, 64)])
def test_runs_are_bit_identical(hip_device, kind, cin, cout):
    from nesie_amd.kernels import HipKernels
    a = run_layer(hip_device, kind, cin, cout, 1100)
    b = run_layer(hip_device, kind, cin, cout, 1100)
    with HipKernels.cu_budget(232):
        c = run_layer(hip_device, kind, cin, cout, 1100)
    for other in (b, c):
        assert bits_equal(a['y'].features, other['y'].features)
        assert torch.equal(a['y'].indices, other['y'].indices)
        for ga, go in zip(a['grads'], other['grads']):
            assert bits_equal(ga, go)


def test_layers_sharing_a_key_build_the_rulebook_once(hip_device):
    from nesie_amd import kernels
    from nesie_amd.mmdet3d_ops import spconv
    rows, _ = value_sites(513, 'subm')
    x = spconv.SparseConvTensor(torch.randn(513, 4, device=hip_device), dev(rows, hip_device),
                                list(VAL_SHAPE), VAL_BATCH)
    first = spconv.SubMConv3d(4, 8, 3, indice_key='subm1').to(hip_device)
    second = spconv.SubMConv3d(8, 8, 3, indice_key='subm1').to(hip_device)
    anonymous = spconv.SubMConv3d(8, 8, 3).to(hip_device)
    rec = Recording()
    with kernels.use_backend(rec):
        y = first(x)
        entry = x.indice_dict['subm1']
        z = second(y)
    assert rec.names().count('spconv_out_sites') == 1
    assert rec.names().count('spconv_gather_table') == 1
    assert rec.names().count('spconv_gather_gemm') == 2
    assert z.indice_dict is x.indice_dict and z.indice_dict['subm1'] is entry
    outids, indices, rules, pair_num, spatial_shape = entry
    assert outids is x.indices and indices is x.indices and spatial_shape == list(VAL_SHAPE)
    assert tuple(rules.nbr.shape) == (513, 27) and tuple(pair_num.shape) == (27,)
    with kernels.use_backend(rec):
        anonymous(z)                       # no key: builds its own, and caches under None
    assert rec.names().count('spconv_out_sites') == 2


def test_forward_and_backward_replay_from_a_graph(hip_device):
    from nesie_amd.mmdet3d_ops import spconv
    rows, _ = value_sites(513, 'subm')
    idx = dev(rows, hip_device)
    torch.manual_seed(3)
    layer = spconv.SubMConv3d(16, 32, 3, indice_key='g').to(hip_device)
    feats = torch.randn(513, 16, device=hip_device, requires_grad=True)
    g_out = torch.randn(513, 32, device=hip_device)
    cache = {}

    def step():
        x = spconv.SparseConvTensor(feats, idx, list(VAL_SHAPE), VAL_BATCH)
        x.indice_dict = cache
        out = layer(x).features
        return (out,) + torch.autograd.grad(out, (feats, layer.weight, layer.bias), g_out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]          # builds and caches the rulebook
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert 'g' in cache
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        with torch.no_grad():
            for t in captured:
                t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert bits_equal(got, want)


# ---- integration -------------------------------------------------------------------------------

def test_voxels_to_sparse_encoder_to_dense(hip_device):
    """points -> dynamic voxelization -> DynamicScatter (mean) -> SparseConvTensor -> two sparse
    conv modules (submanifold, then stride 2) -> SparseBasicBlock -> dense().  BatchNorm in eval
    mode; the ReLUs are taken out so that no threshold decision enters.  Every sparse conv is
    checked on the input the device gave it: its indices against the referee's rulebook, its
    values by the bound."""
    from nesie_amd.mmdet3d_ops import (DynamicScatter, SparseBasicBlock, make_sparse_convmodule,
                                       spconv, voxelization)
    vs, cr = [0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 8.0, 6.0, 4.0]          # grid x 16, y 12, z 8
    shape, batch = [8, 12, 16], 2
    rng = np.random.default_rng(5)
    feats, coors = [], []
    scatter = DynamicScatter(vs, cr, True)
    for b in range(batch):
        pts = rng.uniform(-0.5, 1.0, (700, 4)).astype(np.float32)
        pts[:, :3] = pts[:, :3] * np.float32([6.0, 4.5, 3.0]) + np.float32([1.0, 0.5, 0.2])
        pts = dev(pts, hip_device)
        c = voxelization(pts, vs, cr, -1, -1)
        f, vc = scatter(pts, c)
        feats.append(f)
        coors.append(nn.functional.pad(vc, (1, 0), value=b))
    feats, coors = torch.cat(feats), torch.cat(coors).contiguous()
    assert coors.dtype == torch.int32 and 300 < len(coors) < 1400
    norm = dict(type='BN1d', eps=1e-3, momentum=0.01)
    torch.manual_seed(9)
    net = spconv.SparseSequential(
        make_sparse_convmodule(4, 16, 3, 'subm1', padding=1, norm_cfg=norm),
        make_sparse_convmodule(16, 32, 3, 'down1', stride=2, padding=1, conv_type='SparseConv3d',
                               norm_cfg=norm),
        SparseBasicBlock(32, 32, conv_cfg=dict(type='SubMConv3d', indice_key='subm2'),
                         norm_cfg=norm)).to(hip_device)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net.eval()
    net[0]._modules['2'] = nn.Identity()
    net[1]._modules['2'] = nn.Identity()
    net[2].relu = nn.Identity()
    seen = []
    from nesie_amd.mmdet3d_ops.spconv.conv import SparseConvolution
    convs = [m for m in net.modules() if isinstance(m, SparseConvolution)]
    assert len(convs) == 4
    for m in convs:
        m.register_forward_hook(lambda mod, inp, out: seen.append(
            (mod, inp[0].features.detach().cpu(), inp[0].indices.cpu().numpy(),
             list(inp[0].spatial_shape), out.features.detach(), out.indices.cpu().numpy(),
             list(out.spatial_shape))))
    x = spconv.SparseConvTensor(feats, coors, shape, batch)
    with torch.no_grad():
        out = net(x)
        dense = out.dense()
    assert tuple(dense.shape) == (batch, 32, 4, 6, 8) and out.spatial_shape == [4, 6, 8]
    assert len(seen) == 4 and set(x.indice_dict) == {'subm1', 'down1', 'subm2'}
    for i, (mod, f_in, idx_in, shape_in, f_out, idx_out, shape_out) in enumerate(seen):
        kind = 'subm' if mod.subm else 'conv'
        w_out, w_nbr, _, _ = R.rulebook(idx_in, batch, shape_in, mod.kernel_size, mod.stride,
                                        mod.padding, mod.subm)
        assert np.array_equal(idx_out, w_out)
        assert shape_out == R.geometry(shape_in, mod.kernel_size, mod.stride, mod.padding,
                                       mod.subm)[3]
        args = (kind, f_in, mod.weight.detach().cpu(), None, idx_in, w_out, batch, shape_in,
                mod.stride, mod.padding)
        f64, mag = R.Dense(*args), R.Dense(*args, absolute=True)
        f32 = R.Dense(*args, dtype=torch.float32)
        n = (w_nbr >= 0).sum(1, keepdims=True) * mod.in_channels
        check(f'integration conv {i}', f_out, f64.out.detach(), f32.out.detach(), mag.out.detach(), n)
    # dense() puts the rows where their indices say, zeros elsewhere
    assert torch.equal(dense, R.densify(out.features, out.indices.cpu().numpy(), batch,
                                        out.spatial_shape))
    assert int((dense.abs().sum(1) > 0).sum()) == len(out.indices)
