"""blend_fwd_kernel (the MiniPointNets' first convolution as a 3-NN blend, and the segmented
three_interpolate) against its float32 restatement on the CPU, tests/_blend_ref.py: outputs and
statistics partials compared with torch.equal -- every rounding and every summation order of the
kernel is part of its contract (the training step's bits hang on them)."""
import pytest
import torch

from nesie_amd import kernels
from tests import _blend_ref

pytestmark = pytest.mark.gpu

# (k, segs, g, c, m, b)
CASES = [
    (4, 6, 16, 64, 37, 3),       # one tile per face; batch not a divisor of 8
    (8, 6, 16, 256, 300, 2),     # 16-byte lanes
    (64, 6, 27, 128, 300, 2),    # seg_len not a power of two; tiles straddle proposals
    (2, 1, 64, 192, 50, 1),      # three channels per lane
    (16, 1, 64, 512, 300, 1),    # chunked channels
]
# conv:    wx . rel + statistics, the table one column block per face (the quality head's call)
# plain:   the same without statistics
# interp:  no wx / rel, ONE column block for every face (seg_off = 0), written at c_offset = 3 of
#          c + 3 channels: the segmented three_interpolate; with statistics
# pitched: pitch = segs * c + 3 with seg_off = c, no statistics, no wx
MODES = ['conv', 'plain', 'interp', 'pitched']

_refs = {}


def _reference(case_id, mode):
    """(case, out, partial) on the CPU, computed once per (case, mode) and never modified."""
    key = (case_id, mode)
    if key not in _refs:
        k, segs, g, c, m, b = CASES[case_id]
        seed = 100 * case_id + MODES.index(mode)
        if mode in ('conv', 'plain'):
            case = _blend_ref.make_case(k, segs, g, c, m, b, seed)
        elif mode == 'interp':
            case = _blend_ref.make_case(k, segs, g, c, m, b, seed, with_wx=False, pitch=c, seg_off=0)
        else:       # (+ 3: rows that are 4-byte but not 16-byte aligned)
            case = _blend_ref.make_case(k, segs, g, c, m, b, seed, with_wx=False, pitch=segs * c + 3)
        out = _blend_ref.blend_forward_ref(case)
        _refs[key] = (case, out, _blend_ref.blend_stats_ref(out))
    return _refs[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case_id", range(len(CASES)))
def test_blend_forward_bits(hip_device, case_id, mode):
    case, want, want_part = _reference(case_id, mode)
    k, segs, g, c, m, b = CASES[case_id]
    assert (k * g) % 64 == 0 and c % 64 == 0          # the tile kernel's shapes
    assert (case['idx'] == -1).any() and (case['idx'] == m).any()      # the clamp is exercised
    hip = kernels.backend_for(torch.empty(1, device=hip_device))
    dev = lambda t: None if t is None else t.to(hip_device)
    c_offset = 3 if mode == 'interp' else 0
    c_total = c + c_offset
    with_stats = mode in ('conv', 'interp')
    out = torch.full((b, segs, c_total, k * g), float('nan'), device=hip_device)
    part = torch.full((segs * c, b * (k * g // 64), 2), float('nan'), device=hip_device) if with_stats else None
    hip.blend_conv_forward(dev(case['table']), case['seg_off'], dev(case['idx']), dev(case['weight']),
                           dev(case['rel']), dev(case['wx']), out, segs, g, c, c_offset,
                           stat_partial=part)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isnan(got[:, :, :c_offset]).all()                       # channels outside stay untouched
    assert not torch.isnan(got[:, :, c_offset:]).any()                   # everything inside is written
    assert torch.equal(got[:, :, c_offset:], want)
    if with_stats:
        assert torch.equal(part.cpu(), want_part)
