"""The float32 restatement the GPU bit tests compare against (tests/_blend_ref.py) is itself the
reference's three_interpolate in the segmented layout: without wx it equals the oracle bit for bit."""
import pytest
import torch

from tests import _blend_ref


@pytest.mark.parametrize("k,segs,g,c,m,b,shared", [
    (4, 6, 16, 64, 37, 3, True),        # one column block for every face: the segmented three_interpolate
    (8, 6, 27, 24, 300, 2, False),      # one column block per face
])
def test_restatement_equals_oracle_three_interpolate(oracle_kernels, k, segs, g, c, m, b, shared):
    # (the reference's kernel does not clamp: in-range taps only)
    case = _blend_ref.make_case(k, segs, g, c, m, b, 7, with_wx=False, edge_taps=False,
                                pitch=c if shared else None, seg_off=0 if shared else None)
    want = torch.full((b, segs, c + 3, k * g), float('nan'))
    oracle_kernels.blend_conv_forward(case['table'], case['seg_off'], case['idx'], case['weight'],
                                      None, None, want, segs, g, c, 3)
    assert torch.isnan(want[:, :, :3]).all()
    assert torch.equal(_blend_ref.blend_forward_ref(case), want[:, :, 3:])
