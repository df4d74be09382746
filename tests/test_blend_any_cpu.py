"""Which blend backward serves a shape: ``kernels.blend_backward_form`` (no GPU needed)."""
import pytest

from nesie_amd import kernels

# (c, queries per face, seeds) of the shipped quality heads: side grid, SAQE box grid, Nesie box grid
REFERENCE_SHAPES = [(256, 8192, 1024), (128, 13824, 1024), (256, 32768, 1024)]

# (k, segs, g, c, m): the smallest shapes at which each limit of the tile kernels is crossed
GENERAL_SHAPES = [
    (24, 6, 27, 128, 300),     # 648 queries per face
    (5, 6, 9, 19, 7),          # odd c, pitch 114, 45 queries per face, 7 seeds
    (33, 1, 64, 8, 300),       # c < 64, one face
    (64, 6, 16, 320, 300),     # c > 256
    (64, 6, 16, 128, 2048),    # exactly 2048 seeds
    (64, 1, 64, 64, 2500),     # seed count no multiple of 64
]


@pytest.mark.parametrize('c,per_seg,m', REFERENCE_SHAPES)
def test_reference_shapes_stay_on_the_staged_form(c, per_seg, m):
    assert kernels.blend_backward_form(c, per_seg, m, True) == 'staged'
    assert kernels.blend_backward_form(c, per_seg, m, False) == 'atomic'


@pytest.mark.parametrize('k,segs,g,c,m', GENERAL_SHAPES)
def test_general_shapes_go_to_the_general_form(k, segs, g, c, m):
    assert kernels.blend_backward_form(c, k * g, m, True) == 'any'


@pytest.mark.parametrize('k,segs,g,c,m', [s for s in GENERAL_SHAPES if s[4] < 2048])
def test_shapes_without_a_tile_kernel_go_to_the_general_form_in_both_modes(k, segs, g, c, m):
    assert kernels.blend_backward_form(c, k * g, m, False) == 'any'


def test_atomic_form_takes_tile_shapes_of_any_seed_count():
    assert kernels.blend_backward_form(128, 1024, 4096, False) == 'atomic'
    assert kernels.blend_backward_form(128, 1024, 4096, True) == 'any'
    assert kernels.blend_backward_form(128, 1024, 2047, True) == 'staged'
    assert kernels.blend_backward_form(128, 1024, 2048, True) == 'any'


def test_empty_faces_go_to_the_general_form():
    """n = 0: the general form writes the zeros; the tile kernels return without a launch."""
    assert kernels.blend_backward_form(128, 0, 300, True) == 'any'
    assert kernels.blend_backward_form(128, 0, 300, False) == 'any'


def test_writes_table_follows_the_form():
    hip = kernels.HipKernels
    prev = hip.DETERMINISTIC
    try:
        hip.DETERMINISTIC = True
        assert hip.blend_backward_writes_table(hip, 19, 5 * 6 * 9, 6, 7)
        assert hip.blend_backward_writes_table(hip, 256, 8192 * 6, 6, 1024)
        hip.DETERMINISTIC = False
        assert hip.blend_backward_writes_table(hip, 19, 5 * 6 * 9, 6, 7)
        assert not hip.blend_backward_writes_table(hip, 256, 8192 * 6, 6, 1024)
    finally:
        hip.DETERMINISTIC = prev
