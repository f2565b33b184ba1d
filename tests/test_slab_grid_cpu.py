"""The slab grid the slice-marching operators share (csrc/slab_grid.h: 8 x 32 tiles of axes 1 and 2, axis 0 split into chunks until
about 2 048 workgroups exist, no chunk shorter than the operator's minimum), restated here and held against the two workspace sizes
that are a function of its workgroup count: TV keeps two fp64 partials per workgroup and a minimum chunk of 8, SSIM one partial and
16 and lays the grid over its window starts (every extent minus 6).  No GPU needed."""
import itertools

TILE_Y, TILE_Z, TARGET_BLOCKS = 8, 32, 2048
N1 = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000)
N2 = (1, 8, 9, 255, 256, 257)
N3 = (1, 32, 33, 255, 256, 257)
SHAPES = list(itertools.product(N1, N2, N3)) + [(1024, 1024, 1024)]


def slab_blocks(m1, m2, m3, min_chunk):
    tiles = -(-m2 // TILE_Y) * -(-m3 // TILE_Z)
    want = max(1, min(-(-TARGET_BLOCKS // tiles), -(-m1 // min_chunk)))
    chunk = -(-m1 // want)
    return tiles * -(-m1 // chunk)


def round256(n):
    return (n + 255) & ~255


def test_the_restatement_splits_as_documented():
    assert slab_blocks(40, 9, 33, 8) == 2 * 2 * 5                  # 2 x 2 ragged tiles, 5 chunks of 8
    assert slab_blocks(32, 9, 33, 16) == 2 * 2 * 2                 # SSIM's window starts of a (38, 15, 39) volume: 2 chunks of 16
    assert slab_blocks(1024, 1024, 1024, 8) == 128 * 32            # 4 096 tiles are above the target already: one chunk each
    assert slab_blocks(1000, 1, 1, 8) == 125 and slab_blocks(1000, 1, 1, 16) == 63


def test_tv_workspace_is_two_fp64_partials_per_workgroup():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    size = _abi.lib().naf_tv_workspace_bytes
    for n in SHAPES:
        assert size(*n) == round256(16 * slab_blocks(*n, 8)), n
    assert size(0, 8, 32) == 0 and size(8, 0, 32) == 0 and size(8, 8, 0) == 0


def test_ssim_workspace_is_one_fp64_partial_per_workgroup_of_window_starts():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    size = _abi.lib().naf_ssim_3d_workspace_bytes
    for m in SHAPES:
        n = tuple(e + 6 for e in m)
        assert size(*n) == round256(8 * slab_blocks(*m, 16)), n
    assert size(6, 7, 7) == 0 and size(7, 6, 7) == 0 and size(7, 7, 6) == 0
