"""GPU tests of what ffn_dwfc2_tb (ffn_dwfc2_tb.hip) gained with the direct depthwise loads and
the two-tile, two-barrier schedule: the pipeline's fill and drain (three accumulator rotations,
two h2 tiles, the fc three planes behind the scatter) on z segments of every short length, and
the zero fill of the haloed loads at every face, corner, tile edge and batch boundary.  The
construction, the oracle call and the bars are those of test_gpu_ffn_stage2_tb (rel-L2 <= 5e-5 at
bf16x3, 2e-3 at fp16; Block form with norm2 + Q4 double residual and bare form; per-sample
DropPath factors 0.5, 2.0, 1.0)."""
import pytest
import torch

from tests import cases as C
from tests.test_gpu_ffn_stage2_tb import BARS, _gpu, _ref, _run  # noqa: F401  (_gpu: autouse)

pytestmark = pytest.mark.gpu

# One 4 x 4 tile, so the grid is the z segments alone.  The launcher halves the segment while it
# is longer than 8 planes (few workgroups): depths 1 ... 8 are one segment of that length, 9 ->
# 5 + 4, 10 -> 5 + 5, 11 -> 6 + 5, 13 -> 7 + 6, 17 -> 5 + 5 + 5 + 2.  A segment of n planes runs
# n + 3 iterations: lengths 1 and 2 end before the first rotation is complete, 3 ends with it,
# 4 ... 7 end in every rotation phase and h2 buffer parity.
FILL_DRAIN = [(1, d, 4, 4) for d in (1, 2, 3, 4, 5, 8, 9, 10, 11, 13, 17)]
# (1, 3, 1, 1), (1, 3, 2, 3): smaller than a tile, every halo position outside the volume
# (1, 3, 5, 7): ragged in y and x (tiles of 1 x 3 positions at the far faces)
# (1, 3, 8, 8): four tiles, so halo rows and columns that ARE inside the volume
# (2, 3, 4, 4): two samples: the planes before and behind a sample belong to its neighbour
HALO = [(1, 3, 1, 1), (1, 3, 2, 3), (1, 3, 5, 7), (1, 3, 8, 8), (2, 3, 4, 4)]


@pytest.mark.parametrize("shape", FILL_DRAIN + HALO)
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_direct_vs_oracle(shape, block, prec):
    err = C.rel_l2(_run(shape, block, prec), _ref(shape, block))
    print(f"rel-L2 {err:.3e}")
    assert err <= BARS[prec]


@pytest.mark.parametrize("shape", [(1, 17, 4, 4), (2, 3, 4, 4), (1, 3, 5, 7)])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_direct_repeatable(shape, prec):
    """Two identical calls give bitwise identical outputs."""
    assert torch.equal(_run(shape, True, prec), _run(shape, True, prec))


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_direct_batch_independent(block, prec):
    """Every volume of the B = 3 call is bitwise the same volume run alone at B = 1: no load
    reaches into the neighbouring sample."""
    shape = (3, 9, 6, 7)
    out = _run(shape, block, prec)
    for i in range(shape[0]):
        assert torch.equal(out[i], _run(shape, block, prec, sel=i)[0]), i


@pytest.mark.parametrize("shape", [(3, 17, 4, 4), (3, 17, 36, 40)])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_direct_segment_seams(shape, prec):
    """A volume of depth 17 inside a batch of three is bitwise the volume run alone.  At 4 x 4
    both calls cut it alike; at 36 x 40 the batch has enough tiles for longer segments than
    the single volume gets, so the seams lie elsewhere: a plane's result must not depend on
    where its segment starts or ends (the seam planes are loaded, not zero-filled)."""
    out = _run(shape, True, prec)
    for i in range(shape[0]):
        assert torch.equal(out[i], _run(shape, True, prec, sel=i)[0]), i
