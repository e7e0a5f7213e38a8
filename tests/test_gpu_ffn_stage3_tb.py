"""GPU tests of the stage-3 CCF_FFN back half (C = 192, hidden = 768) on ffn_dwfc3_tb
(ffn_dwfc3_tb.hip), the default for bf16x3 / fp16 at inference: depthwise conv, LN2, GELU, fc and
the Q4 residual in one kernel, the fc weight streamed from L2.  Built like
test_gpu_parity.test_ccf_ffn_stage34_vs_oracle (rule weights, norm2, per-sample DropPath factors
0.5 / 2.0 / 1.0): ops.ccf_ffn against the oracle's R.ccf_ffn in the Block form (norm2 + Q4 double
residual) and the bare form, with the project's bars: rel-L2 <= 5e-5 (bf16x3), 2e-3 (fp16)."""
import functools

import pytest
import torch

from tests import cases as C
from tests import ffn_cases
from tests.ffn_cases import _gpu  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

CH, SEEDS = 192, (37, 38, 39)
BARS = {"bf16x3": 5e-5, "fp16": 2e-3}
_run = functools.partial(ffn_cases.run, CH, SEEDS)  # (shape, block, prec, sel=None)
_ref = functools.partial(ffn_cases.ref, CH, SEEDS)  # (shape, block)


# The segment rule (launch_ffn_dwfc3): ZS = D, halved (rounding up) while ZS > 8 and B x tiles x
# segments < 256.  One 4 x 4 tile, so the grid is the z segments alone: depths 1 ... 8 are one
# segment of that length, 9 -> 5 + 4, 10 -> 5 + 5, 11 -> 6 + 5, 13 -> 7 + 6, 17 -> 5 + 5 + 5 + 2:
# every segment length 1 ... 8, with and without a shorter last segment.  A segment of n planes
# runs n + 3 iterations (four before the first fc, the last fc behind the loop): lengths 1 and 2
# end before the accumulator rotation is complete, 3 ends with it, 4 ... 8 end in every rotation
# phase and h2 buffer (t mod 3).
FILL_DRAIN = [(1, d, 4, 4) for d in (1, 2, 3, 4, 5, 8, 9, 10, 11, 13, 17)]
# (1, 3, 1, 1), (1, 3, 2, 3): smaller than a tile, every halo position outside the volume
# (1, 3, 5, 7): ragged in y and x (tiles of 1 x 3 positions at the far faces)
# (1, 3, 8, 8): four tiles, so halo rows and columns that ARE inside the volume
# (2, 3, 4, 4): two samples: the planes before and behind a sample belong to its neighbour
HALO = [(1, 3, 1, 1), (1, 3, 2, 3), (1, 3, 5, 7), (1, 3, 8, 8), (2, 3, 4, 4)]


@pytest.mark.parametrize("shape", FILL_DRAIN + HALO)
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage3_tb_vs_oracle(shape, block, prec):
    err = C.rel_l2(_run(shape, block, prec), _ref(shape, block))
    print(f"rel-L2 {err:.3e}")
    assert err <= BARS[prec]


@pytest.mark.parametrize("shape", [(1, 17, 4, 4), (2, 3, 4, 4), (1, 3, 5, 7)])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage3_tb_repeatable(shape, prec):
    """Two identical calls give bitwise identical outputs."""
    assert torch.equal(_run(shape, True, prec), _run(shape, True, prec))


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage3_tb_batch_independent(block, prec):
    """Every volume of the B = 3 call is bitwise the same volume run alone at B = 1: no load
    reaches into the neighbouring sample, and neither LN2's reduction nor the fc's k order
    depends on the batch or the grid."""
    shape = (3, 9, 6, 7)
    out = _run(shape, block, prec)
    for i in range(shape[0]):
        assert torch.equal(out[i], _run(shape, block, prec, sel=i)[0]), i


@pytest.mark.parametrize("shape", [(3, 17, 4, 4), (3, 17, 28, 28)])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage3_tb_segment_seams(shape, prec):
    """A volume of depth 17 inside a batch of three is bitwise the volume run alone.  At 4 x 4
    both calls cut it alike (5 + 5 + 5 + 2); at 28 x 28 (49 tiles) the batch stops halving at
    segments of 9 planes (3 x 49 x 2 >= 256) and the single volume goes on to 5, so the seams
    lie elsewhere: a plane's result must not depend on where its segment starts or ends (the
    seam planes are loaded, not zero-filled)."""
    out = _run(shape, True, prec)
    for i in range(shape[0]):
        assert torch.equal(out[i], _run(shape, True, prec, sel=i)[0]), i


@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage3_tb_and_staged_path_meet_the_oracle(prec, monkeypatch):
    """The fused kernel and the staged path (dwconv3d + the fc GEMM with LN2 + GELU in its loader,
    reached with WF_FFN_NO_DWFC=1, read per call) order the LN2 moments and the k sum differently,
    so they are not bitwise equal: each meets the oracle bar; their distance is printed."""
    shape = (2, 8, 8, 8)
    ref = _ref(shape, True)
    fused = _run(shape, True, prec)
    monkeypatch.setenv("WF_FFN_NO_DWFC", "1")
    staged = _run(shape, True, prec)
    monkeypatch.delenv("WF_FFN_NO_DWFC")
    e_f, e_s, e_fs = C.rel_l2(fused, ref), C.rel_l2(staged, ref), C.rel_l2(fused, staged)
    print(f"rel-L2 {prec}: fused vs oracle {e_f:.3e}, staged vs oracle {e_s:.3e}, "
          f"fused vs staged {e_fs:.3e}")
    assert e_f <= BARS[prec] and e_s <= BARS[prec]
