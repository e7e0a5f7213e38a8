"""GPU tests of the stage-1 CCF_FFN back half (C = 48, hidden = 192) on ffn_dwfc_tb4
(ffn_dwfc_tb.hip), the default for bf16x3 / fp16.  Built like test_gpu_ffn_stage2_tb: ops.ccf_ffn
against the oracle's R.ccf_ffn, in the Block form (norm2 + Q4 double residual, per-sample
DropPath factors) and the bare form, with the project's bars: rel-L2 <= 5e-5 (bf16x3), 2e-3
(fp16).  The shapes are the ones at which the kernel's plane-fill pipeline can go wrong: every z
segment length from 1 to 7 (prologue, drain, and the remainders of the E waves' unroll by two
and the D waves' unroll by three), tiles smaller than 4 x 8 with every halo outside the volume,
and more workgroups than CUs."""
import functools

import pytest
import torch

from tests import cases as C
from tests import ffn_cases
from tests.ffn_cases import _gpu  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

CH, SEEDS = 48, (34, 35, 36)
BARS = {"bf16x3": 5e-5, "fp16": 2e-3}
_run = functools.partial(ffn_cases.run, CH, SEEDS)  # (shape, block, prec, sel=None)
_ref = functools.partial(ffn_cases.ref, CH, SEEDS)  # (shape, block)


def _check(shape, block, prec):
    ref = _ref(shape, block)
    err = C.rel_l2(_run(shape, block, prec), ref)
    print(f"rel-L2 {err:.3e}")
    assert err <= BARS[prec]


# One 4 x 8 tile: the launcher splits D into min(8, D) segments of ZS = ceil(D / min(8, D))
# planes while tiles x segments <= CUs, so D = 1, 9, 17, 26, 35, 44, 53 give ZS = 1 ... 7, all but
# the first with a shorter last segment (9 = 4 x 2 + 1, 17 = 5 x 3 + 2, 26 = 6 x 4 + 2, ...).
@pytest.mark.parametrize("depth", [1, 9, 17, 26, 35, 44, 53])
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage1_tb_segment_lengths(depth, block, prec):
    _check((1, depth, 4, 8), block, prec)


# (1, 1, 1, 1): smaller than the tile, one plane, every halo outside the volume
# (1, 2, 3, 5): ragged in x and y
# (3, 9, 6, 7): two tiles in y, ragged, per-sample DropPath factors
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 3, 5), (3, 9, 6, 7)])
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage1_tb_small_and_ragged(shape, block, prec):
    _check(shape, block, prec)


# (2, 10, 64, 64): 256 tiles, one segment of ZS = 10 each (a second segment would need a second
# round of workgroups); (3, 10, 64, 64): 384 workgroups, more than the 256 CUs
@pytest.mark.parametrize("shape", [(2, 10, 64, 64), (3, 10, 64, 64)])
@pytest.mark.parametrize("block", [False, True])
def test_stage1_tb_long_segment_many_workgroups(shape, block):
    _check(shape, block, "bf16x3")


@pytest.mark.parametrize("shape", [(3, 9, 6, 7), (2, 10, 64, 64)])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage1_tb_repeatable(shape, prec):
    """Two identical calls give bitwise identical outputs (a plane read before it had landed
    would differ from call to call)."""
    assert torch.equal(_run(shape, True, prec), _run(shape, True, prec))


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage1_tb_batch_independent(block, prec):
    """Every volume of the B = 3 call is bitwise the same volume run alone at B = 1."""
    shape = (3, 9, 6, 7)
    out = _run(shape, block, prec)
    for i in range(shape[0]):
        assert torch.equal(out[i], _run(shape, block, prec, sel=i)[0]), i
