"""GPU tests of the stage-2 CCF_FFN back half (C = 96, hidden = 384) on ffn_dwfc2_tb
(ffn_dwfc2_tb.hip), the default for bf16x3 / fp16, and of the launcher's choice between it and
ffn_dwfc2_kernel (bf16 h1, tensors of 2 GiB and above).  Built like
test_gpu_parity.test_ccf_ffn_stage2_vs_oracle: ops.ccf_ffn against the oracle's R.ccf_ffn, in
the Block form (norm2 + Q4 double residual, per-sample DropPath factors) and the bare form, with
that test's bars: rel-L2 <= 5e-5 (bf16x3), 2e-3 (fp16), 1e-2 (bf16)."""
import functools

import pytest
import torch

from oracle.weight_rule import rule_state_dict
from tests import cases as C
from tests import ffn_cases
from tests.ffn_cases import DEV, _gpu  # noqa: F401  (_gpu: autouse)

pytestmark = pytest.mark.gpu

CH, SEEDS = 96, (34, 35, 36)
BARS = {"bf16x3": 5e-5, "fp16": 2e-3, "bf16": 1e-2}
_run = functools.partial(ffn_cases.run, CH, SEEDS)  # (shape, block, prec, sel=None)
_ref = functools.partial(ffn_cases.ref, CH, SEEDS)  # (shape, block)


# (1, 1, 1, 1): smaller than the tile, one plane, every halo outside the volume
# (1, 2, 3, 5): ragged in x and y
# (1, 17, 5, 7): z segments with a remainder (the launcher halves 17 -> 9 -> 5: 5 + 5 + 5 + 2)
# (3, 9, 6, 7): per-sample DropPath factors
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 3, 5), (1, 17, 5, 7), (3, 9, 6, 7)])
@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_tb_vs_oracle(shape, block, prec):
    ref = _ref(shape, block)
    err = C.rel_l2(_run(shape, block, prec), ref)
    print(f"rel-L2 {err:.3e}")
    assert err <= BARS[prec]


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_tb_batch_independent(block, prec):
    """Every volume of the B = 3 call is bitwise the same volume run alone at B = 1: neither the
    straddled fc tile's two-wave sum nor LN2's reduction depends on the batch or the grid."""
    shape = (3, 9, 6, 7)
    out = _run(shape, block, prec)
    for i in range(shape[0]):
        assert torch.equal(out[i], _run(shape, block, prec, sel=i)[0]), i


@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_stage2_tb_repeatable(prec):
    """Two identical calls give bitwise identical outputs."""
    shape = (3, 9, 6, 7)
    assert torch.equal(_run(shape, True, prec), _run(shape, True, prec))


@pytest.mark.parametrize("block", [False, True])
def test_stage2_tb_more_tiles_than_cus(block):
    """(2, 8, 48, 48): 288 tiles of 4 x 4 in one z segment, more workgroups than the 256 CUs."""
    shape = (2, 8, 48, 48)
    ref = _ref(shape, block)
    err = C.rel_l2(_run(shape, block, "bf16x3"), ref)
    print(f"rel-L2 {err:.3e}")
    assert err <= BARS["bf16x3"]


def test_stage2_batch_beyond_tb_range():
    """ffn_dwfc2_tb addresses x and its output through 32-bit buffer offsets (2 GiB).  At
    32^3 x 96 that is B >= 171 (170 stays below): the launcher must take ffn_dwfc2_kernel
    instead of failing.  Samples 0 and 170 of a B = 171 call against the same two volumes run
    at B = 2 (ffn_dwfc2_tb): two kernels compared at rel-L2 <= 1e-6, as
    test_ccf_ffn_stage1_batch_beyond_tb4_range does."""
    import waveformer_amd.network_models as NM
    from waveformer_amd import ops
    S, B = 32, 171
    assert B * S ** 3 * CH * 4 >= 2 ** 31 > (B - 1) * S ** 3 * CH * 4
    mlp = NM.CCF_FFN(CH, 4 * CH, img_size=(S,) * 3)
    mlp.load_state_dict(rule_state_dict(mlp.state_dict()))
    mlp = mlp.eval().to(DEV)
    with torch.no_grad(), ops.precision("bf16x3"):
        x = torch.randn((B, S, S, S, CH), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
        out = ops.ccf_ffn(x, None, None, mlp, None)
        pair = torch.stack([x[0], x[-1]])
        ref = ops.ccf_ffn(pair, None, None, mlp, None)
    torch.cuda.synchronize()
    e0, e1 = C.rel_l2(out[0], ref[0]), C.rel_l2(out[-1], ref[1])
    print(f"rel-L2 {e0:.3e} {e1:.3e}")
    assert e0 <= 1e-6 and e1 <= 1e-6
    del x, out


@pytest.mark.parametrize("block", [False, True])
def test_stage2_bf16_keeps_dwfc2_kernel(block):
    """bf16 precision (bf16 h1) still runs ffn_dwfc2_kernel."""
    shape = (1, 17, 5, 7)
    ref = _ref(shape, block)
    err = C.rel_l2(_run(shape, block, "bf16"), ref)
    print(f"rel-L2 {err:.3e}")
    assert err <= BARS["bf16"]
