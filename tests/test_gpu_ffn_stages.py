"""GPU: the stage argument of wf_ccf_ffn_stage, for every stage width of the encoder (C = 48, 96,
192, 384 at (2, 3, 5, 7), Block form with per-sample DropPath factors, bf16x3 and bf16):
one wf_ccf_ffn_fwd call is bitwise the three calls stage 1, 2, 3 on a fresh workspace, and `out`
already holds the final result after stages 1 and 2 exactly when the plan's back half is one
fused kernel (wf_ccf_ffn_plan), whose stage 3 is then a no-op.  Built by tests/ffn_cases."""
import pytest
import torch

from tests import ffn_cases
from tests.ffn_cases import _gpu  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu

SHAPE, SEEDS = (2, 3, 5, 7), (34, 35, 36)


def _back_is_fused(ch, prec):
    from waveformer_amd import _lib
    plan = _lib.query("wf_ccf_ffn_plan", SHAPE[0], ch, 4 * ch, *SHAPE[1:], prec, 0, None)
    assert plan >= 0
    return (plan >> 8) <= 5  # ffn_fused, ffn_dwfc_tb4 / sb, ffn_dwfc2_tb / kernel, ffn_dwfc3_tb


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("ch", [48, 96, 192, 384])
def test_fwd_is_the_three_stages(ch, prec):
    from waveformer_amd import _lib, ops
    p = ops.PRECISIONS[prec]
    B, D, H, W = SHAPE
    with torch.no_grad(), ops.precision(prec):
        x, stats, n2, mlp, bs = ffn_cases.device_inputs(ch, SEEDS, SHAPE, True)
        pw = ops.split_weight(mlp.pwconv.weight, (4 * ch, ch), p)
        fc = ops.split_weight(mlp.fc.weight, prec=p)
        wsb = _lib.query("wf_ccf_ffn_workspace_bytes", B, ch, 4 * ch, D, H, W, p)

        def args(out):  # a fresh workspace per call sequence
            work = torch.zeros(wsb, dtype=torch.uint8, device=x.device)
            return work, (x.data_ptr(), stats.data_ptr(), n2.weight.data_ptr(), n2.bias.data_ptr(),
                          pw.data_ptr(), ops._ptr(mlp.pwconv.bias), mlp.norm1.weight.data_ptr(),
                          mlp.norm1.bias.data_ptr(), float(mlp.norm1.eps),
                          mlp.dwconv.weight.data_ptr(), mlp.dwconv.bias.data_ptr(),
                          mlp.norm2.weight.data_ptr(), mlp.norm2.bias.data_ptr(),
                          float(mlp.norm2.eps), fc.data_ptr(), ops._ptr(mlp.fc.bias),
                          bs.data_ptr(), out.data_ptr(), work.data_ptr(), B, ch, 4 * ch, D, H, W, p,
                          ops._stream())

        whole = torch.zeros_like(x)
        keep0, a = args(whole)
        _lib.call("wf_ccf_ffn_fwd", *a)
        staged = torch.zeros_like(x)
        keep1, a = args(staged)
        _lib.call("wf_ccf_ffn_stage", 1, *a)
        _lib.call("wf_ccf_ffn_stage", 2, *a)
        after2 = staged.clone()
        _lib.call("wf_ccf_ffn_stage", 3, *a)
        torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and whole.abs().max() > 0
    assert torch.equal(whole, staged)
    assert torch.equal(after2, whole) == _back_is_fused(ch, p)
