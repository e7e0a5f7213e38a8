"""What the GPU tests of the CCF_FFN kernels share (test_gpu_ffn_stage*_tb / _direct,
test_gpu_ffn_stages): a CCF_FFN of `ch` channels with the rule weights, the Block's norm2, a
seeded input, the per-sample DropPath factors 0.5 / 2.0 / 1.0, the oracle's output (R.ccf_ffn) in
the Block form (norm2 + Q4 double residual) and the bare form, and the call of ops.ccf_ffn.
`seeds` = (norm2 weight, norm2 bias, input).  Everything is a function of (ch, seeds, shape)
alone: made once, shared by every test that asks for it, never modified."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_waveformer as R
from oracle.weight_rule import rule_state_dict, seeded_randn

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    """Imported by the test modules: skip without a GPU, fail loudly without the library."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()
    yield


@functools.lru_cache(maxsize=None)
def norm2(ch, seeds):
    """The Block's norm2: the module on the CPU (the oracle's) and its copy on the device."""
    n = torch.nn.LayerNorm(ch, eps=1e-6)
    with torch.no_grad():
        n.weight.copy_(seeded_randn((ch,), seeds[0]) * 0.2 + 1)
        n.bias.copy_(seeded_randn((ch,), seeds[1]) * 0.1)
    return n, copy.deepcopy(n).to(DEV)


@functools.lru_cache(maxsize=None)
def model(ch, seeds, shape):
    """(CCF_FFN on the device, its state dict, input, per-sample factors) of one (B, D, H, W)."""
    import waveformer_amd.network_models as NM
    mlp = NM.CCF_FFN(ch, 4 * ch, img_size=shape[1:])
    sd = rule_state_dict(mlp.state_dict())
    mlp.load_state_dict(sd)
    x = seeded_randn(shape + (ch,), seeds[2])
    bs = torch.tensor([0.5, 2.0, 1.0][:shape[0]])
    return mlp.eval().to(DEV), sd, x, bs


@functools.lru_cache(maxsize=None)
def ref(ch, seeds, shape, block):
    """The oracle's output of one shape and form (CPU, fp32)."""
    _, sd, x, bs = model(ch, seeds, shape)
    n2 = norm2(ch, seeds)[0]
    with torch.no_grad():
        if block:
            n = F.layer_norm(x, [ch], n2.weight, n2.bias, 1e-6)
            return x + R.ccf_ffn(sd, "", n) * bs.view(-1, 1, 1, 1, 1)
        return x + (R.ccf_ffn(sd, "", x) - x) * bs.view(-1, 1, 1, 1, 1)


def device_inputs(ch, seeds, shape, block, sel=None):
    """(x, norm2's row statistics or None, norm2 or None, mlp, factors) on the device, of the
    whole batch of `shape` or of its sample `sel` alone (B = 1)."""
    from waveformer_amd import ops
    mlp, _, x, bs = model(ch, seeds, shape)
    if sel is not None:
        x, bs = x[sel:sel + 1], bs[sel:sel + 1]
    xc = x.to(DEV)
    stats = ops.msfuse([], xc, 1e-6)[1] if block else None
    return xc, stats, norm2(ch, seeds)[1] if block else None, mlp, bs.to(DEV)


def run(ch, seeds, shape, block, prec, sel=None):
    """ops.ccf_ffn on the whole batch of `shape`, or on its sample `sel` alone (B = 1)."""
    from waveformer_amd import ops
    with torch.no_grad(), ops.precision(prec):
        return ops.ccf_ffn(*device_inputs(ch, seeds, shape, block, sel))
