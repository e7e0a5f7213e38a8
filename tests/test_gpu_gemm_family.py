"""GPU tests of the MFMA GEMM family's generic entry, ops.linear_rows (wf_linear_fwd): the
plain store epilogue of gemm_rows, gemm_kc and the fallback gemm_ares, which the module tests
reach only through Linear layers.  Each case is bias + act(x) @ w.T (act = GELU(erf) when
gelu_in) against the same product in fp64 on the CPU, with the bars of these operand kinds
(test_gemm_tn_vs_fp64, test_patch_merging_c48_resident_vs_oracle): rel-L2 <= 1e-5 for bf16x3,
<= 2e-3 for fp16.  The operand rounding alone (CPU emulation, fp32 accumulation) gives
4.3-4.4e-6 and 2.9-3.0e-4 on these shapes.

The kernel each case reaches, from a kernel trace (rocprofv3 --kernel-trace) of one
_family_outputs run per precision (profiles/r11/pin_on_parent.txt).  Template arguments
<NT, P, MAP, EPI, ABF16, threads or waves>, MAP 0 = identity, EPI 0 = store, P = 1 for bf16x3
and 2 for fp16, the same kernels in both unless noted; gemm_ares is <BM, P>; grids in
workgroups:

  (45, 48, 192)       gemm_rows<12, P, 0, 0, false, 512>  grid (1, 1)
  (70001, 48, 192)    gemm_rows<12, P, 0, 0, false, 512>  grid (512, 1): 4376 tiles, 4096 waves
  (333, 40, 48)       gemm_rows<3, P, 0, 0, false, 512>   grid (3, 1)
  (1000, 96, 384)     gemm_kc<3, P, 0, 0, false, 8>       grid (8, 8, 1)
  (45003, 96, 384)    gemm_kc<8, P, 0, 0, false, 16>      grid (176, 3, 1)
  (300, 72, 384)      gemm_kc<6, P, 0, 0, false, 8>       grid (3, 4, 1)
  (257, 384, 96)      gemm_kc<3, P, 0, 0, false, 8>       grid (3, 2, 1)
  (130, 1536, 384)    gemm_kc<6, P, 0, 0, false, 8>       grid (2, 4, 1): no split-K
  (777, 72, 40)       gemm_ares<64, P>                    grid (13)
  (50, 384, 20)       gemm_ares<32, 1> grid (2) for bf16x3, gemm_ares<64, 2> grid (1) for fp16"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle.weight_rule import seeded_randn
from tests import cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
BARS = {"bf16x3": 1e-5, "fp16": 2e-3}

# (M, K, N, gelu_in, bias)
CASES = (
    (45, 48, 192, 0, True),       # gemm_rows NT = 12, a partial 16-row tile
    (70001, 48, 192, 0, False),   # gemm_rows, 512 workgroups, more than one tile per wave
    (333, 40, 48, 1, True),       # gemm_rows NT = 3, K not a multiple of 32, GELU loader
    (1000, 96, 384, 0, True),     # gemm_kc NT = 3, odd k-step count (3)
    (45003, 96, 384, 0, False),   # gemm_kc NT = 8 on the 16-wave workgroups (1056 >= 1024)
    (300, 72, 384, 1, True),      # gemm_kc NT = 6 (the minnt rule), K tail of 8
    (257, 384, 96, 0, False),     # gemm_kc NT = 3, 12 k steps
    (130, 1536, 384, 1, True),    # gemm_kc, 48 k steps, no split-K (no scratch)
    (777, 72, 40, 0, True),       # gemm_ares BM = 64, N not a multiple of 16
    (50, 384, 20, 1, False),      # gemm_ares BM = 32 (bf16x3) / 64 (fp16)
)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    yield


@functools.lru_cache(maxsize=None)
def _family_inputs():
    """(x, w, bias or None, fp64 reference) of every case: computed once, never modified."""
    rows = []
    for i, (M, K, N, gelu_in, has_bias) in enumerate(CASES):
        x = seeded_randn((M, K), 900 + 3 * i)
        w = seeded_randn((N, K), 901 + 3 * i) * 0.1
        bias = seeded_randn((N,), 902 + 3 * i) if has_bias else None
        a = x.double()
        if gelu_in:
            a = F.gelu(a)  # erf form
        ref = a @ w.double().t()
        if has_bias:
            ref = ref + bias.double()
        rows.append((x, w, bias, ref))
    return tuple(rows)


def _family_outputs(prec):
    """ops.linear_rows(x, w, bias, gelu_in) over CASES: (output.cpu(), fp64 reference) pairs."""
    from waveformer_amd import ops
    outs = []
    for (M, K, N, gelu_in, _), (x, w, bias, ref) in zip(CASES, _family_inputs()):
        with torch.no_grad(), ops.precision(prec):
            out = ops.linear_rows(x.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV),
                                  bool(gelu_in))
        outs.append((out.cpu(), ref))
    return outs


_first_outputs = functools.lru_cache(maxsize=None)(_family_outputs)


@pytest.mark.parametrize("case", range(len(CASES)), ids=["x".join(map(str, c[:3])) for c in CASES])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_linear_rows_vs_fp64(prec, case):
    out, ref = _first_outputs(prec)[case]
    assert out.shape == ref.shape and out.dtype == torch.float32
    err = C.rel_l2(out, ref)
    print(f"{CASES[case]} {prec}: rel-L2 {err:.3e}")
    assert err <= BARS[prec]


@pytest.mark.parametrize("prec", ["bf16x3", "fp16"])
def test_linear_rows_repeatable(prec):
    """A second call gives bitwise the outputs of the first, case by case."""
    for case, (a, b) in zip(CASES, zip(_first_outputs(prec), _family_outputs(prec))):
        assert torch.equal(a[0], b[0]), case
