"""CPU: what wf_ccf_ffn_stage does for a shape, asked of the library without a launch
(wf_ccf_ffn_plan, csrc/ffn_plan.hpp): the form LN1 + GELU takes, the kernels of the back half, and
the workspace layout.  The table below was derived by reading the dispatch code as it stood before
the plan had a name; the tests assert it, not whatever the library answers.
"fp32" rows hold for bf16x3 and fp16 (fp32 h1).  WF_FFN_LN1_FUSE is latched per process and has
its child-process GPU test in test_gpu_parity.  Host only, no GPU."""
import ctypes

import pytest

from waveformer_amd import _lib

EPI, PASS, PARTIALS, NONE = 0, 1, 2, 3                                   # front
FUSED, TB4, SB, DWFC2_TB, DWFC2_KERNEL, DWFC3_TB, STAGED, STAGED_DWLN = range(8)  # back
FP32, BF16, ANY = (1, 2), (0,), (0, 1, 2)

# (C, hidden, precisions, train, (B, D, H, W), front, back)
TABLE = [
    (48, 192, FP32, 0, (8, 64, 64, 64), EPI, TB4),
    (48, 192, FP32, 0, (42, 64, 64, 64), EPI, TB4),
    (48, 192, FP32, 0, (43, 64, 64, 64), EPI, SB),         # x / out reach 2 GiB
    (48, 192, FP32, 0, (1, 1, 1672, 1672), EPI, TB4),
    (48, 192, FP32, 0, (1, 1, 1673, 1673), EPI, SB),       # one h1 plane reaches 2 GiB
    (48, 192, BF16, 0, (8, 64, 64, 64), EPI, SB),
    (48, 192, ANY, 1, (2, 8, 8, 8), EPI, STAGED),
    (96, 384, FP32, 0, (170, 32, 32, 32), EPI, DWFC2_TB),
    (96, 384, FP32, 0, (171, 32, 32, 32), EPI, DWFC2_KERNEL),
    (96, 384, BF16, 0, (8, 32, 32, 32), EPI, DWFC2_KERNEL),
    (192, 768, FP32, 0, (682, 16, 16, 16), EPI, DWFC3_TB),  # gemm_lnw takes the wide row
    (192, 768, FP32, 0, (683, 16, 16, 16), EPI, STAGED),
    (192, 768, BF16, 0, (8, 16, 16, 16), EPI, STAGED),
    (192, 768, FP32, 1, (2, 16, 16, 16), EPI, STAGED),
    (384, 1536, FP32, 0, (8, 8, 8, 8), PASS, STAGED),
    (384, 1536, FP32, 1, (8, 8, 8, 8), PASS, STAGED),
    (384, 1536, BF16, 0, (8, 8, 8, 8), EPI, STAGED),
    (48, 96, FP32, 0, (1, 4, 4, 4), EPI, STAGED),          # not 4C
    (8, 40, FP32, 0, (1, 4, 4, 4), EPI, STAGED_DWLN),      # hidden % 32 != 0
]
ROWS = [pytest.param(*r, id=f"row{i + 1}") for i, r in enumerate(TABLE)]


def _plan(C, hidden, prec, train, shape, offsets=None):
    B, D, H, W = shape
    return _lib.query("wf_ccf_ffn_plan", B, C, hidden, D, H, W, prec, train, offsets)


def _check(row, front, back):
    C, hidden, precs, train, shape = row[:5]
    for prec in precs:
        got = _plan(C, hidden, prec, train, shape)
        assert (got & 255, got >> 8) == (front, back), (prec, got)


def test_symbol_exported():
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wf_ccf_ffn_plan")
    assert "wf_ccf_ffn_plan" in _lib.SIGNATURES


@pytest.mark.parametrize("C,hidden,precs,train,shape,front,back", ROWS)
def test_dispatch_table(C, hidden, precs, train, shape, front, back, monkeypatch):
    monkeypatch.delenv("WF_FFN_FUSED", raising=False)
    monkeypatch.delenv("WF_FFN_NO_DWFC", raising=False)
    _check((C, hidden, precs, train, shape), front, back)


@pytest.mark.parametrize("C,hidden,precs,train,shape,front,back", ROWS)
def test_no_dwfc_switch(C, hidden, precs, train, shape, front, back, monkeypatch):
    """WF_FFN_NO_DWFC=1 (read per call): every fused back half becomes the staged path, the
    fronts stay."""
    monkeypatch.delenv("WF_FFN_FUSED", raising=False)
    monkeypatch.setenv("WF_FFN_NO_DWFC", "1")
    _check((C, hidden, precs, train, shape), front, STAGED if back <= DWFC3_TB else back)


@pytest.mark.parametrize("C,hidden,precs,train,shape,front,back", ROWS)
def test_whole_ffn_switch(C, hidden, precs, train, shape, front, back, monkeypatch):
    """WF_FFN_FUSED=1 (read per call): the stage-1 shape at inference takes the whole-FFN
    kernel and launches no front; training and the other widths are unchanged."""
    monkeypatch.delenv("WF_FFN_NO_DWFC", raising=False)
    monkeypatch.setenv("WF_FFN_FUSED", "1")
    if (C, hidden, train) == (48, 192, 0):
        front, back = NONE, FUSED
    _check((C, hidden, precs, train, shape), front, back)


def test_errors():
    lib = _lib.load()
    for prec in FP32:  # training keeps h2 before LN2: needs the 32-channel partials
        assert _plan(8, 40, prec, 1, (1, 4, 4, 4)) < 0
        assert b"training needs hidden % 32 == 0" in lib.wf_last_error()
    assert _plan(48, 192, 7, 0, (1, 4, 4, 4)) < 0
    assert b"unknown precision" in lib.wf_last_error()
    assert _plan(44, 192, 1, 0, (1, 4, 4, 4)) < 0
    assert b"multiples of 8" in lib.wf_last_error()
    for shape in [(0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)]:
        assert _plan(48, 192, 1, 0, shape) < 0
        assert b"empty volume" in lib.wf_last_error()


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("C,hidden", [(48, 192), (96, 384), (192, 768), (384, 1536)])
def test_workspace_layout(C, hidden, prec):
    shape = (2, 3, 5, 7)
    M, e = 2 * 3 * 5 * 7, 2 if prec == 0 else 4
    off = (ctypes.c_int64 * 7)(*([-7] * 7))
    assert _plan(C, hidden, prec, 0, shape, off) >= 0
    h1, h2, ln2_pst, ln1_pst, ln1_st, fcs, total = list(off)
    assert total == _lib.query("wf_ccf_ffn_workspace_bytes", 2, C, hidden, 3, 5, 7, prec)
    assert h1 == 0
    assert h2 == (M * hidden * e + 255) // 256 * 256
    assert h2 < ln2_pst < ln1_pst < ln1_st < total
    assert all(o % 256 == 0 for o in (h2, ln2_pst, ln1_pst, ln1_st))
    if (C, hidden) == (192, 768) and prec != 0:  # the stage-3 fc stream area: the last one
        assert ln1_st < fcs < total and fcs % 256 == 0
        assert fcs + 2 * 192 * 768 * 2 == total
    else:
        assert fcs == -1
