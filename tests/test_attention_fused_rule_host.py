"""CPU: the rule that lets the table-bias attention core compute q / k / v itself instead of
reading a staged qkv tensor (the q/k/v-source field of wf_window_attention_plan, attn_plan.hpp
attn_qkv_fused): C = 48 and at least 256 (window, head) pairs in the launch.  C = 96 has a fused
instantiation (qkv_mode 1) but the rule leaves it staged: its B = 8 launch measured slower fused
than the GEMM and the core together.  Host only, no GPU."""
import ctypes

import pytest

from tests.attention_cases import window_attention_plan
from waveformer_amd import _lib

FAKE = 256  # never dereferenced: validation fails first

L3 = [(32, 32, 32), (16, 16, 16), (8, 8, 8)]
L2 = [(16, 16, 16), (8, 8, 8)]


def _dhw(levels):
    flat = [v for l in levels for v in l]
    return (ctypes.c_int64 * max(1, len(flat)))(*flat)


def _fused(B, C, levels, prec=1):
    """The one q/k/v source of the call's launch sets: 1 computed in the core, 0 staged."""
    (src,) = {s["fused"] for s in window_attention_plan(levels, B, C, prec=prec)["sets"]}
    return src


def test_symbols_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wf_window_attention_fwd_levels_mode", "wf_window_attention_plan"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert not hasattr(lib, "wf_window_attention_levels_fused")


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_rule(prec):
    assert _fused(8, 48, L3, prec) == 1   # 584 windows x 3 heads
    # 72 windows x 6 heads = 432 pairs, but the width stays staged: fused 123 us against 101 us
    # for GEMM + core per B = 8 stage-2 launch, so the rule does not take it
    assert _fused(8, 96, L2, prec) == 0
    assert _fused(1, 48, L3, prec) == 0   # 73 x 3 = 219 (window, head) pairs: below 256
    assert _fused(8, 192, [(8, 8, 8)], prec) == 0  # no fused instantiation at this width


def test_rule_threshold_and_bad_lists():
    # 86 windows x 3 = 258 >= 256 > 85 x 3
    assert _fused(86, 48, [(8, 8, 8)]) == 1
    assert _fused(85, 48, [(8, 8, 8)]) == 0
    with pytest.raises(RuntimeError, match="8\\^3 windows"):
        _fused(8, 48, [(12, 12, 12)])
    with pytest.raises(RuntimeError, match="unknown precision"):
        _fused(8, 48, L3, prec=7)


def test_mode_is_validated_on_the_host():
    lib = _lib.load()
    ptrs = (ctypes.c_void_p * 1)(FAKE)

    def fwd(C, mode):
        rc = lib.wf_window_attention_fwd_levels_mode(ptrs, _dhw([(8, 8, 8)]), 1, FAKE, FAKE, FAKE,
                                                     FAKE, FAKE, FAKE, FAKE, 8, C, C // 16, 0.25, 1,
                                                     None, mode)
        return rc, lib.wf_last_error().decode()

    rc, msg = fwd(192, 1)
    assert rc < 0 and "C = 48 and 96" in msg
    rc, msg = fwd(48, 2)
    assert rc < 0 and "qkv_mode" in msg
    for C, mode, text in ((192, 1, "C = 48 and 96"), (48, 2, "qkv_mode")):   # the query agrees
        with pytest.raises(RuntimeError, match=text):
            window_attention_plan([(8, 8, 8)], 8, C, qkv_mode=mode)
