"""CPU: what a window attention call launches, asked of the library without a launch
(wf_window_attention_plan, csrc/attn_plan.hpp): the core, where q / k / v come from, how the
levels are grouped into launch sets, the form of each table-core launch, the workspace layout.
The expected values were derived by reading the dispatch code as it stood before the plan had a
name; the tests assert them, not whatever the library answers.  Host only."""
import ctypes

import pytest

from tests import attention_cases as A
from waveformer_amd import _lib

L3 = [(32, 32, 32), (16, 16, 16), (8, 8, 8)]
L2 = [(16, 16, 16), (8, 8, 8)]
ONE = [(8, 8, 8)]
LEVELS, RASTER = A.PLAN_TABLE, A.PLAN_TABLE | A.PLAN_RASTER

# The encoder's four attention calls at a 64^3 stage-1 raster: the LL levels of stages 1 and 2
# as a list, stage 3's one level and stage 4's level-0 Block (norm1 in the qkv loader) as a raster.
# (C, levels, flags) -> per B: grouping, per set (fused, wh, qsplit, pair_windows), NQ per level.
# wh = windows x heads; 4 / 2 / 1 workgroups per pair below 256 / below 512 / from 512 on; a
# level may take the pair loop (NQ 2) when its own windows x heads reach 256.
STAGES = [
    # stage 1, B = 8: 8 x (64 + 8 + 1) = 584 windows x 3 = 1752: fused; the 32^3 level's 512
    # windows x 3 reach 256, the 16^3 level's 64 x 3 = 192 do not
    (8, 48, L3, LEVELS, A.MERGED, [(1, 1752, 1, 512)], [2, 1, 1]),
    (1, 48, L3, LEVELS, A.MERGED, [(0, 219, 4, 0)], [1, 1, 1]),       # 73 x 3: gemm_rows<9>
    # stage 2: 8 x 9 x 6 = 432 pairs, level 1 alone 384; C = 96 is never fused by the rule
    (8, 96, L2, LEVELS, A.MERGED, [(0, 432, 2, 64)], [2, 1]),          # gemm_kc
    (1, 96, L2, LEVELS, A.MERGED, [(0, 54, 4, 0)], [1, 1]),
    (8, 192, ONE, RASTER, A.ONE_RASTER, [(0, 96, 4, 8)], [1]),         # stage 3: 8 x 12
    (1, 192, ONE, RASTER, A.ONE_RASTER, [(0, 12, 4, 1)], [1]),
    (8, 384, ONE, RASTER | A.PLAN_LN, A.ONE_RASTER, [(0, 192, 4, 8)], [1]),   # stage 4: 8 x 24
    (1, 384, ONE, RASTER | A.PLAN_LN, A.ONE_RASTER, [(0, 24, 4, 1)], [1]),
    (1, 48, ONE, LEVELS, A.MERGED, [(0, 3, 4, 0)], [1]),               # one level 8^3
    # no multi-level GEMM instantiation at C = 192: a launch set per level, 9 windows x 12 heads
    (1, 192, L2, LEVELS, A.NO_LEVELS_GEMM, [(0, 96, 4, 8), (0, 12, 4, 1)], [1, 1]),
    # B = 11, C = 48: the 8^3 level first has 11 x 3 = 33 pairs (one-sub-tile loop), the 16^3 level
    # after it 88 x 3 = 264 >= 256 (pair loop, and fused by the rule): not a prefix
    (11, 48, [(8, 8, 8), (16, 16, 16)], LEVELS, A.PREFIX, [(0, 33, 4, 11), (1, 264, 2, 88)], [1, 2]),
    # the same levels the other way round are one: 264 + 33 = 297 pairs
    (11, 48, [(16, 16, 16), (8, 8, 8)], LEVELS, A.MERGED, [(1, 297, 2, 88)], [2, 1]),
]


def test_symbol_exported():
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wf_window_attention_plan")
    assert "wf_window_attention_plan" in _lib.SIGNATURES


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("B,C,levels,flags,grouping,sets,nq", STAGES)
def test_plan(B, C, levels, flags, grouping, sets, nq, prec):
    p = A.window_attention_plan(levels, B, C, prec=prec, flags=flags)
    assert (p["table"], p["head_dim"], p["grouping"]) == (1, 16, grouping)
    got = [(s["fused"], s["wh"], s["qsplit"], s["pair_windows"]) for s in p["sets"]]
    assert got == sets and p["nq"] == nq
    assert [s["grid"] for s in p["sets"]] == [wh * q for _, wh, q, _ in sets]
    # the layout: qkv then the core's output, 256-B aligned, not overlapping, and the total is
    # what both size queries say
    rows, e = B * sum(d * h * w for d, h, w in levels), 2 if prec == 0 else 4
    assert p["qkv"] == 0 and p["ao"] % 256 == 0 and p["bytes"] % 256 == 0
    assert p["ao"] >= rows * 3 * C * e and p["bytes"] >= p["ao"] + rows * C * e
    dhw = (ctypes.c_int64 * (3 * len(levels)))(*[v for l in levels for v in l])
    if C % 16 == 0 and not flags & A.PLAN_RASTER:
        assert p["bytes"] == _lib.query("wf_window_attention_levels_workspace_bytes", dhw,
                                        len(levels), B, C, prec)
    assert p["bytes"] == sum(_lib.query("wf_window_attention_workspace_bytes", B, C, d, h, w, prec)
                             for d, h, w in levels)


def test_dense_core_and_errors():
    """The dense-bias core (training: LayerNorm and log-sum-exp) at window 4, head_dim 32."""
    p = A.window_attention_plan([(8, 4, 12)], 2, 64, heads=2, ws=4,
                                flags=A.PLAN_RASTER | A.PLAN_LN | A.PLAN_LSE)
    assert (p["table"], p["head_dim"], p["grouping"], p["nq"]) == (0, 32, A.ONE_RASTER, [0])
    # 2 x 6 windows x 2 heads, one workgroup per 64 queries of a pair
    assert p["sets"] == [{"fused": 0, "wh": 24, "qsplit": 0, "pair_windows": 0, "grid": 24}]
    for kw, text in ((dict(flags=A.PLAN_TABLE | A.PLAN_LN), "level list"),
                     (dict(flags=RASTER | A.PLAN_LSE), "inference only"),
                     (dict(flags=RASTER, ws=4), "window 8 and head_dim 16"),
                     (dict(flags=RASTER | A.PLAN_LN, qkv_mode=1), "needs the table bias"),
                     (dict(flags=32), "flags")):
        with pytest.raises(RuntimeError, match=text):
            A.window_attention_plan(ONE, 1, 48, **kw)
