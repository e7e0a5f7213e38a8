"""GPU: window attention over all LL levels of a Block in one launch set
(ops.window_attention(x0, ..., more=...), wf_window_attention_fwd_levels) is bitwise the
per-level calls: a GEMM row does not depend on the rows it shares a launch with, and the merged
core launch runs each level on the loop its own launch takes.  The cases are the two widths the
multi-level GEMM loader is instantiated for (C = 48: gemm_rows, C = 96: gemm_kc), a non-cubic
raster (a swapped axis or a wrong level boundary), levels whose own launches take different
core loops, level sources that are views into larger band buffers (an assumed common
allocation), and a level-2 Block against the same Block assembled by hand from the per-level
op."""
from functools import partial

import pytest
import torch
import torch.nn as nn

from oracle.weight_rule import rule_state_dict, seeded_randn

pytestmark = pytest.mark.gpu

PRECS = ["bf16x3", "fp16"]
CASES = {
    "three_cubic": (1, 48, 3, [(32, 32, 32), (16, 16, 16), (8, 8, 8)]),
    "two_cubic": (2, 96, 6, [(16, 16, 16), (8, 8, 8)]),
    "non_cubic": (2, 48, 3, [(16, 8, 24), (8, 8, 8)]),
    # the finest level alone launches the core's query-pair loop (128 windows x 3 heads >= 256),
    # the coarser ones its one-sub-tile loop; the two loops round differently once a later key
    # tile raises a row's running max by more than 2^16, which inputs of this size do all the time
    "mixed_loops": (2, 48, 3, [(32, 32, 32), (16, 16, 16), (8, 8, 8)]),
}
INPUT_SCALE = {"mixed_loops": 8.0}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()


def _weights(C, heads, seed):
    g = lambda shape, s, scale: (seeded_randn(shape, seed + s) * scale).cuda()
    return dict(wqkv=g((3 * C, C), 1, 0.1), bqkv=g((3 * C,), 2, 0.1), table=g((15 ** 3, heads), 3, 0.5),
                wproj=g((C, C), 4, 0.1), bproj=g((C,), 5, 0.1))


def _attend(xs, w, heads, prec):
    """(merged outputs, per-level outputs) of the levels xs."""
    from waveformer_amd import ops
    scale = 16 ** -0.5
    a = (w["wqkv"], w["bqkv"], w["table"], w["wproj"], w["bproj"], 8, heads, scale)
    merged = ops.window_attention(xs[0], *a, prec=prec, more=tuple(xs[1:]))
    single = [ops.window_attention(x, *a, prec=prec) for x in xs]
    return merged, single


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_levels_equal_per_level_calls(case, prec):
    _gpu()
    from waveformer_amd import ops
    B, C, heads, levels = CASES[case]
    w = _weights(C, heads, 100)
    xs = [seeded_randn((B, *dhw, C), 10 + i).cuda() * INPUT_SCALE.get(case, 1.0)
          for i, dhw in enumerate(levels)]
    merged, single = _attend(xs, w, heads, ops.PRECISIONS[prec])
    assert isinstance(merged, tuple) and len(merged) == len(xs)
    for m, s, x in zip(merged, single, xs):
        assert m.shape == x.shape and torch.isfinite(s).all()
        assert torch.equal(m, s)


@pytest.mark.parametrize("prec", PRECS)
def test_levels_from_band_buffer_views(prec):
    """The level sources as the model passes them: band 0 of each level's (8, B, D, H, W, C)
    band buffer -- allocations of their own, one here at a non-zero offset of its buffer."""
    _gpu()
    from waveformer_amd import ops
    B, C, heads, levels = CASES["two_cubic"]
    w = _weights(C, heads, 200)
    bands = [seeded_randn((8, B, *dhw, C), 20 + i).cuda() for i, dhw in enumerate(levels)]
    xs = [bands[0].unbind(0)[0], bands[1].unbind(0)[3]]
    merged, _ = _attend(xs, w, heads, ops.PRECISIONS[prec])
    _, single = _attend([x.clone() for x in xs], w, heads, ops.PRECISIONS[prec])
    for m, s in zip(merged, single):
        assert torch.equal(m, s)


# case -> B, C, levels, and what wf_window_attention_plan must say: the grouping and each launch
# set's q/k/v source.  The smallest shapes that reach each grouping and source: C = 48 merges
# (gemm_rows<9>), C = 192 has no multi-level GEMM, 11 x 8 windows x 3 heads = 264 pairs are fused.
PLAN_CASES = {
    "merged_staged": (1, 48, [(16, 16, 16), (8, 8, 8)], "MERGED", [0]),
    "per_level": (1, 192, [(16, 16, 16), (8, 8, 8)], "NO_LEVELS_GEMM", [0, 0]),
    "fused": (11, 48, [(16, 16, 16)], "MERGED", [1]),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_workspace_use_is_what_the_plan_says(case):
    """The workspace claims of the plan: a call stays within the plan's `bytes` (per-level launch
    sets re-use the one workspace), and a fused launch set does not write the qkv area.  The
    workspace has ops.GUARD_BYTES of guard behind it and its qkv area is pre-filled."""
    _gpu()
    import ctypes
    from tests import attention_cases as A
    from waveformer_amd import _lib, ops
    B, C, levels, grouping, fused = PLAN_CASES[case]
    heads, prec, scale = C // 16, ops.PRECISIONS["bf16x3"], 16 ** -0.5
    plan = A.window_attention_plan(levels, B, C, prec=prec)
    assert plan["grouping"] == getattr(A, grouping)
    assert [s["fused"] for s in plan["sets"]] == fused
    w = _weights(C, heads, 400)
    xs = [seeded_randn((B, *dhw, C), 50 + i).cuda() for i, dhw in enumerate(levels)]
    work = ops._workspace(plan["bytes"], "cuda", case, guard=True)
    work[:plan["ao"]] = 0x5A
    out = torch.empty((sum(x.numel() // C for x in xs), C), device="cuda")
    wq, wp = ops.split_weight(w["wqkv"], prec=prec), ops.split_weight(w["wproj"], prec=prec)
    _lib.call("wf_window_attention_fwd_levels_mode",
              (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs]),
              (ctypes.c_int64 * (3 * len(xs)))(*[v for dhw in levels for v in dhw]), len(xs),
              wq.data_ptr(), w["bqkv"].data_ptr(), w["table"].data_ptr(), wp.data_ptr(),
              w["bproj"].data_ptr(), out.data_ptr(), work.data_ptr(), B, C, heads, scale, prec,
              ops._stream(), -1)
    assert ops.check_guard(work, plan["bytes"])
    if fused == [1]:
        assert bool((work[:plan["ao"]] == 0x5A).all())
    a = (w["wqkv"], w["bqkv"], w["table"], w["wproj"], w["bproj"], 8, heads, scale)
    single = [ops.window_attention(x, *a, prec=prec).reshape(-1, C) for x in xs]
    assert torch.isfinite(out).all() and torch.equal(out, torch.cat(single))


def test_levels_op_schema_and_fake():
    """waveformer::window_attn_levels: schema and fake-tensor checks (inference only: the op
    registers no autograd), and its one buffer holds the levels' outputs in order."""
    _gpu()
    from waveformer_amd import library, ops
    B, C, heads, levels = CASES["two_cubic"]
    w = _weights(C, heads, 300)
    xs = [seeded_randn((B, *dhw, C), 30 + i).cuda() for i, dhw in enumerate(levels)]
    args = [xs, w["wqkv"], w["bqkv"], w["table"], w["wproj"], w["bproj"], heads, 16 ** -0.5,
            library.SPLIT]
    op = torch.ops.waveformer.window_attn_levels.default
    torch.library.opcheck(op, args, test_utils=["test_schema", "test_faketensor"])
    out = op(*args)
    assert tuple(out.shape) == (sum(x.numel() // C for x in xs), C)
    _, single = _attend(xs, w, heads, library.SPLIT)
    assert torch.equal(out, torch.cat([s.reshape(-1, C) for s in single]))


def test_block_level2_equals_hand_assembly():
    """A level-2 Block (its two attention calls merged under no_grad) against the same Block
    put together from the dwt3d, per-level window_attn, msfuse and ccf_ffn ops."""
    _gpu()
    import waveformer_amd.network_models as NM
    from waveformer_amd.network_models.wave_helper import ffn_op
    blk = NM.Block(96, 6, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), level=2,
                   ms_attention=True, img_size=(32,) * 3)
    blk.load_state_dict(rule_state_dict(blk.state_dict()), strict=True)
    blk = blk.cuda().eval()
    assert blk.attn.window_size == 8 and blk.attn.head_dim == 16
    x = seeded_randn((1, 32, 32, 32, 96), 41).cuda()
    O = torch.ops.waveformer
    with torch.no_grad():
        got, hfs = blk(x)
        srcs, cur = [], x
        for i in range(2):
            b = O.dwt3d(cur, blk.norm1.weight if i == 0 else None,
                        blk.norm1.bias if i == 0 else None,
                        float(blk.norm1.eps) if i == 0 else 0.0).unbind(0)
            cur = b[0]
            srcs.append(blk.attn.forward_raster(cur))
        xh, stats = O.msfuse(srcs, x, None, float(blk.norm2.eps), True)
        want = ffn_op(xh, stats, blk.norm2, blk.mlp, None)
    assert len(hfs) == 2
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
