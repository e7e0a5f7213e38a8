"""GPU: the table-bias attention core computing q / k / v itself from x and the qkv weight
(attn_tbl_kernel_fused, qkv_mode 1) is bitwise the staged path (qkv GEMM launch + core, qkv_mode
0): the fused prologue and sub-tile Q form every value with the GEMM's own MFMA sequence and
round it as the staged store + load pair does, so the comparison is torch.equal -- no tolerance.
The cases reach every query split (4, 2, 1), both tile loops and their boundary inside a merged
launch, both instantiated widths (two and three k steps, the padded K = 48 tail), a row gather
over a non-cubic raster, a second level at a row offset and level sources that are views."""
import pytest
import torch

from oracle.weight_rule import seeded_randn

pytestmark = pytest.mark.gpu

PRECS = ["bf16x3", "bf16", "fp16"]
CASES = {
    # qsplit 4; one-sub-tile loop; K = 48 padded to two k steps
    "small48": (1, 48, 3, [(16, 16, 16)]),
    # three k steps (the gemm_kc width); second level at a row offset
    "two96": (1, 96, 6, [(16, 16, 16), (8, 8, 8)]),
    # qsplit 2; the query-pair loop on the finest level and the single loop on the coarse ones in
    # one launch; inputs x 8: the running max is raised by later key tiles (rescales)
    "mixed": (2, 48, 3, [(32, 32, 32), (16, 16, 16), (8, 8, 8)]),
    # Bw * heads = 576: qsplit 1
    "q1": (3, 48, 3, [(32, 32, 32)]),
    # the row gather
    "noncubic": (2, 48, 3, [(16, 8, 24), (8, 8, 8)]),
}
INPUT_SCALE = {"mixed": 8.0}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()


def _weights(C, heads, seed):
    g = lambda shape, s, scale: (seeded_randn(shape, seed + s) * scale).cuda()
    return dict(wqkv=g((3 * C, C), 1, 0.1), bqkv=g((3 * C,), 2, 0.1), table=g((15 ** 3, heads), 3, 0.5),
                wproj=g((C, C), 4, 0.1), bproj=g((C,), 5, 0.1))


def _attend(xs, w, heads, prec, mode):
    from waveformer_amd import ops
    out = ops.window_attention(xs[0], w["wqkv"], w["bqkv"], w["table"], w["wproj"], w["bproj"], 8,
                               heads, 16 ** -0.5, prec=ops.PRECISIONS[prec], more=tuple(xs[1:]),
                               qkv_mode=mode)
    return out if isinstance(out, tuple) else (out,)


def _inputs(case):
    B, C, heads, levels = CASES[case]
    xs = [seeded_randn((B, *dhw, C), 10 + i).cuda() * INPUT_SCALE.get(case, 1.0)
          for i, dhw in enumerate(levels)]
    return xs, _weights(C, heads, 100), heads


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_equals_staged(case, prec):
    _gpu()
    xs, w, heads = _inputs(case)
    staged = _attend(xs, w, heads, prec, 0)
    fused = _attend(xs, w, heads, prec, 1)
    assert len(fused) == len(staged) == len(xs)
    for f, s, x in zip(fused, staged, xs):
        assert f.shape == x.shape and torch.isfinite(s).all()
        assert torch.equal(f, s)


@pytest.mark.parametrize("prec", PRECS)
def test_fused_equals_staged_on_band_buffer_views(prec):
    """two96's shapes, the levels taken as band 0 / band 3 of (8, B, D, H, W, C) band buffers:
    sources at non-zero offsets of their allocations."""
    _gpu()
    B, C, heads, levels = CASES["two96"]
    w = _weights(C, heads, 200)
    bands = [seeded_randn((8, B, *dhw, C), 20 + i).cuda() for i, dhw in enumerate(levels)]
    xs = [bands[0].unbind(0)[0], bands[1].unbind(0)[3]]
    staged = _attend(xs, w, heads, prec, 0)
    fused = _attend(xs, w, heads, prec, 1)
    for f, s in zip(fused, staged):
        assert torch.isfinite(s).all()
        assert torch.equal(f, s)


def test_rule_equals_fused_on_mixed():
    """mixed has 2 * 73 * 3 = 438 (window, head) pairs: the rule (mode -1) fuses it."""
    _gpu()
    xs, w, heads = _inputs("mixed")
    for f, r in zip(_attend(xs, w, heads, "bf16x3", 1), _attend(xs, w, heads, "bf16x3", -1)):
        assert torch.equal(f, r)


def test_fused_at_an_uninstantiated_width_is_an_error():
    _gpu()
    C, heads = 192, 12
    xs = [seeded_randn((1, 8, 8, 8, C), 31).cuda()]
    with pytest.raises(RuntimeError, match="C = 48 and 96"):
        _attend(xs, _weights(C, heads, 300), heads, "bf16x3", 1)
