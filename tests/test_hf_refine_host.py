"""No GPU: the host side of the HF-refinement training path -- wf_hf_refine_bwd's argument
checks (each a message from the library, raised before any HIP call: this runs without a
device), the workspace query, the fake kernels of waveformer::hf_refine /
hf_refine_backward on the meta device, and HFRefinementRes on CPU tensors.
"""
import ctypes

import pytest
import torch

from waveformer_amd import _lib

FAKE = 0x1000  # a non-null address; the checks under test fail before anything reads it


def _call(C=8, B=1, D=2, H=2, W=2, ldb=None, null=None):
    """wf_hf_refine_bwd with non-null fake pointers (argument `null` passed as NULL)."""
    ldb = D * H * W * C if ldb is None else ldb
    dets = (ctypes.c_void_p * 7)(*[FAKE] * 7)
    if null == "details[3]":
        dets[3] = None
    names = ["details", "dw_w", "dw_b", "in_w", "in_b", "pw_w", "pw_b", "moments", "gy", "gx",
             "g_dw_w", "g_dw_b", "g_in_w", "g_in_b", "g_pw_w", "g_pw_b", "workspace"]
    p = {n: (None if n == null else FAKE) for n in names}
    p["details"] = None if null == "details" else dets
    _lib.call("wf_hf_refine_bwd", p["details"], ldb, p["dw_w"], p["dw_b"], p["in_w"], p["in_b"],
              1e-5, p["pw_w"], p["pw_b"], 1, p["moments"], p["gy"], p["gx"], p["g_dw_w"],
              p["g_dw_b"], p["g_in_w"], p["g_in_b"], p["g_pw_w"], p["g_pw_b"], p["workspace"],
              B, C, D, H, W, None)


@pytest.mark.parametrize("C", [6, 260, 0])
def test_bwd_rejects_unsupported_channels(C):
    with pytest.raises(RuntimeError, match=r"wf_hf_refine_bwd: C must be a multiple of 4 in \[4, 256\]"):
        _call(C=C)


def test_bwd_rejects_empty_and_short_batch_stride():
    with pytest.raises(RuntimeError, match="wf_hf_refine_bwd: empty tensor"):
        _call(D=0)
    with pytest.raises(RuntimeError, match="wf_hf_refine_bwd: batch stride smaller than one"):
        _call(C=8, D=2, H=3, W=4, ldb=2 * 3 * 4 * 8 - 1)


@pytest.mark.parametrize("null", ["details", "details[3]", "dw_w", "in_b", "pw_w", "moments",
                                  "gy", "gx", "g_dw_b", "g_pw_w", "workspace"])
def test_bwd_rejects_null_pointers(null):
    with pytest.raises(RuntimeError, match=r"wf_hf_refine_bwd: .* is NULL"):
        _call(null=null)


def test_bwd_workspace_query():
    q = lambda *a: _lib.query("wf_hf_refine_bwd_workspace_bytes", *a)  # noqa: E731
    base = q(1, 48, 8, 8, 8)
    assert base > 0 and base % 256 == 0
    # at least the four stored tensors (uh, ga / gu, h, gv)
    assert base >= 4 * 7 * 8 * 8 * 8 * 48 * 4
    prev = 0
    for B in range(1, 6):
        cur = q(B, 48, 8, 8, 8)
        assert cur > prev
        prev = cur
    prev = 0
    for S in [(1, 1, 1), (2, 3, 1), (3, 3, 3), (8, 8, 8), (9, 8, 8), (16, 16, 16), (32, 32, 32)]:
        cur = q(2, 192, *S)
        assert cur > prev, S
        prev = cur
    for bad in [(1, 6, 4, 4, 4), (1, 260, 4, 4, 4), (0, 8, 4, 4, 4), (1, 8, 0, 4, 4)]:
        assert q(*bad) == 0


def test_fake_kernels_give_shapes_on_meta():
    import waveformer_amd.library  # noqa: F401
    B, C, D, H, W = 2, 8, 3, 4, 5
    with torch.device("meta"):
        dets = [torch.empty(B, D, H, W, C).permute(0, 4, 1, 2, 3) for _ in range(7)]
        prm = [torch.empty(C, 1, 3, 3, 3), torch.empty(C), torch.empty(C), torch.empty(C),
               torch.empty(C, C, 1, 1, 1), torch.empty(C)]
        out, mom = torch.ops.waveformer.hf_refine(dets, *prm[:4], 1e-5, *prm[4:], True)
        assert out.device.type == "meta" and tuple(out.shape) == (7, B, D, H, W, C)
        assert out.dtype == torch.float32
        assert tuple(mom.shape) == (7, B, C, 2) and mom.dtype == torch.float64
        g = torch.ops.waveformer.hf_refine_backward(out, dets, *prm[:4], 1e-5, *prm[4:], True, mom)
    assert tuple(g[0].shape) == (7, B, D, H, W, C)
    assert [tuple(t.shape) for t in g[1:]] == [tuple(p.shape) for p in prm]


def test_cpu_tensors_fail_loudly_through_the_op():
    import waveformer_amd.library  # noqa: F401
    C = 4
    dets = [torch.zeros(1, C, 2, 2, 2) for _ in range(7)]
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.waveformer.hf_refine(dets, torch.zeros(C, 1, 3, 3, 3), torch.zeros(C),
                                       torch.ones(C), torch.zeros(C), 1e-5,
                                       torch.zeros(C, C, 1, 1, 1), torch.zeros(C), True)


def test_module_cpu_path_unchanged():
    import waveformer_amd.network_models as NM
    torch.manual_seed(0)
    m = NM.HFRefinementRes(8)
    x = torch.randn(1, 8, 3, 4, 5, requires_grad=True)
    assert not m.train_ok(x) and not m.fast_ok(x)
    with torch.no_grad():
        assert not m.train_ok(x.detach()) and not m.fast_ok(x.detach())
    m(x).sum().backward()
    assert bool(torch.isfinite(x.grad).all())
    for p in m.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
