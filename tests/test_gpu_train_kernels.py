"""GPU: the encoder's backward kernels (csrc/train.hip) one entry point at a time.

The module tests (test_train_grads, test_gpu_droppath, test_gpu_grad128) reach these kernels
only at head dim 16, cubic rasters and model widths, mostly through three-number summaries.
Here every C-ABI entry point of the encoder's training path is called on its own, at the
smallest shapes that reach each of its branches, and compared with a plain fp64 reference on
the CPU (torch autograd where the operation has one).

Inputs are oracle.weight_rule.seeded_randn, errors tests.cases.rel_l2 against the fp64
reference, one printed line per test.  Output buffers and workspaces are filled with NaN before
each call: the header promises "every element written", so results must be finite everywhere.

Bars (the project's existing ones):
  1e-6  pure gather / butterfly kernels (test_gpu_wavelet_grad, test_upsample_cl_autograd_adjoint)
  1e-5  kernels with fp32 reductions or exp2f (the fp32-faithful bar); the attention core's
        formulas evaluated in fp32 on the CPU sit 2.2e-7 .. 7.2e-7 from fp64 (randn inputs,
        bias amplitude 1 and 4, N = 8, 27, 125, 512), a wrong kernel is O(1) off
  0     pure data movement (exact equality)
  5e-5 / 2e-4  op-level outputs / gradients whose forward runs bf16x3 MFMAs (test_train_grads)
"""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_waveformer as R
from oracle.weight_rule import seeded_randn
from tests import cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    yield


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _err(got, want):
    """rel-L2 of a GPU result against its fp64 reference; the result must be finite."""
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), "an output element was not written (NaN fill left)"
    return C.rel_l2(got, want)


# ------------------------------------------------------------------------------------------
# 1. wf_window_attention_bwd_core
# ------------------------------------------------------------------------------------------
def _a256(n):
    return (n + 255) // 256 * 256


# (ws, head dim, heads, B, raster, G).  G = the window groups of attn_bwd_groups (train.hip):
# nkb = cdiv(N, 64); G0 = min(cdiv(1024, nkb * heads), Bw); G = cdiv(Bw, cdiv(Bw, G0)).
#   ws 2, 24 heads, Bw = 48: G0 = min(43, 48) = 43, cdiv(48, 43) = 2, G = 24: every group
#     walks two windows (the `first ? ds : dbrow[key] + ds` accumulation)
#   ws 2, 24 heads, Bw = 45: G0 = 43, cdiv(45, 43) = 2, G = 23: group 22 walks one window,
#     the others two
# The test derives G back from the workspace size and fails if the grouping rule moved, so
# that these two rows get re-chosen rather than silently losing their branch.
ATTN_CORE = [
    (8, 16, 3, 1, (8, 8, 8), 1),      # base: 8 key blocks
    (8, 16, 3, 2, (8, 16, 24), 12),   # window grid 1 x 2 x 3, raster rows
    (4, 32, 2, 1, (4, 8, 4), 2),      # <32>, N = 64 exactly
    (2, 64, 1, 1, (2, 2, 2), 1),      # <64>, N = 8 < 64
    (3, 48, 2, 2, (3, 6, 9), 12),     # <48>, N = 27, non-cubic
    (5, 16, 2, 1, (5, 5, 10), 2),     # N = 125: second key and query block partial
    (2, 16, 24, 2, (8, 6, 4), 24),    # Bw = 48 > G = 24: two windows per group, C = 384
    (2, 16, 24, 1, (10, 6, 6), 23),   # Bw = 45, G = 23: groups of uneven length
]


def _attn_core_call(qkv, o, dout, bias, lse2, B, C_, raster, ws, heads, scale, G):
    from waveformer_amd import _lib
    D1, H1, W1 = raster
    N = ws ** 3
    rows = B * D1 * H1 * W1
    wsb = _lib.query("wf_window_attention_bwd_workspace_bytes", B, C_, D1, H1, W1, ws, heads)
    nkb = -(-N // 64)
    assert wsb == _a256(nkb * rows * C_ * 4) + _a256(G * heads * N * N * 4), \
        "attn_bwd_groups changed: re-derive G for the cases (see ATTN_CORE)"
    guard = 4096
    buf = torch.empty(wsb + guard, dtype=torch.uint8, device=DEV)
    buf[:wsb].view(torch.float32).fill_(NAN)
    buf[wsb:].fill_(0xA5)
    dqkv = _nan(rows, 3 * C_)
    dbias = _nan(heads, N, N)
    _lib.call("wf_window_attention_bwd_core", qkv.data_ptr(), o.data_ptr(), dout.data_ptr(),
              bias.data_ptr(), lse2.data_ptr(), dqkv.data_ptr(), dbias.data_ptr(),
              buf.data_ptr(), B, C_, D1, H1, W1, ws, heads, float(scale), _s())
    torch.cuda.synchronize()
    assert bool((buf[wsb:] == 0xA5).all()), "write past wf_window_attention_bwd_workspace_bytes"
    return dqkv, dbias


@pytest.mark.parametrize("ws,hd,heads,B,raster,G", ATTN_CORE)
def test_attention_bwd_core(ws, hd, heads, B, raster, G):
    D1, H1, W1 = raster
    C_ = hd * heads
    N = ws ** 3
    rows = B * D1 * H1 * W1
    Bw = rows // N
    scale = hd ** -0.5
    qkv = seeded_randn((rows, 3 * C_), 1)
    bias = seeded_randn((heads, N, N), 2)
    dout = seeded_randn((rows, C_), 3)

    q64 = qkv.double().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    t = q64.view(Bw, N, 3, heads, hd).permute(2, 0, 3, 1, 4)       # (3, Bw, heads, N, hd)
    S = scale * (t[0] @ t[1].transpose(-2, -1)) + b64
    o64 = (S.softmax(-1) @ t[2]).transpose(1, 2).reshape(rows, C_)
    lse2 = (torch.logsumexp(S, -1) / math.log(2.0)).detach()        # (Bw, heads, N)
    dq_win, db64 = torch.autograd.grad(o64, (q64, b64), dout.double())
    # window-major row wr is raster row win[wr] (the inverse of window_partition)
    win = R.window_partition(torch.arange(rows).view(B, D1, H1, W1, 1), ws).reshape(-1)
    want = torch.empty_like(dq_win)
    want[win] = dq_win

    args = (qkv.to(DEV), o64.detach().float().to(DEV), dout.to(DEV), bias.to(DEV),
            lse2.float().contiguous().to(DEV), B, C_, raster, ws, heads, scale, G)
    dqkv, dbias = _attn_core_call(*args)
    e_q, e_b = _err(dqkv, want), _err(dbias, db64)
    print(f"attn_bwd_core ws{ws} hd{hd} h{heads} B{B} {raster}: dqkv {e_q:.3e} dbias {e_b:.3e}")
    assert e_q <= 1e-5 and e_b <= 1e-5
    dqkv2, dbias2 = _attn_core_call(*args)
    assert torch.equal(dqkv, dqkv2) and torch.equal(dbias, dbias2), "not deterministic"


# ------------------------------------------------------------------------------------------
# 2. waveformer::window_attn, train=True, forward + backward at head dims other than 16
# ------------------------------------------------------------------------------------------
ATTN_OP = [(4, 32, 2, 1, (4, 8, 4), True), (2, 64, 1, 2, (2, 4, 6), False),
           (2, 48, 1, 1, (4, 2, 2), True), (8, 16, 3, 1, (8, 8, 16), True)]


@pytest.mark.parametrize("ws,hd,heads,B,raster,fused", ATTN_OP)
def test_window_attn_op_grads(ws, hd, heads, B, raster, fused):
    from waveformer_amd import library, ops  # noqa: F401  (registers the ops)
    D1, H1, W1 = raster
    C_ = hd * heads
    N = ws ** 3
    T = (2 * ws - 1) ** 3
    eps = 1e-6
    scale = hd ** -0.5
    p = {"x": seeded_randn((B, D1, H1, W1, C_), 10),
         "qkv.weight": seeded_randn((3 * C_, C_), 11) * C_ ** -0.5,
         "qkv.bias": seeded_randn((3 * C_,), 12) * 0.1,
         "relative_position_bias_table": seeded_randn((T, heads), 13) * 0.5,
         "proj.weight": seeded_randn((C_, C_), 14) * C_ ** -0.5,
         "proj.bias": seeded_randn((C_,), 15) * 0.1}
    if fused:
        p["norm1.weight"] = 1 + 0.1 * seeded_randn((C_,), 16)
        p["norm1.bias"] = 0.1 * seeded_randn((C_,), 17)
    g = seeded_randn((B, D1, H1, W1, C_), 18)
    index = R.relative_position_index(ws)

    sd = {k: v.double().requires_grad_(True) for k, v in p.items()}
    sd["relative_position_index"] = index
    xin = sd["x"]
    if fused:
        xin = F.layer_norm(xin, [C_], sd["norm1.weight"], sd["norm1.bias"], eps)
    win = R.window_partition(xin, ws).view(-1, N, C_)
    ref = R.attention(sd, "", win, heads, ws).reshape(B, D1, H1, W1, C_)   # Q1 plain reshape
    ref.backward(g.double())

    dv = {k: v.to(DEV).requires_grad_(True) for k, v in p.items()}
    out, _, _ = torch.ops.waveformer.window_attn(
        dv["x"], dv.get("norm1.weight"), dv.get("norm1.bias"), eps, dv["qkv.weight"],
        dv["qkv.bias"], dv["relative_position_bias_table"], index.to(DEV), dv["proj.weight"],
        dv["proj.bias"], ws, heads, scale, ops.PRECISIONS["bf16x3"], True, False)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    e_o = _err(out, ref)
    errs = {k: _err(dv[k].grad, sd[k].grad) for k in p}
    print(f"window_attn op ws{ws} hd{hd} h{heads} B{B} {raster} norm1={fused}: out {e_o:.3e} "
          + " ".join(f"d{k} {e:.3e}" for k, e in errs.items()))
    assert e_o <= 5e-5
    bad = {k: e for k, e in errs.items() if not e <= 2e-4}
    assert not bad, bad


# ------------------------------------------------------------------------------------------
# 3. wf_ln_act_fwd / wf_ln_act_bwd
# ------------------------------------------------------------------------------------------
def _ln_cases():
    out = []
    small = [(3, 48), (17, 100), (64, 192)]        # J = 1, 2, 3; one / two / four blocks
    for i, (M, N) in enumerate(small):
        for j, (gelu, affine, dadd) in enumerate(itertools.product((0, 1), (True, False),
                                                                   (False, True))):
            out.append((M, N, gelu, affine, dadd, 1e-6 if (i + j) % 2 else 1e-5))
    # J = 4, 8, 16 (no model width uses them), J = 24 full and ragged, the 1024-block cap of
    # the backward with its grid-stride row loop (M > 16 * 1024), many partial blocks
    for M, N in [(33, 250), (20, 500), (9, 1000), (5, 1536), (7, 1535), (5000, 96),
                 (20000, 48)]:
        out.append((M, N, 1, True, True, 1e-5))
        out.append((M, N, 0, False, False, 1e-6))
    return out


@pytest.mark.parametrize("M,N,gelu,affine,dadd,eps", _ln_cases())
def test_ln_act_fwd_bwd(M, N, gelu, affine, dadd, eps):
    from waveformer_amd import _lib
    x = seeded_randn((M, N), 20) * 1.5 + 0.3
    dy = seeded_randn((M, N), 21)
    w = (1 + 0.2 * seeded_randn((N,), 22)) if affine else None
    b = 0.2 * seeded_randn((N,), 23) if affine else None
    da = seeded_randn((M, N), 24) if dadd else None

    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True) if affine else None
    b64 = b.double().requires_grad_(True) if affine else None
    y64 = F.layer_norm(x64, [N], w64, b64, eps)
    if gelu:
        y64 = F.gelu(y64)
    y64.backward(dy.double())
    dx64 = x64.grad + (da.double() if dadd else 0)

    xg, dyg = x.to(DEV), dy.to(DEV)
    wg, bg = (w.to(DEV), b.to(DEV)) if affine else (None, None)
    dag = da.to(DEV) if dadd else None
    y = _nan(M, N)
    _lib.call("wf_ln_act_fwd", xg.data_ptr(), _p(wg), _p(bg), float(eps), int(gelu),
              y.data_ptr(), M, N, _s())
    dx = _nan(M, N)
    dw = db = part = None
    if affine:
        dw, db = _nan(N), _nan(N)
        part = _nan(_lib.query("wf_ln_bwd_workspace_floats", M, N))
    _lib.call("wf_ln_act_bwd", xg.data_ptr(), _p(wg), _p(bg), float(eps), int(gelu),
              dyg.data_ptr(), _p(dag), dx.data_ptr(), _p(part), _p(dw), _p(db), M, N, _s())
    torch.cuda.synchronize()
    errs = {"y": _err(y, y64), "dx": _err(dx, dx64)}
    if affine:
        errs["dw"] = _err(dw, w64.grad)
        errs["db"] = _err(db, b64.grad)
    print(f"ln_act ({M}, {N}) gelu={gelu} affine={affine} dadd={dadd} eps={eps:g}: "
          + " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if not e <= 1e-5}
    assert not bad, bad


# ------------------------------------------------------------------------------------------
# 4. wf_colsum
# ------------------------------------------------------------------------------------------
def _colsum(x, R_, N, scale=None, rps=0):
    from waveformer_amd import _lib
    part = _nan(max(1, _lib.query("wf_colsum_parts", R_)) * max(N, 1))
    out = _nan(N)
    _lib.call("wf_colsum", _p(x), R_, N, _p(scale), rps, part.data_ptr(), out.data_ptr(), _s())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("R_,N", [(0, 5), (1, 1), (255, 63), (257, 65), (1000, 1536),
                                  (300001, 4)])
def test_colsum(R_, N):
    from waveformer_amd import _lib
    x = seeded_randn((R_, N), 30)
    xg = x.to(DEV) if R_ else None
    out = _colsum(xg, R_, N)
    if R_ == 0:
        assert torch.equal(out.cpu(), torch.zeros(N))
        print(f"colsum ({R_}, {N}): zeros")
        return
    if R_ == 300001:
        assert _lib.query("wf_colsum_parts", R_) == 1024  # the cap on the partial count
    e = _err(out, x.double().sum(0))
    print(f"colsum ({R_}, {N}): {e:.3e}")
    assert e <= 1e-5
    assert torch.equal(out, _colsum(xg, R_, N)), "not deterministic"


def test_colsum_row_scale():
    R_, N, rps = 300, 7, 100
    x = seeded_randn((R_, N), 31)
    sc = torch.tensor([1.25, 0.0, 2.0])
    xg, sg = x.to(DEV), sc.to(DEV)
    out = _colsum(xg, R_, N, sg, rps)
    want = (x.double() * sc.double().repeat_interleave(rps)[:, None]).sum(0)
    e = _err(out, want)
    print(f"colsum row_scale ({R_}, {N}) / {rps}: {e:.3e}")
    assert e <= 1e-5
    assert torch.equal(out, _colsum(xg, R_, N, sg, rps)), "not deterministic"


# ------------------------------------------------------------------------------------------
# 5. wf_interp_adjoint_axis / wf_interp_adjoint_axis_ac
# ------------------------------------------------------------------------------------------
def _interp_matrix_t(Lin, Lout, ac):
    """A^T (Lin, Lout) of the fp64 linear interpolation Lin -> Lout: the identity's columns
    pushed through F.interpolate."""
    eye = torch.eye(Lin, dtype=torch.float64)[None]                 # (1, channel i, length)
    return F.interpolate(eye, size=Lout, mode="linear", align_corners=ac)[0]


def _interp_adjoint(Lin, Lout, ac):
    from waveformer_amd import _lib
    At = _interp_matrix_t(Lin, Lout, ac)
    worst = 0.0
    combos = [(outer, inner, False) for outer in (1, 6) for inner in (1, 5, 48)]
    if not ac:
        combos += [(6, inner, True) for inner in (1, 5, 48)]
    for outer, inner, scaled in combos:
        g = seeded_randn((outer, Lout, inner), 40 + inner)
        want = torch.einsum("ip,opn->oin", At, g.double())
        gg = g.to(DEV)
        out = _nan(outer, Lin, inner)
        if ac:
            _lib.call("wf_interp_adjoint_axis_ac", gg.data_ptr(), out.data_ptr(), outer, Lout,
                      Lin, inner, _s())
        else:
            scg = None
            if scaled:  # outer_per_scale = 3 on outer = 6, one factor 0 (a dropped sample)
                sc = torch.tensor([0.0, 4.0 / 3.0])
                want = want * sc.double().repeat_interleave(3)[:, None, None]
                scg = sc.to(DEV)
            _lib.call("wf_interp_adjoint_axis", gg.data_ptr(), out.data_ptr(), outer, Lout,
                      Lin, inner, _p(scg), 3 if scaled else 0, _s())
        torch.cuda.synchronize()
        e = _err(out, want)
        assert e <= 1e-6, (Lin, Lout, outer, inner, scaled, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("Lin,Lout", [(2, 4), (4, 8), (4, 16), (2, 16), (3, 7), (1, 5), (5, 5),
                                      (8, 4)])
def test_interp_adjoint_axis(Lin, Lout):
    e = _interp_adjoint(Lin, Lout, False)
    print(f"interp_adjoint_axis {Lin} -> {Lout}: worst {e:.3e}")


# 2 -> 10, 2 -> 16, 3 -> 18, 2 -> 64: up-sampling ratios r = (Lout - 1) / (Lin - 1) > 5, where
# the gather window of the align_corners=False map used to cut contributions off
@pytest.mark.parametrize("Lin,Lout", [(2, 8), (3, 12), (4, 16), (5, 7), (6, 6), (1, 4), (2, 10),
                                      (2, 16), (3, 18), (2, 64)])
def test_interp_adjoint_axis_ac(Lin, Lout):
    e = _interp_adjoint(Lin, Lout, True)
    print(f"interp_adjoint_axis_ac {Lin} -> {Lout}: worst {e:.3e}")


# ------------------------------------------------------------------------------------------
# 6. Haar adjoints
# ------------------------------------------------------------------------------------------
HAAR_SHAPES = [(1, 1, 2, 2, 2), (2, 3, 4, 6, 10), (1, 48, 8, 4, 6)]       # (B, C, D, H, W)
HAAR_VARIANTS = {"all": range(8), "ll": [0], "details": range(1, 8), "band5": [5],
                 "permuted": range(8), "slices": range(8)}


@pytest.mark.parametrize("variant", list(HAAR_VARIANTS))
@pytest.mark.parametrize("shape", HAAR_SHAPES)
def test_dwt3d_haar_bwd(shape, variant):
    from waveformer_amd import _lib
    B, C_, D, H, W = shape
    d, h, w = D // 2, H // 2, W // 2
    given = list(HAAR_VARIANTS[variant])
    gb = [seeded_randn((B, C_, d, h, w), 50 + k) for k in range(8)]     # NCDHW cotangents

    x64 = seeded_randn(shape, 49).double().requires_grad_(True)
    ll, det = R.dwt3_level(x64, "db1")
    bands = [ll] + [det[k] for k in R.DETAIL_KEYS]
    (want,) = torch.autograd.grad([bands[k] for k in given], x64, [gb[k].double() for k in given])

    # band k viewed as (b, z, y, x, c)
    if variant == "permuted":    # NCDHW storage: the channel stride is d*h*w, not 1
        views = [t.to(DEV).permute(0, 2, 3, 4, 1) for t in gb]
    elif variant == "slices":    # the 8 bands side by side in one (B, d, h, w, 8C) buffer
        buf = torch.cat([t.permute(0, 2, 3, 4, 1) for t in gb], -1).contiguous().to(DEV)
        views = [buf[..., k * C_:(k + 1) * C_] for k in range(8)]
    else:
        views = [t.permute(0, 2, 3, 4, 1).contiguous().to(DEV) for t in gb]
    ptrs = [views[k].data_ptr() if k in given else None for k in range(8)]
    strides = []
    for k in range(8):
        strides.extend(views[k].stride() if k in given else (0,) * 5)
    dx = _nan(B, D, H, W, C_)
    _lib.call("wf_dwt3d_haar_bwd", (ctypes.c_void_p * 8)(*ptrs), (ctypes.c_int64 * 40)(*strides),
              dx.data_ptr(), B, C_, D, H, W, _s())
    torch.cuda.synchronize()
    e = _err(dx.permute(0, 4, 1, 2, 3), want)
    print(f"dwt3d_haar_bwd {shape} {variant}: {e:.3e}")
    assert e <= 1e-6


@pytest.mark.parametrize("layout", ["channel_last", "ncdhw"])
@pytest.mark.parametrize("shape", [(2, 3, 1, 2, 5), (1, 8, 4, 3, 2)])        # (B, C, d, h, w)
def test_haar_analysis_ncdhw(shape, layout):
    from waveformer_amd import _lib
    B, C_, d, h, w = shape
    # `in` = the first C channels of a (B, 2C, 2d, 2h, 2w) tensor: batch stride 2C * volume
    big = seeded_randn((B, 2 * C_, 2 * d, 2 * h, 2 * w), 60)
    ll64, det64 = R.dwt3_level(big[:, :C_].double(), "db1")
    bg = big.to(DEV)
    src = bg[:, :C_]
    ll = _nan(B, C_, d, h, w)
    if layout == "channel_last":
        dets = [_nan(B, d, h, w, C_).permute(0, 4, 1, 2, 3) for _ in range(7)]
    else:
        dets = [_nan(B, C_, d, h, w) for _ in range(7)]
    _lib.call("wf_haar_analysis_ncdhw", src.data_ptr(), src.stride(0), src.stride(1),
              ll.data_ptr(), (ctypes.c_void_p * 7)(*[t.data_ptr() for t in dets]),
              (ctypes.c_int64 * 5)(*dets[0].stride()), B, C_, d, h, w, _s())
    torch.cuda.synchronize()
    errs = [_err(ll, ll64)] + [_err(t, det64[k]) for t, k in zip(dets, R.DETAIL_KEYS)]
    print(f"haar_analysis_ncdhw {shape} {layout}: worst band {max(errs):.3e}")
    assert max(errs) <= 1e-6, errs
    assert torch.equal(bg.cpu(), big), "the input was written"


# ------------------------------------------------------------------------------------------
# 7. bias table, patch merging, patchify, transpose
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,heads,T", [(8, 1, 27), (27, 3, 125), (64, 2, 343), (512, 3, 3375)])
def test_rel_pos_bias_bwd(N, heads, T):
    from waveformer_amd import _lib, library
    if N == 512:
        index = R.relative_position_index(8)    # the module's own (quirk Q2: rows unused too)
    else:
        # random rows below T - 3 (the last three stay unused), and one heavy row: up to 200
        # entries (> 128: three rounds of the 64-lane gather loop) at scattered positions
        gen = torch.Generator().manual_seed(70 + N)
        index = torch.randint(0, T - 3, (N * N,), generator=gen)
        heavy = torch.randperm(N * N, generator=gen)[:min(N * N // 2, 200)]
        index[heavy] = 1
        index = index.view(N, N)
        assert N == 8 or int((index == 1).sum()) > 128
    dbias = seeded_randn((heads, N, N), 71)
    want = torch.zeros(T, heads, dtype=torch.float64)
    want.index_add_(0, index.reshape(-1), dbias.double().permute(1, 2, 0).reshape(N * N, heads))
    unused = torch.ones(T, dtype=torch.bool)
    unused[index.reshape(-1)] = False
    assert unused.any()

    ig, dbg = index.to(DEV), dbias.to(DEV)
    perm, offsets = library._index_groups(ig, T)
    dtable = _nan(T, heads)
    _lib.call("wf_rel_pos_bias_bwd", dbg.data_ptr(), perm.data_ptr(),
              offsets.data_ptr(), dtable.data_ptr(), N, heads, T, _s())
    torch.cuda.synchronize()
    e = _err(dtable, want)
    print(f"rel_pos_bias_bwd N{N} h{heads} T{T}: {e:.3e} ({int(unused.sum())} unused rows)")
    assert e <= 1e-6
    assert bool((dtable.cpu()[unused] == 0).all()), "an unused table row got a gradient"


def _merge_gather_ref(x, v2):
    """The slicing of PatchMerging (v1: duplicated sub-lattices, quirk Q3) / PatchMergingV2
    (itertools.product order) of a channel-last (B, D, H, W, C), written out."""
    if v2:
        parts = [x[:, i::2, j::2, k::2] for i, j, k in itertools.product(range(2), range(2),
                                                                         range(2))]
    else:
        x0 = x[:, 0::2, 0::2, 0::2]
        x1 = x[:, 1::2, 0::2, 0::2]
        x2 = x[:, 0::2, 1::2, 0::2]
        x3 = x[:, 0::2, 0::2, 1::2]
        x4 = x[:, 1::2, 0::2, 1::2]
        x5 = x[:, 0::2, 1::2, 0::2]
        x6 = x[:, 0::2, 0::2, 1::2]
        x7 = x[:, 1::2, 1::2, 1::2]
        parts = [x0, x1, x2, x3, x4, x5, x6, x7]
    return torch.cat(parts, -1)


@pytest.mark.parametrize("v2", [0, 1])
@pytest.mark.parametrize("shape", [(1, 4, 2, 2, 2), (2, 8, 4, 6, 10), (1, 3, 2, 4, 6)])
def test_patch_merging_gather_scatter(shape, v2):
    from waveformer_amd import _lib
    B, C_, D, H, W = shape
    M = B * (D // 2) * (H // 2) * (W // 2)
    x = seeded_randn((B, D, H, W, C_), 80)
    dm = seeded_randn((M, 8 * C_), 81)
    xg, dmg = x.to(DEV), dm.to(DEV)
    merged = _nan(M, 8 * C_)
    _lib.call("wf_patch_merging_gather", xg.data_ptr(), v2, merged.data_ptr(), B, C_, D, H, W,
              _s())
    torch.cuda.synchronize()
    assert torch.equal(merged.cpu(), _merge_gather_ref(x, v2).reshape(M, 8 * C_))

    x64 = x.double().requires_grad_(True)
    _merge_gather_ref(x64, v2).reshape(M, 8 * C_).backward(dm.double())
    dx = _nan(B, D, H, W, C_)
    _lib.call("wf_patch_merging_scatter", dmg.data_ptr(), v2, dx.data_ptr(), B, C_, D, H, W,
              _s())
    torch.cuda.synchronize()
    e = _err(dx, x64.grad)
    print(f"patch_merging gather exact, scatter {shape} v2={v2}: {e:.3e}")
    assert e <= 1e-6


def test_patch_merging_v2_op_grads():
    from waveformer_amd import library, ops  # noqa: F401  (registers the ops)
    B, D, H, W, C_ = 2, 4, 6, 8, 32
    eps = 1e-5
    p = {"x": seeded_randn((B, D, H, W, C_), 82),
         "norm.weight": 1 + 0.1 * seeded_randn((8 * C_,), 83),
         "norm.bias": 0.1 * seeded_randn((8 * C_,), 84),
         "reduction.weight": seeded_randn((2 * C_, 8 * C_), 85) * (8 * C_) ** -0.5}
    g = seeded_randn((B, D // 2, H // 2, W // 2, 2 * C_), 86)
    r = {k: v.double().requires_grad_(True) for k, v in p.items()}
    ref = F.linear(F.layer_norm(_merge_gather_ref(r["x"], 1), [8 * C_], r["norm.weight"],
                                r["norm.bias"], eps), r["reduction.weight"])
    ref.backward(g.double())
    dv = {k: v.to(DEV).requires_grad_(True) for k, v in p.items()}
    out = torch.ops.waveformer.patch_merging(dv["x"], dv["norm.weight"], dv["norm.bias"], eps,
                                             dv["reduction.weight"], True,
                                             ops.PRECISIONS["bf16x3"])
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    e_o = _err(out, ref)
    errs = {k: _err(dv[k].grad, r[k].grad) for k in p}
    print(f"patch_merging v2 op: out {e_o:.3e} " + " ".join(f"d{k} {e:.3e}"
                                                             for k, e in errs.items()))
    assert e_o <= 5e-5
    bad = {k: e for k, e in errs.items() if not e <= 2e-4}
    assert not bad, bad


@pytest.mark.parametrize("Cin", [1, 3, 4])
def test_patchify_gather_scatter(Cin):
    from waveformer_amd import _lib
    B, D, H, W = 2, 3, 2, 5
    M = B * D * H * W
    x = seeded_randn((B, Cin, 2 * D, 2 * H, 2 * W), 90)
    want = x.view(B, Cin, D, 2, H, 2, W, 2).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(M, Cin * 8)
    xg = x.to(DEV)
    rows = _nan(M, Cin * 8)
    _lib.call("wf_patchify", xg.data_ptr(), rows.data_ptr(), 0, B, Cin, D, H, W, _s())
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu(), want)
    assert torch.equal(xg.cpu(), x), "the gather wrote its input"
    back = _nan(*x.shape)
    _lib.call("wf_patchify", back.data_ptr(), rows.data_ptr(), 1, B, Cin, D, H, W, _s())
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), x)
    print(f"patchify Cin={Cin}: gather and scatter exact")


@pytest.mark.parametrize("shape", [(2, 48, 1000), (1, 33, 31), (3, 1, 7)])
def test_transpose_cs(shape):
    from waveformer_amd import _lib
    B, C_, S = shape
    x = seeded_randn(shape, 95)
    xg = x.to(DEV)
    out = _nan(B, S, C_)
    _lib.call("wf_transpose_cs", xg.data_ptr(), out.data_ptr(), B, C_, S, _s())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous())
    print(f"transpose_cs {shape}: exact")
