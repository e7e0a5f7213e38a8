"""GPU: training through the fused HF refinement -- waveformer::hf_refine / hf_refine_backward
(wf_hf_refine_fwd, wf_hf_refine_bwd, csrc/hfref.hip) and its wiring into UnetrIDWTBlock.

(a) the op against HFRefinementRes's own forward + autograd in fp64 on the CPU: out and gx per
    detail tensor, the parameter gradients summed over the 7 tensors and the batch.  All-fp32
    kernels against fp64 (g_pw_w on wf_gemm_tn, bf16x3): rel-L2 <= 1e-5 per tensor.  g_dw_b is
    0 in exact arithmetic (the InstanceNorm removes the conv's mean) and is bounded absolutely:
    |g_dw_b|_inf <= 1e-4 |g_dw_w|_inf.
(b) wf_hf_refine_bwd writes every element of every output, two calls on the same saved moments
    are bitwise identical, the bytes behind the workspace stay untouched.
(c) details that are not dense channel-last views of one band buffer.
(d) UnetrIDWTBlock under autograd takes the op once per level and never the per-tensor module
    path; its gradients against the oracle's idwt_block under autograd in fp64 (rel-L2 <= 2e-4,
    test_train_grads.py's bar for module gradients whose convolutions run at bf16x3); under
    no_grad it is bitwise the inference path.
(e) torch.library.opcheck of waveformer::hf_refine.

ReLU condition: the gradient is discontinuous where the pre-activation a is 0, so a sign of a
that differs between fp32 and fp64 fails a correct kernel.  Every case takes the first band
seed of 7 .. 22 for which the fp64 reference has min |a| >= 1e-5 over all 7 tensors (a
condition on the input, evaluated on the reference alone) and asserts that one exists.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_waveformer as R
from oracle.weight_rule import rule_state_dict, seeded_randn
from tests import cases as C

pytestmark = pytest.mark.gpu

KEYS = R.DETAIL_KEYS
BAR = 1e-5
BAR_BLOCK = 2e-4
MIN_A = 1e-5
SEEDS = range(7, 23)
PARAMS = ("conv1.weight", "conv1.bias", "norm.weight", "norm.bias", "conv2.weight", "conv2.bias")

# C, B, (D, H, W), sigmoid -- each the smallest shape that reaches a given part of the kernels
CASES = [
    (48, 2, (9, 6, 5), True),     # two z segments (ragged last), two (y, x) tiles, batch stride
    (192, 1, (3, 3, 3), True),    # decoder4 width, fewer positions than one workgroup
    (24, 1, (4, 5, 3), True),     # C / 4 not dividing 256 (idle lanes)
    (96, 1, (2, 3, 10), True),    # decoder3 width, D < 3
    (48, 1, (5, 4, 3), False),    # use_sigmoid False
    (4, 1, (3, 2, 2), True),      # the minimum width
]
IDS = [f"C{c}-B{b}-{'x'.join(map(str, s))}-{'sig' if g else 'nosig'}" for c, b, s, g in CASES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()
    yield


def _module(C_, sig):
    import waveformer_amd.network_models as NM
    cfg = None if sig else {"hf_refinement": {"use_sigmoid": False}}
    m = NM.HFRefinementRes(C_, network_config=cfg)
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(seeded_randn(tuple(p.shape), 40 + i) * (0.5 if p.dim() > 1 else 0.2)
                    + (1.0 if p.dim() == 1 and i == 2 else 0.0))
    return m


def _min_abs_a(md, xs):
    """min |a| of the pre-activation a = norm(conv1(x)) over the fp64 tensors xs."""
    with torch.no_grad():
        return min(float(md.norm(md.conv1(x)).abs().min()) for x in xs)


@functools.lru_cache(maxsize=None)
def _reference(idx):
    """Parameters, bands, cotangents and the fp64 CPU reference of CASES[idx], computed once
    and shared: out / gx per detail, the six parameter gradients."""
    C_, B, S, sig = CASES[idx]
    m = _module(C_, sig)
    md = _module(C_, sig).double()
    for seed in SEEDS:
        bands = seeded_randn((8, B) + S + (C_,), seed) * 1.5 + 0.2
        xs = [bands[i + 1].permute(0, 4, 1, 2, 3).double() for i in range(7)]
        mina = _min_abs_a(md, xs)
        if mina >= MIN_A:
            break
    else:
        raise AssertionError(f"no band seed in 7..22 with min|a| >= {MIN_A}")
    cots = [seeded_randn((B, C_) + S, 100 + i) for i in range(7)]
    outs, gxs = [], []
    for x, g in zip(xs, cots):
        x = x.clone().requires_grad_(True)
        y = md(x)
        y.backward(g.double())
        outs.append(y.detach())
        gxs.append(x.grad)
    gp = [p.grad.clone() for p in md.parameters()]
    print(f"case {IDS[idx]}: band seed {seed}, min|a| {mina:.2e}")
    return dict(module=m, bands=bands, cots=cots, out=outs, gx=gxs, gp=gp, seed=seed)


def _check_against(ref, m, dets, leaves, tag):
    """forward + backward of wfa.hf_refine on the cuda module m and the 7 detail tensors dets
    (gradients read from `leaves`, (B, C, D, H, W)-shaped), against the reference."""
    from waveformer_amd import autograd as wfa
    got = wfa.hf_refine(dict(zip(KEYS, dets)), m)
    sum((got[k] * ref["cots"][i].cuda()).sum() for i, k in enumerate(KEYS)).backward()
    errs = {}
    for i, k in enumerate(KEYS):
        errs[f"out[{k}]"] = C.rel_l2(got[k], ref["out"][i])
        errs[f"gx[{k}]"] = C.rel_l2(leaves[i], ref["gx"][i])
    grads = [p.grad for p in m.parameters()]
    for name, g, w in zip(PARAMS, grads, ref["gp"]):
        if name != "conv1.bias":
            errs[f"g {name}"] = C.rel_l2(g, w)
    zero = float(grads[1].abs().max())
    bound = 1e-4 * float(grads[0].abs().max())
    print(f"{tag}: worst out {max(v for k, v in errs.items() if k.startswith('out')):.3e}, "
          f"worst gx {max(v for k, v in errs.items() if k.startswith('gx')):.3e}, "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items() if k.startswith("g "))
          + f", |g conv1.bias|_inf {zero:.3e} (bound {bound:.3e})")
    for k, v in errs.items():
        assert v <= BAR, (k, v)
    assert zero <= bound


# ------------------------------------------------------------------ (a) op vs fp64 autograd
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_hf_refine_op_vs_fp64_autograd(idx):
    """Details as the DWT hands them over: channel-last views of one (8, B, D, H, W, C) band
    buffer.  Measured errors: DESIGN 7.4, "HF refinement under autograd"."""
    ref = _reference(idx)
    C_, _, _, sig = CASES[idx]
    m = _module(C_, sig).cuda()
    bc = ref["bands"].cuda().requires_grad_(True)
    dets = [bc[i + 1].permute(0, 4, 1, 2, 3) for i in range(7)]
    assert m.train_ok(dets[0]) and not m.fast_ok(dets[0])

    class _BandGrads:  # read after backward
        def __getitem__(self, i):
            return bc.grad[i + 1].permute(0, 4, 1, 2, 3)
    _check_against(ref, m, dets, _BandGrads(), IDS[idx])


# ------------------------------------------------- (b) every element written, bitwise repeat
@pytest.mark.parametrize("idx", [0, 2], ids=[IDS[0], IDS[2]])
def test_hf_refine_bwd_writes_everything_and_repeats(idx):
    from waveformer_amd import _lib, ops
    C_, B, S, sig = CASES[idx]
    D, H, W = S
    ref = _reference(idx)
    m = _module(C_, sig).cuda()
    prm = [p.detach() for p in m.parameters()]
    bc = ref["bands"].cuda()
    dets = [bc[i + 1].permute(0, 4, 1, 2, 3) for i in range(7)]
    _, moments = ops._hf_refine_raw(dets, *prm[:4], float(m.norm.eps), *prm[4:], sig)
    saved = moments.clone()
    gy = torch.stack([g.permute(0, 2, 3, 4, 1) for g in ref["cots"]]).contiguous().cuda()
    nbytes = _lib.query("wf_hf_refine_bwd_workspace_bytes", B, C_, D, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    guard = 4096
    ptrs = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in dets])
    runs = []
    for _ in range(2):
        gx = torch.full_like(gy, float("nan"))
        grads = [torch.full_like(p, float("nan")) for p in prm]
        ws = torch.empty(nbytes + guard, dtype=torch.uint8, device="cuda")
        ws[:nbytes].view(torch.float32).fill_(float("nan"))
        ws[nbytes:].fill_(0xA5)
        _lib.call("wf_hf_refine_bwd", ptrs, dets[0].stride(0), *[p.data_ptr() for p in prm[:4]],
                  float(m.norm.eps), prm[4].data_ptr(), prm[5].data_ptr(), int(sig),
                  moments.data_ptr(), gy.data_ptr(), gx.data_ptr(),
                  *[g.data_ptr() for g in grads], ws.data_ptr(), B, C_, D, H, W,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all()), "bytes behind the workspace were written"
        for t in [gx] + grads:
            assert bool(torch.isfinite(t).all())
        runs.append([gx] + grads)
    assert torch.equal(moments, saved)  # read only
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert C.rel_l2(runs[0][0], torch.stack([g.permute(0, 2, 3, 4, 1) for g in ref["gx"]])) <= BAR


# --------------------------------------------------------------------- (c) non-dense inputs
@pytest.mark.parametrize("layout", ["ncdhw", "unequal_batch_strides", "batch_major_bands"])
def test_hf_refine_non_dense_details(layout):
    """Case 1's values in other layouts, which the wrapper turns into dense channel-last
    tensors of one batch stride: contiguous NCDHW tensors, channel-last tensors with unequal
    batch strides, and the slices of a batch-major band buffer (batch stride of 8 samples)."""
    idx = 0
    C_, B, S, sig = CASES[idx]
    ref = _reference(idx)
    m = _module(C_, sig).cuda()
    P = S[0] * S[1] * S[2]
    vals = [ref["bands"][i + 1] for i in range(7)]  # (B, D, H, W, C)
    if layout == "ncdhw":
        leaves = [v.permute(0, 4, 1, 2, 3).contiguous().cuda().requires_grad_(True) for v in vals]
        dets = leaves
    elif layout == "unequal_batch_strides":
        leaves, dets = [], []
        for i, v in enumerate(vals):
            buf = torch.zeros((B, P * C_ + 64 * i), device="cuda")
            buf[:, :P * C_] = v.reshape(B, -1).cuda()
            buf.requires_grad_(True)
            leaves.append(buf)
            dets.append(buf[:, :P * C_].view((B,) + S + (C_,)).permute(0, 4, 1, 2, 3))
        assert len({d.stride(0) for d in dets}) == 7
    else:
        buf = ref["bands"].transpose(0, 1).contiguous().cuda().requires_grad_(True)  # (B, 8, ..)
        leaves = [buf] * 7
        dets = [buf[:, i + 1].permute(0, 4, 1, 2, 3) for i in range(7)]
        assert dets[0].stride(0) == 8 * P * C_

    class _Grads:
        def __getitem__(self, i):
            g = leaves[i].grad
            if layout == "unequal_batch_strides":
                return g[:, :P * C_].view((B,) + S + (C_,)).permute(0, 4, 1, 2, 3)
            if layout == "batch_major_bands":
                return g[:, i + 1].permute(0, 4, 1, 2, 3)
            return g
    _check_against(ref, m, dets, _Grads(), layout)


# ------------------------------------------------------------------------------- (d) wiring
def _block_setup():
    """UnetrIDWTBlock(32 -> 8, two levels, HF refinement) with rule weights, details from
    ops.dwt3d_haar of seeded volumes (per level the first seed meeting the ReLU condition)."""
    from waveformer_amd import ops
    from waveformer_amd.network_models.idwt_upsample import UnetrIDWTBlock
    B, Cd, s = 2, 8, (2, 3, 2)
    blk = UnetrIDWTBlock(3, 32, Cd, stage=2, hf_refinement=True, wavelet="db1", kernel_size=3,
                         norm_name="instance", res_block=True)
    sd = rule_state_dict(blk.state_dict())
    blk.load_state_dict(sd, strict=True)
    sdd = {k: v.double() for k, v in sd.items()}
    hf, seeds = [], []
    for lvl in range(2):  # coarse -> fine
        vol = tuple(2 * n * 2 ** lvl for n in s)
        for seed in SEEDS:
            x = (seeded_randn((B,) + vol + (Cd,), 10 * lvl + seed) * 1.5 + 0.2).cuda()
            bands = ops.dwt3d_haar(x).cpu()
            p = f"hf_ref.{lvl}."
            mina = float("inf")
            for i in range(7):
                xd = bands[i + 1].permute(0, 4, 1, 2, 3).double()
                a = F.instance_norm(
                    F.conv3d(xd, sdd[p + "conv1.weight"], sdd[p + "conv1.bias"], padding=1,
                             groups=Cd),
                    weight=sdd[p + "norm.weight"], bias=sdd[p + "norm.bias"], eps=1e-5)
                mina = min(mina, float(a.abs().min()))
            if mina >= MIN_A:
                break
        else:
            raise AssertionError(f"level {lvl}: no band seed in 7..22 with min|a| >= {MIN_A}")
        print(f"block level {lvl}: band seed {seed}, min|a| {mina:.2e}")
        hf.append(bands)
        seeds.append(seed)
    inp = seeded_randn((B, 32) + s, 31)
    skip = seeded_randn((B, Cd) + tuple(4 * n for n in s), 32)
    return blk, sdd, inp, skip, hf


def test_idwt_block_trains_through_fused_hf_refine():
    from waveformer_amd import autograd as wfa
    from waveformer_amd import ops
    blk, sdd, inp, skip, hf = _block_setup()
    # fp64 reference: the oracle's block under autograd
    sdr = {k: v.clone().requires_grad_(True) for k, v in sdd.items()}
    inp_r = inp.double().requires_grad_(True)
    skip_r = skip.double().requires_grad_(True)
    hf_r = [b.double().requires_grad_(True) for b in hf]
    det_r = tuple({k: b[i + 1].permute(0, 4, 1, 2, 3) for i, k in enumerate(KEYS)} for b in hf_r)
    out_r = R.idwt_block(sdr, "", inp_r, skip_r, det_r, hf_refine=True)
    cot = seeded_randn(tuple(out_r.shape), 33)
    out_r.backward(cot.double())

    blk = blk.cuda()
    inp_g = inp.cuda().requires_grad_(True)
    skip_g = skip.cuda().requires_grad_(True)
    hf_g = [b.cuda().requires_grad_(True) for b in hf]
    det_g = tuple({k: b[i + 1].permute(0, 4, 1, 2, 3) for i, k in enumerate(KEYS)} for b in hf_g)
    calls, norm_fired = [], []
    real = wfa.hf_refine

    def counting(details, mod):
        calls.append(mod)
        return real(details, mod)
    hooks = [m.norm.register_forward_hook(lambda *_: norm_fired.append(1)) for m in blk.hf_ref]
    wfa.hf_refine = counting
    try:
        out_g = blk(inp_g, skip_g, det_g)
    finally:
        wfa.hf_refine = real
        for h in hooks:
            h.remove()
    assert [id(m) for m in calls] == [id(m) for m in blk.hf_ref]  # once per level
    assert not norm_fired  # the per-tensor module path did not run
    out_g.backward(cot.cuda())
    errs = {"out": C.rel_l2(out_g, out_r), "inp": C.rel_l2(inp_g.grad, inp_r.grad),
            "skip": C.rel_l2(skip_g.grad, skip_r.grad)}
    for lvl in range(2):
        for i, k in enumerate(KEYS):
            errs[f"detail {lvl}.{k}"] = C.rel_l2(hf_g[lvl].grad[i + 1], hf_r[lvl].grad[i + 1])
    zero_bias = {}
    for name, p in blk.named_parameters():
        if name.startswith("hf_ref.") and name.endswith("conv1.bias"):
            zero_bias[name] = (float(p.grad.abs().max()),
                               float(dict(blk.named_parameters())[
                                   name.replace("bias", "weight")].grad.abs().max()))
            continue
        errs[name] = C.rel_l2(p.grad, sdr[name].grad)
    for k, v in errs.items():
        print(f"idwt block + HF refinement: {k} rel-L2 {v:.3e}")
    for k, (z, w) in zero_bias.items():
        print(f"idwt block + HF refinement: {k} |g|_inf {z:.3e} (|g weight|_inf {w:.3e})")
    assert any(n.startswith("hf_ref.") for n in errs)
    for k, v in errs.items():
        assert v <= BAR_BLOCK, (k, v)
    for k, (z, w) in zero_bias.items():  # true value 0 (see the module docstring)
        assert z <= 1e-4 * w, k

    # no_grad: bitwise the inference path (ops.hf_refine + ops.idwt3d_haar called directly)
    with torch.no_grad():
        det = tuple({k: b.detach()[i + 1].permute(0, 4, 1, 2, 3) for i, k in enumerate(KEYS)}
                    for b in hf_g)
        got = blk(inp_g.detach(), skip_g.detach(), det)
        lf = blk.conv_lf_block(inp_g.detach())
        ref_hf = tuple(ops.hf_refine(d, blk.hf_ref[i]) for i, d in enumerate(det))
        Bn, Cn = lf.shape[:2]
        buf = ops.empty_cl(Bn, Cn + skip_g.shape[1], *skip_g.shape[2:], lf.device)
        ops.idwt3d_haar(lf, ref_hf, out=buf, skip=skip_g.detach())
        want = blk.conv_block(buf)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------ (e) opcheck
@pytest.mark.parametrize("train", [False, True])
def test_opcheck(train):
    import waveformer_amd.library  # noqa: F401
    C_, B, S = 8, 2, (3, 4, 5)
    g = lambda shape, seed, scale=1.0: (seeded_randn(shape, seed) * scale).cuda()  # noqa: E731
    bands = g((8, B) + S + (C_,), 1)
    dets = [bands[i + 1].permute(0, 4, 1, 2, 3).clone().requires_grad_(train) for i in range(7)]
    args = [dets, g((C_, 1, 3, 3, 3), 2, 0.3).requires_grad_(train),
            g((C_,), 3, 0.1).requires_grad_(train), g((C_,), 4, 0.1).add_(1).requires_grad_(train),
            g((C_,), 5, 0.1).requires_grad_(train), 1e-5,
            g((C_, C_, 1, 1, 1), 6, 0.3).requires_grad_(train),
            g((C_,), 7, 0.1).requires_grad_(train), True]
    tests = ["test_schema", "test_faketensor", "test_autograd_registration"]
    if train:
        tests.append("test_aot_dispatch_dynamic")
    torch.library.opcheck(torch.ops.waveformer.hf_refine.default, args, test_utils=tests)
