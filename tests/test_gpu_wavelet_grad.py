"""GPU: gradients through the general-wavelet ops (db1..db4, odd sizes) -- wf_dwt3d_bwd and
wf_idwt3d_level_bwd behind waveformer::wavedec3_level / waverec3_level, autograd.wavedec3 /
waverec3, WaveletTransform3D(wavelet='db2') and UnetrIDWTBlock(wavelet='db2').

The reference is the oracle's own autograd, fp32 on the CPU, with seeded cotangents on every
output (details included).  Bar: rel-L2 <= 1e-6 per gradient tensor -- the bar of the forward
kernels at up to three levels (test_gpu_wavelets.py::test_wavedec_waverec_vs_oracle); the
backward is the same arithmetic forms applied to the cotangent.  The fp32 oracle gradient itself
is 9.6e-8 from the fp64 one at the largest case.

Adjoint identity on the GPU outputs, in fp64 on the host:
|<A x, g> - <x, A^T g>| <= 1e-6 (|A x| |g| + |x| |A^T g|) -- Cauchy-Schwarz over the two bars.
"""
import functools

import pytest
import torch

from oracle import ref_waveformer as R
from oracle.weight_rule import seeded_randn
from tests import cases as C

pytestmark = pytest.mark.gpu

KEYS = R.DETAIL_KEYS
BAR = 1e-6
CASES = [
    ("db2", (1, 3, 48, 40, 37), 3),   # config 5's "db2 3-level", odd / ragged sizes
    ("db2", (2, 2, 20, 37, 70), 2),   # several x / y tiles of both kernels, several z chunks
    ("db1", (1, 2, 11, 9, 7), 2),     # the level-2 reconstruction is longer than the details
    ("db3", (1, 2, 25, 26, 27), 2),
    ("db4", (1, 1, 31, 18, 40), 2),
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()
    yield


def _flat(co):
    return [co[0]] + [d[k] for d in co[1:] for k in KEYS]


def _unflat(ts):
    ts = list(ts)
    return [ts[0]] + [dict(zip(KEYS, ts[1 + 7 * i:8 + 7 * i])) for i in range((len(ts) - 1) // 7)]


def _to(co, dev):
    return _unflat([t.to(dev) for t in _flat(co)])


def _leaves(co):
    return _unflat([t.detach().clone().requires_grad_(True) for t in _flat(co)])


@functools.lru_cache(maxsize=None)
def _reference(wav, shape, levels):
    """Oracle autograd in fp32 on the CPU, computed once per case and shared (read-only)."""
    x = (seeded_randn(shape, 5) * 2 + 0.3).requires_grad_(True)
    co = _flat(R.wavedec3(x, wav, levels))
    cots = [seeded_randn(tuple(t.shape), 100 + i) for i, t in enumerate(co)]
    (dx,) = torch.autograd.grad(co, x, cots)
    coeffs = _leaves(_unflat(co))
    rec = R.waverec3(coeffs, wav)
    grec = seeded_randn(tuple(rec.shape), 99)
    gco = torch.autograd.grad(rec, _flat(coeffs), grec)
    return {"x": x.detach(), "cots": cots, "dx": dx, "coeffs": _unflat([t.detach() for t in co]),
            "grec": grec, "gco": list(gco)}


@pytest.mark.parametrize("wav,shape,levels", CASES)
def test_wavedec3_gradient(wav, shape, levels):
    from waveformer_amd import autograd as wfa
    ref = _reference(wav, shape, levels)
    x = ref["x"].cuda().requires_grad_(True)
    co = _flat(wfa.wavedec3(x, wav, levels))
    assert [tuple(t.shape) for t in co] == [tuple(t.shape) for t in ref["cots"]]
    (dx,) = torch.autograd.grad(co, x, [g.cuda() for g in ref["cots"]])
    assert tuple(dx.shape) == shape
    err = C.rel_l2(dx, ref["dx"])
    print(f"wavedec3 {wav} {shape} L{levels}: dx rel-L2 {err:.3e}")
    assert err <= BAR


@pytest.mark.parametrize("wav,shape,levels", CASES)
def test_waverec3_gradient(wav, shape, levels):
    from waveformer_amd import autograd as wfa
    ref = _reference(wav, shape, levels)
    coeffs = _leaves(_to(ref["coeffs"], "cuda"))
    rec = wfa.waverec3(coeffs, wav)
    assert tuple(rec.shape) == tuple(ref["grec"].shape)
    gco = torch.autograd.grad(rec, _flat(coeffs), ref["grec"].cuda())
    assert len(gco) == 1 + 7 * levels
    for i, (g, w) in enumerate(zip(gco, ref["gco"])):
        assert tuple(g.shape) == tuple(w.shape)
        err = C.rel_l2(g, w)
        print(f"waverec3 {wav} {shape} L{levels}: coefficient {i} rel-L2 {err:.3e}")
        assert err <= BAR, i


def test_waverec3_gradient_of_cropped_ll_samples_is_zero():
    """The coarser level's reconstruction of the (11, 9, 7) two-level case is one sample longer
    than the finer details; waverec3 crops it, so those samples get gradient exactly 0."""
    from waveformer_amd import autograd as wfa
    wav, shape, levels = CASES[2]
    co = _reference(wav, shape, levels)["coeffs"]
    mid = R.waverec3(co[:2], wav)                      # the LL input of the finest level
    fine = tuple(co[2]["aad"].shape[2:])
    longer = [a - b for a, b in zip(mid.shape[2:], fine)]
    assert all(e in (0, 1) for e in longer) and any(e == 1 for e in longer), (mid.shape, fine)
    lvl = _leaves([mid, co[2]])
    rec = R.waverec3(lvl, wav)
    grec = seeded_randn(tuple(rec.shape), 98)
    want = torch.autograd.grad(rec, _flat(lvl), grec)
    got_in = _leaves(_to([mid, co[2]], "cuda"))
    got = torch.autograd.grad(wfa.waverec3(got_in, wav), _flat(got_in), grec.cuda())
    gll = got[0].cpu()
    assert tuple(gll.shape) == tuple(mid.shape)
    inside = torch.zeros(gll.shape, dtype=torch.bool)
    inside[..., :fine[0], :fine[1], :fine[2]] = True
    assert bool((gll[~inside] == 0).all()) and int((~inside).sum()) > 0
    assert bool((want[0][~inside] == 0).all())
    for g, w in zip(got, want):
        assert C.rel_l2(g, w) <= BAR


def test_waverec3_gradient_strided_paths_equal_contiguous():
    """Channel-last detail views in, the output gradient arriving through
    torch.cat((rec, skip), 1): the same bits as contiguous tensors and a contiguous gradient."""
    from waveformer_amd import autograd as wfa
    B, Cc, n = 2, 5, (9, 7, 12)
    cl = [seeded_randn((B,) + n + (Cc,), 40 + i).cuda() for i in range(8)]
    views = [t.permute(0, 4, 1, 2, 3).detach().requires_grad_(True) for t in cl]
    assert not views[1].is_contiguous() and views[1].stride(1) == 1
    O = tuple(2 * s - 2 for s in n)
    skip = seeded_randn((B, Cc) + O, 60).cuda().requires_grad_(True)
    G = seeded_randn((B, 2 * Cc) + O, 61).cuda()
    rec = wfa.waverec3([views[0], dict(zip(KEYS, views[1:]))], "db2")
    torch.cat((rec, skip), 1).backward(G)
    assert torch.equal(skip.grad, G[:, Cc:])
    dense = [t.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True) for t in cl]
    rec2 = wfa.waverec3([dense[0], dict(zip(KEYS, dense[1:]))], "db2")
    assert torch.equal(rec2, rec)
    rec2.backward(G[:, :Cc].contiguous())
    for v, d in zip(views, dense):
        assert v.grad is not None and tuple(v.grad.shape) == tuple(d.grad.shape)
        assert torch.equal(v.grad, d.grad)
    # and against the oracle
    lv = _leaves([t.detach().cpu() for t in dense[:1]] + [
        {k: t.detach().cpu() for k, t in zip(KEYS, dense[1:])}])
    want = torch.autograd.grad(R.waverec3(lv, "db2"), _flat(lv), G[:, :Cc].cpu())
    for v, w in zip(views, want):
        assert C.rel_l2(v.grad, w) <= BAR


def _dot(a, b):
    return sum(float((s.double().cpu() * t.double().cpu()).sum()) for s, t in zip(a, b))


def _norm(a):
    return _dot(a, a) ** 0.5


def test_adjoint_identity():
    import waveformer_amd.library  # noqa: F401
    ops = torch.ops.waveformer
    shape = (2, 2, 20, 37, 70)
    # one analysis level
    x = seeded_randn(shape, 70).cuda().requires_grad_(True)
    ax = ops.wavedec3_level(x, "db2")
    g = seeded_randn(tuple(ax.shape), 71).cuda()
    (atg,) = torch.autograd.grad(ax, x, g)
    lhs, rhs = _dot([ax], [g]), _dot([x], [atg])
    bound = BAR * (_norm([ax]) * _norm([g]) + _norm([x]) * _norm([atg]))
    print(f"analysis: <Ax,g> {lhs:.9e} <x,Atg> {rhs:.9e} diff {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    # one synthesis level
    n = tuple(ax.shape[3:])
    c = [seeded_randn(shape[:2] + n, 80 + k).cuda().requires_grad_(True) for k in range(8)]
    sc = ops.waverec3_level(c[0], c[1:], "db2")
    g = seeded_randn(tuple(sc.shape), 90).cuda()
    stg = torch.autograd.grad(sc, c, g)
    lhs, rhs = _dot([sc], [g]), _dot(c, stg)
    bound = BAR * (_norm([sc]) * _norm([g]) + _norm(c) * _norm(stg))
    print(f"synthesis: <Sc,g> {lhs:.9e} <c,Stg> {rhs:.9e} diff {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------------------------ modules
def test_wavelet_transform_module_backpropagates():
    import waveformer_amd.network_models as NM
    x0 = seeded_randn((1, 4, 21, 16, 19), 9)
    x = x0.clone().requires_grad_(True)
    ref = _flat(R.wavedec3(x, "db2", 2))
    cots = [seeded_randn(tuple(t.shape), 200 + i) for i, t in enumerate(ref)]
    (want,) = torch.autograd.grad(ref, x, cots)
    xg = x0.cuda().requires_grad_(True)
    ll, yh = NM.WaveletTransform3D(wavelet="db2")(xg, 2)
    got = _flat([ll] + list(yh))
    for a, b in zip(got, ref):
        assert C.rel_l2(a, b) <= BAR
    sum((t * g.cuda()).sum() for t, g in zip(got, cots)).backward()
    assert C.rel_l2(xg.grad, want) <= BAR


def _idwt_block(hf_refinement, in_channels=8):
    from waveformer_amd.network_models.idwt_upsample import UnetrIDWTBlock
    ref = R.wavedec3(seeded_randn((1, 4, 21, 16, 19), 9), "db2", 2)
    torch.manual_seed(0)
    blk = UnetrIDWTBlock(3, in_channels, 4, stage=2, hf_refinement=hf_refinement, wavelet="db2",
                         kernel_size=3, norm_name="instance", res_block=True).eval().cuda()
    inp = seeded_randn((1, in_channels) + tuple(ref[0].shape[2:]), 11).cuda().requires_grad_(True)
    hf = tuple({k: v[:, :4].contiguous().cuda().requires_grad_(True) for k, v in d.items()}
               for d in ref[1:])
    O = tuple(2 * s - 2 for s in hf[-1]["aad"].shape[2:])
    skip = seeded_randn((1, 4) + O, 12).cuda().requires_grad_(True)
    return blk, inp, skip, hf


def _run_block(blk, inp, skip, hf):
    """forward + backward under a seeded cotangent; returns (the conv_block input, the
    conv_lf_block output), both with their gradients retained."""
    kept = {}

    def pre(_m, args):
        args[0].retain_grad()
        kept["cat"] = args[0]

    def post(_m, _args, out):
        out.retain_grad()
        kept["lf"] = out

    h1 = blk.conv_block.register_forward_pre_hook(pre)
    h2 = blk.conv_lf_block.register_forward_hook(post)
    try:
        out = blk(inp, skip, hf)
    finally:
        h1.remove()
        h2.remove()
    (out * seeded_randn(tuple(out.shape), 13).cuda()).sum().backward()
    return kept["cat"], kept["lf"]


def _finite(t):
    return t is not None and bool(torch.isfinite(t).all())


def test_idwt_block_db2_backward():
    blk, inp, skip, hf = _idwt_block(False)
    cat, lf = _run_block(blk, inp, skip, hf)
    for t in [inp, skip] + [v for d in hf for v in d.values()]:
        assert _finite(t.grad)
    for name, p in blk.named_parameters():
        assert _finite(p.grad), name
    # the wavelet part alone: the oracle's autograd of waverec3 under the cotangent that reached
    # the reconstruction, G[:, :C]
    Cc = lf.shape[1]
    G = cat.grad[:, :Cc].detach().cpu().contiguous()
    lv = _leaves([lf.detach().cpu()] + [{k: v.detach().cpu() for k, v in d.items()} for d in hf])
    want = torch.autograd.grad(R.waverec3(lv, "db2"), _flat(lv), G)
    got = [lf.grad] + [d[k].grad for d in hf for k in KEYS]
    for i, (g, w) in enumerate(zip(got, want)):
        err = C.rel_l2(g, w)
        print(f"idwt block: coefficient {i} rel-L2 {err:.3e}")
        assert err <= BAR, i


def test_idwt_block_db2_hf_refinement_backward():
    # HFRefinementRes(in_channels // 2 ** stage) filters the details, which have out_channels
    # channels: in_channels = out_channels * 2 ** stage, as in the network
    blk, inp, skip, hf = _idwt_block(True, in_channels=16)
    _run_block(blk, inp, skip, hf)
    for t in [inp, skip] + [v for d in hf for v in d.values()]:
        assert _finite(t.grad)
    for name, p in blk.named_parameters():
        assert _finite(p.grad), name
    assert any(n.startswith("hf_ref.") for n, _ in blk.named_parameters())


def test_idwt_block_db2_backward_is_repeatable():
    runs = []
    for _ in range(2):
        blk, inp, skip, hf = _idwt_block(False)
        _run_block(blk, inp, skip, hf)
        runs.append([inp.grad, skip.grad] + [d[k].grad for d in hf for k in KEYS]
                    + [p.grad for p in blk.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------- registration
def _op_inputs(name, train):
    x = seeded_randn((2, 3, 9, 6, 11), 1).cuda()
    if name == "wavedec3_level":
        return [x.requires_grad_(train), "db2"]
    from waveformer_amd import ops
    bands = ops.dwt3d(x, "db2")
    return [bands[0].clone().requires_grad_(train),
            [bands[k].clone().requires_grad_(train) for k in range(1, 8)], "db2"]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", ["wavedec3_level", "waverec3_level"])
def test_opcheck(name, train):
    import waveformer_amd.library  # noqa: F401
    op = getattr(torch.ops.waveformer, name).default
    tests = ["test_schema", "test_faketensor", "test_autograd_registration"]
    if train:
        tests.append("test_aot_dispatch_dynamic")
    torch.library.opcheck(op, _op_inputs(name, train), test_utils=tests)


def test_compile_wavelet_transform_fullgraph_matches_eager():
    import waveformer_amd.network_models as NM
    torch._dynamo.reset()
    m = NM.WaveletTransform3D("db2")
    x = seeded_randn((1, 4, 21, 16, 19), 9).cuda()
    cm = torch.compile(m, backend="aot_eager", fullgraph=True)
    with torch.no_grad():
        ll, yh = m(x, 2)
        cll, cyh = cm(x, 2)
    want, got = _flat([ll] + list(yh)), _flat([cll] + list(cyh))
    assert len(got) == len(want) == 15
    for a, b in zip(got, want):
        assert torch.equal(a, b)
