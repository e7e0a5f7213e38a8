"""GPU: the attention softmax against fp64 at large logits, row by row.

The other attention tests compare with a reference only at logits a few nats wide (so the
online softmax never rescales after its first key tile), and reach large logits only by
comparing one HIP variant with another.  Here the logits are large AND known exactly
(tests/attention_cases.py: bias-only inputs, q = 0), the reference is fp64, and the error is
taken per token row: one wrong query row among thousands -- what a bad rescale of one sub-tile,
a wrong lane exchange or a key-mask slip gives -- fails.

Every assertion has three parts: the output is finite; the worst row's
||got_r - ref_r|| / ||ref_r|| meets the per-row bar; the whole-tensor rel-L2 meets the
project's bar of the kind (5e-5 bf16x3, 1e-2 bf16, 2e-3 fp16).  The per-row bar is computed at
run time, never from the kernel: 4 x the worst row error of the CPU operand-rounding emulation
(attention_cases.attention_fp64 at the kind) against fp64 on the same inputs, at least
64 * 2^-24.  The factor covers what the emulation leaves out: fp32 accumulation in tile
order, v_exp_f32's last place, the rescale's extra fp32 roundings.

 * test_table_bias_only: attn_tbl_kernel (ws 8, head_dim 16, C = 48) in its three launch forms
   (qsplit 4 / NQ = 1; qsplit 2 / NQ = 2; qsplit 1 / NQ = 2 twice per wave), staged and fused
   q / k / v where the split is <= 2, at the three operand kinds, on tables that reach: a
   rescale at every tile (ladder_up), kept tiles with exponentials near 2^12 and then a rescale
   (ladder_keep), no rescale and underflowing exponentials (ladder_down), alpha = 0 after
   seven accumulated tiles (one_hot_last), a rescale of a query pair only one sub-tile asked
   for (pair_split), large equal magnitudes (flat_low), and a kept score just under
   mrun + 16 (f16_band).  test_attention_softmax_host.py pins which events each reaches.
   f16_band is the test of the fp16 overflow: with the threshold 16 at every kind the fp16
   kernel made exp2(15.9998) = 65526 an fp16 operand, i.e. inf: 195 of every window's 512 rows came out non-finite
   in all three launch forms, none at bf16 / bf16x3 (profiles/r18/f16_band_on_parent.txt); tbl::kTauFp16 = 15 rescales such a tile.
 * test_table_qk_driven: the `mixed` construction of the bitwise tests (inputs x 8, random
   qkv weight) against fp64, qsplit 4 and 2.  The logits here carry operand-rounding error
   proportional to their size, so ONLY the emulation-derived row bar applies: the project's
   rel-L2 bars are not asserted for these cases (the figure is printed).
 * test_general_bias_only: attn_core_kernel with a dense bias at N = 8, 27, 125, 64, 512, 1728
   (partial key tiles, the key mask next to large logits, 27 tiles), ladders, a moving one-hot
   and the row's only large logit on the last valid key of a partial tile.
 * test_general_train_forward_lse: the same through waveformer::window_attn(train=True), whose
   stored log-sum-exp must be within 4 fp32 ulps of |lse| + 4e-6 of fp64 logsumexp / ln 2.
 * test_general_backward_one_hot: wf_window_attention_bwd_core on the one-hot bias against
   fp64 autograd, per row.

Measured (MI355X), worst row error: emulation -> kernel, per case and kind, the largest over
the launch forms and q / k / v modes (profiles/r18/attn_softmax_errors.txt has every line):

  case                      bf16x3                  bf16                    fp16
  table ladder_up           5.10e-06 -> 5.09e-06    2.86e-03 -> 2.86e-03    3.30e-04 -> 3.30e-04
  table ladder_keep         5.15e-06 -> 5.99e-06    2.67e-03 -> 2.60e-03    3.27e-04 -> 3.27e-04
  table ladder_down         5.46e-06 -> 5.46e-06    2.67e-03 -> 2.67e-03    3.36e-04 -> 3.36e-04
  table one_hot_last        5.64e-06 -> 5.64e-06    3.05e-03 -> 3.05e-03    3.89e-04 -> 3.89e-04
  table pair_split          5.66e-06 -> 5.66e-06    3.62e-03 -> 3.62e-03    4.36e-04 -> 4.36e-04
  table flat_low            3.61e-06 -> 3.61e-06    2.16e-03 -> 2.16e-03    2.85e-04 -> 2.85e-04
  table f16_band            6.91e-06 -> 6.44e-06    4.19e-03 -> 4.19e-03    5.11e-04 -> 5.11e-04
  table qk_mixed            4.76e-04 -> 4.73e-04    3.04e-01 -> 3.04e-01    2.96e-02 -> 2.97e-02
  general ladder_up         5.72e-06 -> 5.75e-06    2.80e-03 -> 2.80e-03    3.87e-04 -> 3.87e-04
  general ladder_down       5.91e-06 -> 5.91e-06    2.81e-03 -> 2.81e-03    4.28e-04 -> 4.28e-04
  general one_hot_last      5.46e-06 -> 5.47e-06    2.77e-03 -> 2.77e-03    3.46e-04 -> 3.46e-04
  general last_valid_key    4.38e-06 -> 4.38e-06    2.42e-03 -> 2.42e-03    3.07e-04 -> 3.07e-04
  (the train=True forward gives the general kernel's bf16x3 figures; its log-sum-exp is at most
  0.18 of its bar, 1.2e-5 absolute)
  backward (fp32)           one_hot_last dqkv 5.34e-06 -> 5.35e-06 (whole tensor 5.3e-06, dbias
                            3.8e-06 absolute against a noise bound of 4.7e-05)
                            one_hot_soft dqkv 7.76e-07 -> 1.18e-06, dbias 3.64e-03 -> 3.64e-03
                            (whole tensor: dqkv 5.3e-07, dbias 1.7e-04 -- above the 1e-5 bar of
                            test_attention_bwd_core, from dP - D cancelling on the spike)
The largest measured / bar ratio is 0.31.  qk_mixed's bf16 row bar is above 1: at logits this
size bf16 operands do not resolve the softmax, and the bar says so.
"""
import math

import pytest
import torch

from tests import attention_cases as A
from oracle.weight_rule import seeded_randn

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()
    yield


def _check(tag, got, ref, emu, kind, rel_bar=True):
    """finite, the per-row bar (from the emulation), the project's whole-tensor bar."""
    got = got.detach().cpu().reshape(ref.shape)
    bar, e_emu = A.row_bar(emu, ref)
    e_row, at = A.row_err(got, ref)
    e_l2 = A.rel_l2(got, ref)
    nonfinite = int((~torch.isfinite(got)).sum())
    print(f"attn_softmax {tag} {kind}: emu_row {e_emu:.3e} bar {bar:.3e} row {e_row:.3e} (row {at}) "
          f"rel_l2 {e_l2:.3e} nonfinite {nonfinite}")
    assert nonfinite == 0, f"{tag}: {nonfinite} non-finite output elements, first bad row {at}"
    assert e_row <= bar, f"{tag}: row {at} is {e_row:.3e} from fp64, bar {bar:.3e}"
    if rel_bar:
        assert e_l2 <= A.REL_L2_BARS[kind], f"{tag}: rel-L2 {e_l2:.3e}"


def _table_attend(x, w, table, kind, mode):
    from waveformer_amd import ops
    return ops.window_attention(x.to(DEV), w["wqkv"].to(DEV), w["bqkv"].to(DEV), table.to(DEV),
                                w["wproj"].to(DEV), w["bproj"].to(DEV), A.WS, A.HEADS, A.HD ** -0.5,
                                prec=ops.PRECISIONS[kind], qkv_mode=mode)


def _modes(form):
    """q / k / v of the launch: the library's rule at qsplit 4 (staged), else staged and fused."""
    return (-1,) if A.FORMS[form][2] == 4 else (0, 1)


TABLE_PARAMS = [(form, name, kind) for form in A.FORMS for name, (_, _, forms) in A.TABLE_CASES.items()
                if form in forms for kind in A.KINDS]


@pytest.mark.parametrize("form,name,kind", TABLE_PARAMS)
def test_table_bias_only(form, name, kind):
    ref = A.table_reference(name, form)
    emu = A.table_emulation(name, form, kind)
    for mode in _modes(form):
        got = _table_attend(A.form_input(form), A.bias_only_weights(A.C), A.table_case(name), kind, mode)
        _check(f"table {name} {form} mode {mode}", got, ref, emu, kind)


@pytest.mark.parametrize("form", ["smallest", "pair_loop"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_table_qk_driven(form, kind):
    """Logits from q.k (inputs x 8): the emulation-derived row bar only -- the operand rounding
    of a logit of size s moves its probability by s x the kind's epsilon, which the project's
    whole-tensor bars (set at logits a few nats wide) do not allow for."""
    ref, x, w = _qk_reference(form)
    args = (A.windows_of(x, A.WS), w["wqkv"], w["bqkv"], A.dense_bias(w["table"], A.WS), w["wproj"],
            w["bproj"], A.HEADS, A.HD ** -0.5)
    emu = A.attention_fp64(*args, kind=kind, denom="exp" if kind == "bf16x3" else "operand").reshape(-1, A.C)
    for mode in _modes(form):
        got = _table_attend(x, w, w["table"], kind, mode)
        _check(f"table qk_mixed {form} mode {mode}", got, ref, emu, kind, rel_bar=False)


_QK = {}


def _qk_reference(form):
    if form not in _QK:
        _QK.clear()
        x = seeded_randn((1, *A.FORMS[form][1], A.C), 10) * 8.0
        w = A.qk_weights(A.C, A.HEADS)
        ref = A.attention_fp64(A.windows_of(x, A.WS), w["wqkv"], w["bqkv"], A.dense_bias(w["table"], A.WS),
                               w["wproj"], w["bproj"], A.HEADS, A.HD ** -0.5).reshape(-1, A.C)
        _QK[form] = (ref, x, w)
    return _QK[form]


# ---- attn_core_kernel -------------------------------------------------------------------------
GENERAL_PARAMS = [(s[:5], b, k) for s in A.GENERAL_SHAPES for b in A.GENERAL_BIASES for k in s[5]]


def _general_inputs(shape, bname):
    ws, hd, heads, windows, raster = shape
    c, n = hd * heads, ws ** 3
    assert windows * n == raster[0] * raster[1] * raster[2]
    x = seeded_randn((1, *raster, c), 60)
    w = A.bias_only_weights(c)
    bias = A.general_bias(bname, heads, n)
    return x, w, bias, (A.windows_of(x, ws), w["wqkv"], w["bqkv"], bias, w["wproj"], w["bproj"], heads,
                        hd ** -0.5)


@pytest.mark.parametrize("shape,bname,kind", GENERAL_PARAMS)
def test_general_bias_only(shape, bname, kind):
    from waveformer_amd import ops
    ws, hd, heads, windows, raster = shape
    x, w, bias, args = _general_inputs(shape, bname)
    ref = A.attention_fp64(*args, bias_only=True).reshape(-1, hd * heads)
    A.check_rows_not_small(ref)
    emu = A.attention_fp64(*args, kind=kind, denom="exp", bias_only=True).reshape(-1, hd * heads)
    got = ops.window_attention(x.to(DEV), w["wqkv"].to(DEV), w["bqkv"].to(DEV), bias.to(DEV),
                               w["wproj"].to(DEV), w["bproj"].to(DEV), ws, heads, hd ** -0.5,
                               prec=ops.PRECISIONS[kind])
    _check(f"general ws{ws} hd{hd} h{heads} {bname}", got, ref, emu, kind)


def _dense_as_table(bias):
    """(table, index) whose gathered bias is the dense `bias`: one table row per (query, key)."""
    heads, n, _ = bias.shape
    return bias.permute(1, 2, 0).reshape(n * n, heads).contiguous(), torch.arange(n * n).view(n, n)


@pytest.mark.parametrize("shape", [s[:5] for s in A.GENERAL_SHAPES])
@pytest.mark.parametrize("bname", A.GENERAL_BIASES)
def test_general_train_forward_lse(shape, bname):
    from waveformer_amd import library, ops  # noqa: F401  (registers the ops)
    ws, hd, heads, windows, raster = shape
    x, w, bias, args = _general_inputs(shape, bname)
    ref = A.attention_fp64(*args, bias_only=True).reshape(-1, hd * heads)
    emu = A.attention_fp64(*args, kind="bf16x3", denom="exp", bias_only=True).reshape(-1, hd * heads)
    table, index = _dense_as_table(bias)
    got, _, lse = torch.ops.waveformer.window_attn(
        x.to(DEV), None, None, 0.0, w["wqkv"].to(DEV), w["bqkv"].to(DEV), table.to(DEV), index.to(DEV),
        w["wproj"].to(DEV), w["bproj"].to(DEV), ws, heads, hd ** -0.5, ops.PRECISIONS["bf16x3"], True,
        False)
    _check(f"train ws{ws} hd{hd} h{heads} {bname}", got, ref, emu, "bf16x3")
    want = (torch.logsumexp(bias.double(), -1) / math.log(2.0)).expand(windows, heads, ws ** 3)
    lse = lse.cpu().double().view(windows, heads, ws ** 3)
    assert torch.isfinite(lse).all()
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 23)
    excess = ((lse - want).abs() / (4 * ulp + 4e-6)).max().item()
    print(f"attn_softmax lse ws{ws} hd{hd} h{heads} {bname}: max |err| {(lse - want).abs().max():.3e} "
          f"= {excess:.3f} of the bar")
    assert excess <= 1.0


# ---- wf_window_attention_bwd_core on the one-hot bias -------------------------------------------
def _bwd_reference(qkv, bias, dout, heads, scale):
    """(dqkv, dbias, o, lse2) of one window: fp64 autograd of softmax(scale q k^T + bias) v."""
    n, c3 = qkv.shape
    hd = c3 // 3 // heads
    q64 = qkv.double().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    q, k, v = q64.view(n, 3, heads, hd).permute(1, 2, 0, 3)                 # (heads, n, hd)
    S = scale * (q @ k.transpose(-2, -1)) + b64
    o = (S.softmax(-1) @ v).transpose(0, 1).reshape(n, c3 // 3)
    lse2 = (torch.logsumexp(S, -1) / math.log(2.0)).detach()
    dq, db = torch.autograd.grad(o, (q64, b64), dout.double())
    return dq, db, o.detach().float(), lse2.float()


def _bwd_fp32(qkv, bias, dout, o, lse2, heads, scale):
    """The kernel's formulas (train.hip attn_bwd_kernel) in fp32 on the CPU, on what it reads.
    The backward runs on the fp32 VALU: there are no 16-bit operands to round, its number format
    is fp32 throughout, so this -- not an operand rounding -- is the emulation its bar comes
    from (the yardstick test_gpu_train_kernels quotes for test_attention_bwd_core)."""
    n, c3 = qkv.shape
    c = c3 // 3
    hd = c // heads
    q, k, v = qkv.view(n, 3, heads, hd).permute(1, 2, 0, 3)
    g = dout.view(n, heads, hd).transpose(0, 1)
    sl2 = torch.tensor(scale, dtype=torch.float32) * float(A.LOG2E32)
    P = torch.exp2((q @ k.transpose(-2, -1)) * sl2 + A.scaled_bias(bias).float() - lse2[..., None])
    dS = P * (g @ v.transpose(-2, -1) - (g * o.view(n, heads, hd).transpose(0, 1)).sum(-1, keepdim=True))
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-2, -1) @ q), P.transpose(-2, -1) @ g
    return torch.stack([dq, dk, dv]).permute(2, 0, 1, 3).reshape(n, 3 * c), dS


@pytest.mark.parametrize("ws,hd,heads", [(8, 16, 3), (5, 16, 2)])
@pytest.mark.parametrize("bname", ["one_hot_last", "one_hot_soft"])
def test_general_backward_one_hot(ws, hd, heads, bname):
    """One window (its window-major rows are the raster rows), q = 0, the moving one-hot bias.
    dqkv rows (dq | dk | dv of a token) against fp64 autograd under the emulation-derived bar;
    the whole-tensor 1e-5 bar of test_attention_bwd_core is printed, not asserted.

    dbias: at 12 nats (one_hot_soft) its rows get the same row bar.  At 90 nats (one_hot_last)
    the true dbias is below 1e-37 -- every probability off the spike is < 2^-129, and on the
    spike dP - D vanishes -- while any fp32 evaluation leaves the cancellation noise of the two
    length-hd dot products there, so a relative row error is noise over noise.  There dbias must
    instead stay inside that noise: |dbias| <= 2 hd 2^-24 max|dO| max|v| (the first-order fp32
    bound of dP - D at P <= 1)."""
    from waveformer_amd import _lib
    n, c = ws ** 3, hd * heads
    scale = hd ** -0.5
    qkv = seeded_randn((n, 3 * c), 70)
    qkv[:, :c] = 0
    qkv[:, 2 * c:] += 1.0
    dout = seeded_randn((n, c), 71)
    bias = A.general_bias(bname, heads, n)
    want_q, want_b, o, lse2 = _bwd_reference(qkv, bias, dout, heads, scale)
    emu_q, emu_b = _bwd_fp32(qkv, bias, dout, o, lse2, heads, scale)
    wsb = _lib.query("wf_window_attention_bwd_workspace_bytes", 1, c, ws, ws, ws, ws, heads)
    work = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dqkv = torch.full((n, 3 * c), float("nan"), device=DEV)
    dbias = torch.full((heads, n, n), float("nan"), device=DEV)
    dev = [t.contiguous().to(DEV) for t in (qkv, o, dout, bias, lse2)]
    _lib.call("wf_window_attention_bwd_core", *[t.data_ptr() for t in dev], dqkv.data_ptr(),
              dbias.data_ptr(), work.data_ptr(), 1, c, ws, ws, ws, ws, heads, float(scale),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dqkv, dbias = dqkv.cpu(), dbias.cpu()
    assert torch.isfinite(dqkv).all() and torch.isfinite(dbias).all()
    checks = [("dqkv", dqkv, want_q, emu_q)]
    if bname == "one_hot_soft":
        checks.append(("dbias", dbias.view(-1, n), want_b.reshape(-1, n), emu_b.reshape(-1, n)))
    else:
        noise = 2 * hd * 2.0 ** -24 * float(dout.abs().max() * qkv[:, 2 * c:].abs().max())
        print(f"attn_softmax bwd ws{ws} hd{hd} h{heads} {bname} dbias fp32: max |dbias| "
              f"{dbias.abs().max():.3e} (fp64 {want_b.abs().max():.3e}), noise bound {noise:.3e}")
        assert want_b.abs().max() < 1e-30 and dbias.abs().max() <= noise
    for name, got, want, emu in checks:
        bar, e_emu = A.row_bar(emu, want)
        e_row, at = A.row_err(got, want)
        print(f"attn_softmax bwd ws{ws} hd{hd} h{heads} {bname} {name} fp32: emu_row {e_emu:.3e} "
              f"bar {bar:.3e} row {e_row:.3e} (row {at}) rel_l2 {A.rel_l2(got, want):.3e}")
        assert e_row <= bar, f"{name}: row {at} is {e_row:.3e} from fp64, bar {bar:.3e}"
