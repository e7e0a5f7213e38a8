"""CPU: the helpers behind test_gpu_attention_softmax.py (tests/attention_cases.py).

 * The operand-rounding emulation with no rounding IS the fp64 reference (1e-12), on a q.k-driven
   input and on a bias-only one (the shared-probability shortcut against the per-window path).
 * The launch rule the cases are built for is the one the library follows, asked of it without a
   launch (wf_window_attention_plan): the split over 4 / 2 / 1 workgroups with its boundaries at
   256 and 512 (window, head)s and the tile loop each takes; and the lazy-rescale thresholds are
   the ones in the kernel source.
 * Every bias-only table case reaches, in every launch form it runs in, each event it claims
   (running_max_events, an fp32 emulation of attn_tbl_tiles' running-max rule alone):
     a  a tile after the first rescales            b  a kept tile with s - mrun > 8
     c  an NQ = 2 rescale only one sub-tile asked  d  a kept score in [mrun + 15.99965, mrun + 16]
   so a case cannot silently lose its branch when a table or the launch rule changes.  (d) is
   the fp16 overflow band: only f16_band may reach it, and only at the threshold 16 -- at fp16's
   own threshold (15) the band rescales instead.
Host only, no GPU."""
import numpy as np
import pytest
import torch

from oracle import ref_waveformer as R
from oracle.weight_rule import seeded_randn
from tests import attention_cases as A


def test_launch_rule_matches_the_source():
    src = A.launch_rule_in_source()
    assert src == {"tau": A.TAU["bf16x3"], "tau_fp16": A.TAU["fp16"]}
    assert A.TAU["bf16"] == A.TAU["bf16x3"]
    assert len(A.FORMS) == 3
    for form, (windows, raster, qsplit, nq) in A.FORMS.items():
        assert windows * A.N == raster[0] * raster[1] * raster[2]
        assert A.launch_form(windows * A.HEADS) == (qsplit, nq), form
    # the thresholds themselves
    assert A.launch_form(255) == (4, 1) and A.launch_form(256) == (2, 2)
    assert A.launch_form(511) == (2, 2) and A.launch_form(512) == (1, 2)


def test_f16_band_entry_is_in_the_band():
    sb = float(np.float32(A.F16_BAND_B) * A.LOG2E32)
    assert 15.9997 <= sb <= 15.99995
    assert torch.tensor(2.0 ** sb).half().isinf()                       # the fp16 operand
    assert torch.tensor(2.0 ** A.TAU["fp16"]).half().isfinite()
    assert torch.tensor(2.0 ** sb).bfloat16().isfinite()


def test_exact_kind_is_the_reference_qk():
    """Emulation with no rounding against the oracle's attention (fp64), chunked over windows."""
    w = A.qk_weights(A.C, A.HEADS)
    x = seeded_randn((3, A.N, A.C), 7).double() * 8.0
    sd = {"qkv.weight": w["wqkv"].double(), "qkv.bias": w["bqkv"].double(),
          "relative_position_bias_table": w["table"].double(),
          "relative_position_index": R.relative_position_index(A.WS),
          "proj.weight": w["wproj"].double(), "proj.bias": w["bproj"].double()}
    ref = R.attention(sd, "", x, A.HEADS, A.WS)
    got = A.attention_fp64(x, w["wqkv"], w["bqkv"], A.dense_bias(w["table"], A.WS), w["wproj"],
                           w["bproj"], A.HEADS, A.HD ** -0.5, chunk=2)
    assert A.rel_l2(got, ref) <= 1e-12 and A.row_err(got, ref)[0] <= 1e-12


@pytest.mark.parametrize("name", ["ladder_keep", "one_hot_last"])
def test_exact_kind_is_the_reference_bias_only(name):
    """The once-per-head probabilities of a bias-only case against the oracle's attention, and
    the per-window path of the emulation against the shortcut."""
    w = A.bias_only_weights(A.C)
    x = seeded_randn((2, A.N, A.C), 8).double()
    table = A.table_case(name).double()
    sd = {"qkv.weight": w["wqkv"].double(), "qkv.bias": w["bqkv"].double(),
          "relative_position_bias_table": torch.nan_to_num(table),
          "relative_position_index": R.relative_position_index(A.WS),
          "proj.weight": w["wproj"].double(), "proj.bias": w["bproj"].double()}
    ref = R.attention(sd, "", x, A.HEADS, A.WS)
    args = (x, w["wqkv"], w["bqkv"], A.table_dense(name), w["wproj"], w["bproj"], A.HEADS,
            A.HD ** -0.5)
    got, lse = A.attention_fp64(*args, bias_only=True, want_lse=True)
    assert torch.isfinite(got).all()
    assert A.rel_l2(got, ref) <= 1e-12 and A.row_err(got, ref)[0] <= 1e-12
    want = torch.logsumexp(A.table_dense(name).double(), -1) / np.log(2.0)
    assert (lse - want).abs().max() <= 1e-9
    for kind in A.KINDS:
        a = A.attention_fp64(*args, kind=kind, denom="operand", bias_only=True)
        b = A.attention_fp64(*args, kind=kind, denom="operand", bias_only=False, chunk=1)
        assert (a - b).abs().max() <= 1e-12, kind    # fp64 summation order only


def test_row_err_finds_the_one_wrong_row():
    ref = seeded_randn((1000, 48), 9).double() + 1.0
    got = ref.clone()
    got[617] *= 1.01
    e, i = A.row_err(got, ref)
    assert i == 617 and abs(e - 0.01) < 1e-12
    assert A.rel_l2(got, ref) < 1e-3            # the whole-tensor metric barely sees it
    got[3, 5] = float("nan")
    assert A.row_err(got, ref) == (float("inf"), 3)


EVENT_CASES = [(n, f) for n, (_, _, forms) in A.TABLE_CASES.items() for f in forms]


@pytest.mark.parametrize("name,form", EVENT_CASES)
def test_table_case_reaches_its_events(name, form):
    _, claims, _ = A.TABLE_CASES[name]
    table = A.table_case(name)
    assert torch.isnan(table[A.TBLN:]).all()          # only the reachable rows are set
    dense = A.table_dense(name)
    assert torch.isfinite(dense).all() and dense.abs().max() <= A.MAX_BIAS
    sb = A.scaled_bias(dense)
    _, _, qsplit, nq = A.FORMS[form]
    ev = A.running_max_events(sb, qsplit, nq, tau=A.TAU["bf16x3"])
    print(f"{name} {form} tau 16: {ev}")
    for k in "abcd":
        if k in claims and not (k == "c" and nq == 1):
            assert ev[k] > 0, (k, ev)
    if "d" not in claims:
        assert ev["d"] == 0, ev
    if name in ("ladder_down", "flat_low"):
        assert ev["a"] == 0, ev                       # the first tile holds the max
    if name == "ladder_up":                           # most (head, group, tile)s rescale
        groups = A.HEADS * (A.N // 16 // nq)
        assert ev["a"] >= 0.6 * 7 * groups, ev
    ev15 = A.running_max_events(sb, qsplit, nq, tau=A.TAU["fp16"])
    print(f"{name} {form} tau 15: {ev15}")
    assert ev15["d"] == 0, ev15
    for k in "abc":
        if k in claims and not (k == "c" and nq == 1):
            assert ev15[k] > 0, (k, ev15)
    if name == "f16_band":
        # every tile that was kept with a band score now rescales
        assert ev["a"] == 0 and ev15["a"] > 0 and ev15["b"] == 0, (ev, ev15)
        # ... and some query first meets the entry after its first tile
        tmax = sb[0].view(A.N, 8, 64).amax(-1)
        assert ((tmax[:, 0] < 1) & (tmax.amax(1) > 15)).any()
