"""Attention softmax cases at large logits: inputs whose logits are known exactly, the fp64
reference, a CPU emulation of the operand rounding of each kind, an fp32 emulation of the
table kernel's running-max rule, and the per-row metric.  A plain helper module shared by
test_attention_softmax_host.py (CPU) and test_gpu_attention_softmax.py (GPU).

Bias-only inputs: rows [0, C) of qkv.weight and qkv.bias are zero, so q = 0 and every score
is exactly fl32(bias * 1.4426950408889634f) -- the MFMA adds K . 0 to an accumulator that
starts at the bias (table kernel), or 0 * scale + bias (attn_core_kernel).  K and V stay
seeded random (V with bias 1.0, so no output row is near zero), proj is the identity, so an
output row is the token's per-head core outputs.  |bias| <= 96 nats: the fp32 rounding of the
scaled bias then moves a probability by at most 96 log2e 2^-24 ln2 ~ 6e-6 relative.

The table kernel (attn_tbl_kernel, ws 8, head_dim 16) reads the (15^3, heads) table through
the reference's index 23 dz + 15 dy + dx (quirk Q2: depth stride 3 ws - 1, so entries collide
and the table is NOT a function of (dz, dy, dx)); its 547 reachable rows are set, the others
hold NaN.  Key tile t (64 keys) is the window's z slice t, so for the query (qz, qy, qx) it
covers the rows 23 (qz + 7 - t) + 15 qy + qx + {15 a + b : a, b < 8}: later tiles read LOWER
rows.  The tables below are written in that row space; which events a table reaches is not
argued here but counted by running_max_events and pinned in test_attention_softmax_host.py.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import re
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import ref_waveformer as R
from oracle.weight_rule import seeded_randn
from tests.cases import rel_l2  # noqa: F401  (the whole-tensor metric of the project's bars)

KINDS = ("bf16x3", "bf16", "fp16")
REL_L2_BARS = {"bf16x3": 5e-5, "bf16": 1e-2, "fp16": 2e-3}   # the project's existing bars
ROW_FACTOR = 4.0              # per-row bar = ROW_FACTOR x the emulation's worst row ...
ROW_FLOOR = 64 * 2.0 ** -24   # ... and at least this
LOG2E32 = np.float32(1.4426950408889634)
MAX_BIAS = 96.0

TAU = {"bf16x3": 16.0, "bf16": 16.0, "fp16": 15.0}   # the lazy-rescale threshold per kind
TBLN = 547
WS, HD, HEADS, C = 8, 16, 3, 48
N = WS ** 3

# launch form -> (windows, raster, qsplit, NQ)
FORMS = {
    "smallest": (1, (8, 8, 8), 4, 1),
    "pair_loop": (96, (32, 32, 48), 2, 2),     # 288 (window, head)s: NQ = 2 once per wave
    "no_split": (176, (32, 32, 88), 1, 2),     # 528: NQ = 2 twice per wave
}


PLAN_TABLE, PLAN_LN, PLAN_LSE, PLAN_RASTER = 1, 2, 4, 8   # wf_window_attention_plan's flags
MERGED, NO_LEVELS_GEMM, PREFIX, ONE_RASTER = range(4)     # ... and its grouping field


def window_attention_plan(levels, B, C, heads=None, ws=WS, prec=1, flags=PLAN_TABLE, qkv_mode=-1):
    """What the library launches for a window attention call, asked without a launch
    (wf_window_attention_plan; the field order is documented in include/waveformer_hip.h).
    Raises RuntimeError with the library's message where the call would be refused."""
    from waveformer_amd import _lib
    flat = [v for l in levels for v in l]
    f = (ctypes.c_int64 * 32)(*([-7] * 32))
    _lib.call("wf_window_attention_plan", (ctypes.c_int64 * max(1, len(flat)))(*flat), len(levels),
              B, C, C // 16 if heads is None else heads, ws, prec, flags, qkv_mode, f)
    f = list(f)
    n = f[3]
    sets = [dict(zip(("fused", "wh", "qsplit", "pair_windows", "grid"), f[8 + 5 * i:13 + 5 * i]))
            for i in range(n)]
    assert f[7] == 0 and not any(f[8 + 5 * n:28]) and not any(f[28 + len(levels):])
    return {"table": f[0], "head_dim": f[1], "grouping": f[2], "qkv": f[4], "ao": f[5],
            "bytes": f[6], "sets": sets, "nq": f[28:28 + len(levels)]}


def launch_form(wh: int) -> Tuple[int, int]:
    """(qsplit, NQ) of a table-kernel launch over wh (window, head)s: wh one-head windows."""
    p = window_attention_plan([(WS, WS, WS)], wh, HD, flags=PLAN_TABLE | PLAN_RASTER)
    assert p["sets"][0]["wh"] == wh and p["sets"][0]["grid"] == wh * p["sets"][0]["qsplit"]
    return p["sets"][0]["qsplit"], p["nq"][0]


def launch_rule_in_source() -> Dict[str, float]:
    """The lazy-rescale thresholds (arithmetic of the kernel, not dispatch), read from its source."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "waveformer_amd", "csrc")
    with open(os.path.join(csrc, "attention.hip")) as f:
        hip = f.read()
    one = lambda pat, text: re.search(pat, text).group(1)  # noqa: E731
    return {
        "tau": float(one(r"constexpr float kTau = ([0-9.]+)f;", hip)),
        "tau_fp16": float(one(r"constexpr float kTauFp16 = ([0-9.]+)f;", hip)),
    }


# ---- metrics ---------------------------------------------------------------------------------
def row_err(got: torch.Tensor, ref: torch.Tensor) -> Tuple[float, int]:
    """(largest per-row ||got_r - ref_r|| / ||ref_r||, its row); rows = all but the last axis.
    A non-finite row counts as infinitely wrong."""
    g = got.detach().double().cpu().reshape(-1, got.shape[-1])
    r = ref.detach().double().cpu().reshape(-1, ref.shape[-1])
    e = (g - r).norm(dim=1) / r.norm(dim=1)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    i = int(e.argmax())
    return float(e[i]), i


def row_bar(emulated: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(the per-row bar of a case and kind, the emulation's own worst row error)."""
    e, _ = row_err(emulated, ref)
    return max(ROW_FACTOR * e, ROW_FLOOR), e


# ---- operand rounding ------------------------------------------------------------------------
def operand_parts(t: torch.Tensor, kind: str) -> List[torch.Tensor]:
    """t as the MFMA operands of a kind: one fp64 tensor, or bf16x3's [hi, lo]."""
    if kind == "exact":
        return [t.double()]
    f = t.float()
    if kind == "bf16":
        return [f.bfloat16().double()]
    if kind == "fp16":
        return [f.half().double()]
    hi = f.bfloat16().float()
    return [hi.double(), (f - hi).bfloat16().double()]


def mm_parts(a: List[torch.Tensor], b: List[torch.Tensor]) -> torch.Tensor:
    """a @ b in fp64; bf16x3: hi hi + hi lo + lo hi."""
    out = a[0] @ b[0]
    if len(a) == 2:
        out = out + a[0] @ b[1] + a[1] @ b[0]
    return out


def stored(t: torch.Tensor, kind: str) -> torch.Tensor:
    """A GEMM-to-GEMM intermediate as the kind stores it: bf16 for bf16, else fp32."""
    if kind == "exact":
        return t
    return t.float().bfloat16().double() if kind == "bf16" else t.float().double()


def linear_kind(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], kind: str) -> torch.Tensor:
    y = mm_parts(operand_parts(x, kind), [p.transpose(-1, -2) for p in operand_parts(w, kind)])
    return stored(y if b is None else y + b.double(), kind)


def scaled_bias(bias: torch.Tensor, kind: str = "bf16x3") -> torch.Tensor:
    """The exp2-domain bias the kernels add: fl32(bias * log2e) (exact for kind "exact")."""
    if kind == "exact":
        return bias.double() * math.log2(math.e)
    return torch.from_numpy(bias.float().numpy() * LOG2E32).double()


def attention_fp64(xw, wqkv, bqkv, bias, wproj, bproj, heads, scale, kind="exact",
                   denom="exp", bias_only=False, chunk=24, want_lse=False):
    """Window attention over xw (Bw, N, C) with the dense bias (heads, N, N) in nats.

    kind "exact": the fp64 reference softmax(q k^T scale + bias) v, then proj.  Another kind:
    the same with q' = fl32(q scale log2e), q', k, v and P rounded to the kind's operands,
    fp64 accumulation, the exact exp2 against the true row max, the kind's storage of qkv and of
    the core output, and the denominator `denom`: "exp" the sum of the fp32 exponentials,
    "operand" the sum of the rounded P.  Operand rounding only: no tile order, no fp32
    accumulation.  bias_only: q = 0, so the probabilities are computed once per head; else the
    windows go `chunk` at a time (24: an fp64 score tensor of 151 MB at N = 512, 3 heads).
    want_lse: also the row log-sum-exp in the log2 domain, (Bw, heads, N)."""
    Bw, n, c = xw.shape
    hd = c // heads
    exact = kind == "exact"
    qkv = linear_kind(xw.double(), wqkv.double(), None if bqkv is None else bqkv, kind)
    q, k, v = qkv.view(Bw, n, 3, heads, hd).permute(2, 0, 3, 1, 4)      # (Bw, heads, n, hd)
    sb = scaled_bias(bias, kind)
    if exact:
        qs = q * (scale * math.log2(math.e))
    else:
        sl2 = float(np.float32(scale) * LOG2E32)
        qs = (stored(q, kind) * sl2).float().double()
    if bias_only:
        assert not q.any(), "bias_only: the q rows of the weight and bias must be zero"
    out = torch.empty(Bw, n, c, dtype=torch.float64)
    lse = torch.empty(Bw, heads, n, dtype=torch.float64)
    step = Bw if bias_only else chunk
    for w0 in range(0, Bw, step):
        vv = v[w0:w0 + step]
        nb = vv.shape[0]
        if bias_only:
            S = sb                                                     # (heads, n, n)
        else:
            S = mm_parts(operand_parts(qs[w0:w0 + step], kind),
                         [p.transpose(-1, -2) for p in operand_parts(k[w0:w0 + step], kind)]) + sb
        m = S.amax(-1, keepdim=True)
        P = torch.exp2(S - m)
        pe = P if exact else P.float().double()
        pp = operand_parts(pe, kind)
        l = (pe if denom == "exp" or exact else sum(pp)).sum(-1, keepdim=True)
        if bias_only:   # (heads, n, n) @ (heads, n, nb * hd)
            vp = [p.permute(1, 2, 0, 3).reshape(heads, n, nb * hd) for p in operand_parts(vv, kind)]
            o = (mm_parts(pp, vp) / l).view(heads, n, nb, hd).permute(2, 0, 1, 3)
        else:
            o = mm_parts(pp, operand_parts(vv, kind)) / l
        lse[w0:w0 + step] = (m + torch.log2(pe.sum(-1, keepdim=True)))[..., 0]
        out[w0:w0 + step] = stored(o.transpose(1, 2).reshape(nb, n, c), kind)
    res = linear_kind(out, wproj.double(), bproj, kind)
    return (res, lse) if want_lse else res


# ---- inputs ----------------------------------------------------------------------------------
def bias_only_weights(c: int, seed: int = 500) -> Dict[str, torch.Tensor]:
    """q rows zero, K / V seeded random, V bias 1.0, proj the identity."""
    wqkv = seeded_randn((3 * c, c), seed + 1) * 0.1
    bqkv = seeded_randn((3 * c,), seed + 2) * 0.1
    wqkv[:c] = 0
    bqkv[:c] = 0
    bqkv[2 * c:] += 1.0
    return dict(wqkv=wqkv, bqkv=bqkv, wproj=torch.eye(c), bproj=torch.zeros(c))


def qk_weights(c: int, heads: int, seed: int = 100) -> Dict[str, torch.Tensor]:
    """The weights of the bitwise tests' `mixed` case (test_gpu_attention_fused_qkv._weights)."""
    g = lambda shape, s, scale: seeded_randn(shape, seed + s) * scale  # noqa: E731
    return dict(wqkv=g((3 * c, c), 1, 0.1), bqkv=g((3 * c,), 2, 0.1), table=g((15 ** 3, heads), 3, 0.5),
                wproj=g((c, c), 4, 0.1), bproj=g((c,), 5, 0.1))


def windows_of(x: torch.Tensor, ws: int) -> torch.Tensor:
    """(B, D, H, W, C) -> (windows, ws^3, C) in the order of the op's output rows."""
    return R.window_partition(x, ws).reshape(-1, ws ** 3, x.shape[-1])


def dense_bias(table: torch.Tensor, ws: int) -> torch.Tensor:
    """(heads, N, N) from the (rows, heads) table through the oracle's relative_position_index."""
    idx = R.relative_position_index(ws)
    n = ws ** 3
    return table[idx.reshape(-1)].reshape(n, n, -1).permute(2, 0, 1).contiguous()


def _table(fn) -> torch.Tensor:
    """(15^3, heads): column h is fn(h) on the 547 reachable rows, NaN on the others."""
    t = torch.full((15 ** 3, HEADS), float("nan"))
    for h in range(HEADS):
        t[:TBLN, h] = torch.as_tensor(fn(h), dtype=torch.float32)
    assert torch.isfinite(t[:TBLN]).all() and t[:TBLN].abs().max() <= MAX_BIAS
    return t


_I = np.arange(TBLN, dtype=np.float64)
F16_BAND_B = 11.0902   # fl32(b log2e) = 15.9998: exp2 of it is 65526 > 65520, inf as an fp16


def _spikes(base, at):
    def fn(h):
        v = np.full(TBLN, float(base))
        for i, val in at:
            v[i + 7 * h] = val
        return v
    return fn


# name -> (table, the events (a)-(d) the case claims at tau = 16, the forms it runs in)
ALL_FORMS = ("smallest", "pair_loop", "no_split")
TABLE_CASES = {
    # 23 rows down per tile x 0.49 .. 0.5 nats x log2e > 16: every tile raises the max past tau
    "ladder_up": (lambda: _table(lambda h: 96 - (0.5 - 0.005 * h) * np.minimum(_I, 384)), "a", ALL_FORMS),
    # 11.4 .. 11.7 per tile: a kept tile with exponentials near 2^12, then a rescale
    "ladder_keep": (lambda: _table(lambda h: 95.8 - (0.345 + 0.003 * h) * _I), "ab", ALL_FORMS),
    # the first tile holds the max: no rescale after it, later exponentials underflow
    "ladder_down": (lambda: _table(lambda h: -95.8 + (0.345 + 0.003 * h) * _I), "", ALL_FORMS),
    # row 20 (+ 7 h) is reached by the queries qz = 0, qy <= 1 only, in tile 7
    "one_hot_last": (lambda: _table(_spikes(-45, [(20, 45)])), "a", ALL_FORMS),
    # spikes of rising height at falling rows: sub-tile st meets each two tiles before st + 8
    "pair_split": (lambda: _table(_spikes(-40, [(400, -20), (250, 0), (100, 20), (20, 40)])), "ac",
                   ("pair_loop", "no_split")),
    "flat_low": (lambda: _table(lambda h: np.full(TBLN, -90.0)), "", ALL_FORMS),
    # one entry 15.9998 above a flat 0 (exp2 domain): kept, and 65526 as an fp16 is inf
    "f16_band": (lambda: _table(_spikes(0, [(100, F16_BAND_B)])), "d", ALL_FORMS),
}


@functools.lru_cache(maxsize=None)
def table_case(name: str) -> torch.Tensor:
    return TABLE_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def table_dense(name: str) -> torch.Tensor:
    return dense_bias(table_case(name), WS)


@functools.lru_cache(maxsize=2)
def form_input(form: str) -> torch.Tensor:
    return seeded_randn((1, *FORMS[form][1], C), 40)


def check_rows_not_small(ref: torch.Tensor) -> None:
    nrm = ref.reshape(-1, ref.shape[-1]).norm(dim=1)
    assert nrm.min() >= 0.1 * nrm.median(), (float(nrm.min()), float(nrm.median()))


@functools.lru_cache(maxsize=4)
def table_reference(name: str, form: str) -> torch.Tensor:
    """fp64 reference rows (windows * 512, C) of a bias-only table case in a launch form."""
    w = bias_only_weights(C)
    ref = attention_fp64(windows_of(form_input(form), WS), w["wqkv"], w["bqkv"], table_dense(name),
                         w["wproj"], w["bproj"], HEADS, HD ** -0.5, bias_only=True).reshape(-1, C)
    check_rows_not_small(ref)
    return ref


def table_emulation(name: str, form: str, kind: str) -> torch.Tensor:
    w = bias_only_weights(C)
    return attention_fp64(windows_of(form_input(form), WS), w["wqkv"], w["bqkv"], table_dense(name),
                          w["wproj"], w["bproj"], HEADS, HD ** -0.5, kind=kind,
                          denom="exp" if kind == "bf16x3" else "operand", bias_only=True).reshape(-1, C)


# ---- the running-max rule of attn_tbl_tiles, in fp32 ------------------------------------------
def running_max_events(sb: torch.Tensor, qsplit: int, nq: int, tau: float = 16.0) -> Dict[str, int]:
    """Bias-only cases: sb is the dense scaled bias (heads, 512, 512) the kernel's scores equal.
    A group is the 16 queries of a sub-tile (NQ = 1) or the 32 of sub-tiles st and st + 8 of the
    workgroup's query range (NQ = 2).  At each 64-key tile the group rescales iff any of its
    queries has a tile max > mrun + tau; each query then sets mrun = max(mrun, own tile max).
    Counts, over heads, groups and tiles:
      a  tiles after the first that rescale
      b  kept tiles whose largest s - mrun is > 8
      c  NQ = 2 rescales where only one of the two sub-tiles asked
      d  scores with s - mrun in [15.99965, 16] on a kept tile"""
    s = sb.float().numpy().astype(np.float32)
    heads, n, _ = s.shape
    nsub = n // 16 // qsplit
    groups = []
    for part in range(qsplit):
        for st in range(nsub):
            if nq == 1:
                groups.append([part * nsub + st])
            elif st % 16 < 8:
                groups.append([part * nsub + st, part * nsub + st + 8])
    assert sorted(t for g in groups for t in g) == list(range(n // 16))
    ev = dict(a=0, b=0, c=0, d=0)
    tau32 = np.float32(tau)
    for h in range(heads):
        for g in groups:
            q = np.concatenate([np.arange(16 * t, 16 * t + 16) for t in g])
            mrun = np.full(len(q), -np.inf, dtype=np.float32)
            for t in range(n // 64):
                tile = s[h][q, 64 * t:64 * t + 64]
                tmax = tile.max(axis=1)
                ask = tmax > mrun + tau32
                if ask.any():
                    ev["a"] += t > 0
                    if nq == 2 and ask[:16].any() != ask[16:].any():
                        ev["c"] += 1
                    mrun = np.maximum(mrun, tmax)
                else:
                    gap = tile - mrun[:, None]
                    ev["b"] += bool(gap.max() > 8)
                    ev["d"] += int(((gap >= np.float32(15.99965)) & (gap <= 16)).sum())
    return {k: int(v) for k, v in ev.items()}


# ---- the general kernel (attn_core_kernel): dense bias, bias-only ------------------------------
# (ws, head_dim, heads, windows, raster, kinds)
GENERAL_SHAPES = [
    (2, 64, 1, 3, (2, 2, 6), KINDS),               # N = 8, far below one tile
    (3, 48, 2, 2, (3, 6, 3), KINDS),               # N = 27
    (5, 16, 2, 1, (5, 5, 5), ("bf16x3",)),         # N = 125: partial second tile
    (4, 32, 2, 2, (4, 4, 8), ("bf16x3",)),         # N = 64 exactly
    (8, 16, 3, 1, (8, 8, 8), ("bf16x3",)),         # N = 512
    (12, 16, 3, 1, (12, 12, 12), ("bf16x3",)),     # N = 1728: 27 tiles
]
GENERAL_BIASES = ("ladder_up", "ladder_down", "one_hot_last", "last_valid_key")


@functools.lru_cache(maxsize=2)
def general_bias(name: str, heads: int, n: int) -> torch.Tensor:
    """Dense (heads, n, n) bias, |.| <= 96, rows differing per query and head."""
    key = torch.arange(n, dtype=torch.float64)
    qi = torch.arange(n, dtype=torch.float64)[:, None]
    hh = torch.arange(heads, dtype=torch.float64)[:, None, None]
    if name in ("ladder_up", "ladder_down"):
        # 192 nats over the row, rotated by the query so every key position takes every rung:
        # per 64-key tile the max rises by 64 * 192 / n nats (> 16 log2 up to N = 512)
        ramp = ((key[None] + 3 * qi + 5 * hh) % n) / max(n - 1, 1)
        b = (ramp * 192 - 96) * (1 if name == "ladder_up" else -1)
        if name == "ladder_up":   # plain rise for the first queries: a rescale at every tile
            b[:, :4] = (key / max(n - 1, 1) * 192 - 96)
    else:
        # one_hot_soft (the backward): 12 nats, so the gradients of the other keys are not 0
        amp = 6.0 if name == "one_hot_soft" else 45.0
        b = torch.full((heads, n, n), -amp, dtype=torch.float64) + 0.25 * torch.sin(key + qi + hh)
        if name != "last_valid_key":    # the spike moves with the query; query 0: the last key
            spike = (n - 1 - 7 * torch.arange(n) - torch.arange(heads)[:, None]) % n
        else:                           # the row's only large logit on the last valid key
            spike = torch.full((heads, n), n - 1)
        b.scatter_(2, spike.reshape(heads, n, 1), amp)
    b = b.float()
    assert b.abs().max() <= MAX_BIAS
    return b
