#!/usr/bin/env python3
"""bench.py -- WaveFormer encoder forward on MI355X (BASELINE.json configs[1]).

    python bench.py [--gpus N --steps K --warmup W --batch B --precision bf16x3|bf16|fp16]
                    [--dump-outputs DIR] [--full]
    python bench.py --workload full --img 192 --precision fp16    (config 5)

One step = one MultiscaleTransformer forward (PatchEmbed -> 4 stages of DWT / window
attention / multi-scale fuse / CCF_FFN / PatchMerging -> proj_out; network_models/waveformer.py
:260-322) over a batch of B synthetic 128^3 x 4 crops already resident in HBM, on the
waveformer_amd HIP kernels.  N > 1 (launched by torch.distributed.run, one process per GPU)
runs N independent replicas -- 128^3 crops do not shard -- and reports the
whole-job rate: B * K * N volumes / the slowest rank's wall time.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps (ms_per_step =
the timed region / K) and prints the line.  --dump-outputs DIR also writes what the last timed
step returned (rank 0's; for the encoder its 4 stage outputs and their detail bands) as
DIR/<name>.npy, float32, at most 64 MB in all; inputs and weights are seeded, so two builds
run with the same arguments are comparable array for array.  With --full the line also carries:
  roofline     : the dominant kernel of the step (the CCF_FFN depthwise conv): its algorithmic
                 bytes per launch / its average launch duration, timed with HIP events on the
                 launch stream (eager repeats of the step after the timed region), against the
                 8 TB/s HBM3E peak (traffic: PMC bytes per launch from profiles/*pmc*.json when
                 present, else null)
  rooflines    : the same for the DWT (north-star HBM target), the multi-scale fuse, and the
                 window attention op (MFMA-bound: algorithmic FLOPs vs the dense bf16 peak)
  cpu_baseline : the oracle (CPU restatement of the reference, fp32 PyTorch) timed on this
                 host on one volume (rank 0, N = 1 only)
  parity       : Dice (TC/WT/ET) of the full Waveformer's labels at 128^3 x 4 against the
                 reference's own labels (tests/golden), run outside the timed region
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

METRIC = "128³×4 volumes/sec fwd (1/2/4/8 MI355X) + Dice Δ vs reference"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, MI355X_MICROARCH.md chip table (spec)
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA (no sparsity)
# bench op name -> regular expression over the kernel names of the PMC summary
# (profiles/*pmc*.json).  The Haar forward's template is <G, V, LN, BANDS>: the 8-band launch
# (dwt3d_haar) and the LL-only one (dwt3d_haar_ll, the Blocks whose detail bands the encoder
# drops) are different instantiations and must not be confused (a
# substring match returned the LL-only kernel's 453 MB for the 805 MB 8-band launch).
PMC_KERNEL = {"ccf_ffn_dwconv": "ffn_fused_kernel" if os.environ.get("WF_FFN_FUSED")
              else "ffn_dwfc_kernel" if os.environ.get("WF_FFN_DWFC_CLASSIC")
              else "ffn_dwfc_ws_kernel" if os.environ.get("WF_FFN_DWFC_WS")
              else "ffn_dwfc_sb_kernel" if os.environ.get("WF_FFN_DWFC_SB")
              else "ffn_dwfc_tb_kernel" if os.environ.get("WF_FFN_DWFC_TB", "4") == "1"
              else "ffn_dwfc_tb4_kernel",
              "dwt3d_haar": r"dwt3d_haar_fwd_kernel<\d+, \d+, (true|false), 8>",
              "dwt3d_haar_ll": r"dwt3d_haar_fwd_kernel<\d+, \d+, (true|false), 1>",
              "window_attention": "attn_tbl_kernel",
              "msfuse": "msfuse", "proj_out": "proj_out"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default: enough for a >= 2 s timed region -- encoder 250, "
                         "full 40, sliding / train 20)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps (default 10 / 3)")
    ap.add_argument("--batch", type=int, default=None,
                    help="volumes per GPU per step (default: 8 for encoder, 1 for train)")
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "bf16", "fp16"])
    ap.add_argument("--graph", type=int, default=1, help="replay the step as a HIP graph")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline figure does not "
                         "need: the per-op rooflines, the Dice parity against the reference's "
                         "labels and the CPU baseline (each can be switched off below).  Without "
                         "it the run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy (float32; "
                         "rank 0's; at most 64 MB in all -- a fixed seeded sample of the elements "
                         "of larger outputs)")
    ap.add_argument("--roofline-op", default="auto")
    ap.add_argument("--cpu-baseline", type=int, default=1, help="with --full: 0 skips it")
    ap.add_argument("--parity", type=int, default=1, help="with --full: 0 skips it")
    ap.add_argument("--op-timers", type=int, default=1,
                    help="with --full: 0 skips the per-op roofline timing after the timed region "
                         "(a rocprof trace then holds the warm-up and the graph replays only)")
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--workload", default="encoder",
                    choices=["encoder", "full", "sliding", "train"],
                    help="encoder: config 2 (the driver's line); full: the whole Waveformer "
                         "forward (with --img 192 --precision fp16: config 5, HF refinement "
                         "branch on, Dice vs the reference's 192^3 labels); sliding: config 3, one "
                         "240x240x155x4 case through the full Waveformer with the windows "
                         "sharded over the ranks and all-gathered over RCCL; train: config 4, "
                         "fwd + DiceCE + bwd + clip + AdamW of the full Waveformer, DDP")
    ap.add_argument("--tta", type=int, default=0, help="sliding: 8-way flip TTA")
    ap.add_argument("--exchange", default="allgather", choices=["allgather", "allreduce"],
                    help="sliding: per-round all-gather of window logits + stitch on every rank,"
                         " or each rank's partial stitch + one all-reduce (SURVEY 8e)")
    ap.add_argument("--miopen-find", type=int, default=0,
                    help="train: cudnn.benchmark (MIOpen find); no convolution of the step runs "
                         "on MIOpen any more (autograd.conv_train), so it only matters for "
                         "non-default module shapes")
    args = ap.parse_args()
    if args.batch is None:
        # encoder: B = 8 is the top of SURVEY 8d's C2 range {1, 2, 4, 8} and fills the 8^3 / 16^3
        # stages better than 4 (902 vs 794 volumes/s measured); train: config 4's B = 4 / GPU
        args.batch = {"train": 4, "full": 2}.get(args.workload, 8)
    if args.steps is None:
        args.steps = {"encoder": 250, "full": 40}.get(args.workload, 20)
    if args.warmup is None:
        args.warmup = 10 if args.workload == "encoder" else 3
    if not args.full:  # a plain run: only what the headline figure needs
        args.cpu_baseline = args.parity = args.op_timers = 0
    return args


# ------------------------------------------------------------------------------------------
# --dump-outputs: the arrays the timed path returned in its last step
# ------------------------------------------------------------------------------------------
DUMP_BUDGET_BYTES = 60 * 10 ** 6  # of array data: with the .npy headers well within 64 MB
DUMP_SEED = 20240607


def named_outputs(out, prefix="out"):
    """Flatten what a step returned (a tensor, or tuples / lists / dicts of them) into
    [(name, tensor)] with names that spell the path: out0, hf1_0_aad, ...  The encoder's
    (outs, hfs) pair becomes out<stage> and hf<stage>_<level>_<band>."""
    if torch.is_tensor(out):
        return [(prefix, out)]
    res = []
    if isinstance(out, dict):
        for k in sorted(out):
            res += named_outputs(out[k], f"{prefix}_{k}")
    elif isinstance(out, (tuple, list)):
        for i, v in enumerate(out):
            res += named_outputs(v, f"{prefix}{i}" if prefix[-1:].isalpha() else f"{prefix}_{i}")
    return res  # None and other non-tensor leaves carry no array


def dump_outputs(dirname, out):
    """Write every tensor of `out` as <dirname>/<name>.npy in float32.  All of them together stay
    under DUMP_BUDGET_BYTES: the budget is split evenly over the tensors, a tensor within its
    share is written whole (its own shape), a larger one as the 1-D array of its elements at
    share / 4 flat indices drawn once from a CPU generator seeded with DUMP_SEED and the
    tensor's position and size -- the same indices for the same arguments, whatever build."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    if isinstance(out, tuple) and len(out) == 2 and isinstance(out[0], (tuple, list)):
        items = named_outputs(out[0], "out") + named_outputs(out[1], "hf")  # encoder (outs, hfs)
    else:
        items = named_outputs(out, "out")
    share = DUMP_BUDGET_BYTES // max(1, len(items)) // 4  # float32 elements per tensor
    written = {}
    for pos, (name, t) in enumerate(items):
        t = t.detach()
        if t.numel() > share:
            g = torch.Generator().manual_seed(DUMP_SEED + 1000003 * pos + t.numel() % 1000003)
            idx = torch.randint(0, t.numel(), (share,), generator=g).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        a = t.float().cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), a)
        written[name] = list(a.shape)
    return written


# ------------------------------------------------------------------------------------------
# per-launch timing of one op with HIP events on its stream
# ------------------------------------------------------------------------------------------
def _stage1(a):
    """ops.ccf_ffn_dwconv(args, positions, hidden) of the stage-1 shape (args[20] = C = 48,
    hidden 192): stage 2 is ffn_dwfc.hip (dwconv + LN2 + GELU + fc + residual), or with
    WF_FFN_FUSED=1 the whole CCF_FFN in one kernel (ffn_fused.hip)."""
    return a[0][20] == 48 and a[2] == 192


def _dw_bytes(a, kw, out):
    """CCF_FFN stage 2.  Stage 1 (C 48 / hidden 192): ffn_dwfc reads h1 (fp32 for bf16x3, bf16
    for bf16) + the residual rows x and their norm2 stats, writes out; the whole-FFN kernel
    reads x + stats and writes out (h1 / h2 stay on chip).  Other stages: read h1 + write h2 +
    the (mean, M2) partial per 32 channels of every position."""
    from waveformer_amd import ops
    P, Hd = a[1], a[2]
    e = 2 if ops.get_precision() == "bf16" else 4  # bf16x3 / fp16 keep fp32 intermediates
    if _stage1(a):
        C = a[0][20]
        io = 2 * P * C * 4 + (P * 8 if a[0][1] else 0)
        return io if os.environ.get("WF_FFN_FUSED") else io + P * Hd * e
    return 2 * P * Hd * e + P * (Hd // 32) * 8


def _attn_flops(a, kw, out):
    """window attention: qkv (2*T*C*3C) + QK^T and PV (2 * 2*T*N*C) + proj (2*T*C*C)."""
    x = a[0]
    T, C = x.numel() // x.shape[-1], x.shape[-1]
    N = a[6] ** 3
    return 2 * T * C * 3 * C + 4 * T * N * C + 2 * T * C * C


def _dwt_grid(a, kw, out):
    """Work-items of the Haar forward's launch on x = a[0] (dwt_haar_fwd in csrc/dwt.hip): one
    row group of G lanes per output position, at most 8192 workgroups of 256 (grid-stride)."""
    B, D, H, W, C = a[0].shape
    c4 = C // 4
    if C == 48:
        G = 16
    elif c4 % 3 == 0 and c4 // 3 in (1, 2, 4, 8, 16, 32, 64):
        G = c4 // 3
    else:
        G = min(64, 1 << max(0, (c4 - 1).bit_length()))
    total = B * D * H * W // 8
    return min(-(-total // (256 // G)), 8192) * 256


def _live_rows(a):
    """sliding_window_stitch(patches, map, starts, image_size, batch, ...): the number of real
    windows (the padded slots of the gathered buffer are never read)."""
    st, batch = a[2], a[4]
    return batch * len(st[0]) * len(st[1]) * len(st[2])


class OpTimer:
    """Wraps waveformer_amd.ops.<name>; records (algorithmic bytes or flops, start, end, reps)
    with HIP events on the current (= launch) stream.

    Each wrapped call first runs the op once untimed, then records the start event and
    re-issues the same (idempotent) launch REPS times before the end event.  The GPU is still
    busy with the untimed launch when the start event is queued, and the host enqueues the
    repeats faster than they run.  So the interval covers REPS back-to-back kernel executions
    and no host launch latency, and it matches the rocprofv3 kernel-trace durations."""

    REPS = 4

    WORK = {
        # CCF_FFN depthwise 3^3 conv (the step's dominant kernel)
        "ccf_ffn_dwconv": _dw_bytes,
        # 1-level Haar: read the (B,D,H,W,C) input once, write 8 bands of 1/8 size
        "dwt3d_haar": lambda a, kw, out: 2 * a[0].numel() * 4,
        # its LL band alone: read the input once, write 1/8 of it
        "dwt3d_haar_ll": lambda a, kw, out: a[0].numel() * 4 + out.numel() * 4,
        # out = shortcut + sum trilinear(src): read shortcut + sources, write out + 8 B stats/row
        "msfuse": lambda a, kw, out: (2 * a[1].numel() + sum(s.numel() for s in a[0])) * 4
        + (0 if out[1] is None else out[1].numel() * 4),
        # LN + transpose: read + write
        "proj_out": lambda a, kw, out: 2 * a[0].numel() * 4,
        # windowed attention (qkv GEMM + core + proj GEMM), FLOPs
        "window_attention": _attn_flops,
        # decoder 3x3x3 convolution (config 3's dominant kernel), FLOPs: 2 * 27 * Cin * Cout
        # per output position
        "conv3d_k3": lambda a, kw, out: 2 * 27 * a[0].shape[1] * a[1].shape[0] * a[0].shape[0]
        * a[0].shape[2] * a[0].shape[3] * a[0].shape[4],
        # config 3 stitch: read every window's logits once, write the (B, C, D, H, W) output
        "sliding_window_stitch": lambda a, kw, out: (a[0][:_live_rows(a)].numel()
                                                     + out.numel()) * 4,
    }

    # launch size (work-items) of the timed launch, for the per-shape PMC lookup
    GRID = {"dwt3d_haar": _dwt_grid, "dwt3d_haar_ll": _dwt_grid}

    def __init__(self, name):
        from waveformer_amd import ops
        self.ops, self.name = ops, name
        self.orig = getattr(ops, name)
        self.rec = []
        self.active = False

        def wrapped(*a, **kw):
            if not self.active:
                return self.orig(*a, **kw)
            out = self.orig(*a, **kw)
            # MFMA operand precision of this launch (the fp16 policy keeps attention and the
            # skip-feature convolutions at bf16x3): 3 issued MFMAs per product for bf16x3
            prec = kw.get("prec") if name == "window_attention" else None
            if prec is None:
                prec = self.ops.prec_id()
            issue = 3 if prec == self.ops.PRECISIONS["bf16x3"] else 1
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(self.REPS):
                self.orig(*a, **kw)
            e.record()
            grid = self.GRID[name](a, kw, out) if name in self.GRID else None
            self.rec.append((self.WORK[name](a, kw, out), s, e, issue, grid))
            return out

        setattr(ops, name, wrapped)
        # the network_models modules import `ops` as a module, so the patch is visible to them

    def summary(self):
        """The largest launch class (max work per launch): its work, mean duration and rate."""
        torch.cuda.synchronize()
        if not self.rec:
            return None
        big = max(r[0] for r in self.rec)
        sel = [(b, s.elapsed_time(e) / self.REPS, i, gr) for b, s, e, i, gr in self.rec if b == big]
        avg_ms = sum(t for _, t, _, _ in sel) / len(sel)
        return {"work_per_launch": big, "avg_ms": avg_ms, "launches": len(sel),
                "rate": big / (avg_ms * 1e-3), "issue": max(i for _, _, i, _ in sel),
                "grid": sel[0][3]}


def pmc_traffic(kernel_re, batch, grid=None):
    """HBM bytes per launch from the newest profiles/*pmc*.json written by tools/pmc_traffic.py
    whose PMC passes ran at this per-GPU batch (summaries without the field were taken at 4);
    None when no summary matches.  `kernel_re` is searched in the kernel names; over every
    matching kernel, the largest launch's bytes (the op timers time the largest launch class),
    or with `grid` (the timed launch's size in work-items) the entry of that launch shape."""
    import re
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "*pmc*.json")), reverse=True)
    for f in files:
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if "kernels" not in d or d.get("per_gpu_batch", 4) != batch:
            continue
        hits = [v for k, v in d["kernels"].items() if re.search(kernel_re, k)]
        if grid is not None:
            vals = [v.get("by_grid", {}).get(str(grid), {}).get("hbm_bytes_per_launch")
                    for v in hits]
        else:
            vals = [v.get("hbm_bytes_per_launch_largest") for v in hits]
        vals = [x for x in vals if x is not None]
        return max(vals) if vals else None
    return None


def pmc_valu(kernel_substr, batch):
    """(counter entry, source file) of a kernel from the newest profiles/*valu*.json written by
    tools/pmc_valu.py at this per-GPU batch; (None, None) when none matches.  The entry's
    valu_issue_frac is priced at 2 cycles per wave64 VALU instruction (the SIMD-32 throughput);
    files written before that fix (no valu_cycles_per_inst key, 4-cycle pricing) are halved."""
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*valu*.json")), reverse=True):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("per_gpu_batch") != batch:
            continue
        for k, v in d["kernels"].items():
            if __import__("re").search(kernel_substr, k):
                v = dict(v)
                if v.get("valu_cycles_per_inst") != 2:
                    v["valu_issue_frac"] = round(v["valu_issue_frac"] / 2, 4)
                return v, os.path.relpath(f, REPO)
        return None, None
    return None, None


def idwt_roofline(batch, dev, layout="cl"):
    """The decoder's level-0 Haar IDWT (UnetrIDWTBlock's waverec3 replacement,
    idwt_upsample.py:160, §8a row a11) at the encoder's stage-0 band shape: 8 bands of
    (B, 48, 64^3) -> (B, 48, 128^3), written into the first half of a 96-channel concat buffer
    as the decoder does.  layout "cl" is the inference decoder's path (idwt_upsample.py's
    channel-last LL and concat buffer, idwt3d_haar_cl4_kernel); "ncdhw" the autograd path's
    (NCDHW LL and output, idwt3d_haar_nc4_kernel).  Algorithmic bytes: read 8 bands + write the
    output, 8 B per output element.  HIP events on the launch stream around REPS back-to-back
    launches."""
    from waveformer_amd import ops
    g = torch.Generator(device=dev).manual_seed(7)
    # the decoder's inputs: detail bands as the channel-last views of the DWT's (8, B, d, h,
    # w, C) output (ops.dwt3d_haar)
    bands = torch.randn(8, batch, 64, 64, 64, 48, device=dev, generator=g)
    det = [{k: bands[i + 1].permute(0, 4, 1, 2, 3) for i, k in enumerate(ops.DETAIL_KEYS)}]
    skip = None
    if layout in ("cl", "cat"):
        ll = bands[0].permute(0, 4, 1, 2, 3)                     # channel-last view
        out = ops.empty_cl(batch, 96, 128, 128, 128, dev)
        if layout == "cat":  # + torch.cat((out, skip), 1) in the same kernel
            skip = ops.empty_cl(batch, 48, 128, 128, 128, dev).normal_(generator=g)
    else:
        ll = bands[0].permute(0, 4, 1, 2, 3).contiguous()
        out = torch.empty(batch, 96, 128, 128, 128, device=dev)
    ops.idwt3d_haar(ll, det, out=out, skip=skip)
    reps = 10
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        ops.idwt3d_haar(ll, det, out=out, skip=skip)
    e.record()
    torch.cuda.synchronize()
    us = s.elapsed_time(e) / reps * 1e3
    alg = 8 * batch * 48 * 128 ** 3  # 8 B per output element (4 B of bands read + 4 B written)
    if layout == "cat":
        alg *= 2  # + the skip: 4 B read + 4 B written per element
    ach = alg / (us * 1e-6) / 1e9
    del bands, ll, det, out, skip
    # the plain and the fused-concat launches are separate instantiations (<false> / <true>),
    # so the counter summary tells them apart
    kname = {"cl": "idwt3d_haar_cl4_kernel<false>", "cat": "idwt3d_haar_cl4_kernel<true>",
             "ncdhw": "idwt3d_haar_nc4"}[layout]
    # one thread per finest 2x2x2 cube (64^3 of them per volume) x 4-channel group
    grid = (-(-batch * 64 ** 3 * 12 // 256)) * 256 if layout != "ncdhw" else None
    return {"bound": "hbm", "kernel": kname, "achieved": round(ach, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
            "traffic": pmc_traffic(kname, batch, grid), "algorithmic_bytes_per_launch": alg,
            "avg_launch_us": round(us, 2), "launches_timed": reps,
            "shape": f"channel-last bands 8 x ({batch}, 64^3, 48) -> ({batch}, 48, 128^3) "
                     f"{'NCDHW' if layout == 'ncdhw' else 'channel-last'} into a 96-channel "
                     f"buffer" + (" + the 48-channel skip into its other half" if layout == "cat" else "")}


def build_encoder(img, device):
    from functools import partial
    import torch.nn as nn
    import waveformer_amd.network_models as NM
    torch.manual_seed(0)  # the reference's own init (trunc_normal / fan-out normal), seeded
    m = NM.MultiscaleTransformer(img_size=(img,) * 3, in_chans=4, embed_dims=[48, 96, 192, 384],
                                 num_heads=[3, 6, 12, 24], depths=[2, 2, 2, 2], qkv_bias=True,
                                 norm_layer=partial(nn.LayerNorm, eps=1e-6))
    return m.eval().to(device)


def build_full(img, device, hf):
    """The whole Waveformer (encoder + IDWT decoder + UnetrBasicBlock / UnetResBlock convs),
    reference init; hf = the HF refinement branch (network_backbone.py:196-197, config 5)."""
    import waveformer_amd.network_models as NM
    torch.manual_seed(0)
    cfg = {"transformer": {"hf_refinement": True}} if hf else None
    m = NM.Waveformer(img_size=(img,) * 3, in_chans=4, out_chans=4, depths=[2, 2, 2, 2],
                      feat_size=[48, 96, 192, 384], num_heads=[3, 6, 12, 24],
                      network_config=cfg)
    return m.eval().to(device)


def cpu_baseline(seconds_budget=20.0):
    """The oracle encoder (fp32 PyTorch on the host CPU) on one 128^3 x 4 volume."""
    from oracle import ref_waveformer as R
    m = build_encoder(128, "cpu")
    sd = m.state_dict()
    x = torch.randn(1, 4, 128, 128, 128, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        R.encoder(sd, x, heads=[3, 6, 12, 24], depths=[2] * 4)  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            R.encoder(sd, x, heads=[3, 6, 12, 24], depths=[2] * 4)
            n += 1
            if time.perf_counter() - t0 > seconds_budget / 2 or n >= 5:
                break
        dt = (time.perf_counter() - t0) / n
    return {"value": 1.0 / dt, "unit": "volumes/s", "cores": torch.get_num_threads(),
            "kind": "port",
            "sample": f"{n} timed encoder forwards (+1 warm-up) of one 128^3x4 volume, B=1, fp32, "
                      f"oracle/ref_waveformer.py (CPU restatement of the reference), "
                      f"{dt:.2f} s/volume"}


def parity_dice(device, case_name="full128"):
    """Full Waveformer (full128: 128^3 x 4; full192hf: 192^3 x 4 with the HF refinement branch,
    config 5) with the golden rule weights at the bench's precision vs the reference's labels."""
    from tests import cases as C
    from waveformer_amd import ops
    case = C.cases()[case_name]
    m, _ = C.build(case, device)
    with torch.no_grad():
        lab = m(C.case_input(case).to(device)).argmax(1).cpu()
    ref = C.g(case_name + "_labels").long()
    d = [C.dice(a, b) for a, b in zip(C.brats_regions(lab), C.brats_regions(ref))]
    del m
    torch.cuda.empty_cache()
    size = case.input_shape[2]
    return {"dice_tc_wt_et": [round(v, 6) for v in d], "dice_delta_max": round(1 - min(d), 6),
            "precision": ops.get_precision(),
            "vs": f"reference Waveformer labels at {size}^3x4"
                  f"{' (HF refinement)' if 'hf' in case_name else ''} "
                  f"(tests/golden/ref_fixtures.npz)"}


def main_sliding(args, world, rank, dev):
    """Config 3: BraTS 240 x 240 x 155 x 4 synthetic case, SlidingWindowInferer(roi 128^3,
    sw_batch 2, overlap 0.5, 'gaussian') over the full Waveformer (4_predict.py:199-205), the
    18 windows (x8 with --tta) dealt round-robin over the ranks, per-round RCCL all-gather of
    the window logits, HIP stitch on every rank.  A step is one case; the ranks share it, so
    the scaling is strong.  Roofline: the stitch kernel (HBM)."""
    import waveformer_amd.network_models as NM
    from waveformer_amd import inferers, ops
    torch.manual_seed(0)
    model = NM.Waveformer(img_size=(128,) * 3, in_chans=4, out_chans=4, depths=[2, 2, 2, 2],
                          feat_size=[48, 96, 192, 384], num_heads=[3, 6, 12, 24]).eval().to(dev)
    x = torch.randn(1, 4, 240, 240, 155, device=dev,
                    generator=torch.Generator(device=dev).manual_seed(4321))
    group = dist.group.WORLD if world > 1 else None
    inf = inferers.SlidingWindowInferer((128,) * 3, sw_batch_size=2, overlap=0.5,
                                        mode="gaussian", cache_roi_weight_map=True,
                                        process_group=group, exchange=args.exchange)
    axes = [0, 1, 2] if args.tta else None

    def step():
        with torch.no_grad():
            if axes:
                return inferers.maybe_mirror_and_predict(x, model, inf, axes)
            return inf(x, model)

    stitch = OpTimer("sliding_window_stitch") if args.full else None
    for _ in range(max(1, args.warmup)):
        y = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, y)
    r = rc = None
    if args.full:  # per-kernel rooflines: one more, eager, step with the op timers on
        conv = OpTimer("conv3d_k3")
        stitch.active = conv.active = True
        step()
        stitch.active = conv.active = False
        r = stitch.summary()
        rc = conv.summary()
    if rank == 0:
        nwin = 18 * (8 if axes else 1)
        out = {
            "metric": "BraTS 240x240x155x4 cases/sec (sliding window, full Waveformer)",
            "value": args.steps / dt, "unit": "cases/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": args.precision,
            "data": "synthetic: randn 1x4x240x240x155 case resident in HBM, reference-init "
                    "random weights",
            "config": {"workload": "SlidingWindowInferer(roi 128^3, sw_batch 2, overlap 0.5, "
                                   "gaussian) over Waveformer 128^3x4, config 3",
                       "windows": nwin, "tta": bool(axes), "exchange": args.exchange,
                       "parallelism": f"windows round-robin over {world} ranks + " + (
                           "RCCL all-gather of window logits per round" if args.exchange ==
                           "allgather" else "each rank's partial stitch + one RCCL all-reduce "
                                            "of the (C + 1) full-size planes")},
            "output_checksum": float(y.double().sum().item()),
        }
        rl = {}
        if rc:  # the dominant kernel of this workload (a third of the step)
            ach = rc["rate"] / 1e12
            issue = rc["issue"]
            rl["conv3d_k3"] = {
                "bound": "mfma", "kernel": "conv3d_k3", "achieved": round(ach, 1),
                "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
                "algorithmic_flops_per_launch": rc["work_per_launch"],
                "avg_launch_us": round(rc["avg_ms"] * 1e3, 2), "launches_timed": rc["launches"],
                "mfma_issue_frac": round(issue * ach / MFMA_BF16_PEAK_TFLOPS, 4),
                "note": "fp32-faithful bf16x3 issues 3 MFMAs per product; frac counts the "
                        "algorithmic fp32 flops, mfma_issue_frac the issued bf16 MFMA work"}
        if r:
            ach = r["rate"] / 1e9
            rl["sliding_window_stitch"] = {
                "bound": "hbm", "kernel": "sliding_window_stitch", "achieved": round(ach, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                "traffic": None, "algorithmic_bytes_per_launch": r["work_per_launch"],
                "avg_launch_us": round(r["avg_ms"] * 1e3, 2), "launches_timed": r["launches"]}
        if rl:
            out["roofline"] = rl.get("conv3d_k3", next(iter(rl.values())))
            out["rooflines"] = rl
        print(json.dumps(_stamp(out, args, world)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main_train(args, world, rank, dev):
    """Config 4: one training step of the full Waveformer on 128^3 x 4 random crops, per GPU
    batch args.batch, as BraTSTrainer does it (3_train.py:96-102, trainer.py:458-466):
    DiceCE(to_onehot_y, softmax) -> backward -> clip_grad_norm_(12) -> AdamW(1e-4).  N > 1: DDP
    over RCCL (bucketed all-reduce of the fp32 gradients, overlapped with the backward).
    Encoder forward = HIP kernels (bf16x3 MFMA), encoder backward = HIP kernels + the
    library's MFMA GEMMs (bf16x3 data gradients, wf_gemm_tn weight gradients), decoder 3^3
    convolutions = HIP forward / input- / weight-gradient kernels, 1x1 / transposed convs = the
    same MFMA GEMMs (no MIOpen convolution, no find; torch.mm only for the 4-channel shapes).
    AdamW runs fused (one kernel per step for all parameters)."""
    import waveformer_amd.network_models as NM
    from waveformer_amd.losses import DiceCELoss
    torch.manual_seed(0)
    # every decoder convolution trains on waveformer_amd kernels / GEMMs (autograd.conv_train);
    # with MIOpen convolutions (round 1) the first step paid minutes of find at B = 4
    torch.backends.cudnn.benchmark = bool(args.miopen_find)
    model = NM.Waveformer(img_size=(args.img,) * 3, in_chans=4, out_chans=4,
                          depths=[2, 2, 2, 2], feat_size=[48, 96, 192, 384],
                          num_heads=[3, 6, 12, 24]).train().to(dev)
    model = model.to(memory_format=torch.channels_last_3d)
    ddp = model
    if world > 1:
        ddp = torch.nn.parallel.DistributedDataParallel(
            model, device_ids=[dev.index], bucket_cap_mb=64, gradient_as_bucket_view=True,
            find_unused_parameters=True)  # as the reference trainer (trainer.py:355-358)
    # fused: one multi-tensor kernel per step instead of the foreach path's ~10 elementwise
    # passes over the parameters (the same AdamW update, trainer.py:452-466)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True)
    loss_fn = DiceCELoss(to_onehot_y=True, softmax=True)
    g = torch.Generator(device=dev).manual_seed(1 + rank)
    x = torch.randn(args.batch, 4, args.img, args.img, args.img, device=dev, generator=g)
    x = x.contiguous(memory_format=torch.channels_last_3d)
    y = torch.randint(0, 4, (args.batch, 1, args.img, args.img, args.img), device=dev,
                      generator=g)
    losses = []

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(ddp(x), y)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 12)
        opt.step()
        return loss

    for i in range(max(1, args.warmup)):
        t1 = time.perf_counter()
        losses.append(step().item())
        print(f"[bench] warm-up step {i}: {time.perf_counter() - t1:.2f} s "
              f"(loss {losses[-1]:.4f})", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses.append(last.item())
    if world > 1:
        dist.barrier()
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": last})
    if rank == 0:
        vols = args.batch * args.steps * world
        out = {
            "metric": "128^3x4 volumes/sec train step (fwd + DiceCE + bwd + AdamW), config 4",
            "value": vols / dt, "unit": "volumes/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "fp32 (bf16x3 MFMA forward, fp32 backward)",
            "data": "synthetic: randn 128^3x4 crops + randint(0,4) labels resident in HBM, "
                    "reference-init random weights",
            "config": {"workload": f"Waveformer {args.img}^3x4 train step, DiceCE, AdamW 1e-4, "
                                   f"clip 12", "global_batch": args.batch * world,
                       "per_gpu_batch": args.batch,
                       "parallelism": f"DDP x{world} (RCCL all-reduce)" if world > 1 else "x1"},
            "loss_first_last": [round(losses[0], 5), round(losses[-1], 5)],
            "peak_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
        }
        print(json.dumps(_stamp(out, args, world)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _stamp(out, args, world):
    """The distinct GPUs behind the ranks; a gloo rehearsal that folds ranks onto fewer GPUs is
    marked as such (its value is not an N-GPU number)."""
    dv = getattr(args, "devices", world)
    out["devices"] = dv
    if dv < world:
        out["rehearsal"] = f"{world} ranks on {dv} GPU(s) over {os.environ.get('WF_BENCH_BACKEND')}"
    return out


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launcher_cmd(argv, n, port):
    """The torch.distributed.run command that starts `n` ranks of this script with the same
    arguments (one process per GPU, rendezvous on 127.0.0.1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr", "127.0.0.1", "--master-port", str(port),
            os.path.abspath(__file__)] + list(argv)


def maybe_launch_ranks(args):
    """`python bench.py --gpus N` from a plain shell (no WORLD_SIZE in the environment): start
    the N ranks as ONE child process -- torch.distributed.run, the way the reference's own
    launcher re-launches itself (light_training/launch.py:81-112) -- and return its exit code.
    Rank 0's JSON line reaches our stdout directly (the child inherits it).  Nothing here has
    touched the GPU: the ranks initialise their own devices.  None when this process is
    already a rank or N == 1."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    import subprocess
    return subprocess.call(launcher_cmd(sys.argv[1:], args.gpus, _free_port()))


def main():
    args = parse()
    rc = maybe_launch_ranks(args)
    if rc is not None:
        sys.exit(rc)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE {world}: launch one rank "
                         f"per GPU (or run `python bench.py --gpus N` and let it start them)")
    backend = os.environ.get("WF_BENCH_BACKEND", "nccl")
    if world > 1:
        # RCCL ("nccl") between the GPUs of a node; WF_BENCH_BACKEND=gloo rehearses the
        # multi-rank path with several ranks sharing fewer GPUs (rank -> LOCAL_RANK % GPUs)
        dist.init_process_group(backend, init_method="env://")
    ngpu = torch.cuda.device_count()
    if local >= ngpu:
        if backend != "gloo":
            raise SystemExit(f"bench.py: LOCAL_RANK {local} but only {ngpu} GPUs visible")
        local = local % max(1, ngpu)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # distinct GPUs behind the ranks (a gloo rehearsal may fold several ranks onto one)
    args.devices = world
    if world > 1:
        locs = [None] * world
        dist.all_gather_object(locs, local)
        args.devices = len(set(locs))
    from waveformer_amd import _lib, ops
    _lib.load()  # fail loudly without the HIP library
    ops.set_precision(args.precision)
    if args.workload == "sliding":
        return main_sliding(args, world, rank, dev)
    if args.workload == "train":
        return main_train(args, world, rank, dev)

    full = args.workload == "full"
    hf = full and args.img == 192  # config 5: 192^3 crops with the HF refinement branch
    model = build_full(args.img, dev, hf) if full else build_encoder(args.img, dev)
    x = torch.randn(args.batch, 4, args.img, args.img, args.img, device=dev,
                    generator=torch.Generator(device=dev).manual_seed(1234 + rank))

    roof_op = args.roofline_op if args.roofline_op != "auto" else "ccf_ffn_dwconv"
    timers = {}
    if args.op_timers:
        timers = {n: OpTimer(n) for n in dict.fromkeys(
            [roof_op, "dwt3d_haar", "dwt3d_haar_ll", "msfuse", "window_attention"]
            + (["conv3d_k3"] if full else []))}

    def step():
        with torch.no_grad():
            return model(x)

    for _ in range(max(1, args.warmup)):
        step()
    torch.cuda.synchronize()

    graph = None
    last = None  # what the last timed step returned (a replayed graph's static outputs)
    if args.graph:
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                last = step()
            graph.replay()
            torch.cuda.synchronize()
        except Exception as e:  # capture unsupported -> eager, said in the output
            graph = last = None
            print(f"[bench] graph capture failed ({e}); timing eager launches", file=sys.stderr)

    def run_steps(k):
        nonlocal last
        for _ in range(k):
            if graph is not None:
                graph.replay()
            else:
                last = step()

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(args.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, last)

    # per-launch roofline timing of the dominant streaming kernel (eager launches, so the HIP
    # events sit on the launch stream around each launch)
    roofs = {}
    if args.op_timers:
        for t in timers.values():
            t.active = True
        with torch.no_grad():
            for _ in range(max(2, min(args.steps, 10))):
                model(x)
        for t in timers.values():
            t.active = False
        roofs = {n: t.summary() for n, t in timers.items()}

    if rank == 0:
        vols = args.batch * args.steps * world
        out = {
            "metric": METRIC if not full else
            f"{args.img}^3x4 volumes/sec fwd, full Waveformer"
            f"{' + HF refinement (config 5)' if hf else ''} + Dice delta vs reference",
            "value": vols / dt,
            "unit": "volumes/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.precision,
            "data": f"synthetic: randn {args.img}^3x4 crops resident in HBM, reference-init "
                    f"random weights",
            "config": {"workload": (f"Waveformer forward (encoder + IDWT decoder"
                                    f"{' + HFRefinementRes' if hf else ''}), "
                                    if full else "MultiscaleTransformer (WaveFormer encoder) "
                                                 "forward, ") + f"{args.img}^3x4 crops",
                       "global_batch": args.batch * world, "per_gpu_batch": args.batch,
                       "precision": args.precision,
                       "parallelism": f"replicas x{world} (no data-path collective)",
                       "hip_graph": graph is not None},
        }
        if dumped is not None:
            out["dumped_outputs"] = dumped  # name -> shape of DIR/<name>.npy
        def roofline(name, r):
            if name in ("window_attention", "conv3d_k3"):
                # MFMA-bound: algorithmic FLOPs vs the dense bf16 / fp16 peak (the same 2.5
                # PFLOP/s on gfx950); bf16x3 issues three MFMAs per product
                ach = r["rate"] / 1e12
                issue = r["issue"]  # of the timed launches (fp16 mode: attention at bf16x3)
                return {"bound": "mfma", "kernel": name, "achieved": round(ach, 2),
                        "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
                        "algorithmic_flops_per_launch": r["work_per_launch"],
                        "avg_launch_us": round(r["avg_ms"] * 1e3, 2),
                        "launches_timed": r["launches"],
                        "mfma_issue_frac": round(issue * ach / MFMA_BF16_PEAK_TFLOPS, 4)}
            ach = r["rate"] / 1e9
            d = {"bound": "hbm", "kernel": name, "achieved": round(ach, 1),
                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                 "traffic": pmc_traffic(PMC_KERNEL.get(name, name), args.batch, r.get("grid")),
                 "algorithmic_bytes_per_launch": r["work_per_launch"],
                 "avg_launch_us": round(r["avg_ms"] * 1e3, 2), "launches_timed": r["launches"]}
            if name == "ccf_ffn_dwconv":
                # its VALU issue fraction (2-cycle SIMD-32 ceiling) from the committed
                # counter pass of the same bench command
                vf, src = pmc_valu(PMC_KERNEL[name], args.batch)
                if vf is not None:
                    d["valu_issue_frac"], d["valu_source"] = vf["valu_issue_frac"], src
            return d

        if roofs.get(roof_op):
            out["roofline"] = roofline(roof_op, roofs[roof_op])
        out["rooflines"] = {n: roofline(n, r) for n, r in roofs.items() if r and n != roof_op}
        if args.op_timers and not full:
            out["rooflines"]["idwt3d_haar"] = idwt_roofline(args.batch, dev, "cl")
            out["rooflines"]["idwt3d_haar_ncdhw"] = idwt_roofline(args.batch, dev, "ncdhw")
            out["rooflines"]["idwt3d_haar_cat"] = idwt_roofline(args.batch, dev, "cat")
        if "window_attention" in out["rooflines"]:
            wa = out["rooflines"]["window_attention"]
            # the core's MFMA issue per useful flop at head_dim 16 (attention.hip attn_tbl):
            # QK^T packs hd = 16 into K = 32 (2x) and bf16x3 adds the lo pass (4x); PV issues
            # vl*P + vh*P_lo + vh*P (3x) plus the MFMA row sums (ones*P_lo, ones*P: +2x):
            # 147,456 issued for 32,768 useful flops per 16 queries x 32 keys = 4.5x (bf16x3);
            # 2.0x with plain 16-bit operands.  A saturated pipe reaches 1 / that of the peak
            # in useful flops -- the ceiling beside north_star's 60 % target
            ipu = 4.5 if wa.get("mfma_issue_frac", 0) > wa.get("frac", 0) * 2 else 2.0
            wa["core_mfma_issued_per_useful"] = ipu
            wa["core_useful_frac_ceiling"] = round(1.0 / ipu, 4)
            vf, src = pmc_valu("attn_tbl_kernel", args.batch)
            if vf is not None:
                wa["core_valu_issue_frac"] = vf["valu_issue_frac"]
                if "mfma_busy_frac" in vf:  # SQ_VALU_MFMA_BUSY_CYCLES: the pipe, not the spec
                    wa["core_mfma_busy_frac"] = vf["mfma_busy_frac"]
                wa["valu_source"] = src
        if args.parity:
            try:
                out["parity"] = parity_dice(dev, "full192hf" if hf else "full128")
            except Exception as e:
                out["parity"] = {"error": str(e)[:200]}
        if args.cpu_baseline and world == 1 and not full:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(_stamp(out, args, world)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
