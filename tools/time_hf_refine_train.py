"""Time forward + backward of the HF refinement (HFRefinementRes over the 7 detail tensors of a
wavelet level, config 5) on the six (module, level) shapes of the 128^3 model, two ways
("HF refinement under autograd"):

  module  the per-tensor path: HFRefinementRes.forward on each of the 7 tensors under autograd
          (depthwise conv op, ATen InstanceNorm3d, ReLU, 1x1-conv GEMM, sigmoid, product)
  fused   waveformer::hf_refine, one wf_hf_refine_fwd + one wf_hf_refine_bwd per level

Device events around forward + backward, rounds interleave the two paths on one device, one
line per shape and batch: median / minimum microseconds of each path and module / fused.  With
--launches the tool also counts kernel launches per path: it starts children of itself under
`rocprofv3 --kernel-trace --stats` (nothing else traced), each running one path for 1 and for
3 steps over the six shapes, and reports (dispatches(3) - dispatches(1)) / 2 per step.

  python tools/time_hf_refine_train.py [--rounds 30] [--batches 2 4] [--launches DIR]
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from waveformer_amd import _lib, ops  # noqa: E402
from waveformer_amd import autograd as wfa  # noqa: E402
from waveformer_amd.network_models import HFRefinementRes  # noqa: E402

# (decoder, level, C, edge) of the 128^3 model: decoder4 one level, decoder3 two, decoder2 three
SHAPES = [("decoder4", 0, 192, 8), ("decoder3", 0, 96, 8), ("decoder3", 1, 96, 16),
          ("decoder2", 0, 48, 8), ("decoder2", 1, 48, 16), ("decoder2", 2, 48, 32)]
KEYS = ops.DETAIL_KEYS


def setup(C, S, B, gen):
    mod = HFRefinementRes(C).cuda()
    bands = (torch.randn((8, B, S, S, S, C), device="cuda", generator=gen) * 1.5 + 0.2)
    bands.requires_grad_(True)
    det = {k: bands[i + 1].permute(0, 4, 1, 2, 3) for i, k in enumerate(KEYS)}
    cots = [torch.randn((B, S, S, S, C), device="cuda", generator=gen).permute(0, 4, 1, 2, 3)
            for _ in range(7)]
    return mod, bands, det, cots


def step(path, mod, bands, det, cots):
    """One forward + backward; gradients dropped first (host only)."""
    bands.grad = None
    for p in mod.parameters():
        p.grad = None
    if path == "module":
        outs = [mod(det[k]) for k in KEYS]
    else:
        o = wfa.hf_refine(det, mod)
        outs = [o[k] for k in KEYS]
    torch.autograd.backward(outs, cots)


def child(path, steps, B):
    """The traced program: `steps` forward + backward steps of one path over the six shapes."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = [setup(C, S, B, gen) for _, _, C, S in SHAPES]
    for _ in range(steps):
        for s in sets:
            step(path, *s)
    torch.cuda.synchronize()


def count_launches(out_dir, B):
    """Kernel dispatches per step (six shapes, forward + backward) of each path."""
    res = {}
    for path in ("module", "fused"):
        rows = {}
        for steps in (1, 3):
            d = os.path.join(out_dir, f"{path}_{steps}")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
                   "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", path,
                   "--steps", str(steps), "--batches", str(B)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=300)
            files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if not files:
                raise RuntimeError(f"no kernel trace under {d}")
            with open(files[0], newline="") as f:
                rows[steps] = sum(1 for _ in csv.DictReader(f))
        res[path] = ((rows[3] - rows[1]) / 2, rows[1], rows[3])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--launches", default=None, metavar="DIR",
                    help="also count launches per path (rocprofv3 children, traces under DIR)")
    ap.add_argument("--child", default=None, choices=["module", "fused"])
    ap.add_argument("--steps", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    _lib.load()
    if a.child:
        child(a.child, a.steps, a.batches[0])
        return
    gen = torch.Generator(device="cuda").manual_seed(0)
    print(f"HF refinement forward + backward, rounds {a.rounds}, device events, us")
    print(f"{'shape':28s} {'module med':>11s} {'min':>9s} {'fused med':>11s} {'min':>9s} "
          f"{'module/fused':>13s}")
    worst = None
    for B in a.batches:
        for dec, lvl, C, S in SHAPES:
            s = setup(C, S, B, gen)
            for path in ("module", "fused"):  # warm-up, and the two paths agree
                for _ in range(3):
                    step(path, *s)
                if path == "module":
                    want = s[1].grad.clone()
            err = float((s[1].grad - want).norm() / want.norm())
            times = {"module": [], "fused": []}
            for _ in range(a.rounds):
                for path in ("module", "fused"):
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(path, *s)
                    e1.record()
                    e1.synchronize()
                    times[path].append(e0.elapsed_time(e1) * 1e3)
            mm, fm = statistics.median(times["module"]), statistics.median(times["fused"])
            ratio = mm / fm
            worst = ratio if worst is None else min(worst, ratio)
            print(f"{dec}.{lvl} B{B} {S}^3 x {C:<12d} {mm:11.1f} {min(times['module']):9.1f} "
                  f"{fm:11.1f} {min(times['fused']):9.1f} {ratio:13.2f}   "
                  f"(input gradient fused vs module rel-L2 {err:.1e})")
    print(f"smallest module / fused ratio: {worst:.2f}")
    if a.launches:
        B = a.batches[0]
        for path, (n, r1, r3) in count_launches(a.launches, B).items():
            print(f"launches per step (six shapes, forward + backward, B = {B}) {path}: {n:.0f}"
                  f"   (dispatches in a 1-step run {r1}, in a 3-step run {r3})")


if __name__ == "__main__":
    main()
