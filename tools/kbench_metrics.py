"""Times the evaluation of one case (waveformer_amd.metrics.region_metrics) on the GPU.

One synthetic 155x240x240 case: per volume three nested off-centre balls (WT radius 30 as class
2, TC radius 18 as class 1, ET radius 10 as class 3), the prediction shifted by a few voxels.
After WARMUP untimed calls it takes REPEATS timings of (a) every stage on its own, HIP events
around the stage's launches, and (b) the whole region_metrics call, a host clock around it
(the call ends in its device-to-host copy, which synchronises), and prints the medians with the
minimum and maximum.  --out FILE also writes the lines there.  Reported, not gated."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformer_amd import metrics, ops  # noqa: E402

SHAPE = (155, 240, 240)


def ball(centre, radius):
    z, y, x = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius * radius


def label_map(c):
    lab = np.zeros(SHAPE, dtype=np.uint8)
    lab[ball(c, 30)] = 2
    lab[ball((c[0] + 4, c[1] - 3, c[2] + 5), 18)] = 1
    lab[ball((c[0] + 2, c[1] - 5, c[2] + 8), 10)] = 3
    return lab


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def line(name, ms):
    return (f"{name:<34s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   "
            f"max {max(ms):9.3f}   ({len(ms)} repeats)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_metrics: needs a GPU")
    dev = torch.device("cuda", 0)
    gt = torch.from_numpy(label_map((70, 100, 130))).to(dev)
    pred = torch.from_numpy(label_map((72, 97, 134))).to(dev)
    bits = metrics.BRATS_REGIONS
    R = len(bits)
    out = [f"evaluation of one {SHAPE[0]}x{SHAPE[1]}x{SHAPE[2]} case, {R} regions, "
           f"{torch.cuda.get_device_name(0)}"]

    # the stages, each on the buffers the stage before it left
    masks = torch.empty((2 * R,) + SHAPE, dtype=torch.uint8, device=dev)
    counts = torch.empty((2 * R,), dtype=torch.int64, device=dev)
    w, n = args.warmup, args.repeats
    out.append(line("region_masks (one label map)",
                    timed(lambda: ops.region_masks(pred, bits, out=masks[:R], counts=counts[:R]), w, n)))
    ops.region_masks(gt, bits, out=masks[R:], counts=counts[R:])
    scores = torch.nn.functional.one_hot(pred.long(), 4).permute(3, 0, 1, 2).contiguous().half()
    out.append(line("region_masks (fp16 scores, C = 4)",
                    timed(lambda: ops.region_masks(scores, bits), w, n)))
    del scores
    out.append(line("overlap_counts", timed(lambda: ops.overlap_counts(masks[:R], masks[R:]), w, n)))
    out.append(line(f"surface_edt_sq ({2 * R} masks)", timed(lambda: ops.surface_edt_sq(masks), w, n)))
    border, d2 = ops.surface_edt_sq(masks)
    hist_fn = lambda: ops.surface_hist(border[:R], d2[R:], border[R:], d2[:R])  # noqa: E731
    out.append(line(f"surface_hist ({R} pairs)", timed(hist_fn, w, n)))
    hist = hist_fn()
    res = torch.empty((R, ops.ORDER_STATS_STRIDE), dtype=torch.int64, device=dev)
    out.append(line("hist_order_stats",
                    timed(lambda: ops.hist_order_stats(hist, (-1, 0, 1, 2), q=(95000, 100000),
                                                       group=2, out=res), w, n)))
    del border, d2, hist, masks
    torch.cuda.empty_cache()

    # the whole call, label maps already on the device
    for _ in range(w):
        metrics.region_metrics(pred, gt)
    wall = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = metrics.region_metrics(pred, gt)
        wall.append((time.perf_counter() - t0) * 1e3)
    out.append(line("region_metrics per case (wall)", wall))
    out.append(f"device-to-host copy per case: {metrics.result_bytes(bits)} bytes (one copy)")
    ext = metrics.region_metrics(pred, gt, extra=True)
    for r, name in enumerate(("TC", "WT", "ET")):
        out.append(f"{name}: dice {got[r, 0]:.6f}  hd95 {got[r, 1]:.6f}  hd {ext[r, 2]:.6f}  "
                   f"assd {ext[r, 5]:.6f}")
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
