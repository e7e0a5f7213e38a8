"""Times the preprocessing of one case (waveformer_amd.preprocessing) on the GPU.

One synthetic 4x155x240x240 case: an off-centre ellipsoid "head" of positive intensities in zeros,
1 % of its voxels zero in every modality (holes for the fill), three nested balls as labels.
After WARMUP untimed calls it takes REPEATS timings of (a) every stage on its own, HIP events
around the stage's launches (the hole fill synchronises inside, so its figure includes the
read-backs), and (b) the whole run_case_npy with the volumes already on the device, a host clock
around it.  It also prints the number of fill rounds the case needs and, where scipy is
importable, the time of the numpy / scipy restatement (tests/preprocess_ref.py) on this host's
CPU.  The process ends itself after --limit seconds.  --out FILE also writes the lines there.

--resample-out FILE adds the resample stage on the cropped, z-scored data: spacing 1 mm -> 1.5 mm
(down) and -> 0.75 mm (up).  In each direction it alternates the fused path
(ops.zoom_cubic_volume: channel_stats and one launch per axis) with the composition of the older
entry points (spline_prefilter(EDGE) on the three axes, zoom_cubic on the padded coefficients,
a clamp to the channels' ranges), times the segmentation resize, and writes the times with the
bytes each path moves (computed from the shapes) and their share of the HBM peak of 8.0 TB/s.
--errors-out FILE writes the largest difference between the two paths at that size.
Reported, not gated."""
import argparse
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformer_amd import ops, preprocessing  # noqa: E402

SHAPE = (155, 240, 240)
CHANNELS = 4


def ball(centre, radius):
    z, y, x = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius * radius


def make_case():
    rs = np.random.RandomState(20)
    z, y, x = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
    head = ((z - 80) / 68.0) ** 2 + ((y - 125) / 95.0) ** 2 + ((x - 118) / 80.0) ** 2 <= 1.0
    head &= rs.random_sample(SHAPE) >= 0.01
    data = np.zeros((CHANNELS,) + SHAPE, dtype=np.float32)
    for c in range(CHANNELS):
        v = np.abs(rs.standard_normal(SHAPE).astype(np.float32)) * (60.0 * (c + 1)) + 20.0
        data[c] = v * head
    seg = np.zeros((1,) + SHAPE, dtype=np.int16)
    seg[0][ball((70, 100, 130), 30)] = 2
    seg[0][ball((74, 97, 135), 18)] = 1
    seg[0][ball((72, 95, 138), 10)] = 3
    seg[0][~head] = 0
    return data, seg


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
    return (f"{name:<40s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   "
            f"max {max(ms):9.3f}   ({len(ms)} repeats)")


HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specified peak


def composed_zoom(x, size, lo, hi):
    """The composition the older entry points offer: three padded prefilter passes, the 64-tap
    zoom, and the clamp to the channels' [min, max] (lo, hi: (N, 1, 1, 1))."""
    coef = ops.spline_prefilter(x, ops.SPLINE_EDGE)
    return torch.minimum(torch.maximum(ops.zoom_cubic(coef, size), lo), hi)


def zoom_bytes(shape, size):
    """fp32 bytes (read + written) of the two paths for N planes shape -> size: (fused, composed)."""
    n = shape[0]
    vox = lambda d: n * d[0] * d[1] * d[2] * 4  # noqa: E731
    cur, fused = list(shape[1:]), vox(shape[1:])  # channel_stats reads the input once
    for a in range(3):
        if cur[a] == size[a]:
            continue
        nxt = list(cur)
        nxt[a] = size[a]
        fused += vox(cur) + vox(nxt)
        cur = nxt
    cur, comp = list(shape[1:]), 2 * vox(shape[1:])  # amin and amax read the input twice
    for a in range(3):
        nxt = list(cur)
        nxt[a] += 2 * ops.SPLINE_PAD
        comp += vox(cur) + vox(nxt)
        cur = nxt
    comp += vox(cur) + vox(size)  # the gather reads every coefficient at least once
    comp += 4 * vox(size)         # maximum and minimum: a read and a write each
    return fused, comp


def resample_stage(norm, seg16, w, n):
    """norm (C, d, h, w) fp32 z-scored, seg16 (d, h, w) int16, both cropped.  Returns (time
    lines, error lines)."""
    from waveformer_amd import resampling
    shape = tuple(int(v) for v in norm.shape)
    lines, errs = [], []
    lo = norm.amin(dim=(1, 2, 3), keepdim=True)
    hi = norm.amax(dim=(1, 2, 3), keepdim=True)
    for name, spacing in (("down, 1 mm -> 1.5 mm", 1.5), ("up, 1 mm -> 0.75 mm", 0.75)):
        size = tuple(int(v) for v in resampling.compute_new_shape(shape[1:], (1.0,) * 3,
                                                                  (spacing,) * 3))
        fused = lambda: ops.zoom_cubic_volume(norm, size, clip=True)  # noqa: E731
        comp = lambda: composed_zoom(norm, size, norm.amin(dim=(1, 2, 3), keepdim=True),  # noqa: E731
                                     norm.amax(dim=(1, 2, 3), keepdim=True))
        for _ in range(w):
            fused(), comp()
        t_f, t_c = [], []
        for _ in range(n):  # alternate the two paths
            t_f += timed(fused, 0, 1)
            t_c += timed(comp, 0, 1)
        t_s = timed(lambda: ops.zoom_seg_linear(seg16, size), w, n)
        b_f, b_c = zoom_bytes(shape, size)
        lines.append(f"{name}: {shape} -> {size}")
        for label, ms, nbytes in (("fused (stats + 3 axis passes)", t_f, b_f),
                                  ("composed (3 prefilters + zoom + clamp)", t_c, b_c)):
            med = statistics.median(ms) * 1e-3
            lines.append(line("  " + label, ms))
            lines.append(f"    bytes moved (from the shapes) {nbytes / 1e6:9.1f} MB = "
                         f"{nbytes / med / 1e9:8.1f} GB/s = {100 * nbytes / med / HBM_PEAK:5.2f} % "
                         f"of the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s")
        lines.append(line("  zoom_seg_linear", t_s))
        a, b = fused(), composed_zoom(norm, size, lo, hi)
        diff = (a - b).abs()
        # both paths are within 95 * 2^-23 * cmax of float64 (tests/test_gpu_resample.py), cmax at
        # least the largest input magnitude: they may differ by twice that
        allowed = 2 * 95 * 2.0 ** -23 * norm.abs().max().item()
        errs.append(f"{name}: {shape} -> {size}: max |fused - composed| {diff.max().item():.3e} "
                    f"(max |value| {b.abs().max().item():.3e}; twice the tests' bound is at least "
                    f"{allowed:.3e}); differing elements {int((diff > 0).sum())} of {diff.numel()}")
        del a, b, diff
    return lines, errs


def cpu_resample(norm_h, seg_h):
    """The numpy / scipy restatement (tests/resample_ref.py) of the down direction, one run."""
    from tests import resample_ref as ref
    from waveformer_amd import resampling
    size = tuple(int(v) for v in resampling.compute_new_shape(norm_h.shape[1:], (1.0,) * 3,
                                                              (1.5,) * 3))
    t = time.perf_counter()
    ref.resample_data_or_seg(norm_h, size)
    t_d = time.perf_counter() - t
    t = time.perf_counter()
    ref.resample_data_or_seg(seg_h[None], size, is_seg=True, order=1)
    return [(f"resize of {norm_h.shape[0]} channels -> {size}", t_d),
            ("resize_segmentation (order 1)", time.perf_counter() - t)]


def cpu_restatement(data, seg):
    """The numpy / scipy restatement of the same case, stage by stage, one run."""
    from tests import preprocess_ref as ref
    out = []
    t = time.perf_counter()
    mask = ref.nonzero_mask(data)
    out.append(("nonzero mask", time.perf_counter() - t))
    t = time.perf_counter()
    filled = ref.fill_holes(mask)
    out.append(("scipy binary_fill_holes", time.perf_counter() - t))
    t = time.perf_counter()
    d, s, _ = ref.crop_to_nonzero(data, seg, filled)
    d = np.ascontiguousarray(d)
    out.append(("bbox + crop copies", time.perf_counter() - t))
    t = time.perf_counter()
    for c in range(d.shape[0]):
        img = d[c]
        d[c] = (img - img.mean()) / max(img.std(), 1e-8)
    out.append((f"{d.shape[0]} z-scores (fp32, numpy)", time.perf_counter() - t))
    t = time.perf_counter()
    ref.sample_foreground_locations(s, [1, 2, 3])
    out.append(("class locations (argwhere + choice)", time.perf_counter() - t))
    return out


def write(path, text):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resample-out", default=None, help="time the resample stage, write it here")
    ap.add_argument("--errors-out", default=None, help="fused against composed resample, here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_preprocess: needs a GPU")
    signal.alarm(args.limit)
    dev = torch.device("cuda", 0)
    data_h, seg_h = make_case()
    data, seg = torch.from_numpy(data_h).to(dev), torch.from_numpy(seg_h).to(dev)
    w, n = args.warmup, args.repeats
    out = [f"preprocessing of one {CHANNELS}x{SHAPE[0]}x{SHAPE[1]}x{SHAPE[2]} case, "
           f"{torch.cuda.get_device_name(0)}"]

    out.append(line("nonzero_mask", timed(lambda: ops.nonzero_mask(data), w, n)))
    mask = ops.nonzero_mask(data)
    out.append(line("fill_holes (+ bbox, read-backs)", timed(lambda: ops.fill_holes(mask), w, n)))
    filled, bbox8, rounds = ops.fill_holes(mask)
    bbox = preprocessing.bbox_from_device(bbox8.cpu().tolist())
    out.append(f"fill rounds that marked a voxel: {rounds}; filled {int(bbox8[6])} voxels "
               f"({int(bbox8[6]) - int(mask.sum())} of them holes); bbox {bbox}")
    out.append(line("box_moments", timed(lambda: ops.box_moments(data, bbox), w, n)))
    stats = ops.box_moments(data, bbox)
    out.append(line("crop_normalize", timed(lambda: ops.crop_normalize(data, bbox, stats), w, n)))
    seg16 = seg[0].contiguous()
    out.append(line("crop_seg", timed(lambda: ops.crop_seg(seg16, filled, bbox), w, n)))
    cropped_seg, _ = ops.crop_seg(seg16, filled, bbox)
    out.append(line("sample_foreground_locations (3 classes)",
                    timed(lambda: preprocessing.sample_foreground_locations(cropped_seg, [1, 2, 3]),
                          w, n)))
    out.append(line("collect_foreground_intensities",
                    timed(lambda: preprocessing.collect_foreground_intensities(seg, data), w, n)))

    p = preprocessing.MultiModalityPreprocessor()
    for _ in range(w):
        p.run_case_npy(data, seg, {"spacing": (1.0, 1.0, 1.0)})
    wall = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = p.run_case_npy(data, seg, {"spacing": (1.0, 1.0, 1.0)})
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    out.append(line("run_case_npy per case (wall)", wall))
    out.append(f"cropped to {tuple(res[0].shape)}, seg {res[1].dtype}")

    try:
        import scipy  # noqa: F401
        cpu = cpu_restatement(data_h, seg_h)
        out.append(f"numpy / scipy {scipy.__version__} restatement on this host's CPU, one run:")
        out += [f"  {name:<38s} {sec * 1e3:9.1f} ms" for name, sec in cpu]
        out.append(f"  {'total':<38s} {sum(s for _, s in cpu) * 1e3:9.1f} ms")
    except ImportError:
        out.append("scipy is not importable here: no CPU restatement timed")
    text = "\n".join(out)
    print(text)
    write(args.out, text)

    if args.resample_out or args.errors_out:
        norm = ops.crop_normalize(data, bbox, stats)
        head = [f"resampling of the cropped, z-scored case, {torch.cuda.get_device_name(0)}"]
        lines, errs = resample_stage(norm, cropped_seg, w, n)
        try:
            import scipy  # noqa: F401
            cpu = cpu_resample(norm.cpu().numpy(), cropped_seg.cpu().numpy())
            lines.append(f"numpy / scipy {scipy.__version__} restatement on this host's CPU, "
                         "down direction, one run:")
            lines += [f"  {name:<46s} {sec * 1e3:9.1f} ms" for name, sec in cpu]
        except ImportError:
            lines.append("scipy is not importable here: no CPU restatement timed")
        print("\n".join(head + lines + errs))
        write(args.resample_out, "\n".join(head + lines))
        write(args.errors_out, "\n".join(head + errs))


if __name__ == "__main__":
    main()
