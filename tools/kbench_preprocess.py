"""Times the preprocessing of one case (waveformer_amd.preprocessing) on the GPU.

One synthetic 4x155x240x240 case: an off-centre ellipsoid "head" of positive intensities in zeros,
1 % of its voxels zero in every modality (holes for the fill), three nested balls as labels.
After WARMUP untimed calls it takes REPEATS timings of (a) every stage on its own, HIP events
around the stage's launches (the hole fill synchronises inside, so its figure includes the
read-backs), and (b) the whole run_case_npy with the volumes already on the device, a host clock
around it.  It also prints the number of fill rounds the case needs and, where scipy is
importable, the time of the numpy / scipy restatement (tests/preprocess_ref.py) on this host's
CPU.  The process ends itself after --limit seconds.  --out FILE also writes the lines there.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends")
    ap.add_argument("--out", default=None)
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
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
