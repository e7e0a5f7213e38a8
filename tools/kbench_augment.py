"""Times the train-time augmentation (waveformer_amd.augment) of one batch on the GPU.

A synthetic 4 x 4 x 128^3 batch (z-scored noise on a smooth field, blocky labels -1 .. 3).  After
WARMUP untimed calls it takes the median of REPEATS HIP-event timings of
apply_train_transforms (a) with one transform drawn for every sample and channel, stage by stage,
(b) with all of them drawn -- the worst case -- and (c) with parameters sampled at the nominal
probabilities, one timing for each of --draws parameter draws (mean, median and maximum over the
draws; the first WARMUP draws are run untimed first).  The volumes are on the device already; the
Gaussian noise is drawn by torch.randn inside the call.  Where scipy is importable it also times
the numpy / scipy restatement (tests/augment_ref.py) of the worst case for ONE sample on this
host's CPU, one run.  The process ends itself after --limit seconds.  --out FILE also writes the
lines there.  Reported, not gated."""
import argparse
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformer_amd import augment  # noqa: E402

BATCH, CHANNELS, SIZE = 4, 4, 128


def make_batch(batch, size):
    rs = np.random.RandomState(21)
    shape = (batch, CHANNELS, size, size, size)
    g = np.linspace(-1, 1, size, dtype=np.float32)
    field = np.cos(2 * g)[:, None, None] * np.sin(1.5 * g + 0.3)[None, :, None] * g[None, None, :]
    data = rs.standard_normal(shape).astype(np.float32) * 0.5 + field
    coarse = rs.choice(np.array([-1, 0, 1, 2, 3], np.float32), size=(batch, 1) + (size // 8,) * 3)
    seg = coarse.repeat(8, 2).repeat(8, 3).repeat(8, 4)
    return data, np.ascontiguousarray(seg)


def all_drawn(batch):
    p = augment.no_params(batch, CHANNELS)
    p.do_rotate[:], p.angles[:] = True, (0.4, -0.3, 0.5)
    p.do_scale[:], p.scale[:] = True, 0.85
    p.noise[:], p.noise_variance[:] = True, 0.05
    p.blur[:], p.blur_sigma[:] = True, 1.0
    p.brightness[:], p.brightness_mult[:] = True, 1.1
    p.contrast[:], p.contrast_factor[:] = True, 0.9
    p.lowres[:], p.lowres_zoom[:] = True, 0.75
    p.gamma_inv[:], p.gamma_inv_gamma[:] = True, 1.2
    p.gamma[:], p.gamma_gamma[:] = True, 0.8
    p.mirror[:] = True
    return p


STAGES = {
    "centre crop only (nothing drawn)": (),
    "spatial (rotation + scale)": ("do_rotate", "angles", "do_scale", "scale"),
    "gaussian noise (torch.randn inside)": ("noise", "noise_variance"),
    "gaussian blur, sigma 1.0": ("blur", "blur_sigma"),
    "brightness": ("brightness", "brightness_mult"),
    "contrast": ("contrast", "contrast_factor"),
    "low resolution, zoom 0.75": ("lowres", "lowres_zoom"),
    "gamma on the inverted image": ("gamma_inv", "gamma_inv_gamma"),
    "gamma": ("gamma", "gamma_gamma"),
    "mirror (three axes)": ("mirror",),
}


def only(fields, batch):
    p, full = augment.no_params(batch, CHANNELS), all_drawn(batch)
    for f in fields:
        setattr(p, f, getattr(full, f))
    return p


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


def cpu_one_sample(data, seg, p):
    from tests import augment_ref as ref
    one = augment.no_params(1, CHANNELS)
    for f in augment.dataclasses.fields(one):
        setattr(one, f.name, getattr(p, f.name)[:1])
    noise = np.random.RandomState(1).standard_normal(data[:1].shape).astype(np.float32)
    t = time.perf_counter()
    ref.whole(data[:1], seg[:1], one, data.shape[2:], noise)
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--draws", type=int, default=100)
    ap.add_argument("--limit", type=int, default=500, help="seconds after which the process ends")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_augment: needs a GPU")
    signal.alarm(args.limit)
    dev = torch.device("cuda", 0)
    B = BATCH
    data_h, seg_h = make_batch(B, SIZE)
    data, seg = torch.from_numpy(data_h).to(dev), torch.from_numpy(seg_h).to(dev)
    w, n = args.warmup, args.repeats

    class Lines(list):          # every line is printed as it is measured
        def append(self, text):
            print(text, flush=True)
            super().append(text)

    out = Lines()
    out.append(f"augmentation of one {B} x {CHANNELS} x {SIZE}^3 batch, "
               f"{torch.cuda.get_device_name(0)}; HIP events, {w} warm-up calls")

    out.append("one transform drawn for every sample and channel:")
    for name, fields in STAGES.items():
        p = only(fields, B)
        out.append("  " + line(name, timed(lambda: augment.apply_train_transforms(data, seg, p),
                                           w, n)))
    full = all_drawn(B)
    out.append(line("all transforms drawn (worst case)",
                    timed(lambda: augment.apply_train_transforms(data, seg, full), w, n)))

    rng = np.random.RandomState(2024)
    draws = [augment.sample_train_params(B, CHANNELS, rng) for _ in range(args.draws)]
    for p in draws[:w]:
        augment.apply_train_transforms(data, seg, p)
    ms = [timed(lambda: augment.apply_train_transforms(data, seg, p), 0, 1)[0] for p in draws]
    out.append(f"{'nominal probabilities':<40s} median {statistics.median(ms):9.3f} ms   mean "
               f"{statistics.fmean(ms):9.3f}   max {max(ms):9.3f}   ({len(ms)} parameter draws, "
               "one timing each)")
    out.append(f"  draws with a spatial transform in some sample: "
               f"{sum(bool((p.do_rotate | p.do_scale).any()) for p in draws)}, with a "
               f"low-resolution channel: {sum(bool(p.lowres.any()) for p in draws)}")

    try:
        import scipy
        sec = cpu_one_sample(data_h, seg_h, full)
        out.append(f"numpy / scipy {scipy.__version__} restatement, all transforms drawn, ONE "
                   f"sample of {CHANNELS} x {SIZE}^3 on this host's CPU, one run: "
                   f"{sec * 1e3:9.1f} ms")
    except ImportError:
        out.append("scipy is not importable here: no CPU restatement timed")
    text = "\n".join(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
