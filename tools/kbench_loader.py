"""Times the making of a training batch from resident cases (waveformer_amd.dataloading) on the GPU.

The workload: B = 4, C = 4, patch 128^3, CASES synthetic cases of 4 x 137 x 191 x 161 fp32 (the size
a BraTS case has after the nonzero crop) with int8 segmentations and class_locations, all on the
device; the boxes are drawn as the loader draws them (the last third of the batch forced onto a
foreground voxel), so they hang over the cases' edges as they do in training.

Device time per batch: GROUP drawn batches are captured into one HIP graph (the launch takes its
table by value, so it can be) and the graph is replayed between two HIP events; a replay of GROUP
torch device-to-device copies of the same number of output bytes is timed the same way, the two
alternating, REPEATS times each after WARMUP untimed replays -- REPEATS * GROUP launches of each.
The copy reads as much as it writes; the batch kernel reads less (the padding is not read, and the
segmentation is read as int8).  Also, from the same run: the same batches launched one by one
from Python (HIP events and a host clock around generate_train_batch: what a training loop
sees), a loader whose every case comes from pinned host memory through the staging slots, and
the numpy restatement (tests/loader_ref.py) on this host's CPU.  The bytes are computed from
the shapes and the drawn boxes.  Reported, not gated.  The process ends itself after --limit
seconds.  --out FILE also writes the lines there."""
import argparse
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformer_amd import dataloading as dl  # noqa: E402
from waveformer_amd import ops  # noqa: E402

SHAPE = (137, 191, 161)
CHANNELS = 4
PATCH = (128, 128, 128)
BATCH = 4
HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specified peak


def make_case(i, dev):
    """(data, seg, properties): z-scored noise, a block of labels 1..3 in background 0 with a rim
    of -1, and up to 1000 voxels per class as preprocessing samples them."""
    g = torch.Generator(device=dev).manual_seed(100 + i)
    data = torch.randn((CHANNELS,) + SHAPE, device=dev, generator=g)
    seg = torch.zeros((1,) + SHAPE, dtype=torch.int8, device=dev)
    seg[:, :3] = -1
    z0, y0, x0 = 20 + 7 * i, 30 + 11 * i, 25 + 9 * i
    for label, r in ((2, 40), (1, 24), (3, 12)):
        seg[0, z0:z0 + r, y0:y0 + r, x0:x0 + r] = label
    rs = np.random.RandomState(i)
    loc = {}
    seg_h = seg[0].cpu().numpy()
    for label in (1, 2, 3):
        rows = np.argwhere(seg_h == label)
        rows = rows[rs.choice(len(rows), min(1000, len(rows)), replace=False)]
        loc[label] = np.concatenate([np.zeros((len(rows), 1), np.int64), rows], 1)
    return data, seg, {"class_locations": loc}


def plan_bytes(plan, shapes, seg_bytes=1):
    """(read, written) bytes of one batch: the voxels of each box inside its case are read once
    per channel (fp32) and once for the segmentation; every output element is written."""
    read = 0
    for key, lb in zip(plan.keys, plan.bbox_lbs):
        inside = 1
        for a in range(3):
            inside *= ops.crop_pad_axis_plan(int(lb[a]), PATCH[a], shapes[key][a])[2]
        read += inside * (CHANNELS * 4 + seg_bytes)
    return read, BATCH * (CHANNELS + 1) * int(np.prod(PATCH)) * 4


def replay_ms(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def line(name, ms, per=1):
    ms = [m / per for m in ms]
    return (f"{name:<58s} median {statistics.median(ms) * 1e3:9.1f} us   min {min(ms) * 1e3:9.1f}   "
            f"max {max(ms) * 1e3:9.1f}   ({len(ms)} timings)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=8)
    ap.add_argument("--group", type=int, default=10, help="batches per captured graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_loader: needs a GPU")
    signal.alarm(args.limit)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    cases = [make_case(i, dev) for i in range(args.cases)]
    store = dl.CaseStore(device=dev)
    for c in cases:
        store.add(*c)
    shapes = [tuple(c[0].shape[1:]) for c in cases]
    loader = dl.DataLoaderMultiProcess(store, PATCH, BATCH, rng=np.random.RandomState(0))
    plans = [loader.draw_batch_plan() for _ in range(args.group)]
    traffic = [plan_bytes(p, shapes) for p in plans]
    rd, wr = sum(t[0] for t in traffic) / len(traffic), traffic[0][1]
    per_case = store.nbytes_device / len(store)
    out = [f"training batch B = {BATCH}, C = {CHANNELS}, patch {PATCH[0]}^3 from {len(store)} "
           f"resident cases of {CHANNELS} x {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} fp32 + int8 seg, "
           f"{torch.cuda.get_device_name(0)}",
           f"bytes per resident case {per_case / 1e6:.1f} MB (data {4 * CHANNELS * np.prod(SHAPE) / 1e6:.1f}"
           f" + seg {np.prod(SHAPE) / 1e6:.1f}); the store holds {store.nbytes_device / 1e6:.1f} MB",
           f"per batch, mean over the {len(plans)} drawn plans: {rd / 1e6:.1f} MB read, "
           f"{wr / 1e6:.1f} MB written; boxes over an edge: "
           f"{sum(int(((p.bbox_lbs < 0) | (p.bbox_lbs + 128 > np.array([shapes[k] for k in p.keys]))).any(1).sum()) for p in plans)}"
           f" of {len(plans) * BATCH}; forced onto foreground: {sum(int(p.force_fg.sum()) for p in plans)}"]

    # ---- device time: captured launches against captured copies -------------------------
    src = torch.randn((wr // 4,), device=dev)
    dst = torch.empty_like(src)
    loader.execute_batch_plan(plans[0])
    dst.copy_(src)
    torch.cuda.synchronize()
    g_batch, g_copy = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g_batch):
        for p in plans:
            keep.append(loader.execute_batch_plan(p))
    with torch.cuda.graph(g_copy):
        for _ in plans:
            dst.copy_(src)
    for _ in range(args.warmup):
        replay_ms(g_batch), replay_ms(g_copy)
    t_b, t_c = [], []
    for _ in range(args.repeats):  # alternate the two
        t_b.append(replay_ms(g_batch))
        t_c.append(replay_ms(g_copy))
    n = len(plans)
    mb, mc = statistics.median(t_b) / n * 1e-3, statistics.median(t_c) / n * 1e-3
    out.append(f"device time per batch, {n} launches per graph replay, "
               f"{args.repeats * n} launches of each:")
    out.append(line("  wf_crop_pad_batch (one launch per batch)", t_b, n))
    out.append(f"    {(rd + wr) / 1e6:.1f} MB moved = {(rd + wr) / mb / 1e9:.0f} GB/s = "
               f"{100 * (rd + wr) / mb / HBM_PEAK:.1f} % of the HBM peak of {HBM_PEAK / 1e12:.1f} TB/s")
    out.append(line(f"  torch copy_ of {wr / 1e6:.1f} MB, device to device", t_c, n))
    out.append(f"    {2 * wr / 1e6:.1f} MB moved = {2 * wr / mc / 1e9:.0f} GB/s = "
               f"{100 * 2 * wr / mc / HBM_PEAK:.1f} % of the HBM peak")
    out.append(f"  batch kernel / copy = {mb / mc:.2f} (more than 1.5 would be a finding)")

    # ---- launched one by one from Python -----------------------------------------------
    def one_by_one(ld, count):
        ev, wall = [], []
        for _ in range(count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            ld.generate_train_batch()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        return ev, wall

    one_by_one(loader, 5)
    ev, wall = one_by_one(loader, 100)
    out.append("generate_train_batch, draw + launch from Python, 100 batches, resident cases:")
    out.append(line("  HIP events around the call", ev))
    out.append(line("  host clock, synchronised before and after", wall))

    # ---- every case from pinned host memory ---------------------------------------------
    host = dl.CaseStore(device_bytes=0, device=dev)
    for c in cases:
        host.add(*c)
    hl = dl.DataLoaderMultiProcess(host, PATCH, BATCH, rng=np.random.RandomState(0))
    one_by_one(hl, 3)
    ev, wall = one_by_one(hl, 30)
    out.append(f"the same from pinned host memory ({host.nbytes_host / 1e6:.1f} MB pinned, "
               f"{BATCH} staging slots, {BATCH * per_case / 1e6:.1f} MB copied per batch), 30 batches:")
    out.append(line("  HIP events around the call", ev))
    out.append(line("  host clock, synchronised before and after", wall))
    out.append(f"    host-to-device rate {BATCH * per_case / (statistics.median(wall) * 1e-3) / 1e9:.1f} GB/s")

    # ---- the numpy restatement on this host's CPU ---------------------------------------
    from tests import loader_ref as ref
    cases_h = [(c["data"].numpy(), c["seg"].numpy()) for c in (host[i] for i in range(len(host)))]
    cpu = []
    for p in plans[:5]:
        t0 = time.perf_counter()
        want = ref.crop_pad_batch([cases_h[k] for k in p.keys], p.bbox_lbs, PATCH)
        cpu.append((time.perf_counter() - t0) * 1e3)
    out.append(line("numpy restatement (slice + zero pad), one core, per batch", cpu))
    got = loader.execute_batch_plan(plans[4])
    same = all(np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32))
               for g, w in zip((got["data"], got["seg"]), want))
    out.append(f"the last of those batches against the kernel's, on the bits: "
               f"{'equal' if same else 'DIFFERENT'}")
    out.append(f"peak device memory of this process {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB")

    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not same:
        raise SystemExit("kbench_loader: the kernel's batch differs from the restatement")


if __name__ == "__main__":
    main()
