"""Generate the data-loader golden fixtures by running the REFERENCE's own loader (CPU, numpy).

    python tests/golden/gen_loader_fixtures.py [--reference /root/reference]

Imports `light_training.dataloading.base_data_loader.DataLoaderMultiProcess` from the read-only
reference checkout (it needs numpy only) and runs it over four small synthetic cases, seeded, so
that tests can hold waveformer_amd.dataloading to the reference's random stream and to its slice +
np.pad without the reference being present.  Writes tests/golden/loader_fixtures.npz:

  case{i}_data (2, d, h, w) fp32, case{i}_seg (1, d, h, w) int8, case{i}_loc{label} (n, 4) int64
      rows (0, z, y, x): the four cases and their class_locations.  Shapes (11, 13, 9),
      (6, 13, 10), (9, 5, 14), (8, 8, 8): with the patch (8, 8, 8) the second is padded by an even
      and the third by an odd amount.  Case 0 has a foreground voxel at the origin and one in the
      far corner, case 1 an empty class list beside a full one, case 3 no foreground at all.
  {mode}_keys (40, 3), {mode}_force (40, 3) bool, {mode}_lbs (40, 3, 3): 40 consecutive batches
      of B = 3 after np.random.seed(5), for mode "last" (the last third of the batch is forced
      onto foreground) and "prob" (probabilistic oversampling); the flag and the box of every
      sample are read off the reference's get_bbox calls.
  {mode}_data (4, 3, 2, 8, 8, 8), {mode}_seg (4, 3, 1, 8, 8, 8) fp32: the first 4 batches.

The archive is written with fixed timestamps: the same reference gives the same bytes.
"""
from __future__ import annotations

import argparse
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = ((11, 13, 9), (6, 13, 10), (9, 5, 14), (8, 8, 8))
CHANNELS = 2
PATCH = (8, 8, 8)
BATCH = 3
SEED = 5
BATCHES, FULL = 40, 4
MODES = (("last", False), ("prob", True))


def make_cases():
    """[(data, seg, class_locations)]: data in eighths (exact in fp32, and it compresses), seg
    int8 with -1 (outside the nonzero crop), 0 and the labels 1, 2."""
    rs = np.random.RandomState(2024)
    cases = []
    for i, shape in enumerate(SHAPES):
        data = (rs.randint(-80, 81, size=(CHANNELS,) + shape) / 8.0).astype(np.float32)
        seg = rs.choice(np.array([-1, 0, 0, 0, 1, 2], dtype=np.int8), size=(1,) + shape)
        if i == 0:
            seg[0, 0, 0, 0] = 1
            seg[0, -1, -1, -1] = 2
        if i == 1:
            seg[seg == 2] = 0
        if i == 3:
            seg[seg > 0] = 0
        loc = {}
        for label in (1, 2):
            rows = np.argwhere(seg == label).astype(np.int64)
            if i == 0:  # keep the two corner voxels among few, so that the draws reach them
                corner = (0, 0, 0, 0) if label == 1 else (0,) + tuple(s - 1 for s in shape)
                pick = rs.choice(len(rows), 5, replace=False)
                rows = np.concatenate([np.array([corner], dtype=np.int64), rows[pick]])
            loc[label] = rows
        cases.append((data, seg.astype(np.int8), loc))
    return cases


def write_npz(path, arrays):
    """np.savez_compressed with the members' timestamps fixed."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from light_training.dataloading.base_data_loader import DataLoaderMultiProcess

    cases = make_cases()
    dataset = [{"data": d, "seg": s, "properties": {"class_locations": loc}}
               for d, s, loc in cases]
    out = {}
    for i, (d, s, loc) in enumerate(cases):
        out[f"case{i}_data"], out[f"case{i}_seg"] = d, s
        for label, rows in loc.items():
            out[f"case{i}_loc{label}"] = rows.reshape(-1, 4)

    for mode, prob in MODES:
        loader = DataLoaderMultiProcess(dataset, PATCH, batch_size=BATCH,
                                        oversample_foreground_percent=0.33,
                                        probabilistic_oversampling=prob)
        seen = []
        inner = loader.get_bbox

        def recording(shape, force_fg, locations, *a, _inner=inner, _seen=seen, **k):
            lbs, ubs = _inner(shape, force_fg, locations, *a, **k)
            _seen.append((bool(force_fg), [int(v) for v in lbs]))
            return lbs, ubs

        loader.get_bbox = recording
        np.random.seed(SEED)
        keys, data, seg = [], [], []
        for n in range(BATCHES):
            batch = next(loader)
            keys.append(np.asarray(batch["keys"], dtype=np.int64))
            if n < FULL:
                assert batch["data"].dtype == np.float32 and batch["seg"].dtype == np.float32
                data.append(batch["data"])
                seg.append(batch["seg"])
        assert len(seen) == BATCHES * BATCH
        out[f"{mode}_keys"] = np.stack(keys)
        out[f"{mode}_force"] = np.array([f for f, _ in seen]).reshape(BATCHES, BATCH)
        out[f"{mode}_lbs"] = np.array([b for _, b in seen], dtype=np.int64).reshape(BATCHES, BATCH, 3)
        out[f"{mode}_data"], out[f"{mode}_seg"] = np.stack(data), np.stack(seg)

        lbs = out[f"{mode}_lbs"].reshape(-1, 3)
        ext = np.array([SHAPES[k] for k in out[f"{mode}_keys"].reshape(-1)])
        print(f"{mode}: {int((lbs < 0).any(1).sum())} of {len(lbs)} boxes hang over a lower edge, "
              f"{int((lbs + np.array(PATCH) > ext).any(1).sum())} over an upper one, "
              f"{int((lbs[:, 2] % 4 != 0).sum())} start at an x that is no multiple of 4, "
              f"{int(out[f'{mode}_force'].sum())} were forced onto foreground")

    path = os.path.join(HERE, "loader_fixtures.npz")
    write_npz(path, out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
