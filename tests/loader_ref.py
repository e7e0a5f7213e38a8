"""numpy restatement of what a training batch is: for every sample the part of the patch box
[lb, lb + patch) that lies inside its case, copied, with zeros for the rest, in the data and in
the segmentation, both float32 (the slice + np.pad of the reference's generate_train_batch).
Written from that description; also loads tests/golden/loader_fixtures.npz."""
import os

import numpy as np

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "loader_fixtures.npz")
PATCH = (8, 8, 8)
BATCH = 3
SEED = 5
MODES = (("last", False), ("prob", True))


def axis_plan(lb, patch, extent):
    """(dst0, src0, n): out[dst0:dst0 + n] = in[src0:src0 + n]; (0, 0, 0) when nothing overlaps."""
    lo, hi = max(lb, 0), min(lb + patch, extent)
    n = max(hi - lo, 0)
    return (lo - lb, lo, n) if n else (0, 0, 0)


def crop_pad(x, lb, patch):
    """x (N, D, H, W) of any dtype -> (N, *patch) float32."""
    out = np.zeros((x.shape[0],) + tuple(patch), dtype=np.float32)
    src, dst = [slice(None)], [slice(None)]
    for a in range(3):
        d0, s0, n = axis_plan(int(lb[a]), int(patch[a]), int(x.shape[1 + a]))
        src.append(slice(s0, s0 + n))
        dst.append(slice(d0, d0 + n))
    out[tuple(dst)] = x[tuple(src)]
    return out


def crop_pad_batch(cases, lbs, patch):
    """cases: [(data, seg)] numpy; -> (data (B, C, *patch), seg (B, S, *patch)) float32."""
    return (np.stack([crop_pad(d, lb, patch) for (d, _), lb in zip(cases, lbs)]),
            np.stack([crop_pad(s, lb, patch) for (_, s), lb in zip(cases, lbs)]))


_cache = {}


def fixtures():
    """The fixture archive as a dict of arrays (read once)."""
    if "fx" not in _cache:
        with np.load(FIXTURES) as z:
            _cache["fx"] = {k: z[k] for k in z.files}
    return _cache["fx"]


def fixture_dataset():
    """[{"data", "seg", "properties": {"class_locations": {1: rows, 2: rows}}}] of the 4 cases."""
    fx = fixtures()
    return [{"data": fx[f"case{i}_data"], "seg": fx[f"case{i}_seg"],
             "properties": {"class_locations": {label: fx[f"case{i}_loc{label}"]
                                                for label in (1, 2)}}}
            for i in range(4)]
