"""Generates tests/golden/metrics_fixtures.npz: small label-map pairs and the region Dice / HD95
values a scipy restatement of medpy.metric.binary gives for them.  Run on a CPU host with scipy;
no test imports scipy, they read only the .npz.

    python tests/golden/gen_metrics_fixtures.py

medpy's hd95(result, reference), restated (medpy/metric/binary.py, __surface_distances):
    footprint = generate_binary_structure(3, 1)
    border = mask ^ binary_erosion(mask, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=None)
    sds = dt[result_border]
    hd95 = np.percentile(np.hstack((sds(result, reference), sds(reference, result))), 95)

Per case NAME the file holds NAME_pred / NAME_gt (uint8 label maps), NAME_float (R, 6) float64
[dice, hd95, hd, asd pred->gt, asd gt->pred, assd] (NaN where a mask of the region is empty:
medpy raises there) and NAME_int (R, 11) int64 [n, lo_sq, hi_sq, max d2, n and max d2 of
pred->gt, n and max d2 of gt->pred, tp, |pred|, |gt|] (-1 for the surface values of an empty
region); lo_sq / hi_sq are the squared distances of ranks k = floor(0.95 (n - 1)) and
min(k + 1, n - 1) of the joint sorted sample.  Regions are BraTS' TC {1, 3}, WT {1, 2, 3}, ET {3}.
"""
import os

import numpy as np
from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

HERE = os.path.dirname(os.path.abspath(__file__))
REGIONS = ((1, 3), (1, 2, 3), (3,))

# name: (shape, centre, radius, jitter of the prediction's centre)
CASES = {
    "w67_h70": ((9, 70, 67), (4, 35, 30), 9, (0, 2, -3)),
    "w130": ((12, 33, 130), (6, 16, 40), 7, (1, -1, 60)),
    "d1": ((1, 20, 21), (0, 10, 10), 6, (0, 1, 1)),
    "h1": ((5, 1, 9), (2, 0, 4), 3, (0, 0, 1)),
    "no_et_pred": ((16, 18, 20), (8, 9, 10), 6, (1, 0, -1)),
}


def ball(shape, centre, radius):
    idx = np.indices(shape)
    return sum((idx[ax] - centre[ax]) ** 2 for ax in range(3)) <= radius * radius


def label_map(shape, c, r, et=True):
    """WT: ball r at c, class 2; TC: ball 0.6 r at c + 1, class 1; ET: ball 0.35 r at c - 1,
    class 3, written in that order."""
    lab = np.zeros(shape, dtype=np.uint8)
    lab[ball(shape, c, r)] = 2
    lab[ball(shape, [v + 1 for v in c], 0.6 * r)] = 1
    if et:
        lab[ball(shape, [v - 1 for v in c], 0.35 * r)] = 3
    return lab


def build(name):
    if name == "both_empty":
        z = np.zeros((4, 4, 4), dtype=np.uint8)
        return z.copy(), z
    if name == "full":
        shape = (6, 5, 7)
        return np.full(shape, 2, dtype=np.uint8), label_map(shape, (3, 2, 3), 2)
    shape, c, r, jit = CASES[name]
    gt = label_map(shape, c, r)
    pred = label_map(shape, [a + b for a, b in zip(c, jit)], r, et=name != "no_et_pred")
    if name == "w67_h70":
        pred[8, 69, 66] = 2  # an isolated voxel on three faces of the volume, far from the rest
    return pred, gt


def surface_distances(result, reference):
    footprint = generate_binary_structure(3, 1)
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=None)
    return dt[result_border]


def region_values(pred_mask, gt_mask):
    f = np.full(6, np.nan)
    i = np.full(11, -1, dtype=np.int64)
    i[8:] = (pred_mask & gt_mask).sum(), pred_mask.sum(), gt_mask.sum()
    if not pred_mask.any() or not gt_mask.any():
        return f, i
    s_ab = surface_distances(pred_mask, gt_mask)
    s_ba = surface_distances(gt_mask, pred_mask)
    both = np.hstack((s_ab, s_ba))
    f[0] = 2.0 * i[8] / float(i[9] + i[10])          # medpy dc
    f[1] = np.percentile(both, 95)                   # medpy hd95
    f[2] = max(s_ab.max(), s_ba.max())               # medpy hd
    f[3], f[4] = s_ab.mean(), s_ba.mean()            # medpy asd, both directions
    f[5] = np.mean((f[3], f[4]))                     # medpy assd
    sq = [np.rint(s * s).astype(np.int64) for s in (s_ab, s_ba)]
    for s, d2 in zip((s_ab, s_ba), sq):
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), s), "EDT is not sqrt(integer)"
    srt = np.sort(np.hstack(sq))
    n = len(srt)
    k = int(np.floor(np.float64(95) / np.float64(100.0) * np.float64(n - 1)))
    i[:8] = (n, srt[k], srt[min(k + 1, n - 1)], srt[-1], len(sq[0]), sq[0].max(), len(sq[1]),
             sq[1].max())
    return f, i


def main():
    out = {}
    empty_regions, interpolating = 0, 0
    for name in list(CASES) + ["both_empty", "full"]:
        pred, gt = build(name)
        fs, is_ = [], []
        for classes in REGIONS:
            f, i = region_values(np.isin(pred, classes), np.isin(gt, classes))
            fs.append(f)
            is_.append(i)
            if name in CASES:
                empty_regions += int(i[0] < 0)
                interpolating += int(i[0] > 0 and i[1] != i[2])
        out[f"{name}_pred"], out[f"{name}_gt"] = pred, gt
        out[f"{name}_float"], out[f"{name}_int"] = np.stack(fs), np.stack(is_)
        print(name, pred.shape)
        print(np.stack(is_))
        print(np.stack(fs))
    assert empty_regions == 1, f"{empty_regions} empty regions over the table's cases, want 1"
    assert interpolating >= 1, "no region whose percentile interpolates between two distances"
    path = os.path.join(HERE, "metrics_fixtures.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
