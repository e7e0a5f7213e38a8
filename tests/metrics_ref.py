"""numpy brute-force oracle of the evaluation metrics (waveformer_amd.metrics), with no scipy:
border by shifted ANDs on a zero-padded mask, squared distances by the minimum over the border
voxels, statistics as medpy / numpy compute them.  Small volumes only (memory ~ voxels x
border voxels)."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_fixtures.npz")
BRATS_BITS = (0b1010, 0b1110, 0b1000)  # TC {1, 3}, WT {1, 2, 3}, ET {3}
CASES = ("w67_h70", "w130", "d1", "h1", "no_et_pred")  # the issue's table
EXTRA_CASES = ("both_empty", "full")
EDT_NONE = 0xFFFFFFFF
# columns of the recorded tables
FLOAT_COLS = ("dice", "hd95", "hd", "asd_pred_to_gt", "asd_gt_to_pred", "assd")
INT_COLS = ("n", "lo_sq", "hi_sq", "max_d2", "n_pred_to_gt", "max_pred_to_gt", "n_gt_to_pred",
            "max_gt_to_pred", "tp", "size_pred", "size_gt")


@functools.lru_cache(maxsize=None)
def fixtures():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def region_masks(labels, bits=BRATS_BITS):
    lab = labels.astype(np.int64)
    return np.stack([((1 << lab) & b) != 0 for b in bits]).astype(np.uint8)


def border(mask):
    """mask & ~erosion by the 6-neighbour cross, the outside of the volume being 0."""
    m = mask.astype(bool)
    p = np.pad(m, 1, constant_values=False)
    er = p[1:-1, 1:-1, 1:-1].copy()
    er &= p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    er &= p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
    er &= p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return (m & ~er).astype(np.uint8)


def edt_sq(bd):
    """Exact squared distance of every voxel to the nearest voxel of `bd`, uint32 (EDT_NONE when
    bd is empty)."""
    pts = np.argwhere(bd)
    if len(pts) == 0:
        return np.full(bd.shape, EDT_NONE, dtype=np.uint32)
    axes = [np.arange(n, dtype=np.int32) for n in bd.shape]
    best = np.full(bd.shape, np.iinfo(np.int32).max, dtype=np.int32)
    for s in range(0, len(pts), 64):
        p = pts[s:s + 64].astype(np.int32)
        dz, dy, dx = ((axes[ax][:, None] - p[None, :, ax]) ** 2 for ax in range(3))
        d = dz[:, None, None, :] + dy[None, :, None, :] + dx[None, None, :, :]
        np.minimum(best, d.min(-1), out=best)
    return best.reshape(bd.shape).astype(np.uint32)


def pair_stats(a, b, q=95, edt_a=None, edt_b=None):
    """Everything recorded per region for masks a (prediction) and b (ground truth): a dict of
    the INT_COLS / FLOAT_COLS values and the two histograms' samples, or None when a mask is
    empty (only tp and the sizes are meaningful then).  edt_a / edt_b: edt_sq of the two borders
    where the caller has them already."""
    a, b = a.astype(bool), b.astype(bool)
    ints = dict.fromkeys(INT_COLS, -1)
    ints.update(tp=int((a & b).sum()), size_pred=int(a.sum()), size_gt=int(b.sum()))
    if not a.any() or not b.any():
        return ints, None, None
    ba, bb = border(a), border(b)
    edt_a = edt_sq(ba) if edt_a is None else edt_a
    edt_b = edt_sq(bb) if edt_b is None else edt_b
    d_ab = edt_b[ba.astype(bool)].astype(np.int64)  # pred's border -> gt's border
    d_ba = edt_a[bb.astype(bool)].astype(np.int64)
    both = np.hstack((d_ab, d_ba))
    s = np.sort(both)
    n = len(s)
    k = int(np.floor(np.float64(q) / np.float64(100.0) * np.float64(n - 1)))
    ints.update(n=n, lo_sq=int(s[k]), hi_sq=int(s[min(k + 1, n - 1)]), max_d2=int(s[-1]),
                n_pred_to_gt=len(d_ab), max_pred_to_gt=int(d_ab.max()), n_gt_to_pred=len(d_ba),
                max_gt_to_pred=int(d_ba.max()))
    r_ab, r_ba = np.sqrt(d_ab.astype(np.float64)), np.sqrt(d_ba.astype(np.float64))
    asd_ab, asd_ba = r_ab.mean(), r_ba.mean()
    floats = dict(dice=2.0 * ints["tp"] / float(ints["size_pred"] + ints["size_gt"]),
                  hd95=np.percentile(np.hstack((r_ab, r_ba)), q),
                  hd=max(r_ab.max(), r_ba.max()), asd_pred_to_gt=asd_ab, asd_gt_to_pred=asd_ba,
                  assd=np.mean((asd_ab, asd_ba)))
    return ints, floats, (d_ab, d_ba)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """Per fixture case, computed once: masks (2, R, D, H, W) [pred, gt], their borders and
    brute-force squared distances, and the per-region pair_stats."""
    fx = fixtures()
    pred, gt = fx[f"{name}_pred"], fx[f"{name}_gt"]
    masks = np.stack([region_masks(pred), region_masks(gt)])
    bd = np.stack([[border(m) for m in side] for side in masks])
    d2 = np.stack([[edt_sq(x) for x in side] for side in bd])
    stats = [pair_stats(masks[0, r], masks[1, r], edt_a=d2[0, r], edt_b=d2[1, r])
             for r in range(masks.shape[1])]
    for arr in (masks, bd, d2):
        arr.setflags(write=False)
    return dict(pred=pred, gt=gt, masks=masks, border=bd, d2=d2, stats=stats)
