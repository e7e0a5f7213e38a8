"""Evaluation on the GPU: per-region Dice and exact HD95 of a prediction against the ground truth.

The reference scores every saved case on the CPU (5_compute_metrics.py: convert_labels, then
medpy.metric.binary.dc and hd95 per region TC / WT / ET).  Here the masks, the overlap counts,
the borders, the exact squared Euclidean distance transform, the surface-distance histograms and
their order statistics are HIP kernels (csrc/metrics.hip, integer arithmetic only), and a case
costs one small device-to-host copy.  What is left to the host is float64 on a handful of
integers: dice = 2 tp / (|a| + |b|), one square root per order statistic and numpy's percentile
interpolation -- the same operations medpy and numpy perform, so the results agree with them to
the last bit whenever the integers do.

`convert_labels`, `cal_metric` and `each_cases_metric` keep the reference script's names and
argument order, so a 5_compute_metrics.py-style caller switches by import.  GPU only: host
inputs are moved to the current device, and there is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

# region r contains class c iff bit c is set; TC, WT, ET as convert_labels builds them
BRATS_REGIONS: Tuple[int, ...] = ((1 << 1) | (1 << 3), (1 << 1) | (1 << 2) | (1 << 3), 1 << 3)
EMPTY_METRIC: Tuple[float, float] = (0.0, 50.0)  # cal_metric's value when a mask is empty
EXTRA_FIELDS = ("dice", "hd95", "hd", "asd_pred_to_gt", "asd_gt_to_pred", "assd")
# the ranks asked of the device relative to base = q (n - 1) // 100: float64's
# floor(q / 100 * (n - 1)) is base or base - 1, and the percentile needs that rank and the next
_RANK_OFFSETS = (-1, 0, 1, 2)
_Q_DEN = 100000  # q is passed to the device as the integer q * 1000 over 10^5

ArrayLike = Union[np.ndarray, torch.Tensor]


def region_bits(regions: Sequence) -> Tuple[int, ...]:
    """Class bitmasks of a region table given as bitmasks (ints) or as collections of class
    values, e.g. [{1, 3}, {1, 2, 3}, {3}]."""
    out = []
    for r in regions:
        if isinstance(r, (int, np.integer)):
            bits = int(r)
        else:
            bits = 0
            for c in r:
                if not 0 <= int(c) <= 7:
                    raise ValueError(f"region class {c}: classes are 0..7")
                bits |= 1 << int(c)
        if not 0 <= bits <= 255:
            raise ValueError(f"region bitmask {bits}: classes are 0..7")
        out.append(bits)
    if not 1 <= len(out) <= 4:
        raise ValueError(f"need 1..4 regions, got {len(out)}")
    return tuple(out)


def percentile_from_order_stats(n: int, lo_sq: int, hi_sq: int, q: float) -> float:
    """np.percentile(np.sqrt(d2), q) of a sample of n squared distances from two of its order
    statistics: with v = q / 100 * (n - 1), k = floor(v) and t = v - k, lo_sq is the element of
    0-based rank k and hi_sq that of rank min(k + 1, n - 1) of the sorted sample.  numpy's
    linear interpolation, in float64: x + (y - x) t for t < 0.5, else y - (y - x) (1 - t)."""
    if n < 1:
        raise ValueError("percentile of an empty sample")
    v = np.float64(q) / np.float64(100.0) * np.float64(n - 1)
    t = v - np.floor(v)
    x = np.sqrt(np.float64(lo_sq))
    y = np.sqrt(np.float64(hi_sq))
    d = y - x
    return float(x + d * t if t < 0.5 else y - d * (np.float64(1.0) - t))


def percentile_rank(n: int, q: float) -> int:
    """k = floor(q / 100 * (n - 1)) as float64 computes it (numpy's lower neighbour)."""
    return int(np.floor(np.float64(q) / np.float64(100.0) * np.float64(n - 1)))


def _spacing(spacing) -> float:
    s = np.atleast_1d(np.asarray(spacing, dtype=np.float64))
    if s.size == 0 or not np.all(s == s[0]):
        raise NotImplementedError(
            f"voxel spacing {spacing!r}: only isotropic spacing is implemented (an anisotropic "
            "one makes the squared surface distances non-integer, which the exact histogram "
            "needs)")
    if not s[0] > 0:
        raise ValueError(f"voxel spacing must be positive, got {spacing!r}")
    return float(s[0])


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("waveformer_amd.metrics runs on the GPU only (no CUDA/HIP device)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_gpu(x: ArrayLike, name: str) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a numpy array or a tensor, got {type(x)}")
    if x.device.type != "cuda":
        x = x.to(_device())
    return x


def _label_map(x: torch.Tensor, name: str) -> torch.Tensor:
    """An integer (or integer-valued) label map as contiguous uint8."""
    if x.dtype != torch.uint8:
        x = x.to(torch.uint8)  # class values are 0..7
    return x.contiguous()


def _case(pred: torch.Tensor, gt: torch.Tensor, bits: Tuple[int, ...], q: float, extra: bool):
    """Launch everything for one case; returns the device buffers to copy: the int64 result
    {R x (tp, |a|, |b|), R x order stats} and, for extra, the histograms."""
    R = len(bits)
    size = tuple(gt.shape)
    masks = torch.empty((2 * R,) + size, dtype=torch.uint8, device=gt.device)
    result = torch.empty((R * 3 + R * ops.ORDER_STATS_STRIDE,), dtype=torch.int64,
                         device=gt.device)
    scratch = torch.empty((2 * R,), dtype=torch.int64, device=gt.device)
    ops.region_masks(pred, bits, out=masks[:R], counts=scratch[:R])
    ops.region_masks(gt, bits, out=masks[R:], counts=scratch[R:])
    ops.overlap_counts(masks[:R], masks[R:], out=result[:R * 3])
    border, d2 = ops.surface_edt_sq(masks)
    hist = ops.surface_hist(border[:R], d2[R:], border[R:], d2[:R])
    qn = int(round(q * 1000))
    ops.hist_order_stats(hist, _RANK_OFFSETS, q=(qn, _Q_DEN), group=2, out=result[R * 3:])
    return result, (hist if extra else None)


def _finish(result: np.ndarray, hist: Optional[np.ndarray], R: int, q: float, spacing: float,
            empty: Tuple[float, float], extra: bool) -> np.ndarray:
    counts = result[:R * 3].reshape(R, 3)
    stats = result[R * 3:].reshape(R, ops.ORDER_STATS_STRIDE)
    out = np.zeros((R, len(EXTRA_FIELDS) if extra else 2), dtype=np.float64)
    for r in range(R):
        tp, na, nb = (int(v) for v in counts[r])
        if na == 0 or nb == 0:
            out[r, 0], out[r, 1] = float(empty[0]), float(empty[1])
            if extra:
                out[r, 2:] = float(empty[1])
            continue
        out[r, 0] = 2.0 * tp / float(na + nb)
        n, top, base = (int(v) for v in stats[r, :3])
        k = percentile_rank(n, q)
        vals = {min(max(base + o, 0), n - 1): int(stats[r, 3 + i])
                for i, o in enumerate(_RANK_OFFSETS)}
        out[r, 1] = percentile_from_order_stats(n, vals[k], vals[min(k + 1, n - 1)], q) * spacing
        if extra:
            out[r, 2] = math.sqrt(top) * spacing
            asd = []
            for d in range(2):
                h = hist[r, d]
                nz = np.flatnonzero(h)  # ascending bins
                s = 0.0
                for b in nz:
                    s += math.sqrt(int(b)) * int(h[b])
                asd.append(s / float(int(h[nz].astype(np.int64).sum())) * spacing)
            out[r, 3], out[r, 4] = asd
            out[r, 5] = (asd[0] + asd[1]) / 2.0
    return out


def region_metrics(pred: ArrayLike, gt: ArrayLike, regions: Sequence = BRATS_REGIONS,
                   spacing=1.0, empty: Tuple[float, float] = EMPTY_METRIC,
                   extra: bool = False) -> np.ndarray:
    """[dice, hd95] per region of a prediction against the ground truth, computed on the GPU.

    pred: a label map (D, H, W), a batch of them (N, D, H, W), or class scores (C, D, H, W) of a
      floating dtype, whose arg-max over C (first index on ties, as torch.argmax) is the label.
    gt: a label map (D, H, W), or (N, D, H, W) beside a batch of predictions.
    regions: up to 4 regions as class bitmasks or collections of class values (classes 0..7);
      the default is BraTS' TC {1, 3}, WT {1, 2, 3}, ET {3}.
    spacing: ONE positive voxel size, multiplied into the distances at the end.  Anisotropic
      spacing raises NotImplementedError: the method rests on squared distances being integers.
    empty: [dice, hd95] of a region where either mask is empty (cal_metric's [0.0, 50]).
    extra: also return hd (the maximum surface distance over both directions), the average
      surface distance pred -> gt and gt -> pred, and their mean assd (EXTRA_FIELDS order;
      an empty region gets empty[1] in all of them).  This copies the histograms to the host.

    Returns a float64 numpy array (R, 2) -- (N, R, 2) for a batch -- in the layout of the
    reference's all_results[i]; (…, R, 6) with extra.  dice = 2 tp / (|a| + |b|) as medpy's dc,
    hd95 = medpy's hd95: the 95th percentile of the surface distances of both directions.
    """
    sp = _spacing(spacing)
    bits = region_bits(regions)
    q = 95.0
    p = _to_gpu(pred, "pred")
    g = _label_map(_to_gpu(gt, "gt"), "gt")
    scores = p.dim() == 4 and p.dtype.is_floating_point
    if scores:
        if g.dim() != 3 or tuple(p.shape[1:]) != tuple(g.shape):
            raise ValueError(f"scores {tuple(p.shape)} do not match gt {tuple(g.shape)}")
        if p.dtype not in (torch.float16, torch.float32):
            p = p.float()
        preds, gts, batched = [p.contiguous()], [g], False
    else:
        p = _label_map(p, "pred")
        if p.shape != g.shape or p.dim() not in (3, 4):
            raise ValueError(f"pred {tuple(p.shape)} and gt {tuple(g.shape)}: expected two "
                             "(D, H, W) or two (N, D, H, W) label maps")
        batched = p.dim() == 4
        preds, gts = (list(p), list(g)) if batched else ([p], [g])
    launched = [_case(pi, gi, bits, q, extra) for pi, gi in zip(preds, gts)]
    # the only device-to-host traffic: one int64 buffer for all cases (and the histograms)
    if len(launched) == 1:
        result = launched[0][0].cpu().numpy()[None]
    else:
        result = torch.stack([r for r, _ in launched]).cpu().numpy()
    outs = []
    for i, (_, h) in enumerate(launched):
        hn = h.cpu().numpy() if h is not None else None
        outs.append(_finish(result[i], hn, len(bits), q, sp, empty, extra))
    return np.stack(outs) if batched else outs[0]


def result_bytes(regions: Sequence = BRATS_REGIONS) -> int:
    """Size of the device-to-host copy region_metrics makes per case (without extra)."""
    R = len(region_bits(regions))
    return (R * 3 + R * ops.ORDER_STATS_STRIDE) * 8


# ------------------------------------------------------------------------------------------
# the reference script's helpers, by name
# ------------------------------------------------------------------------------------------
def convert_labels(labels: ArrayLike) -> torch.Tensor:
    """5_compute_metrics.convert_labels: a label map (...) -> (3, ...) float masks TC, WT, ET.
    3-D inputs run on the GPU kernel; the result is on the GPU."""
    x = _label_map(_to_gpu(labels, "labels"), "labels")
    lead = x.shape[:-3]
    if x.dim() < 3:
        raise ValueError(f"convert_labels: expected at least (D, H, W), got {tuple(x.shape)}")
    flat = x.reshape((-1,) + tuple(x.shape[-3:]))
    if flat.shape[0] != 1:
        raise ValueError("convert_labels: one label map at a time (leading dims of size 1)")
    masks, _, _ = ops.region_masks(flat[0].contiguous(), BRATS_REGIONS)
    return masks.reshape((3,) + tuple(lead) + tuple(x.shape[-3:])).float()


def _binary(x: ArrayLike, name: str) -> torch.Tensor:
    t = _to_gpu(x, name)
    return (t != 0).to(torch.uint8).contiguous()


def cal_metric(gt: ArrayLike, pred: ArrayLike, voxel_spacing=1.0) -> np.ndarray:
    """5_compute_metrics.cal_metric: [dice, hd95] of two binary masks (D, H, W) (non-zero =
    set), [0.0, 50] when either is empty."""
    g, p = _binary(gt, "gt"), _binary(pred, "pred")
    return region_metrics(p, g, regions=(1 << 1,), spacing=voxel_spacing)[0]


def each_cases_metric(gt: ArrayLike, pred: ArrayLike, voxel_spacing=1.0) -> np.ndarray:
    """5_compute_metrics.each_cases_metric: gt and pred are (3, D, H, W) stacks of region
    masks (convert_labels' output); returns (3, 2) [dice, hd95] per region."""
    g, p = _binary(gt, "gt"), _binary(pred, "pred")
    if g.dim() != 4 or g.shape != p.shape:
        raise ValueError(f"each_cases_metric: expected two (R, D, H, W) stacks, got "
                         f"{tuple(g.shape)} and {tuple(p.shape)}")
    # a batch of R binary "label maps", each scored against class 1
    return region_metrics(p, g, regions=(1 << 1,), spacing=voxel_spacing)[:, 0]
