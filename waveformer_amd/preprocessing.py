"""Preprocessing of one case on the GPU: crop to the hole-filled nonzero mask, z-score every
modality, mark the outside in the segmentation and record the `properties` that
waveformer_amd.prediction.Predictor later undoes.

This restates the array transform of the reference's step 2 (2_preprocessing_mri.py ->
light_training/preprocessing/preprocessors/preprocessor_mri.py MultiModalityPreprocessor and its
base default_preprocessor.py DefaultPreprocessor.run_case_npy, :155-228) on HIP kernels
(csrc/preprocess.hip):

  * create_nonzero_mask (cropping/cropping.py:8-21): OR over channels of data[c] != 0 with
    numpy's comparison (-0.0 is zero, a denormal and a NaN are not), then
    scipy.ndimage.binary_fill_holes with its default structure: everything except the background
    joined to the array border by a 6-connected background path;
  * the bounding box of the filled mask in acvl_utils' get_bbox_from_mask form, half-open
    [[z0, z1], [y0, y1], [x0, x1]] -- what Predictor.predict_noncrop_probability slices with;
  * crop_to_nonzero (cropping.py:24-49): data and seg cropped to the box, seg == 0 outside the
    mask becomes -1; without a seg, 0 inside the mask and -1 outside;
  * ZScoreNormalization(use_mask_for_norm=False) (preprocessor_mri.py:48-55,
    normalization/default_normalization_schemes.py:28-50): per channel, mean and population std
    over the WHOLE cropped volume, (x - mean) / max(std, 1e-8) in fp32; the moments are fp64;
  * _sample_foreground_locations and collect_foreground_intensities
    (default_preprocessor.py:414-483): the host draws ranks from numpy's RandomState exactly as
    the reference does, from per-class voxel counts; the device turns a rank into "the k-th set
    voxel in C order".  Nothing of the size of the volume crosses to the host, and the samples
    equal the reference's.

  * resampling (resampling/default_resampling.py, waveformer_amd.resampling): when
    compute_new_shape differs from the cropped shape the reference resizes the normalised data
    (order 3, clamped to each channel's range) and the segmentation (per label, order 1).
    MultiModalityPreprocessor(resample=True) does the same on the device (csrc/resample.hip) and
    draws class_locations on the resampled segmentation; with the default resample=False such a
    case raises NotImplementedError, as before (BraTS at 1 mm isotropic with out_spacing 1 mm
    never resamples).

File I/O (read_data, run,
run_plan: SimpleITK and the dataset plan) is out of scope, and `intensity_statistics_per_channel`
is left out (the reference calls it unused at :428).  Segmentations hold integer labels that fit
int16.  GPU only: host inputs are moved to the current device, and there is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .resampling import compute_new_shape, resample_data_or_seg_to_shape  # noqa: F401

ArrayLike = Union[np.ndarray, torch.Tensor]
NUM_SAMPLES = 10000          # default_preprocessor.py:415, :457
MIN_PERCENT_COVERAGE = 0.01  # :458
PROPERTY_KEYS = ("original_spacing_trans", "target_spacing_trans", "shape_before_cropping",
                 "bbox_used_for_cropping", "shape_after_cropping_before_resample",
                 "shape_after_resample", "class_locations")


# ------------------------------------------------------------------------------------------
# host arithmetic (no GPU needed)
# ------------------------------------------------------------------------------------------
def target_num_samples(n: int, num_samples: int = NUM_SAMPLES,
                       min_percent_coverage: float = MIN_PERCENT_COVERAGE) -> int:
    """default_preprocessor.py:475-476: max(min(num_samples, n), ceil(n * coverage))."""
    return max(min(num_samples, n), int(np.ceil(n * min_percent_coverage)))


def draw_location_ranks(counts: Sequence[int], seed: int = 1234) -> List[Optional[np.ndarray]]:
    """The ranks _sample_foreground_locations picks for classes with `counts` voxels each, in
    class order from ONE RandomState(seed): choice(n, target, replace=False) per present class,
    None (and no draw) for an absent one (:460-479)."""
    rs = np.random.RandomState(seed)
    out: List[Optional[np.ndarray]] = []
    for n in counts:
        n = int(n)
        out.append(rs.choice(n, target_num_samples(n), replace=False).astype(np.int64)
                   if n > 0 else None)
    return out


def draw_intensity_ranks(num_fg: int, channels: int, seed: int = 1234,
                         num_samples: int = NUM_SAMPLES) -> List[Optional[np.ndarray]]:
    """The ranks collect_foreground_intensities picks: rs.choice(array, k, replace=True) is
    array[rs.choice(len(array), k, replace=True)] on the same stream, one stream across the
    channels (:425-441)."""
    rs = np.random.RandomState(seed)
    return [rs.choice(int(num_fg), num_samples, replace=True).astype(np.int64)
            if num_fg > 0 else None for _ in range(channels)]


def bbox_from_device(bbox8: Sequence[int]) -> List[List[int]]:
    """The 8 integers of wf_fill_holes -> [[z0, z1], [y0, y1], [x0, x1]]; an empty mask raises
    ValueError (get_bbox_from_mask fails on it as well: nothing to crop to)."""
    v = [int(t) for t in bbox8]
    if v[6] == 0:
        raise ValueError("the nonzero mask is empty: every voxel of every channel is zero")
    return [[v[0], v[1]], [v[2], v[3]], [v[4], v[5]]]


# ------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------
def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("waveformer_amd.preprocessing runs on the GPU only (no CUDA/HIP device)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_gpu(x: ArrayLike, name: str) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a numpy array or a tensor, got {type(x)}")
    if x.device.type != "cuda":
        x = x.to(_device())
    return x


def _images(data: ArrayLike, name: str = "data") -> torch.Tensor:
    x = _to_gpu(data, name)
    if x.dim() != 4:
        raise ValueError(f"{name}: expected (C, D, H, W), got {tuple(x.shape)}")
    return x.to(torch.float32).contiguous()


def _labels(seg: ArrayLike, size: Tuple[int, ...], name: str = "seg") -> torch.Tensor:
    """A (1, D, H, W) or (D, H, W) segmentation as a contiguous (D, H, W) int16 device tensor."""
    x = _to_gpu(seg, name)
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if tuple(x.shape) != tuple(size):
        raise ValueError(f"{name}: expected (1, {', '.join(str(s) for s in size)}), got "
                         f"{tuple(x.shape)}")
    return x.to(torch.int16).contiguous()


def _filled_mask(data: torch.Tensor):
    return ops.fill_holes(ops.nonzero_mask(data))


# ------------------------------------------------------------------------------------------
# the reference's functions, by name
# ------------------------------------------------------------------------------------------
def create_nonzero_mask(data: ArrayLike) -> torch.Tensor:
    """cropping.py:8-21: the hole-filled nonzero mask of data (C, D, H, W), a (D, H, W) bool
    tensor on the GPU."""
    return _filled_mask(_images(data))[0].bool()


def crop_to_nonzero(data: ArrayLike, seg: Optional[ArrayLike] = None, nonzero_label: int = -1):
    """cropping.py:24-49: (data[:, box], seg, bbox) with data (C, d, h, w) fp32 and seg
    (1, d, h, w) int16 on the GPU and bbox = [[z0, z1], [y0, y1], [x0, x1]] on the host.  With
    a seg, seg == 0 outside the filled mask becomes nonzero_label; without one, the seg is 0
    inside the mask and nonzero_label outside.  An all-zero case raises ValueError."""
    x = _images(data)
    s = None if seg is None else _labels(seg, tuple(x.shape[1:]))
    filled, bbox8, _ = _filled_mask(x)
    bbox = bbox_from_device(bbox8.cpu().tolist())
    out = ops.crop_normalize(x, bbox)
    seg_out, _ = ops.crop_seg(s, filled, bbox, nonzero_label)
    return out, seg_out[None], bbox


def sample_foreground_locations(seg: ArrayLike, classes_or_regions: Sequence[int],
                                seed: int = 1234) -> Dict[int, Union[np.ndarray, list]]:
    """default_preprocessor.py:454-483 (_sample_foreground_locations): per class c,
    np.argwhere(seg == c)[RandomState(seed).choice(n, target, replace=False)] with
    target = max(min(10000, n), ceil(0.01 n)), one RandomState across the classes in order; an
    absent class gives [].  seg: (1, D, H, W); the rows are (0, z, y, x) int64, on the host.
    Regions (tuples of classes) are not implemented."""
    for c in classes_or_regions:
        if isinstance(c, (tuple, list)):
            raise NotImplementedError("sample_foreground_locations: regions are not implemented, "
                                      "only single classes")
    x = _to_gpu(seg, "seg")
    lab = _labels(x, tuple(x.shape[-3:]))
    classes = [int(c) for c in classes_or_regions]
    if not classes:
        return {}
    sels = [ops.Selection(lab, ops.SELECT_EQ, c) for c in classes]
    counts = torch.cat([s.total for s in sels]).cpu().tolist()  # one small copy for all classes
    picked = []
    for sel, ranks in zip(sels, draw_location_ranks(counts, seed)):
        picked.append(None if ranks is None else sel.pick(torch.from_numpy(ranks).to(lab.device)))
    return {c: ([] if p is None else p.cpu().numpy()) for c, p in zip(classes, picked)}


def collect_foreground_intensities(segmentation: ArrayLike, images: ArrayLike, seed: int = 1234,
                                   num_samples: int = NUM_SAMPLES):
    """default_preprocessor.py:414-452: per channel i,
    RandomState(seed).choice(images[i][segmentation[0] > 0], num_samples, replace=True), one
    stream across the channels, on the UNCROPPED inputs; [] per channel without foreground.
    Returns (intensities_per_channel, []): fp32 numpy arrays on the host, and an empty list in
    place of the reference's unused intensity_statistics_per_channel."""
    x = _images(images, "images")
    lab = _labels(segmentation, tuple(x.shape[1:]), "segmentation")
    sel = ops.Selection(lab, ops.SELECT_GT, 0)
    num_fg = int(sel.total.cpu().item())
    out = []
    for i, ranks in enumerate(draw_intensity_ranks(num_fg, x.shape[0], seed, num_samples)):
        out.append([] if ranks is None
                   else sel.pick(torch.from_numpy(ranks).to(lab.device), image=x[i]))
    return [o if isinstance(o, list) else o.cpu().numpy() for o in out], []


class MultiModalityPreprocessor:
    """preprocessor_mri.py:32 MultiModalityPreprocessor, the array part: same constructor
    arguments, with out_spacing and all_labels (which the reference's run() sets) as keywords,
    and resample: whether a case whose spacing differs from out_spacing is resampled on the GPU
    (waveformer_amd.resampling) or refused."""

    def __init__(self, base_dir=None, image_dir=None, data_filenames=(), seg_filename="", *,
                 out_spacing: Sequence[float] = (1.0, 1.0, 1.0),
                 all_labels: Sequence[int] = (1, 2, 3), resample: bool = False) -> None:
        self.base_dir = base_dir
        self.image_dir = image_dir
        self.data_filenames = data_filenames
        self.seg_filename = seg_filename
        self.out_spacing = list(out_spacing)
        self.all_labels = list(all_labels)
        self.resample = bool(resample)  # False: a case that needs resampling is refused
        self.foreground_intensity_properties_per_channel: dict = {}
        self.last_fill_rounds: Optional[int] = None  # sweep rounds of the last case's hole fill

    def _normalize(self, data: ArrayLike, seg=None,
                   foreground_intensity_properties_per_channel: Optional[dict] = None
                   ) -> torch.Tensor:
        """preprocessor_mri.py:48-55: ZScoreNormalization(use_mask_for_norm=False) of every
        channel over the whole volume; seg and the intensity properties are unused, as there.
        A contiguous fp32 device tensor is normalised in place."""
        x = _images(data)
        whole = [[0, s] for s in x.shape[1:]]
        return ops.crop_normalize(x, whole, ops.box_moments(x, whole), out=x)

    def run_case_npy(self, data: ArrayLike, seg: Optional[ArrayLike], properties: dict):
        """default_preprocessor.py:155-228.  data (C, D, H, W), seg (1, D, H, W) or None,
        properties with "spacing" (as SimpleITK gives it, x first).  Returns (data (C, d, h, w)
        fp32, seg (1, d, h, w) int8 -- int16 if its maximum exceeds 127) on the GPU and fills
        PROPERTY_KEYS in properties; class_locations holds host arrays.  When the spacings ask
        for a resample: with resample=True the reference's order -- crop, normalise, resample
        the data (order 3), resample the segmentation (order 1), class_locations on the
        resampled segmentation, then the int8 / int16 cast; otherwise NotImplementedError.
        ValueError for an all-zero case."""
        x = _images(data)
        size = tuple(int(v) for v in x.shape[1:])
        s = None if seg is None else _labels(seg, size)
        original_spacing_trans = list(properties["spacing"])[::-1]
        properties["original_spacing_trans"] = original_spacing_trans
        properties["target_spacing_trans"] = self.out_spacing
        properties["shape_before_cropping"] = size
        filled, bbox8, self.last_fill_rounds = _filled_mask(x)
        bbox = bbox_from_device(bbox8.cpu().tolist())
        properties["bbox_used_for_cropping"] = bbox
        cropped = tuple(b[1] - b[0] for b in bbox)
        properties["shape_after_cropping_before_resample"] = cropped
        new_shape = compute_new_shape(cropped, original_spacing_trans, self.out_spacing)
        resampled = tuple(int(v) for v in new_shape) != cropped
        if resampled and not self.resample:
            raise NotImplementedError(
                f"spacing {original_spacing_trans} -> {self.out_spacing} resamples {cropped} to "
                f"{tuple(int(v) for v in new_shape)}: resampling is off (resample=False)")
        out = ops.crop_normalize(x, bbox, ops.box_moments(x, bbox))
        properties["shape_after_resample"] = new_shape
        seg16, maxv = ops.crop_seg(s, filled, bbox, -1)
        seg_out = seg16[None]
        if resampled:
            # the reference passes the spacing as read (x first) here; with force_separate_z
            # left at False neither spacing enters the decision
            spacing = list(properties["spacing"])
            out = resample_data_or_seg_to_shape(out, new_shape, spacing, self.out_spacing,
                                                order=3, order_z=0)
            seg_out = resample_data_or_seg_to_shape(seg_out, new_shape, spacing,
                                                    self.out_spacing, is_seg=True, order=1,
                                                    order_z=0)
            maxv = seg_out.max()  # stays on the device until the one read below
        properties["class_locations"] = sample_foreground_locations(seg_out, self.all_labels)
        if int(maxv.cpu().item()) <= 127:
            seg_out = seg_out.to(torch.int8)
        return out, seg_out

    def read_data(self, case_name):
        raise NotImplementedError("read_data is SimpleITK file I/O: read the volumes yourself and "
                                  "call run_case_npy")

    def run(self, *args, **kwargs):
        raise NotImplementedError("run walks a dataset directory and writes files: out of scope, "
                                  "call run_case_npy per case")

    def run_plan(self, *args, **kwargs):
        raise NotImplementedError("run_plan analyses a dataset on disk: out of scope")
