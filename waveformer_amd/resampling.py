"""Resampling of a case to the target spacing on the GPU, under the names and signatures of the
reference's light_training/preprocessing/resampling/default_resampling.py.

The decision logic (get_do_separate_z, get_lowres_axis, the force_separate_z states and the
len(axis) == 2 / 3 cases) is restated in full.  What runs on the device is the branch that
DefaultPreprocessor.run_case_npy reaches (force_separate_z=False, so do_separate_z is False): the
3-D resize of every channel,

  * data, order 3: skimage.transform.resize(order=3, mode='edge', anti_aliasing=False), i.e.
    scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True), then resize's clip=True: the
    clamp to the channel's input [min, max] (ops.zoom_cubic_volume, csrc/resample.hip);
  * data, order 0: zoom(order=0) (ops.zoom_nearest), which needs no clamp;
  * segmentation, order 1: batchgenerators' resize_segmentation: per label of the input in
    ascending order, resize(seg == c, order=1) >= 0.5 writes c into zeros, which is "the
    largest label whose trilinear weight sum is >= 0.5, else 0" (ops.zoom_seg_linear);
  * segmentation, order 0: zoom(order=0) of the labels.

Everything else raises NotImplementedError naming the argument: do_separate_z=True (the per-slice
2-D resize plus map_coordinates along the anisotropic axis), other orders.  Device tensors go in
and out; host arrays are moved to the current device.  GPU only, no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

ArrayLike = Union[np.ndarray, torch.Tensor]
Spacing = Union[Tuple[float, ...], List[float], np.ndarray]
ANISO_THRESHOLD = 3  # default_resampling.py:11


# ------------------------------------------------------------------------------------------
# host arithmetic (no GPU needed)
# ------------------------------------------------------------------------------------------
def get_do_separate_z(spacing: Spacing, anisotropy_threshold=ANISO_THRESHOLD) -> bool:
    """default_resampling.py:13-15."""
    return bool((np.max(spacing) / np.min(spacing)) > anisotropy_threshold)


def get_lowres_axis(new_spacing: Spacing) -> np.ndarray:
    """default_resampling.py:18-20: the axes whose spacing is the largest."""
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def compute_new_shape(old_shape: Sequence[int], old_spacing: Spacing,
                      new_spacing: Spacing) -> np.ndarray:
    """default_resampling.py:23-30, with Python's int(round(...)) (half to even)."""
    if not (len(old_spacing) == len(old_shape) == len(new_spacing)):
        raise ValueError("compute_new_shape: shape and spacings must have one length")
    return np.array([int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)])


def decide_separate_z(current_spacing: Spacing, new_spacing: Spacing,
                      force_separate_z: Optional[bool] = False,
                      separate_z_anisotropy_threshold: float = ANISO_THRESHOLD):
    """default_resampling.py:91-117 (the same lines open resample_data_or_seg_to_spacing, :40-66):
    (do_separate_z, axis) from the two spacings and force_separate_z (True, False or None)."""
    if force_separate_z is not None:
        do_separate_z = bool(force_separate_z)
        axis = get_lowres_axis(current_spacing) if force_separate_z else None
    elif get_do_separate_z(current_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(current_spacing)
    elif get_do_separate_z(new_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(new_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) in (2, 3):
        # 3: every axis has the same spacing; 2: spacings like (0.24, 1.25, 1.25), where the
        # reference does not resample the out-of-plane axis separately either
        do_separate_z = False
    return do_separate_z, axis


# ------------------------------------------------------------------------------------------
# the device part
# ------------------------------------------------------------------------------------------
def _to_gpu4(data: ArrayLike) -> torch.Tensor:
    if isinstance(data, np.ndarray):
        data = torch.from_numpy(np.ascontiguousarray(data))
    if not isinstance(data, torch.Tensor):
        raise TypeError(f"data: expected a numpy array or a tensor, got {type(data)}")
    if data.dim() != 4:
        raise ValueError(f"data must be (c, x, y, z), got {tuple(data.shape)}")
    if data.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("waveformer_amd.resampling runs on the GPU only (no CUDA/HIP device)")
        data = data.to(torch.device("cuda", torch.cuda.current_device()))
    return data


def resample_data_or_seg(data: ArrayLike, new_shape: Sequence[int], is_seg: bool = False,
                         axis=None, order: int = 3, do_separate_z: bool = False,
                         order_z: int = 0) -> torch.Tensor:
    """default_resampling.py:126-217.  data (C, D, H, W) -> (C, *new_shape) in data's dtype, on
    the GPU; data itself (moved to the GPU) when the shape does not change.  Supported: the 3-D
    branch with order 0 or 3 for data and 0 or 1 for a segmentation (integer labels that fit
    int16)."""
    new_shape = tuple(int(v) for v in new_shape)
    if len(new_shape) != 3:
        raise ValueError(f"new_shape must have three entries, got {new_shape!r}")
    if not hasattr(data, "shape") or len(data.shape) != 4:
        raise ValueError("data must be (c, x, y, z)")
    if tuple(int(v) for v in data.shape[1:]) == new_shape:
        return _to_gpu4(data)
    # the options are checked before anything moves to the device
    if do_separate_z:
        raise NotImplementedError(
            "resample_data_or_seg: do_separate_z=True (a 2-D resize per slice, then order_z "
            "along the anisotropic axis) is not implemented; only the 3-D branch is")
    if is_seg and order not in (0, 1):
        raise NotImplementedError(f"resample_data_or_seg: order={order} for a segmentation is "
                                  "not implemented, only 0 and 1")
    if not is_seg and order not in (0, 3):
        raise NotImplementedError(f"resample_data_or_seg: order={order} for data is not "
                                  "implemented, only 0 and 3")
    x = _to_gpu4(data)
    dtype = x.dtype
    if is_seg and order == 1:
        lab = x.to(torch.int16).contiguous()
        out = torch.stack([ops.zoom_seg_linear(lab[c], new_shape) for c in range(lab.shape[0])])
        return out.to(dtype)
    planes = x.to(torch.float32).contiguous()
    if order == 0:  # labels up to 2^24 and fp32 data pass through fp32 planes unchanged
        out = ops.zoom_nearest(planes, new_shape)
    else:
        out = ops.zoom_cubic_volume(planes, new_shape, clip=True)
    return out.to(dtype)


def resample_data_or_seg_to_shape(data: ArrayLike, new_shape: Sequence[int],
                                  current_spacing: Spacing, new_spacing: Spacing,
                                  is_seg: bool = False, order: int = 3, order_z: int = 0,
                                  force_separate_z: Optional[bool] = False,
                                  separate_z_anisotropy_threshold: float = ANISO_THRESHOLD
                                  ) -> torch.Tensor:
    """default_resampling.py:78-123."""
    do_separate_z, axis = decide_separate_z(current_spacing, new_spacing, force_separate_z,
                                            separate_z_anisotropy_threshold)
    return resample_data_or_seg(data, new_shape, is_seg, axis, order, do_separate_z,
                                order_z=order_z)


def resample_data_or_seg_to_spacing(data: ArrayLike, current_spacing: Spacing,
                                    new_spacing: Spacing, is_seg: bool = False, order: int = 3,
                                    order_z: int = 0, force_separate_z: Optional[bool] = False,
                                    separate_z_anisotropy_threshold: float = ANISO_THRESHOLD
                                    ) -> torch.Tensor:
    """default_resampling.py:33-75: the new shape follows from the spacings and the shape of a
    channel (the reference slices data[0].shape once more at :71-72 and then fails its own
    length assertion; the channel's shape is what it means)."""
    do_separate_z, axis = decide_separate_z(current_spacing, new_spacing, force_separate_z,
                                            separate_z_anisotropy_threshold)
    if not hasattr(data, "shape") or len(data.shape) != 4:
        raise ValueError("data must be (c, x, y, z)")
    new_shape = compute_new_shape(tuple(int(v) for v in data.shape[1:]), current_spacing,
                                  new_spacing)
    return resample_data_or_seg(data, new_shape, is_seg, axis, order, do_separate_z,
                                order_z=order_z)
