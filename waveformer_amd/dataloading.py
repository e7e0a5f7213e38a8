"""Training batches on the GPU: light_training/dataloading/base_data_loader.py without the worker
processes.  The preprocessed cases stay where preprocessing left them (CaseStore: on the device
while they fit, in pinned host memory after that) and a batch is one copy kernel
(ops.crop_pad_batch): for every sample the patch box is sliced out of its case and zero-padded to
the patch size, data and segmentation both, as generate_train_batch does with numpy on the host.

Random decisions and kernels are separate, as in waveformer_amd.augment.  draw_batch_plan() draws
every decision of one batch on the host into a BatchPlan -- which cases, which samples are forced
onto a foreground voxel, where each box starts -- and execute_batch_plan() is deterministic given
it.  Unlike augment's sampler, the draw DOES reproduce the reference's random stream: the same
calls in the same order (choice(keys, B, True, None) once per batch; per sample the uniform() of
probabilistic oversampling first, then randint(lb, ub + 1) per axis or choice(len(classes)) and
choice(len(voxels))), so one seed gives the reference's keys and boxes.  rng=None draws from
numpy's global stream, which is what the reference uses.

Reading .npy / .pkl files, worker processes and the reference's unused data_global / seg_global
branch are not here.  With DDP the caller passes each rank its own rng.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

SEG_DTYPES = (torch.int8, torch.int16, torch.float32)


# ------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class BatchPlan:
    """Every random decision of one batch."""
    keys: np.ndarray      # (B,) the cases, as choice(keys, B, True, None) returned them
    force_fg: np.ndarray  # (B,) bool: the box was asked to contain a foreground voxel
    bbox_lbs: np.ndarray  # (B, 3) int64: the lower corner (z, y, x) of each box; may be negative

    @property
    def batch(self) -> int:
        return int(self.bbox_lbs.shape[0])


def _stream(rng):
    return np.random if rng is None else rng


def _patch3(patch_size) -> Tuple[int, int, int]:
    patch = tuple(int(v) for v in patch_size)
    if len(patch) != 3 or min(patch) < 1:
        raise ValueError(f"patch_size must be three positive sizes, got {patch_size!r}")
    return patch


def draw_bbox(data_shape: Sequence[int], force_fg: bool, class_locations: Optional[dict],
              patch_size: Sequence[int], need_to_pad: Sequence[int] = (0, 0, 0), rng=None,
              overwrite_class=None, verbose: bool = False) -> Tuple[List[int], List[int]]:
    """The reference's get_bbox: (bbox_lbs, bbox_ubs) of one sample.  A case smaller than the
    patch is padded on both sides, the odd voxel above: lbs = (-n) // 2 (a floor: n = 3 gives
    -2), ubs = shape + n // 2 + n % 2 - patch.  A forced box is centred on a drawn voxel of a drawn
    class and clamped from below only, so it may hang over the upper edge; a case without
    foreground falls back to the random draw.  class_locations rows are (channel, z, y, x)."""
    rng = _stream(rng)
    dim = len(data_shape)
    need_to_pad = np.array(need_to_pad).astype(int).copy()
    for d in range(dim):
        if need_to_pad[d] + data_shape[d] < patch_size[d]:
            need_to_pad[d] = patch_size[d] - data_shape[d]
    lbs = [-need_to_pad[i] // 2 for i in range(dim)]
    ubs = [data_shape[i] + need_to_pad[i] // 2 + need_to_pad[i] % 2 - patch_size[i]
           for i in range(dim)]

    voxels = None
    if force_fg:
        assert class_locations is not None, "if force_fg is set class_locations cannot be None"
        if overwrite_class is not None:
            assert overwrite_class in class_locations.keys(), \
                'desired class ("overwrite_class") does not have class_locations (missing key)'
        eligible = [i for i in class_locations.keys() if len(class_locations[i]) > 0]
        if len(eligible) == 0:
            selected = None
            if verbose:
                print("case does not contain any foreground classes")
        elif overwrite_class is None or overwrite_class not in eligible:
            selected = eligible[rng.choice(len(eligible))]
        else:
            selected = overwrite_class
        voxels = class_locations[selected] if selected is not None else None

    if voxels is not None and len(voxels) > 0:
        voxel = voxels[rng.choice(len(voxels))]
        bbox_lbs = [max(lbs[i], voxel[i + 1] - patch_size[i] // 2) for i in range(dim)]
    else:
        bbox_lbs = [rng.randint(lbs[i], ubs[i] + 1) for i in range(dim)]
    bbox_ubs = [bbox_lbs[i] + patch_size[i] for i in range(dim)]
    return bbox_lbs, bbox_ubs


def draw_batch_plan(dataset, patch_size: Sequence[int], batch_size: int = 2,
                    oversample_foreground_percent: float = 0.33,
                    probabilistic_oversampling: bool = False, rng=None,
                    keys: Optional[Sequence[int]] = None,
                    need_to_pad: Sequence[int] = (0, 0, 0)) -> BatchPlan:
    """One batch's decisions from the reference's random stream (the module docstring has the
    order of the calls).  dataset[key] gives {"data", "seg", "properties"}; only the data's shape
    and properties["class_locations"] are looked at, nothing is copied."""
    stream = _stream(rng)
    B = int(batch_size)
    keys = list(range(len(dataset))) if keys is None else list(keys)
    selected = stream.choice(keys, B, True, None)
    force = np.zeros((B,), dtype=bool)
    lbs = np.zeros((B, 3), dtype=np.int64)
    for j, key in enumerate(selected):
        if probabilistic_oversampling:
            force[j] = stream.uniform() < oversample_foreground_percent
        else:
            force[j] = not j < round(B * (1 - oversample_foreground_percent))
        item = dataset[key]
        shape = tuple(int(v) for v in item["data"].shape[1:])
        lbs[j], _ = draw_bbox(shape, bool(force[j]), item["properties"]["class_locations"],
                              patch_size, need_to_pad, rng)
    return BatchPlan(keys=selected, force_fg=force, bbox_lbs=lbs)


# ------------------------------------------------------------------------------------------
# where the cases live
# ------------------------------------------------------------------------------------------
def _as_tensor(a, dtype: Optional[torch.dtype]) -> torch.Tensor:
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a if dtype is None or a.dtype == dtype else a.to(dtype)


class CaseStore:
    """The preprocessed cases of a training set, as a `dataset` for DataLoaderMultiProcess:
    store[i] is {"data", "seg", "properties"}.  Cases stay on the device until `device_bytes`
    bytes are used (None: no limit); from the first case that does not fit, every later case is
    kept in pinned host memory and goes through the loader's staging slots.  nbytes_device /
    nbytes_host: what is held where."""

    def __init__(self, device_bytes: Optional[int] = None, device=None):
        if device_bytes is not None and int(device_bytes) < 0:
            raise ValueError(f"device_bytes must be None or >= 0, got {device_bytes!r}")
        self.device_bytes = None if device_bytes is None else int(device_bytes)
        self.device = torch.device("cuda" if device is None else device)
        self.nbytes_device = 0
        self.nbytes_host = 0
        self.max_host_data_numel = 0   # the loader sizes its staging slots with these two
        self.max_host_seg_bytes = 0
        self._spilled = False
        self._cases: List[dict] = []

    def __len__(self) -> int:
        return len(self._cases)

    def __getitem__(self, i) -> dict:
        return self._cases[int(i)]

    def on_device(self, i) -> bool:
        return self._cases[int(i)]["data"].device.type != "cpu"

    def fits(self, nbytes: int) -> bool:
        """Whether a case of nbytes would be kept on the device if added now."""
        return not self._spilled and (self.device_bytes is None or
                                      self.nbytes_device + int(nbytes) <= self.device_bytes)

    def add(self, data, seg, properties: dict) -> int:
        """data (C, d, h, w) fp32 and seg (S, d, h, w) int8 / int16 / fp32 -- what
        MultiModalityPreprocessor.run_case_npy returns, or numpy arrays / memmaps of the same --
        and the case's properties with host "class_locations".  Returns the case's key."""
        if getattr(data, "ndim", 0) != 4 or getattr(seg, "ndim", 0) != 4 or \
                tuple(seg.shape[1:]) != tuple(data.shape[1:]):
            raise ValueError(f"expected data (C, d, h, w) and seg (S, d, h, w), got "
                             f"{tuple(getattr(data, 'shape', ()))} and "
                             f"{tuple(getattr(seg, 'shape', ()))}")
        if "class_locations" not in properties:
            raise ValueError('properties need "class_locations" (run_case_npy fills it)')
        data = _as_tensor(data, torch.float32)
        seg = _as_tensor(seg, None)
        if seg.dtype not in SEG_DTYPES:
            raise TypeError(f"seg must be int8, int16 or float32, got {seg.dtype}")
        nbytes = data.numel() * 4 + seg.numel() * seg.element_size()
        if self.fits(nbytes):
            data = data.to(self.device).contiguous()
            seg = seg.to(self.device).contiguous()
            self.nbytes_device += nbytes
        else:
            self._spilled = True
            data, seg = self._host(data), self._host(seg)
            self.nbytes_host += nbytes
            self.max_host_data_numel = max(self.max_host_data_numel, data.numel())
            self.max_host_seg_bytes = max(self.max_host_seg_bytes,
                                          seg.numel() * seg.element_size())
        self._cases.append({"data": data, "seg": seg, "properties": properties})
        return len(self._cases) - 1

    @staticmethod
    def _host(t: torch.Tensor) -> torch.Tensor:
        t = t.cpu().contiguous()
        # pinned, so that the loader's copy to the device is asynchronous; a host without a GPU
        # cannot pin and cannot load either
        return t.pin_memory() if torch.cuda.is_available() and not t.is_pinned() else t


# ------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------
class _Staging:
    """batch_size reusable device slots for cases that live on the host: a fp32 buffer and a
    byte buffer each, grown to the largest case seen (a CaseStore says it up front)."""

    def __init__(self, slots: int, device, data_numel: int = 0, seg_bytes: int = 0):
        self.device = device
        self.data = [None] * slots
        self.seg = [None] * slots
        self.data_numel, self.seg_bytes = int(data_numel), int(seg_bytes)

    def put(self, slot: int, data: torch.Tensor, seg: torch.Tensor):
        nd, ns = data.numel(), seg.numel() * seg.element_size()
        self.data_numel, self.seg_bytes = max(self.data_numel, nd), max(self.seg_bytes, ns)
        if self.data[slot] is None or self.data[slot].numel() < self.data_numel:
            self.data[slot] = torch.empty((self.data_numel,), dtype=torch.float32,
                                          device=self.device)
        if self.seg[slot] is None or self.seg[slot].numel() < self.seg_bytes:
            self.seg[slot] = torch.empty((self.seg_bytes,), dtype=torch.uint8, device=self.device)
        d = self.data[slot][:nd].view(data.shape)
        s = self.seg[slot][:ns].view(seg.dtype).view(seg.shape)
        d.copy_(data, non_blocking=True)   # on the current stream, before the batch's launch
        s.copy_(seg, non_blocking=True)
        return d, s


class DataLoaderMultiProcess:
    """The reference's loader by its names: generate_train_batch / __next__ give {"data":
    (B, C, *patch) fp32, "seg": (B, S, *patch) fp32 -- both on the device, padded with 0 --,
    "properties": the cases' properties, "keys": the drawn cases}.  dataset: a CaseStore, or
    anything whose [i] is {"data", "seg", "properties"} of tensors or numpy arrays.  rng: an
    np.random.RandomState; None draws from numpy's global stream as the reference does."""

    def __init__(self, dataset, patch_size, batch_size: int = 2,
                 oversample_foreground_percent: float = 0.33,
                 probabilistic_oversampling: bool = False, rng=None, device=None):
        self.dataset = dataset
        self.patch_size = _patch3(patch_size)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size!r}")
        self.keys = [i for i in range(len(dataset))]
        self.oversample_foreground_percent = oversample_foreground_percent
        self.probabilistic_oversampling = bool(probabilistic_oversampling)
        self.need_to_pad = (np.array([0, 0, 0])).astype(int)
        self.get_do_oversample = self._probabilistic_oversampling if probabilistic_oversampling \
            else self._oversample_last_XX_percent
        self.rng = rng
        self.data_shape = None
        self.seg_shape = None
        self.device = torch.device(device if device is not None
                                   else getattr(dataset, "device", "cuda"))
        self._staging: Optional[_Staging] = None

    # ---- the draw --------------------------------------------------------------------
    def determine_shapes(self):
        item = self.dataset[0]
        C, S = int(item["data"].shape[0]), int(item["seg"].shape[0])
        return (self.batch_size, C) + self.patch_size, (self.batch_size, S) + self.patch_size

    def _oversample_last_XX_percent(self, sample_idx: int) -> bool:
        """The last third of the batch (round() is Python's, to even)."""
        return not sample_idx < round(self.batch_size * (1 - self.oversample_foreground_percent))

    def _probabilistic_oversampling(self, sample_idx: int) -> bool:
        return _stream(self.rng).uniform() < self.oversample_foreground_percent

    def get_bbox(self, data_shape, force_fg: bool, class_locations: Union[dict, None],
                 overwrite_class=None, verbose: bool = False):
        return draw_bbox(data_shape, force_fg, class_locations, self.patch_size,
                         self.need_to_pad, self.rng, overwrite_class, verbose)

    def draw_batch_plan(self) -> BatchPlan:
        return draw_batch_plan(self.dataset, self.patch_size, self.batch_size,
                               self.oversample_foreground_percent,
                               self.probabilistic_oversampling, self.rng, self.keys,
                               self.need_to_pad)

    # ---- the execution ---------------------------------------------------------------
    def execute_batch_plan(self, plan: BatchPlan) -> Dict[str, object]:
        """The batch of a plan: deterministic.  Cases on the host are copied into the staging
        slots (non_blocking, current stream) before the one launch that makes the batch."""
        if plan.batch != self.batch_size:
            raise ValueError(f"the plan is for {plan.batch} samples, the loader for "
                             f"{self.batch_size}")
        if self.data_shape is None:
            self.data_shape, self.seg_shape = self.determine_shapes()
        cases, props = [], []
        for j, key in enumerate(plan.keys):
            item = self.dataset[key]
            data, seg = item["data"], item["seg"]
            props.append(item["properties"])
            if not isinstance(data, torch.Tensor) or data.device.type == "cpu":
                data, seg = self._stage(j, _as_tensor(data, torch.float32), _as_tensor(seg, None))
            cases.append((data, seg))
        kinds = {seg.dtype for _, seg in cases}
        if len(kinds) > 1:  # int8 beside int16 cases (a label above 127): one kind per launch
            wide = torch.float32 if torch.float32 in kinds else torch.int16
            cases = [(d, s.to(wide)) for d, s in cases]
        data, seg = ops.crop_pad_batch(cases, plan.bbox_lbs.tolist(), self.patch_size)
        if tuple(data.shape) != self.data_shape or tuple(seg.shape) != self.seg_shape:
            raise ValueError(f"the batch is {tuple(data.shape)} / {tuple(seg.shape)}, the first "
                             f"case promised {self.data_shape} / {self.seg_shape}")
        return {"data": data, "seg": seg, "properties": props, "keys": plan.keys}

    def _stage(self, slot: int, data: torch.Tensor, seg: torch.Tensor):
        if self._staging is None:
            self._staging = _Staging(self.batch_size, self.device,
                                     getattr(self.dataset, "max_host_data_numel", 0),
                                     getattr(self.dataset, "max_host_seg_bytes", 0))
        return self._staging.put(slot, data, seg)

    def generate_train_batch(self) -> Dict[str, object]:
        return self.execute_batch_plan(self.draw_batch_plan())

    def __next__(self):
        return self.generate_train_batch()

    def __iter__(self):
        return self
