"""numpy / scipy restatement, in float64, of the resampling step of the reference's preprocessing
(light_training/preprocessing/resampling/default_resampling.py): the 3-D branch of
resample_data_or_seg, batchgenerators' resize_segmentation, and the decision helpers.  skimage is
not needed: skimage.transform.resize(mode='edge', anti_aliasing=False) of skimage >= 0.19 is
scipy.ndimage.zoom(mode='nearest', grid_mode=True) followed, with resize's default clip=True, by
a clamp to the input's [min, max] (skimage.transform._warps._clip_warp_output).

The inputs of the fixture cases are drawn here from seeded RandomStates with numpy alone, so that
tests/golden/preprocess_resample_fixtures.npz holds outputs only
(gen_preprocess_resample_fixtures.py records them with scipy; the GPU tests need no scipy).
"""
import os

import numpy as np

from tests import augment_ref
from tests import preprocess_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "preprocess_resample_fixtures.npz")
PAD = augment_ref.PAD
TIE_EPS = augment_ref.TIE_EPS
ANISO_THRESHOLD = 3
AXIS_ORDER = (0, 1, 2)   # ops.ZOOM_AXIS_ORDER
MIN_CLAMPED = 0.10       # share of the fp64 outputs the clamp must set in every data case
MAX_TIES = 0.05          # share of a segmentation case's voxels the tie mask may cover


# ------------------------------------------------------------------------------------------
# decision helpers (default_resampling.py:13-30 and :91-117)
# ------------------------------------------------------------------------------------------
def get_do_separate_z(spacing, anisotropy_threshold=ANISO_THRESHOLD):
    """:13-15."""
    return (np.max(spacing) / np.min(spacing)) > anisotropy_threshold


def get_lowres_axis(new_spacing):
    """:18-20."""
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def compute_new_shape(old_shape, old_spacing, new_spacing):
    """:23-30."""
    assert len(old_spacing) == len(old_shape) == len(new_spacing)
    return np.array([int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)])


def decide_separate_z(current_spacing, new_spacing, force_separate_z=False,
                      separate_z_anisotropy_threshold=ANISO_THRESHOLD):
    """:91-117, statement by statement: (do_separate_z, axis)."""
    if force_separate_z is not None:
        do_separate_z = force_separate_z
        if force_separate_z:
            axis = get_lowres_axis(current_spacing)
        else:
            axis = None
    else:
        if get_do_separate_z(current_spacing, separate_z_anisotropy_threshold):
            do_separate_z = True
            axis = get_lowres_axis(current_spacing)
        elif get_do_separate_z(new_spacing, separate_z_anisotropy_threshold):
            do_separate_z = True
            axis = get_lowres_axis(new_spacing)
        else:
            do_separate_z = False
            axis = None
    if axis is not None:
        if len(axis) == 3:
            do_separate_z = False
        elif len(axis) == 2:
            do_separate_z = False
    return do_separate_z, axis


# ------------------------------------------------------------------------------------------
# resample_data_or_seg, 3-D branch (:126-217 with do_separate_z False)
# ------------------------------------------------------------------------------------------
def _zoom(x, new_shape, order):
    from scipy import ndimage
    out = ndimage.zoom(x, np.array(new_shape) / np.array(x.shape), order=order, mode="nearest",
                       grid_mode=True)
    assert out.shape == tuple(new_shape), (out.shape, new_shape)
    return out


def resize_data(x, new_shape, order=3):
    """:212 for one channel of data: resize(x.astype(float), new_shape, order, mode='edge',
    anti_aliasing=False), clip=True.  Returns (result, result before the clamp), float64."""
    x = x.astype(float)
    raw = _zoom(x, new_shape, order)
    return np.clip(raw, x.min(), x.max()), raw


def resize_segmentation(seg, new_shape, order=1):
    """batchgenerators.augmentations.utils.resize_segmentation for one label map (D, H, W).
    Returns (result, tie): tie marks the voxels where some label's interpolated indicator lies
    within TIE_EPS of 0.5, where an implementation may legitimately decide the other way."""
    tie = np.zeros(tuple(new_shape), bool)
    if order == 0:
        return _zoom(seg.astype(float), new_shape, 0).astype(seg.dtype), tie
    result = np.zeros(tuple(new_shape), seg.dtype)
    for c in np.unique(seg):
        v = _zoom((seg == c).astype(float), new_shape, order)
        result[v >= 0.5] = c
        tie |= np.abs(v - 0.5) < TIE_EPS
    return result, tie


def resample_data_or_seg(data, new_shape, is_seg=False, order=3):
    """:126-217 without separate z: (C, D, H, W) -> (C, *new_shape) in data's dtype; the input
    itself when the shape does not change."""
    assert data.ndim == 4 and len(new_shape) == 3
    if tuple(data.shape[1:]) == tuple(int(v) for v in new_shape):
        return data
    if is_seg:
        out = [resize_segmentation(data[c], new_shape, order)[0] for c in range(len(data))]
    else:
        out = [resize_data(data[c], new_shape, order)[0] for c in range(len(data))]
    return np.stack(out).astype(data.dtype)


# ------------------------------------------------------------------------------------------
# the separable form the kernel computes, in float64: its intermediates give cmax
# ------------------------------------------------------------------------------------------
def cubic_weights(t):
    """scipy's order-3 B-spline weights of the taps floor(x) - 1 .. floor(x) + 2."""
    z = 1.0 - t
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return w0, w1, w2, 1.0 - w0 - w1 - w2


def zoom_axis(x, axis, on):
    """One axis of zoom(order=3, mode='nearest', grid_mode=True): (coefficients of the
    edge-padded line, interpolated result)."""
    n = x.shape[axis]
    coef = augment_ref.spline_filter_axis(x, axis, "edge")
    pos = (np.arange(on) + 0.5) * (n / on) - 0.5 + PAD
    f = np.floor(pos)
    shape = [1] * x.ndim
    shape[axis] = on
    out = 0.0
    for k, w in enumerate(cubic_weights(pos - f)):
        idx = f.astype(int) - 1 + k
        assert idx.min() >= 0 and idx.max() < n + 2 * PAD
        out = out + w.reshape(shape) * np.take(coef, idx, axis=axis)
    return coef, out


def separable_zoom(x, new_shape):
    """The three passes in AXIS_ORDER, unchanged axes skipped: (result before the clamp, cmax),
    cmax the largest magnitude among the input and every intermediate."""
    x = x.astype(float)
    cmax = np.abs(x).max()
    for a in AXIS_ORDER:
        if x.shape[a] == new_shape[a]:
            continue
        coef, x = zoom_axis(x, a, new_shape[a])
        cmax = max(cmax, np.abs(coef).max(), np.abs(x).max())
    return x, float(cmax)


# ------------------------------------------------------------------------------------------
# seeded inputs (numpy only)
# ------------------------------------------------------------------------------------------
def _smooth(x, rounds=2):
    """[1 2 1] / 4 along every axis longer than 1, edge padded."""
    for _ in range(rounds):
        for a in range(x.ndim):
            if x.shape[a] == 1:
                continue
            pad = [(0, 0)] * x.ndim
            pad[a] = (1, 1)
            p = np.pad(x, pad, mode="edge")
            n = x.shape[a]
            x = (np.take(p, np.arange(n), axis=a) + 2.0 * np.take(p, np.arange(n) + 1, axis=a)
                 + np.take(p, np.arange(n) + 2, axis=a)) / 4.0
    return x


def make_data(shape, channels, seed):
    """(channels, *shape) float32: smoothed noise, everything below a per-channel quantile set to
    0, then z-scored per channel in fp32.  The background is flat at the channel's minimum, so
    the cubic undershoots along its edge and the clamp acts; the quantile and the scale differ
    per channel, so the channels' ranges do."""
    rs = np.random.RandomState(seed)
    out = np.empty((channels,) + tuple(shape), np.float32)
    for c in range(channels):
        x = _smooth(rs.standard_normal(shape)) * (3.0 + 2.0 * c) + 4.0
        thr = np.quantile(x, 0.35 + 0.2 * c)
        assert thr > 0.0
        x = np.where(x < thr, 0.0, x).astype(np.float32)
        out[c] = (x - x.mean(dtype=np.float32)) / x.std(dtype=np.float32)
        assert out[c].min() == out[c][x == 0.0].max()
    return out


def make_seg(shape, seed):
    """(*shape) int16: smoothed noise cut at its quartiles into the labels 0..3, and -1 in the
    outer shell of every axis of length >= 4."""
    rs = np.random.RandomState(seed)
    x = _smooth(rs.standard_normal(shape))
    seg = np.digitize(x, np.quantile(x, [0.25, 0.5, 0.75])).astype(np.int16)
    for a, n in enumerate(shape):
        if n >= 4:
            idx = [slice(None)] * 3
            for e in (0, n - 1):
                idx[a] = e
                seg[tuple(idx)] = -1
    return seg


# name: (input shape, output shape, planes).  down / up / exact halving / one axis unchanged /
# singleton axis / axes shorter than the four taps / one axis longer than a segment in each
# position / an inner extent (70) that is no multiple of the 64-line tile and exceeds it
CASES = {
    "down": ((20, 24, 18), (13, 17, 11), 2),
    "up": ((9, 12, 10), (14, 19, 23), 1),
    "half": ((16, 12, 20), (8, 6, 10), 1),
    "mixed": ((11, 16, 30), (11, 21, 19), 1),
    "single": ((1, 9, 17), (1, 14, 11), 1),
    "tiny": ((2, 3, 4), (5, 2, 7), 1),
    "long_w": ((3, 5, 300), (4, 5, 211), 1),
    "long_h": ((5, 300, 3), (5, 211, 4), 1),
    "long_d": ((300, 3, 5), (211, 4, 5), 1),
    "wide": ((6, 7, 70), (5, 9, 75), 2),
}
# all weights of this case are 0.5 or 1, so every sum is exact in any order and more than half
# of its voxels have a label at exactly 0.5: compared on every voxel, no tie mask
EXACT_SEG_CASE = "half"
SEEDS = {name: 100 + i for i, name in enumerate(CASES)}

# end to end: preprocess_ref.blob_case, read with spacing (x, y, z) = E2E_SPACING
E2E_BLOB = dict(shape=(20, 24, 28), lo=(3, 5, 6), hi=(15, 20, 19), channels=2, seed=23)
E2E_SPACING = (1.0, 1.0, 2.0)
E2E_OUT_SPACING = (1.0, 1.5, 0.75)
E2E_CROPPED = (12, 15, 13)
E2E_NEW_SHAPE = (24, 10, 17)


def data_input(name):
    shape, _, planes = CASES[name]
    return make_data(shape, planes, SEEDS[name])


def seg_input(name):
    return make_seg(CASES[name][0], SEEDS[name] + 50)


def e2e_inputs():
    return preprocess_ref.blob_case(**E2E_BLOB)


def e2e_before_resample():
    """What run_case_npy resamples: the cropped, z-scored (float64) data and the cropped seg."""
    data, seg = e2e_inputs()
    filled = preprocess_ref.nonzero_mask(data)  # a solid box: nothing to fill
    cdata, cseg, _ = preprocess_ref.crop_to_nonzero(data, seg, filled)
    assert cdata.shape[1:] == E2E_CROPPED
    norm = np.stack([preprocess_ref.zscore64(cdata[c])[0] for c in range(len(cdata))])
    return norm, cseg


def pack(mask):
    return np.packbits(np.ascontiguousarray(mask).astype(bool).ravel())


def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


def _data_record(out, key, planes, new_shape):
    res, raws, cmax = [], [], []
    for x in planes:
        clamped, raw = resize_data(x, new_shape)
        sep, cm = separable_zoom(x, new_shape)
        # the axis-aligned zoom is the product of its axis passes
        assert np.abs(sep - raw).max() <= 1e-12 * cm, (key, np.abs(sep - raw).max())
        res.append(clamped)
        raws.append(raw)
        cmax.append(cm)
    out[f"{key}_data"] = np.stack(res)
    out[f"{key}_raw"] = np.stack(raws)  # before the clamp: where the clamp must act
    out[f"{key}_cmax"] = np.array(cmax)
    return np.stack(res), np.stack(raws)


def _seg_record(out, key, seg, new_shape):
    res, tie = resize_segmentation(seg, new_shape, 1)
    out[f"{key}_seg"] = res.astype(np.int8)
    if key != EXACT_SEG_CASE:  # that case is compared on every voxel: it has no mask to cap
        assert tie.mean() <= MAX_TIES, (key, tie.mean())
        out[f"{key}_tie"] = pack(tie)
    out[f"{key}_seg0"] = resize_segmentation(seg, new_shape, 0)[0].astype(np.int8)


def build_fixtures():
    """Everything gen_preprocess_resample_fixtures.py stores (needs scipy)."""
    out = {}
    for name, (shape, new_shape, _) in CASES.items():
        x = data_input(name)
        clamped, raw = _data_record(out, name, x, new_shape)
        share = (clamped != raw).mean(axis=(1, 2, 3))
        assert (share >= MIN_CLAMPED).all(), (name, share)
        _seg_record(out, name, seg_input(name), new_shape)
    norm, cseg = e2e_before_resample()
    _data_record(out, "e2e", norm.astype(np.float32), E2E_NEW_SHAPE)
    _seg_record(out, "e2e", cseg[0], E2E_NEW_SHAPE)
    return out


_fixtures = None


def fixtures():
    global _fixtures
    if _fixtures is None:
        with np.load(GOLDEN) as z:
            _fixtures = {k: z[k] for k in z.files}
    return _fixtures
