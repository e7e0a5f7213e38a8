"""numpy / scipy restatement of the train-time augmentation that waveformer_amd.augment runs on
the GPU: batchgenerators' transforms as light_training/augment/train_augment.py composes them.
float64 inside; where batchgenerators writes a result back into its float32 batch, `whole`
casts as it does.  Every function names the batchgenerators function it restates.  skimage is
not needed: skimage.transform.resize(mode='edge', anti_aliasing=False) of skimage >= 0.19 is
scipy.ndimage.zoom(mode='nearest', grid_mode=True).

The inputs of the fixture cases are drawn here from seeded RandomStates, so that
tests/golden/augment_fixtures.npz holds outputs only (gen_augment_fixtures.py records them with
scipy; the GPU tests need no scipy).
"""
import numpy as np

PAD = 12  # scipy's _prepad_for_spline_filter for mode='nearest'
POLE = np.sqrt(3.0) - 2.0
TIE_EPS = 1e-5


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------
def make_volume(shape, seed):
    """A smooth-plus-noise float32 volume (C, D, H, W) of roughly unit variance, mean 0.3."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(shape)
    g = np.meshgrid(*[np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape[1:]],
                    indexing="ij")
    x = x * 0.5 + 0.3 + np.cos(2.0 * g[0] + g[1]) * np.sin(1.5 * g[2] + 0.3)
    return x.astype(np.float32)


def make_seg(shape, labels, seed):
    """A blocky label map (1, D, H, W) float32 over `labels`: a coarse random grid blown up."""
    rs = np.random.RandomState(seed)
    coarse = rs.choice(np.asarray(labels, dtype=np.float32), size=[-(-n // 4) for n in shape])
    seg = coarse.repeat(4, 0).repeat(4, 1).repeat(4, 2)[:shape[0], :shape[1], :shape[2]]
    return np.ascontiguousarray(seg[None]).astype(np.float32)


# ------------------------------------------------------------------------------------------
# spatial: batchgenerators.augmentations.spatial_transformations.augment_spatial
# ------------------------------------------------------------------------------------------
def rotation_matrix(ax, ay, az):
    """utils.rotate_coords_3d's matrix: create_matrix_rotation_x_3d, _y_, _z_ multiplied in that
    order onto the identity."""
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return np.dot(np.dot(np.dot(np.identity(3), rx), ry), rz)


def spatial_coords(patch_size, in_shape, angles, scale):
    """create_zero_centered_coordinate_mesh, rotate_coords_3d, scale_coords and the centre of
    augment_spatial(random_crop=False): coordinates (3, *patch_size) into the input."""
    mesh = np.array(np.meshgrid(*[np.arange(n) for n in patch_size], indexing="ij")).astype(float)
    for d in range(3):
        mesh[d] -= (np.array(patch_size).astype(float)[d] - 1) / 2.0
    if angles is not None:
        rot = rotation_matrix(*angles)
        mesh = np.dot(mesh.reshape(3, -1).transpose(), rot).transpose().reshape(mesh.shape)
    if scale is not None:
        mesh = mesh * scale
    for d in range(3):
        mesh[d] += in_shape[d] / 2.0 - 0.5
    return mesh


def spatial_data(vol, coords):
    """interpolate_img(order=3, 'constant', cval=0) of one channel: float64."""
    from scipy.ndimage import map_coordinates
    return map_coordinates(vol.astype(float), coords, order=3, mode="constant", cval=0.0)


def spatial_seg(seg, coords):
    """interpolate_img(order=1, 'constant', cval=-1, is_seg=True) of a label map (D, H, W).
    Returns (result, tie): tie marks the voxels where some label's interpolated indicator lies
    within TIE_EPS of 0.5, where an implementation may legitimately decide the other way."""
    from scipy.ndimage import map_coordinates
    result = np.zeros(coords.shape[1:], seg.dtype)
    tie = np.zeros(coords.shape[1:], bool)
    for c in np.sort(np.unique(seg)):
        v = map_coordinates((seg == c).astype(float), coords, order=1, mode="constant", cval=-1.0)
        result[v >= 0.5] = c
        tie |= np.abs(v - 0.5) <= TIE_EPS
    return result, tie


def center_crop(x, patch_size):
    """crop_and_pad_augmentations.center_crop_aug on the trailing three axes."""
    lb = [(x.shape[-3 + d] - patch_size[d]) // 2 for d in range(3)]
    return x[..., lb[0]:lb[0] + patch_size[0], lb[1]:lb[1] + patch_size[1],
             lb[2]:lb[2] + patch_size[2]]


def spline_filter_axis(x, axis, mode):
    """The prefilter the two interpolations run, one axis of (N, D, H, W): 'mirror' is what
    map_coordinates(mode='constant') filters with; 'edge' pads PAD edge samples on that axis and
    filters with 'mirror', as zoom(mode='nearest') does on all axes at once."""
    from scipy.ndimage import spline_filter1d
    x = np.asarray(x, dtype=float)
    if mode == "edge":
        pad = [(0, 0)] * x.ndim
        pad[axis] = (PAD, PAD)
        x = np.pad(x, pad, mode="edge")
    return spline_filter1d(x, order=3, axis=axis, mode="mirror")


def spline_fir_axis(x, axis, mode, taps=18):
    """What the kernel computes, in float64: the prefilter as the symmetric FIR sqrt(3) pole^|k|
    cut off after `taps` samples, over the mirrored (edge-padded) line."""
    x = np.asarray(x, dtype=float)
    if mode == "edge":
        pad = [(0, 0)] * x.ndim
        pad[axis] = (PAD, PAD)
        x = np.pad(x, pad, mode="edge")
    n = x.shape[axis]
    if n == 1:
        return x.copy()
    j = np.arange(-taps, n + taps) % (2 * (n - 1))
    src = np.where(j < n, j, 2 * (n - 1) - j)
    ext = np.take(x, src, axis=axis)
    out = np.zeros_like(x)
    for k in range(-taps, taps + 1):
        out += np.sqrt(3.0) * POLE ** abs(k) * np.take(ext, np.arange(n) + taps + k, axis=axis)
    return out


# ------------------------------------------------------------------------------------------
# intensity transforms (one channel each, float64)
# ------------------------------------------------------------------------------------------
def gaussian_noise(x, variance, noise):
    """noise_augmentations.augment_gaussian_noise: x + normal(0, variance); `noise` is the
    standard normal sample, so the draw is noise * variance (the variance is used as the scale)."""
    return x.astype(float) + float(variance) * noise.astype(float)


def gaussian_blur(x, sigma):
    """noise_augmentations.augment_gaussian_blur: gaussian_filter(channel, sigma, order=0)."""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(x.astype(float), sigma, order=0)


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius): the centre and one side."""
    radius = int(truncate * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    phi = phi / phi.sum()
    return phi[radius:]


def brightness(x, multiplier):
    """color_augmentations.augment_brightness_multiplicative."""
    return x.astype(float) * float(multiplier)


def contrast(x, factor):
    """color_augmentations.augment_contrast(preserve_range=True), one channel."""
    x = x.astype(float)
    mn, lo, hi = x.mean(), x.min(), x.max()
    return np.clip((x - mn) * factor + mn, lo, hi)


def low_resolution(x, zoom):
    """resample_augmentations.augment_linear_downsampling_scipy, one channel: order 0 down to
    round(shape * zoom), order 3 back up, skimage.transform.resize(mode='edge',
    anti_aliasing=False) both ways.  Returns (result, target shape)."""
    from scipy import ndimage
    shp = np.array(x.shape)
    target = np.round(shp * zoom).astype(int)
    down = ndimage.zoom(x.astype(float), target / shp, order=0, mode="nearest", grid_mode=True)
    assert down.shape == tuple(target), (down.shape, target)
    up = ndimage.zoom(down, shp / target, order=3, mode="nearest", grid_mode=True)
    assert up.shape == x.shape, (up.shape, x.shape)
    return up, tuple(int(v) for v in target)


def zoom_nearest(x, target):
    from scipy import ndimage
    return ndimage.zoom(x.astype(float), np.array(target) / np.array(x.shape), order=0,
                        mode="nearest", grid_mode=True)


def gamma(x, g, invert, epsilon=1e-7):
    """color_augmentations.augment_gamma(retain_stats=True), one channel."""
    x = x.astype(float)
    if invert:
        x = -x
    mn, sd = x.mean(), x.std()
    minm = x.min()
    rnge = x.max() - minm
    x = np.power((x - minm) / float(rnge + epsilon), g) * rnge + minm
    x = x - x.mean()
    x = x / (x.std() + 1e-8) * sd
    x = x + mn
    return -x if invert else x


def stats(x):
    x = x.astype(float)
    return np.array([x.mean(), x.std(), x.min(), x.max()])


# ------------------------------------------------------------------------------------------
# the whole pipeline: Compose(...) of get_train_transforms on one batch
# ------------------------------------------------------------------------------------------
def whole(data, seg, p, patch_size, noise=None):
    """data (B, C, D, H, W) float32, seg (B, 1, D, H, W) float32, p: the parameter record of
    waveformer_amd.augment.sample_train_params (read by attribute).  Returns a dict with the
    float64 result of the last data transform before its cast ("data"), "seg", the tie mask of
    the seg interpolation ("tie") and "amax", the largest magnitude any stage produced."""
    B, C = data.shape[:2]
    out = np.zeros((B, C) + tuple(patch_size), np.float32)
    last = np.zeros(out.shape, float)
    oseg = np.zeros((B, 1) + tuple(patch_size), np.float32)
    tie = np.zeros(oseg.shape, bool)
    amax = 0.0
    for b in range(B):
        if p.do_rotate[b] or p.do_scale[b]:
            coords = spatial_coords(patch_size, data.shape[2:], p.angles[b] if p.do_rotate[b] else
                                    None, p.scale[b] if p.do_scale[b] else None)
            x = np.stack([spatial_data(data[b, c], coords) for c in range(C)])
            oseg[b, 0], tie[b, 0] = spatial_seg(seg[b, 0], coords)
        else:
            x = center_crop(data[b], patch_size).astype(float)
            oseg[b, 0] = center_crop(seg[b], patch_size)[0]
        amax = max(amax, np.abs(x).max())
        cur = x.astype(np.float32)

        def step(c, val):
            nonlocal amax
            amax = max(amax, np.abs(val).max())
            last[b, c] = val
            cur[c] = val.astype(np.float32)

        last[b] = x
        if p.noise[b]:
            for c in range(C):
                step(c, gaussian_noise(cur[c], p.noise_variance[b], noise[b, c]))
        for c in range(C):
            if p.blur[b, c]:
                step(c, gaussian_blur(cur[c], p.blur_sigma[b, c]))
        if p.brightness[b]:
            for c in range(C):
                step(c, brightness(cur[c], p.brightness_mult[b, c]))
        if p.contrast[b]:
            for c in range(C):
                step(c, contrast(cur[c], p.contrast_factor[b, c]))
        for c in range(C):
            if p.lowres[b, c]:
                step(c, low_resolution(cur[c], p.lowres_zoom[b, c])[0])
        if p.gamma_inv[b]:
            for c in range(C):
                step(c, gamma(cur[c], p.gamma_inv_gamma[b, c], True))
        if p.gamma[b]:
            for c in range(C):
                step(c, gamma(cur[c], p.gamma_gamma[b, c], False))
        for d in range(3):
            if p.mirror[b, d]:
                last[b] = np.flip(last[b], 1 + d)
                cur = np.flip(cur, 1 + d)
                oseg[b] = np.flip(oseg[b], 1 + d)
                tie[b] = np.flip(tie[b], 1 + d)
        out[b] = cur
    oseg[oseg == -1] = 0  # RemoveLabelTransform(-1, 0)
    return {"data": last, "seg": oseg, "tie": tie, "amax": float(amax)}


# ------------------------------------------------------------------------------------------
# the fixture cases (shared by gen_augment_fixtures.py and the tests)
# ------------------------------------------------------------------------------------------
SHAPES = {"a": (2, 13, 17, 19), "b": (1, 3, 5, 67), "c": (1, 1, 1, 65), "d": (1, 2, 2, 2),
          "e": (1, 16, 20, 24)}
SEEDS = {"a": 11, "b": 12, "c": 13, "d": 14, "e": 15}
SEG_LABELS = (-1, 0, 1, 2, 3)
A30 = np.pi / 6
E_PATCH = (13, 17, 19)

# name -> (volume, channels used, patch size, angles or None, scale or None, seg labels)
SPATIAL_CASES = {
    # one quarter turn about x: every coordinate is an integer to within one rounding (the host
    # test asserts that none crosses a border), so floor() and the >= 0.5 rule work on grid
    # points, and one axis leaves the volume by whole voxels
    "rot90": ("a", 1, None, (np.pi / 2, 0.0, 0.0), None, SEG_LABELS),
    "ext07": ("a", 1, None, (A30, -A30, A30), 0.7, SEG_LABELS),
    "ext14": ("a", 1, None, (-A30, A30, -A30), 1.4, SEG_LABELS),
    "seg200": ("a", 0, None, (A30, -A30, A30), 0.7, (0, 200)),
    "resize": ("e", 1, E_PATCH, (0.2, -0.1, 0.3), 1.1, SEG_LABELS),
    "row": ("b", 1, None, (0.05, 0.02, -0.03), 0.93, SEG_LABELS),
    # a line has no room to rotate: any tilt takes the two unit axes out of [0, 0]
    "line": ("c", 1, None, None, 0.87, SEG_LABELS),
    "tiny": ("d", 1, None, None, 0.9, SEG_LABELS),
}
# name -> (volume, zoom); the channel is 0
LOWRES_CASES = {"half": ("a", 0.5), "full": ("a", 0.98), "row": ("b", 0.5), "line": ("c", 0.6),
                "one": ("d", 0.5)}
# name -> (volume, sigma); radius 2 and radius 4 on axes shorter than the radius
BLUR_CASES = {"s05": ("a", 0.5), "s10_row": ("b", 1.0), "s10_tiny": ("d", 1.0)}
CONTRAST_FACTORS = (0.8, 1.2)
GAMMAS_INV = (0.8, 1.3)
GAMMAS = (0.7, 1.5)
# the inputs of the edge-mode prefilter are what the low-resolution transform filters: a volume
# after the nearest-neighbour reduction
PREFILTER_MIRROR = ("a", "b", "c", "d")
PREFILTER_EDGE = {"a": 0.5, "b": 0.5, "c": 0.6, "d": 0.5}


def volume(name):
    return make_volume(SHAPES[name], SEEDS[name])


def seg_volume(name, labels=SEG_LABELS):
    return make_seg(SHAPES[name][1:], labels, SEEDS[name] + 100)


def edge_input(name):
    """Channel 0 of a volume after the order-0 reduction, (1, d, h, w) float32: numpy only."""
    x = volume(name)[0]
    target = np.round(np.array(x.shape) * PREFILTER_EDGE[name]).astype(int)
    idx = [np.clip(np.floor((np.arange(t) + 0.5) * (n / t) - 0.5 + 0.5).astype(int), 0, n - 1)
           for n, t in zip(x.shape, target)]
    return np.ascontiguousarray(x[np.ix_(*idx)][None])


def whole_params():
    """One sample of two channels with every transform drawn.  Both gammas are above 1: below
    1 the power's slope is unbounded at the channel's minimum, and what the earlier stages
    leave in fp32 would be amplified without bound -- gamma below 1 is tested on its own, on
    bitwise equal input."""
    from waveformer_amd import augment
    p = augment.no_params(1, 2)
    p.do_rotate[:] = True
    p.angles[0] = (0.3, -0.2, 0.25)
    p.do_scale[:] = True
    p.scale[:] = 1.15
    p.noise[:] = True
    p.noise_variance[:] = 0.07
    p.blur[:] = True
    p.blur_sigma[0] = (0.6, 0.9)
    p.brightness[:] = True
    p.brightness_mult[0] = (0.8, 1.2)
    p.contrast[:] = True
    p.contrast_factor[0] = (1.2, 0.8)
    p.lowres[:] = True
    p.lowres_zoom[0] = (0.6, 0.8)
    p.gamma_inv[:] = True
    p.gamma_inv_gamma[0] = (1.2, 1.4)
    p.gamma[:] = True
    p.gamma_gamma[0] = (1.3, 1.1)
    p.mirror[0] = (True, False, True)
    return p


def whole_inputs():
    data = volume("a")[None]
    seg = seg_volume("a")[None]
    noise = np.random.RandomState(77).standard_normal(data.shape).astype(np.float32)
    return data, seg, noise


def spatial_case(name):
    vol, nch, patch, angles, scale, labels = SPATIAL_CASES[name]
    data = volume(vol)[:nch]
    seg = seg_volume(vol, labels)[0]
    patch = tuple(patch or SHAPES[vol][1:])
    return data, seg, patch, angles, scale


def build_fixtures():
    """Every recorded output, as a dict of arrays (needs scipy)."""
    out = {}
    for name in PREFILTER_MIRROR:
        for axis in range(3):
            out[f"pre_mirror_{name}_{axis}"] = spline_filter_axis(volume(name)[:1], 1 + axis,
                                                                  "mirror")
    for name in PREFILTER_EDGE:
        for axis in range(3):
            out[f"pre_edge_{name}_{axis}"] = spline_filter_axis(edge_input(name), 1 + axis, "edge")
    for name in SPATIAL_CASES:
        data, seg, patch, angles, scale = spatial_case(name)
        coords = spatial_coords(patch, data.shape[1:] if len(data) else seg.shape, angles, scale)
        if len(data):
            out[f"sp_{name}_data"] = np.stack([spatial_data(v, coords) for v in data])
            # the largest magnitude among the input and the coefficients after each filtered axis
            cm, c = np.abs(data).max(), data.astype(float)
            for axis in range(3):
                c = spline_filter_axis(c, 1 + axis, "mirror")
                cm = max(cm, np.abs(c).max())
            out[f"sp_{name}_cmax"] = np.array(cm)
        res, tie = spatial_seg(seg, coords)
        out[f"sp_{name}_seg"] = res.astype(np.int16)
        out[f"sp_{name}_tie"] = np.packbits(tie)
    for name, (vol, zoom) in LOWRES_CASES.items():
        x = volume(vol)[0]
        up, target = low_resolution(x, zoom)
        down = zoom_nearest(x, target)
        out[f"lr_{name}"] = up
        out[f"lr_{name}_down"] = down.astype(np.float32)
        cm, c = np.abs(down).max(), down[None]
        for axis in range(3):
            c = spline_filter_axis(c, 1 + axis, "edge")
            cm = max(cm, np.abs(c).max())
        out[f"lr_{name}_cmax"] = np.array(cm)
    for name, (vol, sigma) in BLUR_CASES.items():
        out[f"bl_{name}"] = gaussian_blur(volume(vol)[0], sigma)
    a = volume("a")
    out["ct_a"] = np.stack([contrast(a[c], CONTRAST_FACTORS[c]) for c in range(2)])
    out["gm_inv_a"] = np.stack([gamma(a[c], GAMMAS_INV[c], True) for c in range(2)])
    out["gm_a"] = np.stack([gamma(a[c], GAMMAS[c], False) for c in range(2)])
    data, seg, noise = whole_inputs()
    w = whole(data, seg, whole_params(), data.shape[2:], noise)
    out["wh_data"] = w["data"]
    out["wh_seg"] = w["seg"].astype(np.int16)
    out["wh_tie"] = np.packbits(w["tie"])
    out["wh_amax"] = np.array(w["amax"])
    return out
