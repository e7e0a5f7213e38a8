"""numpy restatement of the reference's per-case preprocessing (light_training/preprocessing:
cropping/cropping.py, preprocessors/default_preprocessor.py :155-228 and :414-483,
normalization/default_normalization_schemes.py :28-50, resampling/default_resampling.py :23-30)
and the deterministic cases the preprocessing tests share.  scipy is used for the hole fill only
and imported only there: the GPU tests read tests/golden/preprocess_fixtures.npz instead.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "preprocess_fixtures.npz")
NUM_SAMPLES = 10000
_fixtures = None


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
def nonzero_mask(data):
    """cropping.py:16-19 (without the fill)."""
    m = np.zeros(data.shape[1:], dtype=bool)
    for c in range(data.shape[0]):
        m = m | (data[c] != 0)
    return m


def fill_holes(mask):
    from scipy.ndimage import binary_fill_holes
    return binary_fill_holes(mask)


def bbox_from_mask(mask):
    """acvl_utils get_bbox_from_mask: half-open [[z0, z1], [y0, y1], [x0, x1]]."""
    if not mask.any():
        raise ValueError("empty mask")
    out = []
    for axis in range(3):
        other = tuple(a for a in range(3) if a != axis)
        idx = np.flatnonzero(mask.any(axis=other))
        out.append([int(idx[0]), int(idx[-1]) + 1])
    return out


def crop_to_nonzero(data, seg, filled, nonzero_label=-1):
    """cropping.py:24-49 given the filled mask (so that no scipy is needed here)."""
    bbox = bbox_from_mask(filled)
    sl = tuple(slice(b[0], b[1]) for b in bbox)
    data = data[(slice(None),) + sl]
    m = filled[sl][None]
    if seg is not None:
        seg = seg[(slice(None),) + sl].copy()
        seg[(seg == 0) & (~m)] = nonzero_label
    else:
        m = m.astype(np.int8)
        m[m == 0] = nonzero_label
        m[m > 0] = 0
        seg = m
    return data, seg, bbox


def seg_dtype(seg):
    """default_preprocessor.py:208-211."""
    return np.int16 if np.max(seg) > 127 else np.int8


def zscore64(image):
    """ZScoreNormalization(use_mask_for_norm=False) in float64: (ref, mean, std)."""
    x = image.astype(np.float64)
    mean, std = x.mean(), x.std()
    return (x - mean) / max(std, 1e-8), mean, std


def zscore_bound(ref, mean, std):
    """|out - ref| <= 2^-23 (|mean| / std + 3 |ref|): one rounding of the mean (2^-24 |mean|,
    divided by std), three fp32 operations (subtract, divide / multiply, the rounding of std or
    its reciprocal: 2^-24 |ref| each), times a margin of 2."""
    return 2.0 ** -23 * (abs(mean) / max(std, 1e-8) + 3.0 * np.abs(ref))


def compute_new_shape(old_shape, old_spacing, new_spacing):
    return np.array([int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)])


def sample_foreground_locations(seg, classes, seed=1234):
    """default_preprocessor.py:454-483 for single classes."""
    rndst = np.random.RandomState(seed)
    out = {}
    for c in classes:
        all_locs = np.argwhere(seg == c)
        if len(all_locs) == 0:
            out[c] = []
            continue
        target = min(NUM_SAMPLES, len(all_locs))
        target = max(target, int(np.ceil(len(all_locs) * 0.01)))
        out[c] = all_locs[rndst.choice(len(all_locs), target, replace=False)]
    return out


def collect_foreground_intensities(segmentation, images, seed=1234, num_samples=NUM_SAMPLES):
    """default_preprocessor.py:414-441 (the sampled intensities only)."""
    rs = np.random.RandomState(seed)
    fg = segmentation[0] > 0
    out = []
    for i in range(len(images)):
        px = images[i][fg]
        out.append(rs.choice(px, num_samples, replace=True) if len(px) > 0 else [])
    return out


# ------------------------------------------------------------------------------------------
# hole-fill cases
# ------------------------------------------------------------------------------------------
def _shell():
    m = np.zeros((9, 9, 9), dtype=bool)
    m[1:8, 1:8, 1:8] = True
    m[2:7, 2:7, 2:7] = False  # the cavity
    return m


def _tunnel():
    m = _shell()
    m[4, 4, 1] = False  # a one-voxel tunnel through the x = 1 wall
    return m


def _edge_diagonal():
    m = np.zeros((9, 9, 9), dtype=bool)
    m[1:8, 1:8, 1:8] = True
    m[4, 4, 4] = False     # the cavity
    m[4:8, 5, 5] = False   # a corridor to the outside that touches it across an edge only
    return m


def _cup():
    m = np.zeros((9, 9, 9), dtype=bool)
    m[0:6, 2:7, 2:7] = True
    m[0:5, 3:6, 3:6] = False  # open to the z = 0 array face
    return m


def _serpentine():
    """All foreground but a one-voxel corridor from the x = 0 face through every odd (z, y) row
    of a 9 x 9 x 33 block, row after row: 16 rows of 31, about 500 steps to its far end."""
    D, H, W = 9, 9, 33
    m = np.ones((D, H, W), dtype=bool)
    rows = []
    for iz, z in enumerate(range(1, D - 1, 2)):
        ys = list(range(1, H - 1, 2))
        rows += [(z, y) for y in (ys if iz % 2 == 0 else ys[::-1])]
    m[rows[0][0], rows[0][1], 0] = False  # the mouth
    end = W - 2  # the x at which the corridor leaves the current row
    for k, (z, y) in enumerate(rows):
        m[z, y, 1:W - 1] = False
        if k + 1 < len(rows):
            nz, ny = rows[k + 1]
            m[(z + nz) // 2, (y + ny) // 2, end] = False
            end = 1 if end == W - 2 else W - 2
    return m


def _random(shape, density, seed):
    return np.random.RandomState(seed).random_sample(shape) < density


def _ellipsoid():
    D, H, W = 77, 120, 120
    z, y, x = np.ogrid[:D, :H, :W]
    e = ((z - 38) / 30.0) ** 2 + ((y - 60) / 50.0) ** 2 + ((x - 58) / 45.0) ** 2 <= 1.0
    return e ^ (np.random.RandomState(77).random_sample((D, H, W)) < 0.02)  # 2 % pepper


CONSTRUCTED = {
    "shell": _shell,
    "tunnel": _tunnel,
    "edge_diagonal": _edge_diagonal,
    "cup": _cup,
    "serpentine": _serpentine,
    "empty": lambda: np.zeros((5, 6, 7), dtype=bool),
    "full": lambda: np.ones((5, 6, 7), dtype=bool),
}
RANDOM = {
    "rand50": lambda: _random((17, 19, 23), 0.5, 1),
    "rand70": lambda: _random((17, 19, 23), 0.7, 2),
    "s3x5x130": lambda: _random((3, 5, 130), 0.6, 3),
    "s7x13x67": lambda: _random((7, 13, 67), 0.65, 4),
    "s1x1x65": lambda: _random((1, 1, 65), 0.5, 5),
    "s65x1x1": lambda: _random((65, 1, 1), 0.5, 6),
}
FILL_CASES = {**CONSTRUCTED, **RANDOM}  # their filled masks are in the fixture as packed bits
HASH_CASE = "ellipsoid"                 # bbox, count and SHA-256 only


def fill_case(name):
    return _ellipsoid() if name == HASH_CASE else FILL_CASES[name]()


def pack(mask):
    return np.packbits(np.ascontiguousarray(mask).astype(bool).ravel())


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(bool)


def mask_hash(mask):
    return hashlib.sha256(pack(mask).tobytes()).hexdigest()


def build_fixtures():
    """Everything gen_preprocess_fixtures.py stores (needs scipy)."""
    out = {}
    for name in FILL_CASES:
        out[f"{name}_filled"] = pack(fill_holes(fill_case(name)))
    f = fill_holes(fill_case(HASH_CASE))
    out[f"{HASH_CASE}_bbox"] = np.array(bbox_from_mask(f), dtype=np.int64)
    out[f"{HASH_CASE}_count"] = np.array(int(f.sum()), dtype=np.int64)
    out[f"{HASH_CASE}_sha256"] = np.array(mask_hash(f))
    return out


def fixtures():
    global _fixtures
    if _fixtures is None:
        with np.load(GOLDEN) as z:
            _fixtures = {k: z[k] for k in z.files}
    return _fixtures


def filled_reference(name):
    return unpack(fixtures()[f"{name}_filled"], fill_case(name).shape)


# ------------------------------------------------------------------------------------------
# crop / normalisation / sampling cases
# ------------------------------------------------------------------------------------------
def blob_case(shape=(20, 24, 28), lo=(3, 5, 6), hi=(15, 20, 19), channels=2, seed=11,
              mean=300.0, std=200.0):
    """An off-centre box of nonzero intensities in zeros, with labels 1..3 inside it."""
    rs = np.random.RandomState(seed)
    data = np.zeros((channels,) + tuple(shape), dtype=np.float32)
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    inner = tuple(b - a for a, b in zip(lo, hi))
    for c in range(channels):
        data[(c,) + sl] = (rs.standard_normal(inner) * std + mean * (c + 1)).astype(np.float32)
    seg = np.zeros((1,) + tuple(shape), dtype=np.int16)
    seg[(0,) + sl] = rs.randint(0, 4, size=inner)
    return data, seg
