"""GPU: the preprocessing kernels (csrc/preprocess.hip) stage by stage and
waveformer_amd.preprocessing end to end, against the numpy restatement of tests/preprocess_ref.py
and the recorded scipy hole fills of tests/golden/preprocess_fixtures.npz (no scipy here).

Tolerances:
  * masks, filled masks, bounding boxes, counts, cropped data and segmentations, sampled
    locations and intensities: EXACT.
  * the z-scored data, per element against float64:  |out - ref| <= 2^-23 (|mean| / std + 3 |ref|)
    (preprocess_ref.zscore_bound: one rounding of the mean, three fp32 operations, a margin of 2).
  * the fp64 moments against numpy's float64: 1e-9 (|mean| + std) resp. 1e-9 std.  A float64 sum
    of n <= 1e5 terms is within n 2^-53 ~ 1e-11 of the sum of their magnitudes; the shifted
    variance sum(d^2)/n - (sum(d)/n)^2 with d = x - x[0], |mean - x[0]| <= 5 std amplifies that by
    at most 1 + 5^2 = 26; 1e-9 leaves a factor of a few.  They are bitwise repeatable.
"""
import numpy as np
import pytest
import torch

from tests import preprocess_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from waveformer_amd import _lib
    _lib.load()
    yield


def _ops():
    from waveformer_amd import ops
    return ops


def _pp():
    from waveformer_amd import preprocessing
    return preprocessing


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fill(mask):
    """Fill twice with guard bytes behind the workspace; the two runs must agree bitwise."""
    ops = _ops()
    m = _dev(mask.astype(np.uint8))
    f1, b1, r1 = ops.fill_holes(m, guard=True)
    f2, b2, r2 = ops.fill_holes(m, guard=True)
    assert f1.dtype == torch.uint8 and torch.equal(f1, f2) and torch.equal(b1, b2) and r1 == r2
    return f1.cpu().numpy(), b1.cpu().tolist(), r1


def _check_bbox(bbox8, filled):
    n = int(filled.sum())
    assert bbox8[6] == n and bbox8[7] == 0
    if n:
        assert [bbox8[0:2], bbox8[2:4], bbox8[4:6]] == ref.bbox_from_mask(filled)
    else:
        assert bbox8[:6] == [0] * 6


# ------------------------------------------------------------------------------------------
# hole fill
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.FILL_CASES))
def test_fill_matches_scipy(name):
    mask = ref.fill_case(name)
    want = ref.filled_reference(name)
    got, bbox8, rounds = _fill(mask)
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    _check_bbox(bbox8, want)
    assert 0 <= rounds <= int((~mask).sum())


def test_fill_by_construction():
    got = {n: _fill(ref.fill_case(n)) for n in ref.CONSTRUCTED}
    f = {n: g[0].astype(bool) for n, g in got.items()}
    m = {n: ref.fill_case(n) for n in ref.CONSTRUCTED}
    assert f["shell"][2:7, 2:7, 2:7].all()                       # a closed cavity is filled
    assert not f["tunnel"][2:7, 2:7, 2:7].any()                  # a one-voxel face tunnel opens it
    assert f["edge_diagonal"][4, 4, 4] and not f["edge_diagonal"][4, 5, 5]  # 6-, not 26-connected
    assert np.array_equal(f["cup"], m["cup"])                    # open to an array face
    assert np.array_equal(f["serpentine"], m["serpentine"])      # the corridor's far end is outside
    assert got["serpentine"][2] > 8                              # more rounds than one batch
    assert not f["empty"].any() and got["empty"][1][6] == 0
    assert f["full"].all() and got["full"][2] == 0


def test_fill_ellipsoid_by_hash():
    fx = ref.fixtures()
    got, bbox8, rounds = _fill(ref.fill_case(ref.HASH_CASE))
    assert bbox8[6] == int(fx["ellipsoid_count"])
    assert [bbox8[0:2], bbox8[2:4], bbox8[4:6]] == fx["ellipsoid_bbox"].tolist()
    assert ref.mask_hash(got) == str(fx["ellipsoid_sha256"])
    print(f"ellipsoid 77x120x120: {rounds} fill rounds")


def test_fill_in_place():
    ops = _ops()
    mask = ref.fill_case("rand70")
    m = _dev(mask.astype(np.uint8) * 7)  # any non-zero value is set
    f, _, _ = ops.fill_holes(m)
    assert np.array_equal(f.cpu().numpy().astype(bool), ref.filled_reference("rand70"))
    assert np.array_equal(m.cpu().numpy(), mask.astype(np.uint8) * 7)  # the input is left alone


# ------------------------------------------------------------------------------------------
# nonzero mask
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,shape", [(1, (3, 5, 7)), (4, (3, 5, 7)), (1, (4, 4, 8)), (4, (4, 4, 8))])
def test_nonzero_mask_compares_like_numpy(C, shape):
    # (3, 5, 7): 105 voxels, the scalar path; (4, 4, 8): the 16-byte path
    ops = _ops()
    data = np.zeros((C,) + shape, dtype=np.float32)
    flat = data.reshape(C, -1)
    flat[0, 1] = np.float32(1e-45)          # a denormal: nonzero
    flat[C - 1, 2] = np.float32(np.nan)     # NaN != 0
    flat[0, 3] = np.float32(-0.0)           # -0.0 == 0
    flat[C - 1, 5] = -2.5
    flat[C // 2, 6] = np.float32(-1e-45)
    flat[0, -1] = 3.0
    assert flat.view(np.uint32)[0, 1] == 1 and flat.view(np.uint32)[0, 3] == 0x80000000
    want = (data.view(np.uint32) & 0x7fffffff).any(axis=0)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(want, ref.nonzero_mask(data))  # numpy's != agrees with the bits
    assert want.reshape(-1)[[1, 2, 5, 6, -1]].all() and not want.reshape(-1)[3]
    got = ops.nonzero_mask(_dev(data))
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
    # an offset view is not 16-byte aligned: the scalar path must give the same
    buf = torch.zeros(data.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = _dev(data).reshape(-1)
    got2 = ops.nonzero_mask(buf[1:].view((C,) + shape))
    assert torch.equal(got, got2)


# ------------------------------------------------------------------------------------------
# bounding box, crop, segmentation
# ------------------------------------------------------------------------------------------
def _solid_case(shape, lo, hi, channels=2, seed=0, seg=None):
    """Solid boxes have no holes: the filled mask is the nonzero mask, no scipy needed."""
    data, s = ref.blob_case(shape, lo, hi, channels=channels, seed=seed)
    assert (data[0][tuple(slice(a, b) for a, b in zip(lo, hi))] != 0).all()
    return data, (s if seg == "given" else None)


CROP_CASES = {
    # name: (shape, lo, hi): x offset / width multiples of 4 (16-byte path) or not (scalar)
    "vec": ((10, 12, 16), (2, 3, 4), (7, 9, 12)),
    "scalar_offset": ((10, 12, 16), (2, 3, 3), (7, 9, 11)),
    "scalar_width": ((10, 12, 16), (1, 0, 4), (10, 11, 13)),
    "odd_volume": ((5, 7, 9), (1, 2, 3), (4, 6, 8)),
    "single_voxel": ((6, 7, 8), (3, 4, 5), (4, 5, 6)),
    "touches_every_end": ((6, 8, 12), (0, 0, 0), (6, 8, 12)),
}


@pytest.mark.parametrize("with_seg", ["given", "absent"])
@pytest.mark.parametrize("name", sorted(CROP_CASES))
def test_crop_to_nonzero(name, with_seg):
    pp = _pp()
    shape, lo, hi = CROP_CASES[name]
    data, seg = _solid_case(shape, lo, hi, seg=with_seg)
    if name == "touches_every_end":  # only the corners are nonzero: the box is the volume
        keep = np.zeros(shape, dtype=bool)
        keep[::shape[0] - 1, ::shape[1] - 1, ::shape[2] - 1] = True
        data = data * keep
    filled = ref.nonzero_mask(data)
    want_data, want_seg, want_bbox = ref.crop_to_nonzero(data, seg, filled)
    got_data, got_seg, got_bbox = pp.crop_to_nonzero(data, seg)
    assert got_bbox == want_bbox == [[a, b] for a, b in zip(lo, hi)]
    assert got_data.dtype == torch.float32 and got_seg.dtype == torch.int16
    assert np.array_equal(got_data.cpu().numpy(), want_data)
    assert np.array_equal(got_seg.cpu().numpy(), want_seg)
    if name == "touches_every_end" and seg is None:
        assert int((want_seg == -1).sum()) == int(np.prod(shape)) - 8


def test_crop_marks_only_zero_labels_outside_the_mask():
    pp = _pp()
    data, seg = ref.blob_case((8, 9, 10), (1, 1, 1), (7, 8, 9), seed=5)
    data[:, 3:5, 3:5, 3:5] = 0          # a hole open through ...
    data[:, 3:5, 3:5, 0:3] = 0          # ... a tunnel to the x = 0 face: it stays outside
    seg[0, 3, 3, 3] = 0
    seg[0, 4, 4, 4] = 2                 # a label outside the mask is kept
    filled = ref.nonzero_mask(data)     # every background voxel here reaches the border
    want_data, want_seg, want_bbox = ref.crop_to_nonzero(data, seg, filled)
    got_data, got_seg, got_bbox = pp.crop_to_nonzero(data, seg)
    assert got_bbox == want_bbox
    assert np.array_equal(got_seg.cpu().numpy(), want_seg)
    z, y, x = (3 - b[0] for b in want_bbox)
    assert want_seg[0, z, y, x] == -1 and want_seg[0, z + 1, y + 1, x + 1] == 2
    got_data7, got_seg7, _ = pp.crop_to_nonzero(data, seg, nonzero_label=7)
    assert got_seg7[0, z, y, x].item() == 7


def test_all_zero_case_raises():
    pp = _pp()
    data = np.zeros((2, 4, 5, 6), dtype=np.float32)
    data[1, 2, 2, 2] = -0.0
    with pytest.raises(ValueError, match="empty"):
        pp.crop_to_nonzero(data)
    with pytest.raises(ValueError, match="empty"):
        pp.MultiModalityPreprocessor().run_case_npy(data, None, {"spacing": (1.0, 1.0, 1.0)})


def test_seg_dtype_follows_its_maximum():
    pp = _pp()
    data, seg = ref.blob_case((8, 9, 10), (1, 2, 3), (7, 8, 9), seed=6)
    p = pp.MultiModalityPreprocessor()
    _, s8 = p.run_case_npy(data, seg, {"spacing": (1.0, 1.0, 1.0)})
    assert s8.dtype == torch.int8
    seg[0, 4, 4, 4] = 200
    props = {"spacing": (1.0, 1.0, 1.0)}
    _, s16 = p.run_case_npy(data, seg, props)
    assert s16.dtype == torch.int16
    _, want_seg, _ = ref.crop_to_nonzero(data, seg, ref.nonzero_mask(data))
    assert ref.seg_dtype(want_seg) == np.int16
    assert np.array_equal(s16.cpu().numpy(), want_seg)
    _, s_absent = p.run_case_npy(data, None, {"spacing": (1.0, 1.0, 1.0)})
    assert s_absent.dtype == torch.int8 and set(np.unique(s_absent.cpu().numpy())) <= {-1, 0}


# ------------------------------------------------------------------------------------------
# normalisation
# ------------------------------------------------------------------------------------------
MOMENTS = [(300.0, 200.0), (5000.0, 30.0), (0.01, 0.003), (-40.0, 1000.0)]
# the whole of an odd volume (scalar accesses), and a 16-byte-aligned box inside a larger one
NORM_LAYOUTS = {"scalar": ((37, 41, 53), [[0, 37], [0, 41], [0, 53]]),
                "vec": ((14, 18, 24), [[1, 13], [2, 17], [4, 20]]),
                "scalar_box": ((14, 18, 24), [[1, 13], [2, 17], [3, 20]])}


@pytest.mark.parametrize("layout", sorted(NORM_LAYOUTS))
def test_zscore_against_float64(layout):
    ops = _ops()
    shape, box = NORM_LAYOUTS[layout]
    rs = np.random.RandomState(21)
    data = np.stack([(rs.standard_normal(shape) * s + m).astype(np.float32) for m, s in MOMENTS])
    x = _dev(data)
    stats = ops.box_moments(x, box, guard=True)
    assert torch.equal(stats, ops.box_moments(x, box, guard=True))  # bitwise repeatable
    got = ops.crop_normalize(x, box, stats).cpu().numpy()
    st = stats.cpu().numpy()
    sl = tuple(slice(a, b) for a, b in box)
    for c in range(len(MOMENTS)):
        want, mean, std = ref.zscore64(data[c][sl])
        assert abs(st[c, 0] - mean) <= 1e-9 * (abs(mean) + std), (c, st[c, 0], mean)
        assert abs(st[c, 1] - std) <= 1e-9 * std, (c, st[c, 1], std)
        err = np.abs(got[c].astype(np.float64) - want)
        bound = ref.zscore_bound(want, mean, std)
        worst = float((err / bound).max())
        print(f"{layout} channel {c}: max |err| / bound = {worst:.3f}")
        assert (err <= bound).all(), (layout, c, worst)


def test_normalize_in_place_and_constant_channel():
    pp = _pp()
    rs = np.random.RandomState(22)
    data = rs.standard_normal((3, 6, 10, 12)).astype(np.float32) * 50 + 100
    data[1] = np.float32(1234.567)      # constant and nonzero: exact zeros
    data[2] = 0.0                        # std 0 -> divided by 1e-8: still exact zeros
    x = _dev(data)
    out = pp.MultiModalityPreprocessor()._normalize(x, None, {})
    assert out.data_ptr() == x.data_ptr()
    got = out.cpu().numpy()
    assert (got[1] == 0).all() and (got[2] == 0).all()
    want, mean, std = ref.zscore64(data[0])
    assert (np.abs(got[0] - want) <= ref.zscore_bound(want, mean, std)).all()


# ------------------------------------------------------------------------------------------
# sampling
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampling_case():
    # class 1: below 10000 voxels; class 2: above; class 3: absent; 5 % background
    rs = np.random.RandomState(31)
    seg = rs.choice([0, 1, 2, 5], size=(1, 33, 47, 61), p=[0.05, 0.04, 0.61, 0.3]).astype(np.int16)
    images = rs.standard_normal((2, 33, 47, 61)).astype(np.float32)
    return seg, images


def test_class_locations_equal_the_restatement(sampling_case):
    pp = _pp()
    seg, _ = sampling_case
    classes = [1, 3, 2, 5]
    n = {c: int((seg == c).sum()) for c in classes}
    assert 0 < n[1] < 10000 < n[2] and n[3] == 0
    want = ref.sample_foreground_locations(seg, classes)
    got = pp.sample_foreground_locations(seg, classes)
    assert list(got) == classes and got[3] == []
    for c in (1, 2, 5):
        assert got[c].dtype == np.int64 and got[c].shape == want[c].shape
        assert np.array_equal(got[c], want[c])


def test_class_locations_of_a_slab_above_a_million_voxels():
    # 0.01 n > 10000: the coverage term decides the sample size
    pp = _pp()
    seg = np.zeros((1, 128, 128, 70), dtype=np.int16)
    seg[0, :, :, 3:67] = 4
    n = 128 * 128 * 64
    want = ref.sample_foreground_locations(seg, [4])
    got = pp.sample_foreground_locations(_dev(seg), [4])
    assert want[4].shape == (int(np.ceil(0.01 * n)), 4) and want[4].shape[0] > 10000
    assert np.array_equal(got[4], want[4])


def test_foreground_intensities_equal_the_restatement(sampling_case):
    pp = _pp()
    seg, images = sampling_case
    want = ref.collect_foreground_intensities(seg, images)
    got, stats = pp.collect_foreground_intensities(seg, images)
    assert stats == [] and len(got) == 2
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == (10000,)
        assert np.array_equal(g, w)
    none, _ = pp.collect_foreground_intensities(np.zeros_like(seg), images)
    assert none == [[], []]


def test_ranks_out_of_range_are_flagged():
    ops = _ops()
    lab = torch.zeros((2, 3, 70), dtype=torch.int16, device=DEV)
    lab[1, 2, 69] = 1
    lab[0, 0, 0] = 1
    sel = ops.Selection(lab, ops.SELECT_EQ, 1, guard=True)
    assert sel.total.item() == 2
    got = sel.pick(torch.tensor([1, 0, 2, -1], dtype=torch.int64, device=DEV)).cpu().tolist()
    assert got == [[0, 1, 2, 69], [0, 0, 0, 0], [-1] * 4, [-1] * 4]


# ------------------------------------------------------------------------------------------
# the whole case
# ------------------------------------------------------------------------------------------
def test_run_case_round_trip_with_predictor():
    pp = _pp()
    from waveformer_amd.prediction import Predictor
    data, seg = ref.blob_case((20, 24, 28), (3, 5, 6), (15, 20, 19), channels=4, seed=41)
    props = {"spacing": (1.0, 1.0, 1.0)}
    p = pp.MultiModalityPreprocessor(out_spacing=(1.0, 1.0, 1.0), all_labels=(1, 2, 3))
    out, seg_out = p.run_case_npy(data, seg, props)
    for k in pp.PROPERTY_KEYS:
        assert k in props, k
    assert props["bbox_used_for_cropping"] == [[3, 15], [5, 20], [6, 19]]
    assert tuple(props["shape_before_cropping"]) == (20, 24, 28)
    assert tuple(props["shape_after_cropping_before_resample"]) == (12, 15, 13)
    assert list(props["shape_after_resample"]) == [12, 15, 13]
    assert props["original_spacing_trans"] == [1.0, 1.0, 1.0]
    # against the restatement
    filled = ref.nonzero_mask(data)  # a solid box: nothing to fill
    want_data, want_seg, _ = ref.crop_to_nonzero(data, seg, filled)
    assert seg_out.dtype == torch.int8 and np.array_equal(seg_out.cpu().numpy(), want_seg)
    got = out.cpu().numpy()
    for c in range(4):
        want, mean, std = ref.zscore64(want_data[c])
        assert (np.abs(got[c] - want) <= ref.zscore_bound(want, mean, std)).all()
    want_locs = ref.sample_foreground_locations(want_seg, [1, 2, 3])
    for c in (1, 2, 3):
        assert np.array_equal(props["class_locations"][c], want_locs[c])
    # the cropped seg as the "prediction": every label returns to its voxel
    pred = seg_out[0].clamp(min=0).to(torch.uint8)
    back = Predictor.predict_noncrop_probability(pred, props)
    assert back.shape == (20, 24, 28) and np.array_equal(back, seg[0].astype(np.uint8))


def test_resampling_is_refused():
    pp = _pp()
    data, seg = ref.blob_case((8, 9, 10), (1, 2, 3), (7, 8, 9), seed=7)
    with pytest.raises(NotImplementedError, match="resampl"):
        pp.MultiModalityPreprocessor().run_case_npy(data, seg, {"spacing": (1.0, 1.0, 2.0)})
