"""GPU: the resampling kernels (csrc/resample.hip), waveformer_amd.resampling and
MultiModalityPreprocessor(resample=True) end to end, against the float64 outputs of
tests/resample_ref.py recorded in tests/golden/preprocess_resample_fixtures.npz (no scipy here).
Every call runs twice and must repeat bitwise.

Tolerances.  U = 2^-23; every bound is per element against the float64 fixture.
  * Data: K_SPLINE U cmax with K_SPLINE = 95, the bound tests/test_gpu_augment.py sets for the
    cubic zoom (derived there); cmax is the largest magnitude among the input and every
    intermediate of the float64 separable form, after each axis' prefilter and after each axis'
    interpolation (recorded).  The clamp is 1-Lipschitz, so it does not widen the bound.  Where
    the float64 result before the clamp lies beyond the plane's minimum or maximum by more than
    the bound, the output must EQUAL that minimum or maximum.
  * Segmentation, order 1: exact outside the recorded tie mask (some label's float64 indicator
    within 1e-5 of 0.5), which covers at most 5 % of a case; the exact-halving case has weights
    0.5 and 1 only and is compared on every voxel.  Order 0: exact everywhere.
  * End to end: the same bounds.  The z-scored input of the resize carries the z-score's own
    fp32 error, at most 2^-23 (|mean| / std + 3 |x|) ~ 15 U here (tests/preprocess_ref.py), which
    three passes of Lebesgue constant below 1.6 amplify to below 60 U, against a bound of
    95 U cmax with cmax above 4.
"""
import numpy as np
import pytest
import torch

from tests import preprocess_ref
from tests import resample_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -23
K_SPLINE = 95.0


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


def _rs():
    from waveformer_amd import resampling
    return resampling


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _twice(fn):
    a, b = fn(), fn()
    assert a.dtype == b.dtype and torch.equal(a, b), "the two runs differ"
    return a


def _check_data(name, got, x, key):
    """got (N, *new) fp32 against the fixture of `key`; x (N, *old) the fp32 input, whose range
    the clamp uses."""
    fx = ref.fixtures()
    want, raw, cmax = fx[f"{key}_data"], fx[f"{key}_raw"], fx[f"{key}_cmax"]
    assert got.dtype == torch.float32
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    for c in range(len(want)):
        bound = K_SPLINE * U * cmax[c]
        err = np.abs(got[c].astype(np.float64) - want[c])
        lo, hi = x[c].min(), x[c].max()
        below, above = raw[c] < float(lo) - bound, raw[c] > float(hi) + bound
        print(f"{name}[{c}]: worst |err| {err.max():.3e}, bound {bound:.3e}, worst ratio "
              f"{err.max() / bound:.3f}; clamped low {int(below.sum())}, high {int(above.sum())} "
              f"of {want[c].size}")
        assert np.all(err <= bound), f"{name}[{c}]: {int((err > bound).sum())} beyond the bound"
        assert np.all(got[c][below] == lo) and np.all(got[c][above] == hi), \
            f"{name}[{c}]: not clamped to the plane's own range"
        assert got[c].min() >= lo and got[c].max() <= hi


def _check_seg(name, got, key, masked=True):
    fx = ref.fixtures()
    want = fx[f"{key}_seg"]
    got = got.detach().cpu().numpy().reshape(want.shape)
    diff = got != want
    if masked:
        tie = ref.unpack(fx[f"{key}_tie"], want.shape)
        assert tie.mean() <= ref.MAX_TIES
    else:
        tie = np.zeros(want.shape, bool)
    print(f"{name}: {int(diff.sum())} of {want.size} voxels differ, {int(tie.sum())} may")
    assert not np.any(diff & ~tie), f"{name}: differs outside the tie mask"


# ------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_zoom_cubic_volume(name):
    ops = _ops()
    x = ref.data_input(name)
    d = _dev(x)
    got = _twice(lambda: ops.zoom_cubic_volume(d, ref.CASES[name][1], clip=True))
    _check_data(name, got, x, name)
    assert torch.equal(d.cpu(), torch.from_numpy(x)), "the input was written"


@pytest.mark.parametrize("name", ["down", "tiny", "long_h"])
def test_unclamped_zoom(name):
    """clip=False: the raw zoom, within the same bound, and it does leave the input's range."""
    ops = _ops()
    fx = ref.fixtures()
    x = ref.data_input(name)
    got = _twice(lambda: ops.zoom_cubic_volume(_dev(x), ref.CASES[name][1], clip=False))
    got = got.cpu().numpy().astype(np.float64)
    for c in range(len(x)):
        bound = K_SPLINE * U * fx[f"{name}_cmax"][c]
        err = np.abs(got[c] - fx[f"{name}_raw"][c])
        print(f"{name}[{c}] unclamped: worst ratio {err.max() / bound:.3f}")
        assert np.all(err <= bound)
        assert got[c].min() < x[c].min()


def test_single_axis_passes_compose_in_any_order():
    """The axis passes commute up to rounding: W, H, D gives the fixture within the bound as
    well (the clamp on the last pass)."""
    ops = _ops()
    x = ref.data_input("down")
    new = ref.CASES["down"][1]
    d = _dev(x)
    stats = ops.channel_stats(d.view(2, -1))
    a = ops.spline_zoom_axis(d, 2, new[2])
    b = ops.spline_zoom_axis(a, 1, new[1])
    got = ops.spline_zoom_axis(b, 0, new[0], clip=stats)
    _check_data("down (W, H, D)", got, x, "down")


def test_same_shape_returns_the_input():
    ops = _ops()
    d = _dev(ref.data_input("tiny"))
    assert ops.zoom_cubic_volume(d, d.shape[1:]) is d
    out = _rs().resample_data_or_seg(d, d.shape[1:])
    assert out is d


def test_resample_data_or_seg_to_shape_and_spacing():
    rs = _rs()
    x = ref.data_input("down")
    new = ref.CASES["down"][1]
    got = _twice(lambda: rs.resample_data_or_seg_to_shape(x, new, (1, 1, 1), (1.5, 1.4, 1.6)))
    assert got.device.type == "cuda"
    _check_data("to_shape", got, x, "down")
    # (20, 24, 18) at 1 mm -> spacing (20/13, 24/17, 18/11) rounds to the same shape
    spacing = [a / b for a, b in zip(x.shape[1:], new)]
    got2 = rs.resample_data_or_seg_to_spacing(_dev(x), (1.0, 1.0, 1.0), spacing)
    assert torch.equal(got, got2)


def test_data_order_zero_is_exact():
    rs = _rs()
    x = ref.data_input("up")
    new = ref.CASES["up"][1]
    got = _twice(lambda: rs.resample_data_or_seg(x, new, order=0)).cpu().numpy()
    # nearest: every output is an input value at zoom's rounded coordinate
    idx = [np.clip(np.floor((np.arange(on) + 0.5) * (n / on) - 0.5 + 0.5).astype(int), 0, n - 1)
           for n, on in zip(x.shape[1:], new)]
    want = x[0][np.ix_(*idx)]
    assert np.array_equal(got[0], want)


# ------------------------------------------------------------------------------------------
# segmentation
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_zoom_seg_linear(name):
    ops = _ops()
    seg = _dev(ref.seg_input(name))
    got = _twice(lambda: ops.zoom_seg_linear(seg, ref.CASES[name][1]))
    assert got.dtype == torch.int16
    _check_seg(name, got, name, masked=name != ref.EXACT_SEG_CASE)


@pytest.mark.parametrize("name", ["down", "up", "half", "single", "tiny"])
def test_seg_order_zero_is_exact(name):
    rs = _rs()
    seg = ref.seg_input(name)[None]
    got = _twice(lambda: rs.resample_data_or_seg(seg, ref.CASES[name][1], is_seg=True, order=0))
    assert got.dtype == torch.int16
    assert np.array_equal(got.cpu().numpy()[0], ref.fixtures()[f"{name}_seg0"])


def test_seg_through_the_reference_interface_keeps_its_dtype():
    rs = _rs()
    for dtype in (np.int8, np.int16, np.float32):
        seg = ref.seg_input("mixed")[None].astype(dtype)
        got = rs.resample_data_or_seg_to_shape(seg, ref.CASES["mixed"][1], (1, 1, 1), (1, 1, 1),
                                               is_seg=True, order=1)
        assert got.dtype == torch.from_numpy(seg).dtype
        _check_seg(f"mixed as {np.dtype(dtype).name}", got[0], "mixed")


# ------------------------------------------------------------------------------------------
# the whole case
# ------------------------------------------------------------------------------------------
def _run_case(resample, spacing, out_spacing):
    from waveformer_amd import preprocessing as pp
    data, seg = ref.e2e_inputs()
    props = {"spacing": spacing}
    p = pp.MultiModalityPreprocessor(out_spacing=out_spacing, all_labels=(1, 2, 3),
                                     resample=resample)
    out, seg_out = p.run_case_npy(data, seg, props)
    return out, seg_out, props


def test_run_case_resamples():
    from waveformer_amd import preprocessing as pp
    out, seg_out, props = _run_case(True, ref.E2E_SPACING, ref.E2E_OUT_SPACING)
    out2, seg_out2, props2 = _run_case(True, ref.E2E_SPACING, ref.E2E_OUT_SPACING)
    assert torch.equal(out, out2) and torch.equal(seg_out, seg_out2)
    for k in pp.PROPERTY_KEYS:
        assert k in props, k
    assert props["original_spacing_trans"] == [2.0, 1.0, 1.0]
    assert props["target_spacing_trans"] == list(ref.E2E_OUT_SPACING)
    assert props["bbox_used_for_cropping"] == [[3, 15], [5, 20], [6, 19]]
    assert tuple(props["shape_after_cropping_before_resample"]) == ref.E2E_CROPPED
    assert tuple(int(v) for v in props["shape_after_resample"]) == ref.E2E_NEW_SHAPE
    assert tuple(out.shape) == (2,) + ref.E2E_NEW_SHAPE and out.dtype == torch.float32
    assert tuple(seg_out.shape) == (1,) + ref.E2E_NEW_SHAPE and seg_out.dtype == torch.int8
    # the clamp's range is that of the device's own z-scored crop: what a run without a
    # resample returns, bitwise (test_run_case_without_a_resample_is_unchanged)
    norm = _run_case(False, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))[0].cpu().numpy()
    assert np.abs(norm - ref.e2e_before_resample()[0]).max() < 1e-5
    _check_data("e2e", out, norm, "e2e")
    _check_seg("e2e", seg_out[0], "e2e")
    # class_locations are drawn on the RESAMPLED segmentation
    got_seg = seg_out.cpu().numpy()
    want_locs = preprocess_ref.sample_foreground_locations(got_seg, [1, 2, 3])
    for c in (1, 2, 3):
        assert len(want_locs[c]) > 0
        assert np.array_equal(props["class_locations"][c], want_locs[c])
        assert np.array_equal(props2["class_locations"][c], want_locs[c])


def test_run_case_without_a_resample_is_unchanged():
    a, sa, pa = _run_case(False, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    b, sb, pb = _run_case(True, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    assert torch.equal(a, b) and sa.dtype == sb.dtype and torch.equal(sa, sb)
    assert list(pa["shape_after_resample"]) == list(pb["shape_after_resample"]) == \
        list(ref.E2E_CROPPED)
    for c in (1, 2, 3):
        assert np.array_equal(pa["class_locations"][c], pb["class_locations"][c])
    with pytest.raises(NotImplementedError, match="resampl"):
        _run_case(False, ref.E2E_SPACING, ref.E2E_OUT_SPACING)
