"""GPU: the augmentation kernels (csrc/augment.hip) stage by stage and
waveformer_amd.augment.apply_train_transforms end to end, against the float64 outputs of
tests/augment_ref.py recorded in tests/golden/augment_fixtures.npz (no scipy here).  Every
kernel call runs twice (with guard bytes where it has a workspace) and must repeat bitwise.

Tolerances.  U = 2^-23; every bound is per element against the float64 fixture.
  * Centre crop, identity, mirror, nearest reduction, planes that are not drawn: EXACT.
  * Segmentation: may differ from the fixture only where the restatement's own weight sum of
    some label lies within 1e-5 of 0.5 (the recorded tie mask), on at most 0.5 % of the voxels.
  * One prefilter axis: 5 U max|input|.  The FIR sqrt(3) p^|k| is summed from the tails inwards
    by FMAs; the partial sums are bounded by the remaining weights, which gives
    sqrt(3) (2 sum k p^k + 2 sum p^k + 1) 2^-24 = 4.73 * 2^-24; the a + b of a tap pair adds
    1.27 * 2^-24, the rounded coefficients 3 * 2^-24 (the filter's l1 norm): 9.0 * 2^-24 = 4.5 U.
    The cut after 18 taps leaves at most 6.4e-11 max|input| = 0.0005 U.  Worst measured ratio
    to the bound: 0.20.
  * Spatial transform and low-resolution round trip: 95 U cmax, cmax the largest magnitude
    among the input and the float64 coefficients after each axis (recorded).  Three passes, each
    amplifying what it receives by at most the l1 norm 3: 5 (9 + 3 + 1) = 65; the 64 taps: 18 for
    the three axes' weights (1 - w0 - w1 - w2 and its terms), 4.5 for the fraction rounded to
    fp32, 6 for three nested 4-term FMA sums, rounded up to 30.  Worst measured ratio: 0.028.
  * Blur: 11 U max|input|: per axis (radius + 3) 2^-24 <= 3.5 U for positive weights of sum 1.
    Worst measured ratio: 0.051.
  * Brightness: 1 U max|output| (one rounding; worst ratio 0.31).  Noise: 2 U max|output| (two
    roundings; 0.19).
  * Contrast: 5 U max|input| (three roundings on values up to 2.5 max, the rounded mean).
    Worst measured ratio: 0.144.
  * Gamma: (20 g + 2) U max|input|, g = std before / std after the power (from the float64
    restatement).  The normalised value carries 3 * 2^-24 relative, the power gamma <= 1.5
    times that plus powf's 1 ulp, the scaling back two roundings on a range <= 2 max: 8.5 U max
    before the statistics are restored; restoring subtracts a mean and divides by a std that
    each carry the same error, times g.  Worst measured ratio: 0.102.
  * The whole pipeline: K_WHOLE U amax, amax the largest magnitude any stage produced
    (recorded).  Not derived: the later stages amplify what the earlier ones leave, the cubic
    round trip and the two gammas by factors that depend on the data.  Worst measured error on
    the GPU 7.52e-7 = 2.61 U amax; with the margin of 4, rounded up: K_WHOLE = 12.
"""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -23
K_PRE, K_SPLINE, K_BLUR, K_CONTRAST, K_WHOLE = 5.0, 95.0, 11.0, 5.0, 12.0
FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "augment_fixtures.npz"))


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


def _aug():
    from waveformer_amd import augment
    return augment


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _twice(fn):
    """Run fn twice; the results (tensors, or tuples / dicts of them) must agree bitwise."""
    a, b = fn(), fn()
    flat = lambda r: list(r.values()) if isinstance(r, dict) else list(r) \
        if isinstance(r, (tuple, list)) else [r]  # noqa: E731
    for x, y in zip(flat(a), flat(b)):
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y), "the two runs differ"
    return a


def _close(name, got, want, bound):
    """|got - want| <= bound per element; prints the worst ratio before asserting."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    print(f"{name}: worst |err| {err.max():.3e}, bound {np.min(bound):.3e}, "
          f"worst ratio {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} elements beyond the bound"


def _seg_matches(name, got, key):
    want = FIX[f"{key}_seg"].astype(np.float32)
    tie = np.unpackbits(FIX[f"{key}_tie"])[:want.size].reshape(want.shape).astype(bool)
    got = got.detach().cpu().numpy().reshape(want.shape)
    diff = got != want
    print(f"{name}: {int(diff.sum())} of {want.size} voxels differ, {int(tie.sum())} may")
    assert not np.any(diff & ~tie), f"{name}: differs outside the tie mask"
    assert diff.sum() <= 0.005 * want.size


# ------------------------------------------------------------------------------------------
# prefilter
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", ref.PREFILTER_MIRROR)
def test_prefilter_mirror(name, axis):
    ops = _ops()
    x = ref.volume(name)[:1]
    got = _twice(lambda: ops.spline_prefilter_axis(_dev(x), axis, ops.SPLINE_MIRROR))
    _close(f"mirror {name} axis {axis}", got, FIX[f"pre_mirror_{name}_{axis}"],
           K_PRE * U * np.abs(x).max())
    if x.shape[1 + axis] == 1:  # scipy leaves such an axis alone
        assert torch.equal(got, _dev(x))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(ref.PREFILTER_EDGE))
def test_prefilter_edge(name, axis):
    ops = _ops()
    x = ref.edge_input(name)
    got = _twice(lambda: ops.spline_prefilter_axis(_dev(x), axis, ops.SPLINE_EDGE))
    assert got.shape[1 + axis] == x.shape[1 + axis] + 2 * ops.SPLINE_PAD
    _close(f"edge {name} axis {axis}", got, FIX[f"pre_edge_{name}_{axis}"],
           K_PRE * U * np.abs(x).max())


# ------------------------------------------------------------------------------------------
# spatial transform
# ------------------------------------------------------------------------------------------
def _spatial(data, seg, patch, angles, scale):
    ops, aug = _ops(), _aug()
    in_shape = seg.shape
    m = aug.affine_matrix(angles, scale, in_shape)

    def run():
        coef = ops.spline_prefilter(_dev(data), ops.SPLINE_MIRROR) if len(data) else None
        return ops.affine_sample(coef, _dev(seg), m, patch)
    return _twice(run)


@pytest.mark.parametrize("name", sorted(ref.SPATIAL_CASES))
def test_spatial_transform(name):
    """rot90: coordinates on the grid; ext07 / ext14: the extreme angles at both ends of the
    scale range (most of ext14 is cval); seg200: one label of 200; resize: 16 x 20 x 24 to
    13 x 17 x 19; row, line, tiny: 3 x 5 x 67, 1 x 1 x 65, 2 x 2 x 2.  The segmentations hold
    -1, 0, 1, 2, 3."""
    data, seg, patch, angles, scale = ref.spatial_case(name)
    out, oseg = _spatial(data, seg, patch, angles, scale)
    if len(data):
        want = FIX[f"sp_{name}_data"]
        _close(f"spatial {name}", out, want, K_SPLINE * U * float(FIX[f"sp_{name}_cmax"]))
        # cval exactly where the restatement has it
        assert np.array_equal(out.cpu().numpy() == 0, want == 0)
    _seg_matches(f"spatial {name} seg", oseg, f"sp_{name}")
    labels = set(np.unique(oseg.cpu().numpy()).tolist())
    assert labels <= set(np.unique(seg).tolist()) | {0.0}


def test_spatial_identity_is_the_input_bitwise():
    """Nothing drawn: the centre-crop path returns the input, and the seg with -1 -> 0."""
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    d, s = _dev(data), _dev(seg)
    out = _twice(lambda: aug.apply_train_transforms(d, s, aug.no_params(1, 2)))
    assert torch.equal(out["data"], d)
    assert (seg == -1).any()
    assert torch.equal(out["seg"], torch.where(s == -1, torch.zeros_like(s), s))
    assert out["data"].data_ptr() != d.data_ptr()


def test_spatial_unit_scale_interpolates_the_input():
    """A drawn scale of exactly 1 takes the interpolation path at the grid points: prefilter and
    64 taps give the input back within the spline bound, and the seg exactly."""
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    data = np.ascontiguousarray(data[:, :1])
    p = aug.no_params(1, 1)
    p.do_scale[:] = True
    out = _twice(lambda: aug.apply_train_transforms(_dev(data), _dev(seg), p))
    _close("unit scale", out["data"], data.astype(np.float64),
           K_SPLINE * U * float(FIX["sp_rot90_cmax"]))
    want = seg.copy()
    want[want == -1] = 0
    assert np.array_equal(out["seg"].cpu().numpy(), want)


def test_spatial_centre_crop_is_exact():
    aug = _aug()
    data, seg = ref.volume("e")[None], ref.seg_volume("e")[None]
    out = aug.apply_train_transforms(_dev(data), _dev(seg), aug.no_params(1, 1), ref.E_PATCH)
    assert np.array_equal(out["data"].cpu().numpy(), ref.center_crop(data, ref.E_PATCH))
    want = ref.center_crop(seg, ref.E_PATCH).copy()
    want[want == -1] = 0
    assert np.array_equal(out["seg"].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------
# low resolution
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.LOWRES_CASES))
def test_low_resolution(name):
    """half: zoom 0.5; full: a zoom that rounds to the full shape; one: every axis rounds to 1;
    row, line: 3 x 5 x 67 and 1 x 1 x 65."""
    ops = _ops()
    vol, zoom = ref.LOWRES_CASES[name]
    x = ref.volume(vol)[:1]
    want_down = FIX[f"lr_{name}_down"]
    target = want_down.shape
    assert target == tuple(np.round(np.array(x.shape[1:]) * zoom).astype(int))
    if name == "full":
        assert target == x.shape[1:]
    if name == "one":
        assert target == (1, 1, 1)
    down = _twice(lambda: ops.zoom_nearest(_dev(x), target))
    assert np.array_equal(down.cpu().numpy()[0], want_down)  # exact
    up = _twice(lambda: ops.zoom_cubic(ops.spline_prefilter(down, ops.SPLINE_EDGE), x.shape[1:]))
    _close(f"low resolution {name}", up[0], FIX[f"lr_{name}"],
           K_SPLINE * U * float(FIX[f"lr_{name}_cmax"]))


def test_low_resolution_leaves_other_channels_alone():
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    p = aug.no_params(1, 2)
    p.lowres[0, 0] = True
    p.lowres_zoom[0, 0] = 0.5
    out = _twice(lambda: aug.apply_train_transforms(_dev(data), _dev(seg), p, guard=True))
    assert np.array_equal(out["data"][0, 1].cpu().numpy(), data[0, 1])
    _close("low resolution channel 0", out["data"][0, 0], FIX["lr_half"],
           K_SPLINE * U * float(FIX["lr_half_cmax"]))


# ------------------------------------------------------------------------------------------
# blur
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.BLUR_CASES))
def test_blur(name):
    """sigma 0.5 (radius 2), and sigma 1.0 (radius 4) on axes of 3 and of 2: shorter than the
    radius, so the reflection wraps more than once."""
    ops = _ops()
    vol, sigma = ref.BLUR_CASES[name]
    x = ref.volume(vol)[:1]
    assert len(ops.gaussian_weights(sigma)) - 1 == int(4 * sigma + 0.5)
    np.testing.assert_allclose(ops.gaussian_weights(sigma), ref.gaussian_weights(sigma), rtol=1e-15)
    got = _twice(lambda: ops.gauss_blur(_dev(x), sigma))
    _close(f"blur {name}", got[0], FIX[f"bl_{name}"], K_BLUR * U * np.abs(x).max())


# ------------------------------------------------------------------------------------------
# statistics, contrast, gamma
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol", ["a", "b", "c", "d"])
def test_channel_stats(vol):
    """fp64 statistics of fp32 data against numpy's float64: 1e-12 (|mean| + std) -- a float64
    sum of n <= 1e4 terms around the block's first value is within n 2^-53 ~ 1e-12 of the sum of
    their magnitudes; min and max exact."""
    ops = _ops()
    x = ref.volume(vol)
    flat = x.reshape(x.shape[0], -1)
    got = _twice(lambda: ops.channel_stats(_dev(flat), guard=True)).cpu().numpy()
    for c in range(flat.shape[0]):
        want = ref.stats(flat[c])
        tol = 1e-12 * (abs(want[0]) + want[1]) + 1e-300
        assert abs(got[c, 0] - want[0]) <= tol and abs(got[c, 1] - want[1]) <= tol
        assert got[c, 2] == want[2] and got[c, 3] == want[3]


def test_channel_stats_many_blocks():
    """More than one workgroup per plane (5 x 40 x 41 x 43 = 70520 voxels each, 18 partials)."""
    ops = _ops()
    x = np.random.RandomState(5).standard_normal((5, 40 * 41 * 43)).astype(np.float32) * 3 + 7
    got = _twice(lambda: ops.channel_stats(_dev(x), guard=True)).cpu().numpy()
    for c in range(5):
        want = ref.stats(x[c])
        assert abs(got[c, 0] - want[0]) <= 1e-11 * (abs(want[0]) + want[1])
        assert abs(got[c, 1] - want[1]) <= 1e-11 * (abs(want[0]) + want[1])
        assert got[c, 2] == want[2] and got[c, 3] == want[3]


def _one_step(aug, data, seg, **fields):
    p = aug.no_params(data.shape[0], data.shape[1])
    for k, v in fields.items():
        getattr(p, k)[...] = v
    return _twice(lambda: aug.apply_train_transforms(_dev(data), _dev(seg), p, guard=True))


def test_contrast():
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    out = _one_step(aug, data, seg, contrast=True, contrast_factor=ref.CONTRAST_FACTORS)
    want = FIX["ct_a"]
    assert (want == want.max(axis=(1, 2, 3), keepdims=True)).sum() > 2  # the clip is exercised
    _close("contrast", out["data"][0], want, K_CONTRAST * U * np.abs(data).max())


def test_brightness():
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    out = _one_step(aug, data, seg, brightness=True, brightness_mult=(0.75, 1.25))
    want = np.stack([ref.brightness(data[0, c], m) for c, m in enumerate((0.75, 1.25))])
    _close("brightness", out["data"][0], want, 1.0 * U * np.abs(want).max())


def test_noise():
    aug = _aug()
    data, seg, noise = ref.whole_inputs()
    p = aug.no_params(1, 2)
    p.noise[:] = True
    p.noise_variance[:] = 0.1
    out = _twice(lambda: aug.apply_train_transforms(_dev(data), _dev(seg), p, noise=_dev(noise)))
    want = ref.gaussian_noise(data[0], 0.1, noise[0])
    _close("noise", out["data"][0], want, 2.0 * U * np.abs(want).max())  # two roundings


def _gamma_bound(x, g, invert):
    y = -x.astype(np.float64) if invert else x.astype(np.float64)
    pw = np.power((y - y.min()) / (y.max() - y.min() + 1e-7), g) * (y.max() - y.min()) + y.min()
    gain = y.std() / pw.std()
    return (20.0 * gain + 2.0) * U * np.abs(x).max()


@pytest.mark.parametrize("invert", [True, False])
def test_gamma(invert):
    """One gamma below 1 and one above, per channel, with and without inversion."""
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    gammas = ref.GAMMAS_INV if invert else ref.GAMMAS
    fields = {"gamma_inv": True, "gamma_inv_gamma": gammas} if invert else \
        {"gamma": True, "gamma_gamma": gammas}
    out = _one_step(aug, data, seg, **fields)
    want = FIX["gm_inv_a" if invert else "gm_a"]
    for c in range(2):
        _close(f"gamma invert={invert} channel {c}", out["data"][0, c], want[c],
               _gamma_bound(data[0, c], gammas[c], invert))


def test_contrast_and_gamma_on_constant_channels():
    """std 0 and range 0: contrast, gamma and gamma on the inverted image leave a constant
    channel exactly as it is (the restatement does: 0 / 1e-7 = 0, 0 / 1e-8 * 0 = 0)."""
    aug = _aug()
    data = np.empty((1, 2, 5, 6, 7), np.float32)
    data[0, 0], data[0, 1] = 1.7, -0.3
    seg = np.zeros((1, 1, 5, 6, 7), np.float32)
    for c in range(2):
        assert np.array_equal(ref.contrast(data[0, c], 0.8), data[0, c].astype(float))
        assert np.array_equal(ref.gamma(data[0, c], 0.8, True), data[0, c].astype(float))
    for fields in ({"contrast": True, "contrast_factor": (0.8, 1.2)},
                   {"gamma_inv": True, "gamma_inv_gamma": (0.8, 1.3)},
                   {"gamma": True, "gamma_gamma": (0.7, 1.5)}):
        out = _one_step(aug, data, seg, **fields)
        assert np.array_equal(out["data"].cpu().numpy(), data), fields


# ------------------------------------------------------------------------------------------
# the whole call
# ------------------------------------------------------------------------------------------
def test_whole_pipeline():
    """Every transform drawn, both channels, three mirrored axes of which two flip."""
    aug = _aug()
    data, seg, noise = ref.whole_inputs()
    p = ref.whole_params()
    d, s, n = _dev(data), _dev(seg), _dev(noise)
    out = _twice(lambda: aug.apply_train_transforms(d, s, p, noise=n, guard=True))
    assert torch.equal(d.cpu(), torch.from_numpy(data))  # the input is not written
    assert out["data"].dtype == torch.float32 and out["seg"].dtype == torch.float32
    _seg_matches("whole seg", out["seg"], "wh")
    assert not (out["seg"] == -1).any()
    _close("whole", out["data"], FIX["wh_data"], K_WHOLE * U * float(FIX["wh_amax"]))


def test_callable_keeps_the_reference_interface():
    aug = _aug()
    data, seg, _ = ref.whole_inputs()
    data, seg = np.concatenate([data] * 3), np.concatenate([seg] * 3)
    tr = aug.get_train_transforms((13, 17, 19), mirror_axes=(0, 1, 2))
    tr.rng.seed(3)
    out = tr(data=_dev(data), seg=_dev(seg))
    assert set(out) == {"data", "seg"}
    assert out["data"].shape == (3, 2, 13, 17, 19) and out["seg"].shape == (3, 1, 13, 17, 19)
    assert out["data"].is_cuda and out["data"].dtype == torch.float32
    assert torch.isfinite(out["data"]).all() and not (out["seg"] == -1).any()
    val = aug.get_validation_transforms()(data=_dev(data), seg=_dev(seg))
    assert torch.equal(val["data"], _dev(data)) and not (val["seg"] == -1).any()
    with pytest.raises(RuntimeError, match="GPU only"):
        tr(data=torch.from_numpy(data), seg=torch.from_numpy(seg))
