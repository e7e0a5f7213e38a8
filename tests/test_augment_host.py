"""CPU: the host side of waveformer_amd.augment -- that tests/augment_ref.py reproduces the
committed fixture, the prefilter identities the kernels rest on, the sampler's distributions,
and the argument validation of every augmentation entry point (which runs before any HIP call)."""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as ref
from waveformer_amd import _lib
from waveformer_amd import augment as aug

FAKE = 256  # never dereferenced: validation fails first
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_fixtures.npz")


def test_restatement_reproduces_the_fixture():
    pytest.importorskip("scipy")
    fix = np.load(FIXTURE)
    out = ref.build_fixtures()
    assert sorted(out) == sorted(fix.files)
    for k, v in out.items():
        assert fix[k].shape == np.shape(v) and fix[k].dtype == np.asarray(v).dtype, k
        if np.asarray(v).dtype.kind == "f":
            # the same scipy gives the same bits; another build may round the last place
            np.testing.assert_allclose(fix[k], v, rtol=1e-12, atol=1e-13, err_msg=k)
        else:
            assert np.array_equal(fix[k], v), k


def test_fixture_parameters_keep_the_seg_ties_under_the_cap():
    """The GPU test lets the segmentation differ only inside the recorded tie mask, on at most
    0.5 % of a case's voxels: the mask itself is under that cap in every case."""
    fix = np.load(FIXTURE)
    keys = [k for k in fix.files if k.endswith("_tie")]
    assert len(keys) == len(ref.SPATIAL_CASES) + 1
    for k in keys:
        n = fix[k[:-4] + "_seg"].size
        ties = int(np.unpackbits(fix[k])[:n].sum())
        assert ties <= 0.005 * n, (k, ties, n)
    # every label survives somewhere, the single label of 200 included
    assert set(np.unique(fix["sp_ext07_seg"])) == {-1, 0, 1, 2, 3}
    assert set(np.unique(fix["sp_seg200_seg"])) == {0, 200}
    assert -1 not in fix["wh_seg"]


def test_quarter_turn_coordinates_are_on_the_grid():
    """The rot90 case: cos(pi / 2) = 6e-17 moves a coordinate by at most one place of its
    rounding (8.9e-16 below 8), and never across a border of the volume: the sum of a border
    coordinate and the perturbation rounds to the border or to its inner neighbour, whatever
    order the products are added in.  So the inside test is decided alike by the restatement
    and by the kernel's own arithmetic, and the points that leave leave by a whole voxel."""
    _, seg, patch, angles, scale = ref.spatial_case("rot90")
    coords = ref.spatial_coords(patch, seg.shape, angles, scale)
    m = aug.affine_matrix(angles, scale, seg.shape)
    mesh = np.stack(np.meshgrid(*[np.arange(n) - (n - 1) / 2.0 for n in patch], indexing="ij"))
    mine = ((mesh[0] * m[:, 0].reshape(3, 1, 1, 1) + mesh[1] * m[:, 1].reshape(3, 1, 1, 1))
            + mesh[2] * m[:, 2].reshape(3, 1, 1, 1)) + m[:, 3].reshape(3, 1, 1, 1)
    for c in (coords, mine):
        assert np.abs(c - np.round(c)).max() <= 9e-16
        for d in range(3):
            inside = (c[d] >= 0) & (c[d] <= seg.shape[d] - 1)
            assert np.array_equal(inside, (np.round(c[d]) >= 0) & (np.round(c[d]) <= seg.shape[d] - 1))
    assert np.array_equal(np.round(mine), np.round(coords))
    assert (coords[1] < 0).any() and (coords[1] > seg.shape[1] - 1).any()  # one axis leaves


@pytest.mark.parametrize("angles,scale", [((0.3, -0.2, 0.25), 1.15), ((ref.A30,) * 3, 0.7),
                                          (None, 1.4), ((0.1, 0.0, 0.0), None)])
def test_affine_matrix_gives_the_restatements_coordinates(angles, scale):
    patch, shape = (5, 6, 7), (9, 8, 11)
    coords = ref.spatial_coords(patch, shape, angles, scale)
    m = aug.affine_matrix(angles, scale, shape)
    mesh = np.stack(np.meshgrid(*[np.arange(n) - (n - 1) / 2.0 for n in patch], indexing="ij"))
    mine = np.einsum("ji,i...->j...", m[:, :3], mesh) + m[:, 3].reshape(3, 1, 1, 1)
    np.testing.assert_allclose(mine, coords, rtol=0, atol=1e-13)


def test_prefilter_identities():
    """What the kernels rest on: map_coordinates(mode='constant') is spline_filter(mode='mirror')
    followed by prefilter=False, bitwise; zoom(order=3, mode='nearest', grid_mode=True) is edge
    padding by 12, the mirror prefilter and sampling at (o + 0.5) in / out - 0.5 + 12; and the
    recursion equals its impulse response sqrt(3) pole^|k| cut after 18 taps to 1e-9."""
    ndi = pytest.importorskip("scipy.ndimage")
    x = ref.volume("a")[0].astype(float)
    coords = ref.spatial_coords(x.shape, x.shape, (0.3, -0.2, 0.25), 1.1)
    a = ndi.map_coordinates(x, coords, order=3, mode="constant", cval=0.0)
    b = ndi.map_coordinates(ndi.spline_filter(x, order=3, mode="mirror"), coords, order=3,
                            mode="constant", cval=0.0, prefilter=False)
    assert np.array_equal(a, b)

    low = ref.edge_input("a")[0].astype(float)
    out_shape = x.shape
    want = ndi.zoom(low, np.array(out_shape) / np.array(low.shape), order=3, mode="nearest",
                    grid_mode=True)
    coef = ndi.spline_filter(np.pad(low, ref.PAD, mode="edge"), order=3, mode="mirror")
    grid = np.meshgrid(*[(np.arange(o) + 0.5) * (n / o) - 0.5 + ref.PAD
                         for n, o in zip(low.shape, out_shape)], indexing="ij")
    got = ndi.map_coordinates(coef, np.array(grid), order=3, mode="mirror", prefilter=False)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)

    for name in ref.PREFILTER_MIRROR:
        for axis in range(3):
            v = ref.volume(name)[:1]
            np.testing.assert_allclose(ref.spline_fir_axis(v, 1 + axis, "mirror"),
                                       ref.spline_filter_axis(v, 1 + axis, "mirror"),
                                       rtol=0, atol=1e-9)
            e = ref.edge_input(name)
            np.testing.assert_allclose(ref.spline_fir_axis(e, 1 + axis, "edge"),
                                       ref.spline_filter_axis(e, 1 + axis, "edge"),
                                       rtol=0, atol=1e-9)
    # an axis of length 1 is left alone
    one = ref.volume("c")[:1]
    assert np.array_equal(ref.spline_filter_axis(one, 1, "mirror"), one.astype(float))
    assert abs(ref.POLE) ** 16 < 2.0 ** -30


def test_edge_input_is_scipys_nearest_reduction():
    pytest.importorskip("scipy")
    for name, zoom in ref.PREFILTER_EDGE.items():
        x = ref.volume(name)[0]
        target = np.round(np.array(x.shape) * zoom).astype(int)
        assert np.array_equal(ref.edge_input(name)[0], ref.zoom_nearest(x, target))


def test_gaussian_weights_are_scipys():
    pytest.importorskip("scipy")
    from scipy.ndimage import _filters
    from waveformer_amd import ops
    for sigma in (0.5, 0.73, 1.0):
        radius = int(4.0 * sigma + 0.5)
        want = _filters._gaussian_kernel1d(sigma, 0, radius)[radius:]
        np.testing.assert_allclose(ops.gaussian_weights(sigma), want, rtol=1e-15)
        np.testing.assert_allclose(ref.gaussian_weights(sigma), want, rtol=1e-15)
    assert len(ops.gaussian_weights(0.5)) == 3 and len(ops.gaussian_weights(1.0)) == 5


def _within(k, n, p):
    return abs(k - n * p) <= 4.0 * np.sqrt(n * p * (1 - p))


def test_sampler_distributions():
    """20 000 samples of 2 channels: every realised probability within 4 binomial standard
    deviations of its nominal value, every drawn value inside its range."""
    n, C = 20000, 2
    p = aug.sample_train_params(n, C, np.random.RandomState(2024), mirror_axes=(0, 2))
    for flag, prob in (("do_rotate", aug.P_ROTATE), ("do_scale", aug.P_SCALE),
                       ("noise", aug.P_NOISE), ("brightness", aug.P_BRIGHTNESS),
                       ("contrast", aug.P_CONTRAST), ("gamma_inv", aug.P_GAMMA_INV),
                       ("gamma", aug.P_GAMMA)):
        assert _within(getattr(p, flag).sum(), n, prob), flag
    for flag, ps, pc in (("blur", aug.P_BLUR, aug.P_BLUR_CHANNEL),
                         ("lowres", aug.P_LOWRES, aug.P_LOWRES_CHANNEL)):
        f = getattr(p, flag)
        assert _within(f.sum(), n * C, ps * pc), flag
        # the per-sample gate: a sample has a drawn channel with probability ps (1 - (1 - pc)^C)
        assert _within(f.any(axis=1).sum(), n, ps * (1 - (1 - pc) ** C)), flag
    assert _within(p.mirror[:, 0].sum(), n, 0.5) and _within(p.mirror[:, 2].sum(), n, 0.5)
    assert not p.mirror[:, 1].any()

    def inside(values, flags, lo, hi):
        v = values[flags]
        return v.size > 0 and (v >= lo).all() and (v <= hi).all()

    assert inside(p.angles, p.do_rotate, -aug.ANGLE, aug.ANGLE)
    assert abs(aug.ANGLE - np.pi / 6) < 1e-15
    assert inside(p.scale, p.do_scale, 0.7, 1.4)
    assert inside(p.noise_variance, p.noise, 0.0, 0.1)
    assert inside(p.blur_sigma, p.blur, 0.5, 1.0)
    assert inside(p.brightness_mult, p.brightness, 0.75, 1.25)
    assert inside(p.contrast_factor, p.contrast, 0.75, 1.25)
    assert inside(p.lowres_zoom, p.lowres, 0.5, 1.0)
    assert inside(p.gamma_inv_gamma, p.gamma_inv, 0.7, 1.5)
    assert inside(p.gamma_gamma, p.gamma, 0.7, 1.5)
    # the coin of the two-sided ranges: half below 1, half above
    for values, flags in ((p.scale, p.do_scale), (p.contrast_factor, p.contrast),
                          (p.gamma_gamma, p.gamma)):
        v = values[flags]
        assert _within((v < 1).sum(), v.size, 0.5)
    # one scale for all axes, one angle per axis
    assert p.scale.shape == (n,) and p.angles.shape == (n, 3)
    # what is not drawn stays neutral
    assert (p.scale[~p.do_scale] == 1).all() and (p.angles[~p.do_rotate] == 0).all()


def test_sampler_variants_and_determinism():
    a = aug.sample_train_params(64, 4, np.random.RandomState(1))
    b = aug.sample_train_params(64, 4, np.random.RandomState(1))
    for f in aug.dataclasses.fields(a):
        assert np.array_equal(getattr(a, f.name), getattr(b, f.name)), f.name
    only_sp = aug.sample_train_params(400, 2, np.random.RandomState(1), intensity=False)
    assert not (only_sp.noise.any() or only_sp.blur.any() or only_sp.gamma.any()
                or only_sp.lowres.any() or only_sp.contrast.any() or only_sp.brightness.any())
    assert only_sp.do_rotate.any() and only_sp.mirror.any()
    none = aug.sample_train_params(400, 2, np.random.RandomState(1), mirror_axes=None,
                                   spatial=False, intensity=False)
    ref_none = aug.no_params(400, 2)
    for f in aug.dataclasses.fields(none):
        assert np.array_equal(getattr(none, f.name), getattr(ref_none, f.name)), f.name
    assert aug.get_train_transforms_nomirror((8, 8, 8), (0, 1, 2)).mirror_axes == ()
    assert aug.get_train_transforms_onlymirror((8, 8, 8), (0, 1)).spatial is False
    assert aug.get_train_transforms_onlyspatial((8, 8, 8)).intensity is False
    t = aug.get_train_transforms_noaug((8, 8, 8), (0,))
    assert (t.spatial, t.intensity, t.mirror_axes, t.patch_size) == (False, False, (), None)
    assert aug.get_train_transforms((8, 9, 10), (0, 1, 2)).patch_size == (8, 9, 10)
    with pytest.raises(ValueError, match="mirror_axes"):
        aug.sample_train_params(1, 1, np.random.RandomState(0), mirror_axes=(3,))


def test_apply_validates_on_the_host():
    data = torch.zeros((2, 3, 8, 9, 10))
    seg = torch.zeros((2, 1, 8, 9, 10))
    p = aug.no_params(2, 3)
    with pytest.raises(ValueError, match="fp32"):
        aug.apply_train_transforms(data.double(), seg, p)
    with pytest.raises(ValueError, match="seg: expected"):
        aug.apply_train_transforms(data, seg[:, :, :4], p)
    with pytest.raises(ValueError, match="params are for"):
        aug.apply_train_transforms(data, seg, aug.no_params(2, 4))
    with pytest.raises(ValueError, match="exceeds"):
        aug.apply_train_transforms(data, seg, p, patch_size=(8, 9, 11))
    with pytest.raises(ValueError, match="noise: expected"):
        aug.apply_train_transforms(data, seg, p, noise=torch.zeros((2, 3, 8, 9, 9)))
    bad = aug.no_params(2, 3)
    bad.blur_sigma[0, 0] = 0.0
    with pytest.raises(ValueError, match="blur_sigma"):
        aug.apply_train_transforms(data, seg, bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        aug.apply_train_transforms(data, seg, p)


def test_entry_points_validate_before_any_hip_call():
    w = (_lib.ctypes.c_float * 3)(0.5, 0.2, 0.05)
    m = (_lib.ctypes.c_double * 12)(*([0.0] * 12))
    inf = (_lib.ctypes.c_double * 12)(*([float("inf")] * 12))
    cases = [
        ("empty volume", "wf_spline_prefilter_axis", (FAKE, FAKE + 256, 1, 4, 0, 4, 0, 0, None)),
        ("axis", "wf_spline_prefilter_axis", (FAKE, FAKE + 256, 1, 4, 4, 4, 3, 0, None)),
        ("mode", "wf_spline_prefilter_axis", (FAKE, FAKE + 256, 1, 4, 4, 4, 0, 2, None)),
        ("2\\^31", "wf_spline_prefilter_axis", (FAKE, FAKE + 256, 1, 2048, 2048, 512, 0, 0, None)),
        ("in is NULL", "wf_spline_prefilter_axis", (None, FAKE, 1, 4, 4, 4, 0, 0, None)),
        ("different buffers", "wf_spline_prefilter_axis", (FAKE, FAKE, 1, 4, 4, 4, 0, 0, None)),
        ("radius", "wf_gauss_blur_axis", (FAKE, FAKE + 256, 1, 4, 4, 4, 0, w, 21, None)),
        ("weights is NULL", "wf_gauss_blur_axis", (FAKE, FAKE + 256, 1, 4, 4, 4, 0, None, 2, None)),
        ("different buffers", "wf_gauss_blur_axis", (FAKE, FAKE, 1, 4, 4, 4, 0, w, 2, None)),
        ("both NULL", "wf_affine_sample", (None, None, m, 1, 4, 4, 4, 4, 4, 4, None, None, None)),
        ("channels", "wf_affine_sample", (FAKE, None, m, 65, 4, 4, 4, 4, 4, 4, FAKE, None, None)),
        ("matrix is NULL", "wf_affine_sample", (FAKE, None, None, 1, 4, 4, 4, 4, 4, 4, FAKE, None,
                                                None)),
        ("finite", "wf_affine_sample", (FAKE, None, inf, 1, 4, 4, 4, 4, 4, 4, FAKE, None, None)),
        ("out is NULL", "wf_affine_sample", (FAKE, None, m, 1, 4, 4, 4, 4, 4, 4, None, None, None)),
        ("out_seg is NULL", "wf_affine_sample", (None, FAKE, m, 1, 4, 4, 4, 4, 4, 4, None, None,
                                                 None)),
        ("empty volume", "wf_zoom_nearest", (FAKE, 1, 4, 4, 4, 4, 0, 4, FAKE, None)),
        ("out is NULL", "wf_zoom_nearest", (FAKE, 1, 4, 4, 4, 2, 2, 2, None, None)),
        ("coef is NULL", "wf_zoom_cubic", (None, 1, 4, 4, 4, 8, 8, 8, FAKE, None)),
        ("unknown op", "wf_augment_pointwise", (FAKE, 1, 64, 5, FAKE, None, None, None, None, 0,
                                                None)),
        ("nothing to do", "wf_augment_pointwise", (FAKE, 1, 64, 0, None, None, None, None, None, 0,
                                                   None)),
        ("params is NULL", "wf_augment_pointwise", (FAKE, 1, 64, 1, None, None, None, None, None,
                                                    0, None)),
        ("stats_a is NULL", "wf_augment_pointwise", (FAKE, 1, 64, 2, FAKE, None, None, None, None,
                                                     0, None)),
        ("stats_b is NULL", "wf_augment_pointwise", (FAKE, 1, 64, 4, FAKE, FAKE, None, None, None,
                                                     0, None)),
        ("workspace smaller", "wf_augment_pointwise", (FAKE, 1, 64, 1, FAKE, None, None, FAKE,
                                                       FAKE, 8, None)),
        ("aligned", "wf_augment_pointwise", (FAKE, 1, 64, 1, FAKE, None, None, FAKE, FAKE + 4,
                                             1 << 20, None)),
        ("must not be an input", "wf_augment_pointwise", (FAKE, 1, 64, 2, FAKE, FAKE + 512, None,
                                                          FAKE + 512, FAKE, 1 << 20, None)),
        ("stats is NULL", "wf_channel_stats", (FAKE, 1, 64, None, FAKE, 1 << 20, None)),
        ("planes", "wf_channel_stats", (FAKE, 0, 64, FAKE, FAKE, 1 << 20, None)),
    ]
    for match, name, args in cases:
        with pytest.raises(RuntimeError, match=match):
            _lib.call(name, *args)
    assert _lib.query("wf_augment_pointwise_workspace_bytes", 0, 64) == -1
    # 16 planes of 128^3: 256 partials of 6 doubles per plane
    assert _lib.query("wf_augment_pointwise_workspace_bytes", 16, 128 ** 3) == 16 * 256 * 6 * 8
