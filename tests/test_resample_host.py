"""CPU: the host side of the resampling step -- waveformer_amd.resampling's decision helpers
against hand-written values and the restatement, compute_new_shape, the unsupported options, the
committed fixture against scipy where scipy is importable, and the segment arithmetic of
wf_spline_zoom_axis (csrc/zoom_plan.hpp through wf_spline_zoom_axis_plan) by brute force."""
import math

import numpy as np
import pytest

from tests import resample_ref as ref
from waveformer_amd import _lib, ops
from waveformer_amd import preprocessing as pp
from waveformer_amd import resampling as rs

FAKE = 256  # never dereferenced: validation fails first


# ------------------------------------------------------------------------------------------
# decision helpers
# ------------------------------------------------------------------------------------------
def test_thresholds():
    assert rs.ANISO_THRESHOLD == 3
    assert rs.get_do_separate_z((1.0, 1.0, 3.0)) is False       # the ratio must exceed 3
    assert rs.get_do_separate_z((1.0, 1.0, 3.01)) is True
    assert rs.get_do_separate_z((0.5, 1.0, 1.4)) is False
    assert rs.get_do_separate_z((1.0, 1.0, 2.5), anisotropy_threshold=2) is True
    assert rs.get_lowres_axis((1.0, 1.0, 5.0)).tolist() == [2]
    assert rs.get_lowres_axis((5.0, 1.0, 1.0)).tolist() == [0]
    assert rs.get_lowres_axis((0.24, 1.25, 1.25)).tolist() == [1, 2]
    assert rs.get_lowres_axis((1.0, 1.0, 1.0)).tolist() == [0, 1, 2]


@pytest.mark.parametrize("cur, new, force, want", [
    # force_separate_z False: never, and no axis
    ((1.0, 1.0, 5.0), (1.0, 1.0, 1.0), False, (False, None)),
    ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), False, (False, None)),
    # True: the low-resolution axes of the CURRENT spacing; two or three of them switch it off
    ((1.0, 1.0, 5.0), (1.0, 1.0, 1.0), True, (True, [2])),
    ((1.0, 1.0, 1.2), (1.0, 1.0, 1.0), True, (True, [2])),
    ((0.24, 1.25, 1.25), (1.0, 1.0, 1.0), True, (False, [1, 2])),
    ((1.0, 1.0, 1.0), (1.0, 1.0, 5.0), True, (False, [0, 1, 2])),
    # None: decided by the anisotropy of the current spacing, then of the new one
    ((1.0, 1.0, 5.0), (1.0, 1.0, 1.0), None, (True, [2])),
    ((1.0, 1.0, 1.0), (1.0, 4.0, 1.0), None, (True, [1])),
    ((1.0, 1.0, 2.0), (1.0, 1.0, 1.0), None, (False, None)),
    ((0.24, 1.25, 1.25), (1.0, 1.0, 1.0), None, (False, [1, 2])),
    ((1.0, 1.0, 1.0), (0.2, 1.0, 1.0), None, (False, [1, 2])),
])
def test_decide_separate_z(cur, new, force, want):
    for fn in (rs.decide_separate_z, ref.decide_separate_z):
        do, axis = fn(cur, new, force)
        assert bool(do) is want[0]
        assert (axis is None) if want[1] is None else (list(axis) == want[1])


def test_compute_new_shape_rounds_half_to_even():
    assert rs.compute_new_shape((10, 10, 10), (1, 1, 1), (1, 1, 1)).tolist() == [10, 10, 10]
    assert rs.compute_new_shape((5, 7, 9), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)).tolist() == [2, 4, 4]
    assert rs.compute_new_shape((12, 15, 13), (2.0, 1.0, 1.0), (1.0, 1.5, 0.75)).tolist() == \
        list(ref.E2E_NEW_SHAPE)
    assert rs.compute_new_shape((155, 240, 240), (1, 1, 1), (1.5, 1.5, 1.5)).tolist() == \
        [103, 160, 160]
    assert pp.compute_new_shape is rs.compute_new_shape
    with pytest.raises(ValueError):
        rs.compute_new_shape((1, 2), (1, 1, 1), (1, 1, 1))
    rng = np.random.RandomState(0)
    for _ in range(50):
        shp, a, b = rng.randint(1, 300, 3), rng.uniform(0.3, 3, 3), rng.uniform(0.3, 3, 3)
        assert rs.compute_new_shape(shp, a, b).tolist() == ref.compute_new_shape(shp, a, b).tolist()


# ------------------------------------------------------------------------------------------
# unsupported options, checked before anything moves to a device
# ------------------------------------------------------------------------------------------
def test_unsupported_options_name_their_argument():
    x = np.zeros((1, 4, 5, 6), np.float32)
    s = np.zeros((1, 4, 5, 6), np.int16)
    with pytest.raises(NotImplementedError, match="do_separate_z"):
        rs.resample_data_or_seg(x, (5, 5, 5), do_separate_z=True, axis=[0])
    with pytest.raises(NotImplementedError, match="do_separate_z"):
        rs.resample_data_or_seg_to_shape(x, (5, 5, 5), (1, 1, 5), (1, 1, 1), force_separate_z=None)
    with pytest.raises(NotImplementedError, match="do_separate_z"):
        rs.resample_data_or_seg_to_spacing(x, (1, 1, 5), (1, 1, 1), force_separate_z=True)
    for order in (1, 2, 4, 5):
        with pytest.raises(NotImplementedError, match=f"order={order}"):
            rs.resample_data_or_seg(x, (5, 5, 5), order=order)
    for order in (2, 3):
        with pytest.raises(NotImplementedError, match=f"order={order}"):
            rs.resample_data_or_seg(s, (5, 5, 5), is_seg=True, order=order)
    with pytest.raises(ValueError):
        rs.resample_data_or_seg(x[0], (5, 5, 5))
    with pytest.raises(ValueError):
        rs.resample_data_or_seg(x, (5, 5))


def test_preprocessor_keeps_its_default():
    assert pp.MultiModalityPreprocessor().resample is False
    assert pp.MultiModalityPreprocessor(resample=True).resample is True


def test_entry_points_validate_before_any_hip_call():
    for match, name, args in [
        ("empty volume", "wf_spline_zoom_axis", (FAKE, FAKE + 64, 1, 4, 0, 4, 0, 4, None, None)),
        ("empty volume", "wf_spline_zoom_axis", (FAKE, FAKE + 64, 1, 4, 4, 4, 0, 0, None, None)),
        ("axis", "wf_spline_zoom_axis", (FAKE, FAKE + 64, 1, 4, 4, 4, 3, 4, None, None)),
        ("different buffers", "wf_spline_zoom_axis", (FAKE, FAKE, 1, 4, 4, 4, 0, 5, None, None)),
        ("in is NULL", "wf_spline_zoom_axis", (None, FAKE, 1, 4, 4, 4, 0, 5, None, None)),
        ("2\\^31", "wf_spline_zoom_axis", (FAKE, FAKE + 64, 1, 1024, 1024, 1024, 0, 4096, None,
                                         None)),
        ("seg is NULL", "wf_zoom_seg_linear", (None, 4, 4, 4, 2, 2, 2, FAKE, None)),
        ("empty volume", "wf_zoom_seg_linear", (FAKE, 4, 4, 4, 2, 0, 2, FAKE + 64, None)),
        ("different buffers", "wf_zoom_seg_linear", (FAKE, 4, 4, 4, 2, 2, 2, FAKE, None)),
    ]:
        with pytest.raises(RuntimeError, match=match):
            _lib.call(name, *args)
    assert _lib.query("wf_spline_zoom_axis_plan", 0, 4, 0, None) < 0
    assert _lib.query("wf_spline_zoom_axis_plan", 4, 1 << 31, 0, None) < 0


def test_new_exports_are_bound():
    for name in ("wf_spline_zoom_axis", "wf_spline_zoom_axis_plan", "wf_zoom_seg_linear"):
        assert name in _lib.SIGNATURES
    assert _lib.load().wf_abi_version() == _lib.ABI_VERSION >= 27


# ------------------------------------------------------------------------------------------
# the segment arithmetic
# ------------------------------------------------------------------------------------------
def _check_plan(n, on):
    """Every output lies in exactly one segment; every cubic tap of every output lies among the
    coefficients its segment stages, every prefilter tap of those among the staged samples, and
    both fit the staging."""
    segs = ops.spline_zoom_axis_plan(n, on)
    P = n + 2 * ref.PAD
    nxt = 0
    for s in segs:
        assert s["o0"] == nxt and s["o1"] > s["o0"], (n, on, s)
        nxt = s["o1"]
        assert s["jhi"] - s["jlo"] + 1 <= s["coef_cap"] == 60, (n, on, s)
        assert s["shi"] - s["slo"] + 1 <= s["samp_cap"] == 96, (n, on, s)
        assert 0 <= s["slo"] <= s["shi"] <= n - 1, (n, on, s)
        for o in range(s["o0"], s["o1"]):
            f = math.floor((o + 0.5) * (n / on) - 0.5 + ref.PAD)
            assert s["jlo"] <= f - 1 and f + 2 <= s["jhi"], (n, on, o, s)
            assert 0 <= f - 1 and f + 2 <= P - 1, (n, on, o)  # no tap leaves the padded line
        for j in (s["jlo"], s["jhi"]):  # the index map is monotone: the ends bound the rest
            for q in (j - 18, j + 18):
                m = q % (2 * (P - 1))
                m = m if m < P else 2 * (P - 1) - m
                src = min(max(m - ref.PAD, 0), n - 1)
                assert s["slo"] <= src <= s["shi"], (n, on, j, q, s)
    assert nxt == on
    return len(segs)


def test_plan_brute_force_small():
    for n in range(1, 41):
        for on in range(1, 41):
            _check_plan(n, on)


@pytest.mark.parametrize("n, on", [(300, 211), (211, 300), (240, 160), (240, 320), (155, 103),
                                   (1000, 7), (7, 1000), (4096, 4095), (1, 500), (500, 1),
                                   (100000, 99999)])
def test_plan_long_axes(n, on):
    nseg = _check_plan(n, on)
    if min(n, on) >= 200:
        assert nseg > 1


def test_plan_index_map_is_monotone():
    """What lets the two ends of a segment bound its samples: over the padded indices a
    segment's taps can reach, [-8, n + 31], the edge-padded index map never decreases."""
    for n in (1, 2, 3, 5, 17, 64):
        P = n + 2 * ref.PAD
        prev = 0
        for q in range(-8, n + 32):
            m = q % (2 * (P - 1))
            m = m if m < P else 2 * (P - 1) - m
            src = min(max(m - ref.PAD, 0), n - 1)
            assert src >= prev
            prev = src


# ------------------------------------------------------------------------------------------
# the restatement and the committed fixture
# ------------------------------------------------------------------------------------------
def test_inputs_are_what_they_claim():
    for name, (shape, new_shape, planes) in ref.CASES.items():
        x = ref.data_input(name)
        assert x.shape == (planes,) + shape and x.dtype == np.float32
        for c in range(planes):  # a flat background at the minimum
            assert (x[c] == x[c].min()).mean() > 0.3
        seg = ref.seg_input(name)
        assert seg.shape == shape and set(np.unique(seg)) <= {-1, 0, 1, 2, 3}
    x = ref.data_input("down")
    assert x[0].min() != x[1].min() and x[0].max() != x[1].max()


def test_fixture_holds_every_case():
    fx = ref.fixtures()
    for name, (shape, new_shape, planes) in list(ref.CASES.items()) + \
            [("e2e", (ref.E2E_CROPPED, ref.E2E_NEW_SHAPE, 2))]:
        assert fx[f"{name}_data"].shape == (planes,) + new_shape
        assert fx[f"{name}_raw"].shape == (planes,) + new_shape
        assert fx[f"{name}_cmax"].shape == (planes,)
        assert fx[f"{name}_seg"].shape == new_shape and fx[f"{name}_seg0"].shape == new_shape
        if name != ref.EXACT_SEG_CASE:
            tie = ref.unpack(fx[f"{name}_tie"], new_shape)
            assert tie.mean() <= ref.MAX_TIES
        clamped = (fx[f"{name}_data"] != fx[f"{name}_raw"]).mean(axis=(1, 2, 3))
        if name != "e2e":
            assert (clamped >= ref.MIN_CLAMPED).all(), (name, clamped)


def test_committed_fixture_is_what_scipy_gives():
    pytest.importorskip("scipy")
    fx = ref.fixtures()
    fresh = ref.build_fixtures()
    assert sorted(fresh) == sorted(fx)
    for k in fresh:
        if fresh[k].dtype.kind == "f":
            assert np.allclose(fresh[k], fx[k], rtol=0, atol=1e-12), k
        else:
            assert np.array_equal(fresh[k], fx[k]), k


def test_restatement_of_the_whole_function():
    pytest.importorskip("scipy")
    fx = ref.fixtures()
    x = ref.data_input("down")
    out = ref.resample_data_or_seg(x, ref.CASES["down"][1])
    assert out.dtype == np.float32 and np.array_equal(out, fx["down_data"].astype(np.float32))
    assert ref.resample_data_or_seg(x, x.shape[1:]) is x
    seg = ref.seg_input("down")[None]
    out = ref.resample_data_or_seg(seg, ref.CASES["down"][1], is_seg=True, order=1)
    assert out.dtype == np.int16 and np.array_equal(out[0], fx["down_seg"])
