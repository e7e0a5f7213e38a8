"""CPU: the host side of waveformer_amd.preprocessing -- shape arithmetic, the rank draws
against numpy's RandomState.choice on arrays, the properties' form, the argument validation of
every preprocessing entry point (which runs before any HIP call), and that the committed hole-fill
fixture is what scipy gives."""
import numpy as np
import pytest

from tests import preprocess_ref as ref
from waveformer_amd import _lib
from waveformer_amd import preprocessing as pp

FAKE = 256  # never dereferenced: validation fails first


def test_compute_new_shape_rounds_like_python():
    assert pp.compute_new_shape((155, 240, 240), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)).tolist() == \
        [155, 240, 240]
    # 2.5 -> 2 and 3.5 -> 4: Python's round is half to even, unlike floor(x + 0.5)
    assert pp.compute_new_shape((5, 7, 9), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)).tolist() == [2, 4, 4]
    assert pp.compute_new_shape((10, 11, 12), (1.0, 0.5, 2.0), (1.0, 1.0, 1.0)).tolist() == \
        [10, 6, 24]
    got = pp.compute_new_shape((33, 47, 21), (0.7, 1.3, 2.0), (1.0, 1.0, 1.5))
    assert np.array_equal(got, ref.compute_new_shape((33, 47, 21), (0.7, 1.3, 2.0), (1.0, 1.0, 1.5)))
    with pytest.raises(ValueError):
        pp.compute_new_shape((1, 2), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))


def test_target_num_samples():
    assert pp.target_num_samples(17) == 17
    assert pp.target_num_samples(10000) == 10000
    assert pp.target_num_samples(500000) == 10000
    assert pp.target_num_samples(1000001) == 10001
    assert pp.target_num_samples(128 * 128 * 64) == 10486


def test_location_ranks_reproduce_choice_on_arrays():
    # a (1, 12, 40, 50) seg with a small class, a class above 10000 voxels and an absent one
    rs = np.random.RandomState(3)
    seg = rs.choice([0, 1, 2], size=(1, 12, 40, 50), p=[0.3, 0.1, 0.6]).astype(np.int16)
    classes = [1, 3, 2]
    want = ref.sample_foreground_locations(seg, classes)
    counts = [int((seg == c).sum()) for c in classes]
    assert counts[0] < 10000 < counts[2] and counts[1] == 0
    ranks = pp.draw_location_ranks(counts)
    assert ranks[1] is None and want[3] == []
    for c, r in zip(classes, ranks):
        if r is not None:
            assert r.dtype == np.int64
            assert np.array_equal(np.argwhere(seg == c)[r], want[c])


def test_intensity_ranks_reproduce_choice_on_arrays():
    rs = np.random.RandomState(4)
    seg = (rs.random_sample((1, 9, 10, 11)) < 0.3).astype(np.int16)
    images = rs.standard_normal((3, 9, 10, 11)).astype(np.float32)
    want = ref.collect_foreground_intensities(seg, images)
    fg = seg[0] > 0
    ranks = pp.draw_intensity_ranks(int(fg.sum()), 3)
    for i in range(3):
        assert np.array_equal(images[i][fg][ranks[i]], want[i])
    assert pp.draw_intensity_ranks(0, 2) == [None, None]


def test_bbox_form_and_property_keys():
    # half-open pairs, the form Predictor.predict_noncrop_probability slices with
    assert pp.bbox_from_device([1, 5, 2, 6, 3, 7, 64, 0]) == [[1, 5], [2, 6], [3, 7]]
    with pytest.raises(ValueError, match="empty"):
        pp.bbox_from_device([0, 0, 0, 0, 0, 0, 0, 0])
    for k in ("shape_before_cropping", "bbox_used_for_cropping",
              "shape_after_cropping_before_resample", "original_spacing_trans",
              "target_spacing_trans", "shape_after_resample", "class_locations"):
        assert k in pp.PROPERTY_KEYS
    m = np.zeros((6, 7, 8), dtype=bool)
    m[2:4, 1:6, 5:8] = True
    assert ref.bbox_from_mask(m) == [[2, 4], [1, 6], [5, 8]]


def test_file_io_is_refused():
    p = pp.MultiModalityPreprocessor("base", "images", ["t1.nii.gz"], "seg.nii.gz")
    assert p.out_spacing == [1.0, 1.0, 1.0] and p.all_labels == [1, 2, 3]
    for call in (lambda: p.read_data("case"), lambda: p.run([1, 1, 1], "out", [1, 2, 3]),
                 lambda: p.run_plan()):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match="regions"):
        pp.sample_foreground_locations(np.zeros((1, 2, 2, 2), dtype=np.int16), [(1, 2)])


def _box(*v):
    import ctypes
    return (ctypes.c_int64 * 6)(*v)


def test_entry_points_validate_before_any_hip_call():
    box = _box(0, 2, 0, 2, 0, 2)
    q = _lib.query
    assert q("wf_fill_holes_workspace_bytes", 4, 4, 4) >= 64 + 32
    assert q("wf_fill_holes_workspace_bytes", 0, 4, 4) == -1
    assert q("wf_box_moments_workspace_bytes", 4, 155, 240, 240) >= 4 * 2 * 8
    assert q("wf_box_moments_workspace_bytes", 0, 4, 4, 4) == -1
    assert q("wf_select_workspace_bytes", 2048) >= 3 * 8 + 2 * 4
    assert q("wf_select_workspace_bytes", 0) == -1
    bad = [
        ("channels", "wf_nonzero_mask", (FAKE, 0, 4, 4, 4, FAKE, None)),
        ("empty volume", "wf_nonzero_mask", (FAKE, 1, 4, 0, 4, FAKE, None)),
        ("2\\^31", "wf_nonzero_mask", (FAKE, 1, 2048, 2048, 512, FAKE, None)),
        ("data is NULL", "wf_nonzero_mask", (None, 1, 4, 4, 4, FAKE, None)),
        ("mask is NULL", "wf_nonzero_mask", (FAKE, 1, 4, 4, 4, None, None)),
        ("empty volume", "wf_fill_holes", (FAKE, 4, 4, 0, FAKE, FAKE, FAKE, 256, None, None)),
        ("mask is NULL", "wf_fill_holes", (None, 4, 4, 4, FAKE, FAKE, FAKE, 256, None, None)),
        ("filled is NULL", "wf_fill_holes", (FAKE, 4, 4, 4, None, FAKE, FAKE, 256, None, None)),
        ("bbox is NULL", "wf_fill_holes", (FAKE, 4, 4, 4, FAKE, None, FAKE, 256, None, None)),
        ("workspace is NULL", "wf_fill_holes", (FAKE, 4, 4, 4, FAKE, FAKE, None, 256, None, None)),
        ("workspace smaller", "wf_fill_holes", (FAKE, 4, 4, 4, FAKE, FAKE, FAKE, 8, None, None)),
        ("aligned", "wf_fill_holes", (FAKE, 4, 4, 4, FAKE, FAKE, FAKE + 4, 256, None, None)),
        ("channels", "wf_box_moments", (FAKE, 65, 4, 4, 4, box, FAKE, FAKE, 1 << 20, None)),
        ("box is NULL", "wf_box_moments", (FAKE, 1, 4, 4, 4, None, FAKE, FAKE, 1 << 20, None)),
        ("half-open", "wf_box_moments", (FAKE, 1, 4, 4, 4, _box(0, 5, 0, 2, 0, 2), FAKE, FAKE,
                                         1 << 20, None)),
        ("half-open", "wf_box_moments", (FAKE, 1, 4, 4, 4, _box(2, 2, 0, 2, 0, 2), FAKE, FAKE,
                                         1 << 20, None)),
        ("stats is NULL", "wf_box_moments", (FAKE, 1, 4, 4, 4, box, None, FAKE, 1 << 20, None)),
        ("workspace smaller", "wf_box_moments", (FAKE, 1, 4, 4, 4, box, FAKE, FAKE, 8, None)),
        ("half-open", "wf_crop_normalize", (FAKE, 1, 4, 4, 4, _box(0, 2, -1, 2, 0, 2), None, FAKE,
                                            None)),
        ("out is NULL", "wf_crop_normalize", (FAKE, 1, 4, 4, 4, box, None, None, None)),
        ("in place", "wf_crop_normalize", (FAKE, 1, 4, 4, 4, box, None, FAKE, None)),
        ("filled is NULL", "wf_crop_seg", (None, None, 4, 4, 4, box, -1, FAKE, FAKE, None)),
        ("maxv is NULL", "wf_crop_seg", (None, FAKE, 4, 4, 4, box, -1, FAKE, None, None)),
        ("int16", "wf_crop_seg", (None, FAKE, 4, 4, 4, box, 40000, FAKE, FAKE, None)),
        ("mode", "wf_select_scan", (FAKE, 64, 2, 0, FAKE, 1 << 20, FAKE, None)),
        ("labels is NULL", "wf_select_scan", (None, 64, 0, 0, FAKE, 1 << 20, FAKE, None)),
        ("total is NULL", "wf_select_scan", (FAKE, 64, 0, 0, FAKE, 1 << 20, None, None)),
        ("workspace smaller", "wf_select_scan", (FAKE, 64, 0, 0, FAKE, 8, FAKE, None)),
        ("both NULL", "wf_select_pick", (FAKE, 4, 4, 4, 0, 1, FAKE, 1 << 20, FAKE, 3, None, None,
                                         None, None)),
        ("image is NULL", "wf_select_pick", (FAKE, 4, 4, 4, 0, 1, FAKE, 1 << 20, FAKE, 3, None,
                                             None, FAKE, None)),
        ("ranks is NULL", "wf_select_pick", (FAKE, 4, 4, 4, 0, 1, FAKE, 1 << 20, None, 3, FAKE,
                                             None, None, None)),
        ("nq", "wf_select_pick", (FAKE, 4, 4, 4, 0, 1, FAKE, 1 << 20, FAKE, 0, FAKE, None, None,
                                  None)),
    ]
    for match, name, args in bad:
        with pytest.raises(RuntimeError, match=match):
            _lib.call(name, *args)


def test_fill_cases_are_what_they_claim():
    """The constructed cases against the recorded scipy result: which cavities scipy fills."""
    f = {n: ref.filled_reference(n) for n in ref.CONSTRUCTED}
    m = {n: ref.fill_case(n) for n in ref.CONSTRUCTED}
    assert f["shell"][2:7, 2:7, 2:7].all() and not m["shell"][4, 4, 4]
    assert np.array_equal(f["tunnel"], m["tunnel"]) and not f["tunnel"][4, 4, 4]
    assert f["edge_diagonal"][4, 4, 4] and not f["edge_diagonal"][4, 5, 5]
    assert np.array_equal(f["cup"], m["cup"]) and not f["cup"][2, 4, 4]
    assert np.array_equal(f["serpentine"], m["serpentine"])
    assert int((~m["serpentine"]).sum()) > 500  # far longer than any line of 9 x 9 x 33
    assert not f["empty"].any() and f["full"].all()


def test_committed_fixture_is_what_scipy_gives():
    pytest.importorskip("scipy")
    want = ref.build_fixtures()
    have = ref.fixtures()
    assert sorted(want) == sorted(have)
    for k in want:
        assert np.array_equal(np.asarray(want[k]), have[k]), k
