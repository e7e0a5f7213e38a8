"""CPU: the host side of waveformer_amd.dataloading -- the draw against the reference's recorded
random stream (tests/golden/loader_fixtures.npz), get_bbox's corner cases, the per-axis segment
arithmetic of wf_crop_pad_batch (csrc/loader_plan.hpp through wf_crop_pad_axis_plan) against
three lines of Python, the entry's validation, and CaseStore's bookkeeping.  No GPU is touched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loader_ref as ref
from waveformer_amd import _lib, ops
from waveformer_amd import dataloading as dl

FAKE = 256  # never dereferenced: validation fails first


# ------------------------------------------------------------------------------------------
# the draw reproduces the reference's stream
# ------------------------------------------------------------------------------------------
def _draw_40(prob, rng):
    ds = ref.fixture_dataset()
    plans = [dl.draw_batch_plan(ds, ref.PATCH, ref.BATCH, 0.33, prob, rng) for _ in range(40)]
    return (np.stack([p.keys for p in plans]), np.stack([p.force_fg for p in plans]),
            np.stack([p.bbox_lbs for p in plans]))


@pytest.mark.parametrize("mode,prob", ref.MODES)
@pytest.mark.parametrize("stream", ["RandomState", "global"])
def test_draw_matches_the_reference_stream(mode, prob, stream):
    fx = ref.fixtures()
    if stream == "RandomState":
        keys, force, lbs = _draw_40(prob, np.random.RandomState(ref.SEED))
    else:
        state = np.random.get_state()
        try:
            np.random.seed(ref.SEED)
            keys, force, lbs = _draw_40(prob, None)
        finally:
            np.random.set_state(state)
    assert np.array_equal(keys, fx[f"{mode}_keys"])
    assert np.array_equal(force, fx[f"{mode}_force"])
    assert np.array_equal(lbs, fx[f"{mode}_lbs"])
    assert lbs.dtype == np.int64 and force.dtype == bool


@pytest.mark.parametrize("mode,prob", ref.MODES)
def test_loader_methods_draw_the_same_plan(mode, prob):
    # the class draws through the same function, with its own rng
    fx = ref.fixtures()
    loader = dl.DataLoaderMultiProcess(ref.fixture_dataset(), ref.PATCH, ref.BATCH, 0.33, prob,
                                       rng=np.random.RandomState(ref.SEED), device="cpu")
    assert loader.keys == [0, 1, 2, 3]
    assert loader.determine_shapes() == ((3, 2, 8, 8, 8), (3, 1, 8, 8, 8))
    for n in range(3):
        plan = loader.draw_batch_plan()
        assert np.array_equal(plan.keys, fx[f"{mode}_keys"][n])
        assert np.array_equal(plan.force_fg, fx[f"{mode}_force"][n])
        assert np.array_equal(plan.bbox_lbs, fx[f"{mode}_lbs"][n])


def test_the_fixture_reaches_every_clipping_branch():
    fx = ref.fixtures()
    shapes = np.array([fx[f"case{i}_data"].shape[1:] for i in range(4)])
    for mode, _ in ref.MODES:
        lbs = fx[f"{mode}_lbs"].reshape(-1, 3)
        ext = shapes[fx[f"{mode}_keys"].reshape(-1)]
        low, high = (lbs < 0).any(1), (lbs + 8 > ext).any(1)
        assert low.sum() >= 20 and high.sum() >= 20 and (low & high).sum() >= 5
        assert (lbs[:, 2] % 4 != 0).sum() >= 20 and (lbs[:, 2] % 4 == 0).sum() >= 20


# ------------------------------------------------------------------------------------------
# get_bbox on its own
# ------------------------------------------------------------------------------------------
class _Scripted:
    """A stream that returns what the test scripted and records the calls."""

    def __init__(self, choices=(), randints=()):
        self.choices, self.randints, self.calls = list(choices), list(randints), []

    def choice(self, n):
        self.calls.append(("choice", n))
        return self.choices.pop(0)

    def randint(self, lo, hi):
        self.calls.append(("randint", int(lo), int(hi)))
        return self.randints.pop(0)


def _loader(patch, rng):
    return dl.DataLoaderMultiProcess(ref.fixture_dataset(), patch, 3, rng=rng, device="cpu")


def test_oversample_last_third_rounds_to_even():
    for B, first_forced in ((2, 1), (3, 2), (4, 3), (5, 3), (7, 5), (1, 1)):
        loader = dl.DataLoaderMultiProcess(ref.fixture_dataset(), (8, 8, 8), B, device="cpu")
        flags = [loader._oversample_last_XX_percent(j) for j in range(B)]
        assert flags == [j >= first_forced for j in range(B)], (B, flags)
    # round(0.5) is 0 and round(2.5) is 2: to even, not half up
    loader = dl.DataLoaderMultiProcess(ref.fixture_dataset(), (8, 8, 8), 1,
                                       oversample_foreground_percent=0.5, device="cpu")
    assert loader._oversample_last_XX_percent(0) is True
    loader = dl.DataLoaderMultiProcess(ref.fixture_dataset(), (8, 8, 8), 5,
                                       oversample_foreground_percent=0.5, device="cpu")
    assert [loader._oversample_last_XX_percent(j) for j in range(5)] == [False, False, True, True,
                                                                         True]


def test_get_bbox_odd_need_to_pad_is_a_floor():
    # extent 5 under a patch of 8: need_to_pad 3, lbs = (-3) // 2 = -2, ubs = 5 + 1 + 1 - 8 = -1
    rng = _Scripted(randints=[0, -2, 3])
    lbs, ubs = _loader((8, 8, 8), rng).get_bbox((9, 5, 14), False, None)
    assert rng.calls == [("randint", 0, 2), ("randint", -2, 0), ("randint", 0, 7)]
    assert lbs == [0, -2, 3] and ubs == [8, 6, 11]
    # an even pad: extent 6 -> lbs -1, ubs 6 + 1 + 0 - 8 = -1: one position
    rng = _Scripted(randints=[-1, 0, 0])
    _loader((8, 8, 8), rng).get_bbox((6, 13, 10), False, None)
    assert rng.calls[0] == ("randint", -1, 0)


@pytest.mark.parametrize("voxel,want", [
    ((0, 0, 0, 0), [0, 0, 0]),          # clamped from below to lbs
    ((0, 10, 12, 8), [6, 8, 4]),        # the far corner: the box hangs over every upper edge
    ((0, 0, 12, 0), [0, 8, 0]),
    ((0, 10, 0, 8), [6, 0, 4]),
    ((0, 5, 6, 4), [1, 2, 0]),
])
def test_get_bbox_forced_voxel_is_clamped_below_only(voxel, want):
    loc = {1: np.zeros((0, 4), np.int64), 2: np.array([(0, 1, 1, 1), voxel], np.int64)}
    rng = _Scripted(choices=[0, 1])
    lbs, ubs = _loader((8, 8, 8), rng).get_bbox((11, 13, 9), True, loc)
    # one eligible class (the empty list is dropped), then the voxel among its two
    assert rng.calls == [("choice", 1), ("choice", 2)]
    assert [int(v) for v in lbs] == want
    assert [int(u) for u in ubs] == [w + 8 for w in want]


def test_get_bbox_forced_on_a_small_case_keeps_the_lower_pad():
    # extent 5, patch 8: voxel 0 - 4 = -4 is clamped to lbs = -2
    loc = {1: np.array([(0, 0, 0, 0)], np.int64)}
    lbs, _ = _loader((8, 8, 8), _Scripted(choices=[0, 0])).get_bbox((9, 5, 14), True, loc)
    assert [int(v) for v in lbs] == [0, -2, 0]


@pytest.mark.parametrize("loc", [{}, {1: np.zeros((0, 4), np.int64), 2: []}])
def test_get_bbox_without_foreground_falls_back_to_random(loc):
    rng = _Scripted(randints=[1, 2, 0])
    lbs, _ = _loader((8, 8, 8), rng).get_bbox((11, 13, 9), True, loc)
    assert rng.calls == [("randint", 0, 4), ("randint", 0, 6), ("randint", 0, 2)]
    assert lbs == [1, 2, 0]


def test_get_bbox_forced_needs_class_locations():
    with pytest.raises(AssertionError):
        _loader((8, 8, 8), _Scripted()).get_bbox((11, 13, 9), True, None)


# ------------------------------------------------------------------------------------------
# the segment arithmetic of one axis
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch,extent", [(8, 11), (8, 6), (5, 5), (1, 1)])
def test_axis_plan_against_python(patch, extent):
    for lb in range(-patch - 1, extent + 2):
        lo, hi = max(lb, 0), min(lb + patch, extent)
        n = max(hi - lo, 0)
        want = (lo - lb, lo, n) if n else (0, 0, 0)
        got = ops.crop_pad_axis_plan(lb, patch, extent)
        assert got == want == ref.axis_plan(lb, patch, extent), (lb, patch, extent, got, want)
        dst0, src0, n = got
        assert 0 <= dst0 and dst0 + n <= patch and 0 <= src0 and src0 + n <= extent


def test_axis_plan_far_outside_and_bad_sizes():
    assert ops.crop_pad_axis_plan(-(1 << 62), 8, 11) == (0, 0, 0)
    assert ops.crop_pad_axis_plan((1 << 62), 8, 11) == (0, 0, 0)
    assert ops.crop_pad_axis_plan(-7, 8, (1 << 31) - 1) == (7, 0, 1)
    buf = (ctypes.c_int64 * 3)()
    for lb, patch, extent in ((0, 0, 4), (0, 4, 0), (0, 1 << 31, 4), (0, 4, 1 << 31)):
        with pytest.raises(RuntimeError, match="patch, extent"):
            _lib.call("wf_crop_pad_axis_plan", lb, patch, extent, buf)
    with pytest.raises(RuntimeError, match="NULL"):
        _lib.call("wf_crop_pad_axis_plan", 0, 4, 4, None)


# ------------------------------------------------------------------------------------------
# validation before any HIP call
# ------------------------------------------------------------------------------------------
def _records(*rows):
    return (ctypes.c_int64 * (8 * len(rows)))(*[v for r in rows for v in r])


GOOD = (FAKE, FAKE, 4, 4, 4, 0, 0, 0)


def _call(records, B=1, C=1, S=1, kind=0, patch=(4, 4, 4), out=(FAKE, FAKE)):
    _lib.call("wf_crop_pad_batch", records, B, C, S, kind, *patch, out[0], out[1], None)


def test_new_exports_are_bound():
    for name in ("wf_crop_pad_batch", "wf_crop_pad_axis_plan"):
        assert name in _lib.SIGNATURES
    assert _lib.load().wf_abi_version() == _lib.ABI_VERSION >= 29


def test_crop_pad_batch_validates_on_the_host():
    with pytest.raises(RuntimeError, match="1 <= B"):
        _call(_records(GOOD), B=0)
    with pytest.raises(RuntimeError, match="C >= 1"):
        _call(_records(GOOD), C=0)
    with pytest.raises(RuntimeError, match="C >= 1"):
        _call(_records(GOOD), S=0)
    with pytest.raises(RuntimeError, match="4095"):
        _call(_records(GOOD), C=4000, S=96)
    for kind in (-1, 3):
        with pytest.raises(RuntimeError, match="seg_kind"):
            _call(_records(GOOD), kind=kind)
    for patch in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        with pytest.raises(RuntimeError, match="at least 1 voxel"):
            _call(_records(GOOD), patch=patch)
    for patch in ((2048, 1024, 1024), (1 << 31, 1, 1), (1 << 16, 1 << 16, 1)):
        with pytest.raises(RuntimeError, match=r"below 2\^31 voxels \(the outputs"):
            _call(_records(GOOD), patch=patch)
    with pytest.raises(RuntimeError, match="records is NULL"):
        _call(None)
    with pytest.raises(RuntimeError, match="out_data is NULL"):
        _call(_records(GOOD), out=(None, FAKE))
    with pytest.raises(RuntimeError, match="out_seg is NULL"):
        _call(_records(GOOD), out=(FAKE, None))
    for bad in ((0, FAKE, 4, 4, 4, 0, 0, 0), (FAKE, 0, 4, 4, 4, 0, 0, 0)):
        with pytest.raises(RuntimeError, match="record 1 has a NULL"):
            _call(_records(GOOD, bad), B=2)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, -2)):
        with pytest.raises(RuntimeError, match="record 0 has an extent below 1"):
            _call(_records((FAKE, FAKE) + dims + (0, 0, 0)))
    with pytest.raises(RuntimeError, match=r"record 0: D\*H\*W"):
        _call(_records((FAKE, FAKE, 2048, 1024, 1024, 0, 0, 0)))
    # the error is the library's thread-local message
    assert b"wf_crop_pad_batch" in _lib.load().wf_last_error()


def test_ops_wrapper_refuses_bad_inputs_before_the_library():
    d, s = torch.zeros((2, 4, 4, 4)), torch.zeros((1, 4, 4, 4), dtype=torch.int8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.crop_pad_batch([(d, s)], [(0, 0, 0)], (4, 4, 4))
    with pytest.raises(ValueError, match="empty batch"):
        ops.crop_pad_batch([], [], (4, 4, 4))
    with pytest.raises(ValueError, match="lower corners"):
        ops.crop_pad_batch([(d, s)], [(0, 0)], (4, 4, 4))
    with pytest.raises(ValueError, match="three positive sizes"):
        ops.crop_pad_batch([(d, s)], [(0, 0, 0)], (4, 4))
    with pytest.raises(TypeError, match="int8, int16 or float32"):
        ops.crop_pad_batch([(d, s.to(torch.int32))], [(0, 0, 0)], (4, 4, 4))


# ------------------------------------------------------------------------------------------
# CaseStore
# ------------------------------------------------------------------------------------------
def _nbytes(item):
    return item["data"].nbytes + item["seg"].nbytes


def test_case_store_keeps_everything_on_the_host_with_no_device_budget():
    ds = ref.fixture_dataset()
    store = dl.CaseStore(device_bytes=0)
    for i, item in enumerate(ds):
        assert store.fits(_nbytes(item)) is False
        assert store.add(item["data"], item["seg"], item["properties"]) == i
    assert len(store) == 4 and store.nbytes_device == 0
    assert store.nbytes_host == sum(_nbytes(item) for item in ds)
    assert store.max_host_data_numel == max(item["data"].size for item in ds)
    assert store.max_host_seg_bytes == max(item["seg"].nbytes for item in ds)
    for i, item in enumerate(ds):
        got = store[i]
        assert sorted(got) == ["data", "properties", "seg"]
        assert got["data"].dtype == torch.float32 and got["seg"].dtype == torch.int8
        assert not store.on_device(i)
        assert np.array_equal(got["data"].numpy(), item["data"])
        assert np.array_equal(got["seg"].numpy(), item["seg"])
        assert got["properties"] is item["properties"]
    # a host store is a dataset for the draw: the same plans as from the arrays
    fx = ref.fixtures()
    plan = dl.draw_batch_plan(store, ref.PATCH, ref.BATCH, rng=np.random.RandomState(ref.SEED))
    assert np.array_equal(plan.bbox_lbs, fx["last_lbs"][0])


def test_case_store_split_point():
    ds = ref.fixture_dataset()
    sizes = [_nbytes(item) for item in ds]
    store = dl.CaseStore(device_bytes=sizes[0] + sizes[1])
    assert store.fits(sizes[0]) and store.fits(sizes[0] + sizes[1])
    assert not store.fits(sizes[0] + sizes[1] + 1)
    assert dl.CaseStore().fits(1 << 60)  # None: no limit
    # once a case has gone to the host, later ones follow it even if they would fit
    store = dl.CaseStore(device_bytes=sizes[3])
    store.add(ds[0]["data"], ds[0]["seg"], ds[0]["properties"])   # larger than the budget
    assert store.nbytes_host == sizes[0] and not store.fits(sizes[3])
    store.add(ds[3]["data"], ds[3]["seg"], ds[3]["properties"])
    assert store.nbytes_host == sizes[0] + sizes[3] and store.nbytes_device == 0


def test_case_store_refuses_bad_cases():
    ds = ref.fixture_dataset()
    store = dl.CaseStore(device_bytes=0)
    with pytest.raises(ValueError, match="device_bytes"):
        dl.CaseStore(device_bytes=-1)
    with pytest.raises(ValueError, match="expected data"):
        store.add(ds[0]["data"][0], ds[0]["seg"], ds[0]["properties"])
    with pytest.raises(ValueError, match="expected data"):
        store.add(ds[0]["data"], ds[1]["seg"], ds[0]["properties"])
    with pytest.raises(ValueError, match="class_locations"):
        store.add(ds[0]["data"], ds[0]["seg"], {})
    with pytest.raises(TypeError, match="int8, int16 or float32"):
        store.add(ds[0]["data"], ds[0]["seg"].astype(np.int64), ds[0]["properties"])
    assert len(store) == 0
