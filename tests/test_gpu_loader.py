"""GPU: wf_crop_pad_batch (ops.crop_pad_batch) bitwise against the numpy restatement
tests/loader_ref.py, and waveformer_amd.dataloading's loader over a CaseStore against the batches
the reference's loader produced (tests/golden/loader_fixtures.npz).

Every run writes into outputs pre-filled with NaN (an element left unwritten shows), followed by
64 guard bytes that must stay as they were, and is repeated once: the second result must be the
first, bit for bit.  A copy kernel has no rounding, so every comparison is on the bits."""
import numpy as np
import pytest
import torch

from tests import loader_ref as ref
from waveformer_amd import augment, ops
from waveformer_amd import dataloading as dl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16                      # floats: 64 bytes behind each output
GUARD_BITS = -1515870811        # 0xA5A5A5A5 as int32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(shape, offset=0):
    """An output of `shape` filled with NaN inside a flat buffer, `offset` floats in, with GUARD
    floats of a fixed pattern behind it.  Returns (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), float("nan"), device=DEV)
    buf[offset + n:].view(torch.int32).fill_(GUARD_BITS)
    return buf[offset:offset + n].view(shape), buf


def _check(cases_np, lbs, patch, out_offset=0, dev_cases=None):
    """Run the batch twice into guarded NaN outputs and compare with the restatement."""
    want_d, want_s = ref.crop_pad_batch(cases_np, lbs, patch)
    if dev_cases is None:
        dev_cases = [(torch.from_numpy(d).to(DEV), torch.from_numpy(s).to(DEV))
                     for d, s in cases_np]
    results = []
    for _ in range(2):
        od, bd = _guarded(want_d.shape, out_offset)
        os_, bs = _guarded(want_s.shape, out_offset)
        got = ops.crop_pad_batch(dev_cases, lbs, patch, out=(od, os_))
        assert got[0] is od and got[1] is os_
        torch.cuda.synchronize()
        for buf, n in ((bd, od.numel()), (bs, os_.numel())):
            assert bool((buf[out_offset + n:].view(torch.int32) == GUARD_BITS).all()), \
                "guard bytes behind an output were written"
            assert bool((buf[:out_offset] != buf[:out_offset]).all()), "bytes before an output"
        results.append((od.cpu(), os_.cpu()))
    for got_d, got_s in results:
        assert not torch.isnan(got_d).any() and not torch.isnan(got_s).any(), "unwritten elements"
        assert np.array_equal(got_d.numpy().view(np.int32), want_d.view(np.int32))
        assert np.array_equal(got_s.numpy().view(np.int32), want_s.view(np.int32))
    assert torch.equal(_bits(results[0][0]), _bits(results[1][0]))
    assert torch.equal(_bits(results[0][1]), _bits(results[1][1]))
    return results[0]


def _case(shape, C=2, seg_dtype=np.int8, S=1, seed=0):
    rs = np.random.RandomState(seed)
    data = rs.standard_normal((C,) + tuple(shape)).astype(np.float32)
    if seg_dtype == np.int8:
        seg = rs.choice(np.array([-1, 0, 1, 2, 3], np.int8), size=(S,) + tuple(shape))
    elif seg_dtype == np.int16:
        seg = rs.choice(np.array([-1, 0, 1, 300, -300], np.int16), size=(S,) + tuple(shape))
    else:
        seg = rs.choice(np.array([-1.0, 0.0, 1.5, 2.0], np.float32), size=(S,) + tuple(shape))
    return data, seg.astype(seg_dtype)


def _fixture_cases():
    return [(item["data"], item["seg"]) for item in ref.fixture_dataset()]


# boxes on the four fixture cases (11, 13, 9), (6, 13, 10), (9, 5, 14), (8, 8, 8)
LOW = [(-3, -1, -2), (-1, -5, -4), (-2, -2, 0), (-7, -7, -7)]
HIGH = [(5, 7, 3), (0, 6, 4), (3, 0, 9), (1, 2, 3)]
BOTH = [(-1, 6, -3), (-1, 6, 5), (4, -2, 8), (-1, -1, -1)]


@pytest.mark.parametrize("patch", [(8, 8, 8), (5, 6, 7)])
@pytest.mark.parametrize("name,lbs", [("inside", [(1, 2, 0), (0, 3, 1), (1, 0, 4), (0, 0, 0)]),
                                      ("low", LOW), ("high", HIGH), ("both", BOTH)])
def test_fixture_cases_over_the_edges(patch, name, lbs):
    # (5, 6, 7): rows of 7 floats, so the last group of a row is a scalar-store tail
    _check(_fixture_cases(), lbs, patch)


@pytest.mark.parametrize("patch", [(8, 8, 8), (5, 6, 7)])
@pytest.mark.parametrize("xoff", [0, 4, 8, -4, 12, 3])
def test_case_on_the_16_byte_load_path(patch, xoff):
    # (8, 8, 16): W, the plane and (with patch x = 8) the offsets 0 / 4 / 8 are multiples of 4,
    # the only shape here whose data rows are read 16 bytes at a time; -4 and 12 hang over an x
    # edge on that path, 3 and the patch of 7 take the dword path on the same case
    case = _case((8, 8, 16), seed=1)
    _check([case], [(0, 0, xoff)], patch)
    _check([case, case], [(-2, 3, xoff), (2, -3, xoff)], patch)


@pytest.mark.parametrize("seg_dtype,marker", [(np.int8, -1), (np.int16, 300), (np.float32, 1.5)])
@pytest.mark.parametrize("shape", [(8, 8, 16), (7, 9, 10)])
def test_segmentation_kinds(seg_dtype, marker, shape):
    case = _case(shape, seg_dtype=seg_dtype, seed=2)
    assert (case[1] == marker).any() and (case[1] == -1).any()
    for lb in ((0, 0, 0), (-1, 2, 4), (3, -2, -4)):
        _, seg = _check([case], [lb], (8, 8, 8))
        assert (seg == float(marker)).any()
    # a -1 stays -1.0f
    _, seg = _check([case], [(0, 0, 0)], tuple(min(8, s) for s in shape))
    assert np.array_equal(seg[0].numpy(), case[1][:, :seg.shape[2], :seg.shape[3], :seg.shape[4]]
                          .astype(np.float32))


@pytest.mark.parametrize("C,S", [(1, 1), (4, 1), (3, 2)])
def test_channel_counts(C, S):
    cases = [_case((8, 8, 16), C=C, S=S, seed=3), _case((5, 9, 7), C=C, S=S, seed=4)]
    _check(cases, [(0, 0, 4), (-2, 3, -1)], (8, 8, 8))
    _check(cases, [(1, -1, 5), (0, 4, 2)], (5, 6, 7))


def test_case_smaller_than_the_patch_with_an_odd_pad():
    # extents (5, 3, 6) under (8, 8, 8): pads 3 / 5 / 2, the boxes get_bbox allows: lb in
    # [(-n) // 2, n // 2 + n % 2 + extent - patch]
    case = _case((5, 3, 6), seed=5)
    for lb in ((-2, -3, -1), (-1, -2, -1), (-2, -2, -1)):
        d, _ = _check([case], [lb], (8, 8, 8))
        assert np.count_nonzero(d.numpy()) == np.count_nonzero(case[0])  # the whole case is in


@pytest.mark.parametrize("lb", [(-8, 0, 0), (0, 13, 0), (0, 0, 9), (11, 13, 9), (-20, -20, -20),
                                (0, 0, -8), (1 << 40, 0, 0), (0, -(1 << 40), 0)])
def test_box_wholly_outside_gives_zeros(lb):
    cases = _fixture_cases()[:1]
    d, s = _check(cases, [lb], (8, 8, 8))
    assert not d.any() and not s.any()


@pytest.mark.parametrize("B", [1, 3, 17])
def test_batch_sizes(B):
    # 17: two launches, of 16 and of 1 record
    base = _fixture_cases() + [_case((8, 8, 16), seed=6)]
    rs = np.random.RandomState(B)
    cases = [base[i % len(base)] for i in range(B)]
    lbs = [tuple(int(rs.randint(-6, s)) for s in c[0].shape[1:]) for c in cases]
    lbs[-1] = (0, 0, 4) if B > 1 else lbs[-1]
    _check(cases, lbs, (8, 8, 8))
    _check(cases, lbs, (5, 6, 7))


def test_unaligned_output_and_source():
    # an output that starts 4 bytes off a 16-byte boundary: scalar stores although the rows are
    # multiples of 4; a source 4 bytes off: dword loads although every size is a multiple of 4
    case = _case((8, 8, 16), seed=7)
    _check([case], [(0, 0, 4)], (8, 8, 8), out_offset=1)
    _check([case], [(-1, 1, -4)], (8, 8, 8), out_offset=3)
    flat = torch.zeros((case[0].size + 1,), device=DEV)
    flat[1:] = torch.from_numpy(case[0]).to(DEV).reshape(-1)
    sflat = torch.zeros((case[1].size + 1,), dtype=torch.int8, device=DEV)
    sflat[1:] = torch.from_numpy(case[1]).to(DEV).reshape(-1)
    dev = [(flat[1:].view(case[0].shape), sflat[1:].view(case[1].shape))]
    assert dev[0][0].data_ptr() % 16 == 4 and dev[0][1].data_ptr() % 4 == 1
    _check([case], [(0, 0, 4)], (8, 8, 8), dev_cases=dev)
    _check([case], [(2, -2, 12)], (8, 8, 8), dev_cases=dev)


def test_wrapper_makes_inputs_contiguous_and_checks_the_batch():
    d, s = _case((8, 8, 16), seed=8)
    wide = torch.from_numpy(np.concatenate([d, d], 3)).to(DEV)[..., :16]   # a strided view
    assert not wide.is_contiguous()
    _check([(d, s)], [(1, 1, 4)], (8, 8, 8),
           dev_cases=[(wide, torch.from_numpy(s).to(DEV))])
    dd, ss = torch.from_numpy(d).to(DEV), torch.from_numpy(s).to(DEV)
    with pytest.raises(TypeError):
        ops.crop_pad_batch([(dd, ss), (dd, ss.to(torch.int16))], [(0, 0, 0)] * 2, (8, 8, 8))
    with pytest.raises(ValueError, match="channels"):
        ops.crop_pad_batch([(dd, ss), (dd[:1], ss)], [(0, 0, 0)] * 2, (8, 8, 8))
    with pytest.raises(ValueError, match="does not match"):
        ops.crop_pad_batch([(dd, ss[:, :4])], [(0, 0, 0)], (8, 8, 8))
    with pytest.raises(ValueError, match="expected"):
        ops.crop_pad_batch([(dd, ss)], [(0, 0, 0)], (8, 8, 8),
                           out=(torch.empty((1, 2, 8, 8, 4), device=DEV),
                                torch.empty((1, 1, 8, 8, 8), device=DEV)))


# ------------------------------------------------------------------------------------------
# the loader over a CaseStore
# ------------------------------------------------------------------------------------------
def _store(device_bytes):
    store = dl.CaseStore(device_bytes=device_bytes, device=DEV)
    for item in ref.fixture_dataset():
        store.add(item["data"], item["seg"], item["properties"])
    return store


def _sizes():
    return [item["data"].nbytes + item["seg"].nbytes for item in ref.fixture_dataset()]


@pytest.mark.parametrize("mode,prob", ref.MODES)
@pytest.mark.parametrize("staged", [False, True])
def test_loader_reproduces_the_reference_batches(mode, prob, staged):
    fx, sizes = ref.fixtures(), _sizes()
    store = _store(sizes[0] + sizes[1] if staged else None)
    if staged:  # cases 2 and 3 come through the staging slots, from pinned memory
        assert [store.on_device(i) for i in range(4)] == [True, True, False, False]
        assert store.nbytes_device == sizes[0] + sizes[1]
        assert store.nbytes_host == sizes[2] + sizes[3]
        assert store[2]["data"].is_pinned() and store[3]["seg"].is_pinned()
    else:
        assert all(store.on_device(i) for i in range(4))
        assert store.nbytes_device == sum(sizes) and store.nbytes_host == 0
    loader = dl.DataLoaderMultiProcess(store, ref.PATCH, ref.BATCH, 0.33, prob,
                                       rng=np.random.RandomState(ref.SEED))
    for n in range(40):
        if n < 4:
            batch = next(loader)
            assert sorted(batch) == ["data", "keys", "properties", "seg"]
            assert np.array_equal(batch["keys"], fx[f"{mode}_keys"][n])
            for name in ("data", "seg"):
                got = batch[name]
                assert got.device.type == "cuda" and got.dtype == torch.float32
                assert np.array_equal(got.cpu().numpy().view(np.int32),
                                      fx[f"{mode}_{name}"][n].view(np.int32)), (name, n)
            assert [p is store[k]["properties"] for p, k in
                    zip(batch["properties"], batch["keys"])] == [True] * ref.BATCH
        else:
            plan = loader.draw_batch_plan()
            assert np.array_equal(plan.keys, fx[f"{mode}_keys"][n])
            assert np.array_equal(plan.force_fg, fx[f"{mode}_force"][n])
            assert np.array_equal(plan.bbox_lbs, fx[f"{mode}_lbs"][n])
    # the plans of the first four, from a fresh stream, execute to the same batches
    loader.rng = np.random.RandomState(ref.SEED)
    plan = loader.draw_batch_plan()
    assert np.array_equal(plan.bbox_lbs, fx[f"{mode}_lbs"][0])
    assert np.array_equal(plan.force_fg, fx[f"{mode}_force"][0])
    again = loader.execute_batch_plan(plan)
    assert np.array_equal(again["data"].cpu().numpy().view(np.int32),
                          fx[f"{mode}_data"][0].view(np.int32))


def test_loader_over_plain_numpy_cases_and_mixed_seg_kinds():
    # a dataset of numpy arrays is staged case by case; an int16 case beside int8 ones widens
    # the batch's segmentations on the device
    ds = ref.fixture_dataset()
    ds[1] = dict(ds[1], seg=ds[1]["seg"].astype(np.int16))
    loader = dl.DataLoaderMultiProcess(ds, ref.PATCH, 4, rng=np.random.RandomState(1), device=DEV)
    plan = dl.BatchPlan(keys=np.array([0, 1, 2, 1]), force_fg=np.zeros(4, bool),
                        bbox_lbs=np.array([(1, 2, 0), (-1, 3, 1), (0, -2, 5), (-1, 6, -3)]))
    batch = loader.execute_batch_plan(plan)
    want_d, want_s = ref.crop_pad_batch([(ds[k]["data"], ds[k]["seg"]) for k in plan.keys],
                                        plan.bbox_lbs, ref.PATCH)
    assert np.array_equal(batch["data"].cpu().numpy().view(np.int32), want_d.view(np.int32))
    assert np.array_equal(batch["seg"].cpu().numpy().view(np.int32), want_s.view(np.int32))


def test_batch_feeds_the_train_transforms():
    loader = dl.DataLoaderMultiProcess(_store(None), ref.PATCH, ref.BATCH,
                                       rng=np.random.RandomState(ref.SEED))
    batch = next(loader)
    out = augment.get_train_transforms_noaug(ref.PATCH)(**batch)
    assert torch.equal(_bits(out["data"]), _bits(batch["data"]))
    assert out["seg"].shape == batch["seg"].shape
    # RemoveLabel(-1 -> 0) is the transform's, everything else of the segmentation is the batch's
    want = torch.where(batch["seg"] == -1, torch.zeros_like(batch["seg"]), batch["seg"])
    assert torch.equal(out["seg"], want)
