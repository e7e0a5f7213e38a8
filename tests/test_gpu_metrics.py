"""GPU: the evaluation kernels (csrc/metrics.hip) stage by stage and waveformer_amd.metrics end
to end, against the recorded scipy/medpy-restatement fixture (tests/golden/metrics_fixtures.npz)
and the numpy brute-force oracle of tests/metrics_ref.py.

Tolerances:
  * masks, counts, labels, borders, squared distances, histograms, order statistics: EXACT --
    they are integers.
  * dice, hd95: relative 1e-12 against the fixture (one float64 division, resp. one square root
    per order statistic and one interpolation, the same operations on both sides); hd exact
    (one square root of an exact integer).
  * asd, assd: relative 1e-12 (a float64 sum over at most a few thousand terms in ascending
    bin order against numpy's pairwise mean: error <= terms x 2^-53 ~ 2e-13).
"""
import numpy as np
import pytest
import torch

from tests import metrics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_CASES = ref.CASES + ref.EXTRA_CASES
RTOL = 1e-12


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


def _metrics():
    from waveformer_amd import metrics
    return metrics


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _expected(name):
    """(R, 6) expected [dice, hd95, hd, asd, asd, assd]: the fixture, with the reference's
    [0.0, 50] convention where a mask is empty."""
    fx = ref.fixtures()
    f = fx[f"{name}_float"].copy()
    empty = fx[f"{name}_int"][:, 0] < 0
    f[empty, 0] = 0.0
    f[empty, 1:] = 50.0
    return f, empty


@pytest.mark.parametrize("name", ALL_CASES)
def test_region_masks_and_overlap_counts(name):
    ops = _ops()
    case = ref.case_reference(name)
    got = []
    for side, key in enumerate(("pred", "gt")):
        masks, labels, counts = ops.region_masks(_dev(case[key]), ref.BRATS_BITS)
        assert masks.dtype == torch.uint8
        assert np.array_equal(masks.cpu().numpy(), case["masks"][side])
        assert np.array_equal(labels.cpu().numpy(), case[key])
        assert counts.cpu().tolist() == [int(m.sum()) for m in case["masks"][side]]
        got.append(masks)
    oc = ops.overlap_counts(got[0], got[1]).cpu().numpy()
    want = ref.fixtures()[f"{name}_int"][:, 8:11]
    assert oc.dtype == np.int64 and np.array_equal(oc, want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_argmax_with_planted_ties(dtype):
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    s = torch.randn((4, 7, 9, 11), generator=g).to(dtype)
    s[:, 0, 0, 0] = 0.5                      # all four equal -> class 0
    s[:, 1, 2, 3] = torch.tensor([2.0, -1.0, 2.0, 0.0]).to(dtype)   # 0 and 2 tie -> 0
    s[:, 2, 3, 4] = torch.tensor([-1.0, 3.0, 0.0, 3.0]).to(dtype)   # 1 and 3 tie -> 1
    s[:, 3, 4, 5] = torch.tensor([0.0, 1.5, 1.5, 1.5]).to(dtype)    # 1, 2, 3 tie -> 1
    s[:, 6, 8, 10] = torch.tensor([-2.0, -2.0, -3.0, -2.0]).to(dtype)  # 0, 1, 3 tie -> 0
    s[:, 4, 4, 4] = torch.tensor([0.0, 0.0, 1.0, 1.0]).to(dtype)    # 2 and 3 tie -> 2
    want = torch.argmax(s, dim=0).to(torch.uint8)
    assert want[1, 2, 3] == 0 and want[2, 3, 4] == 1 and want[3, 4, 5] == 1 and want[4, 4, 4] == 2
    masks, labels, counts = ops.region_masks(s.to(DEV), ref.BRATS_BITS)
    assert torch.equal(labels.cpu(), want)
    wm = ref.region_masks(want.numpy())
    assert np.array_equal(masks.cpu().numpy(), wm)
    assert counts.cpu().tolist() == [int(m.sum()) for m in wm]


@pytest.mark.parametrize("name", ALL_CASES)
def test_border_and_squared_distance_at_every_voxel(name):
    ops = _ops()
    case = ref.case_reference(name)
    R = case["masks"].shape[1]
    masks = _dev(case["masks"].reshape((2 * R,) + case["masks"].shape[2:]))
    border, d2 = ops.surface_edt_sq(masks)
    assert border.dtype == torch.uint8 and d2.dtype == torch.uint32
    gb = border.cpu().numpy().reshape(case["border"].shape)
    gd = d2.cpu().numpy().reshape(case["d2"].shape)
    for side in range(2):
        for r in range(R):
            assert np.array_equal(gb[side, r], case["border"][side, r]), (name, side, r, "border")
            bad = np.argwhere(gd[side, r] != case["d2"][side, r])
            assert len(bad) == 0, (name, side, r, "first wrong voxel", bad[0],
                                   gd[side, r][tuple(bad[0])], case["d2"][side, r][tuple(bad[0])])


def _hist_of(case):
    ops = _ops()
    R = case["masks"].shape[1]
    masks = _dev(case["masks"].reshape((2 * R,) + case["masks"].shape[2:]))
    border, d2 = ops.surface_edt_sq(masks)
    return ops.surface_hist(border[:R], d2[R:], border[R:], d2[:R])


@pytest.mark.parametrize("name", ALL_CASES)
def test_histograms_and_order_statistics(name):
    ops, metrics = _ops(), _metrics()
    case = ref.case_reference(name)
    ints = ref.fixtures()[f"{name}_int"]
    shape = case["pred"].shape
    hist = _hist_of(case)
    nbins = sum(v * v for v in shape) + 1
    assert tuple(hist.shape) == (3, 2, nbins) and hist.dtype == torch.uint32
    h = hist.cpu().numpy()
    both = ops.hist_order_stats(hist, (-1, 0, 1, 2), q=(95000, 100000), group=2).cpu().numpy()
    each = ops.hist_order_stats(hist, (0,), group=1).cpu().numpy().reshape(3, 2, 8)
    for r, (_, _, samples) in enumerate(case["stats"]):
        if samples is None:  # a mask is empty: nothing is counted
            assert not h[r].any()
            assert list(both[r]) == [0, -1, 0, -1, -1, -1, -1, 0]
            continue
        for d in range(2):
            assert np.array_equal(h[r, d], np.bincount(samples[d], minlength=nbins)), (name, r, d)
            n, top = ints[r, 4 + 2 * d], ints[r, 5 + 2 * d]
            assert list(each[r, d, :3]) == [n, top, 0]
            assert each[r, d, 3] == samples[d].min()       # absolute rank 0
        n, lo_sq, hi_sq, top = (int(v) for v in ints[r, :4])
        assert both[r, 0] == n and both[r, 1] == top
        base = int(both[r, 2])
        assert base == 95 * (n - 1) // 100
        srt = np.sort(np.hstack(samples))
        for i, o in enumerate((-1, 0, 1, 2)):
            assert both[r, 3 + i] == srt[min(max(base + o, 0), n - 1)], (name, r, o)
        k = metrics.percentile_rank(n, 95)
        got = {min(max(base + o, 0), n - 1): int(both[r, 3 + i]) for i, o in enumerate((-1, 0, 1, 2))}
        assert got[k] == lo_sq and got[min(k + 1, n - 1)] == hi_sq


@pytest.mark.parametrize("name", ALL_CASES)
def test_region_metrics_end_to_end(name):
    metrics = _metrics()
    case = ref.case_reference(name)
    want, empty = _expected(name)
    got = metrics.region_metrics(case["pred"], case["gt"], extra=True)
    assert got.dtype == np.float64 and got.shape == (3, 6)
    two = metrics.region_metrics(_dev(case["pred"]), _dev(case["gt"]))
    assert two.shape == (3, 2) and np.array_equal(two, got[:, :2])
    for r in range(3):
        if empty[r]:
            assert list(got[r, :2]) == [0.0, 50.0]
            continue
        np.testing.assert_allclose(got[r, :2], want[r, :2], rtol=RTOL, atol=0)
        assert got[r, 2] == want[r, 2]                                    # hd: exact
        np.testing.assert_allclose(got[r, 3:], want[r, 3:], rtol=RTOL, atol=0)
    if name == "both_empty":
        assert np.array_equal(two, np.tile([0.0, 50.0], (3, 1)))
    assert empty.sum() == {"no_et_pred": 1, "both_empty": 3, "full": 2}.get(name, 0)


def test_batched_form_and_spacing():
    metrics = _metrics()
    case = ref.case_reference("no_et_pred")
    pred = np.stack([case["pred"], case["gt"]])
    gt = np.stack([case["gt"], case["gt"]])
    got = metrics.region_metrics(pred, gt)
    assert got.shape == (2, 3, 2)
    for i in range(2):
        assert np.array_equal(got[i], metrics.region_metrics(pred[i], gt[i]))
    assert np.array_equal(got[1], np.tile([1.0, 0.0], (3, 1)))  # gt against itself
    scaled = metrics.region_metrics(pred[0], gt[0], spacing=[2.0, 2.0, 2.0])
    assert np.array_equal(scaled[:2, 0], got[0, :2, 0])
    assert np.array_equal(scaled[:2, 1], got[0, :2, 1] * 2.0)
    assert list(scaled[2]) == [0.0, 50.0]
    with pytest.raises(NotImplementedError, match="isotropic"):
        metrics.region_metrics(pred[0], gt[0], spacing=(1.0, 1.0, 2.0))


def test_scores_input_takes_the_argmax():
    metrics = _metrics()
    case = ref.case_reference("no_et_pred")
    onehot = np.stack([case["pred"] == c for c in range(4)]).astype(np.float16)
    got = metrics.region_metrics(torch.from_numpy(onehot).to(DEV), case["gt"])
    assert np.array_equal(got, metrics.region_metrics(case["pred"], case["gt"]))


@pytest.mark.parametrize("name", ["w67_h70", "no_et_pred"])
def test_reference_named_helpers(name):
    metrics = _metrics()
    case = ref.case_reference(name)
    want = metrics.region_metrics(case["pred"], case["gt"])
    gt3 = metrics.convert_labels(torch.from_numpy(case["gt"].astype(np.int32)))
    pred3 = metrics.convert_labels(case["pred"])
    assert gt3.dtype == torch.float32 and tuple(gt3.shape) == (3,) + case["gt"].shape
    assert np.array_equal(gt3.cpu().numpy(), case["masks"][1].astype(np.float32))
    # the reference's call: each_cases_metric(gt_array, pred_array, [1, 1, 1]) on numpy stacks
    m = metrics.each_cases_metric(gt3.cpu().numpy(), pred3.cpu().numpy(), [1, 1, 1])
    assert m.shape == (3, 2) and np.array_equal(m, want)
    for r in range(3):
        one = metrics.cal_metric(gt3[r], pred3[r], [1, 1, 1])
        assert one.shape == (2,) and np.array_equal(one, want[r])


def test_identical_masks():
    metrics = _metrics()
    lab = ref.case_reference("w67_h70")["gt"]
    got = metrics.region_metrics(lab, lab.copy(), extra=True)
    assert np.array_equal(got[:, 0], np.ones(3)) and np.array_equal(got[:, 1:], np.zeros((3, 5)))


@pytest.mark.parametrize("shape,p,q", [((5, 6, 7), (1, 0, 6), (4, 5, 2)),
                                        ((155, 240, 240), (0, 0, 0), (154, 239, 239))])
def test_two_single_voxel_masks(shape, p, q):
    ops, metrics = _ops(), _metrics()
    pred = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    gt = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    pred[p] = 3
    gt[q] = 3
    d2 = sum((a - b) ** 2 for a, b in zip(p, q))
    if shape == (155, 240, 240):
        assert d2 == 137958 and ops.surface_hist_bins(shape) == 139226
    # the stages: n = 2 and both order statistics at |p - q|^2
    masks = torch.stack([pred, gt]).ne(0).to(torch.uint8)
    border, dist = ops.surface_edt_sq(masks)
    assert int(border.sum()) == 2
    hist = ops.surface_hist(border[:1], dist[1:], border[1:], dist[:1])
    st = ops.hist_order_stats(hist, (0, 1), group=2).cpu().tolist()[0]
    assert st[:5] == [2, d2, 0, d2, d2]
    di = dist.view(torch.int32)
    assert int(di[0][q]) == d2 and int(di[1][p]) == d2 and int(di[0][p]) == 0
    got = metrics.region_metrics(pred, gt, extra=True)
    want = np.sqrt(np.float64(d2))
    for r in range(3):  # class 3 is in TC, WT and ET
        assert got[r, 0] == 0.0 and np.array_equal(got[r, 1:], np.full(5, want))


def test_swapping_pred_and_gt_changes_nothing():
    metrics = _metrics()
    for name in ("w67_h70", "d1", "full"):
        case = ref.case_reference(name)
        a = metrics.region_metrics(case["pred"], case["gt"], extra=True)
        b = metrics.region_metrics(case["gt"], case["pred"], extra=True)
        assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(a[:, 5], b[:, 5])
        assert np.array_equal(a[:, 3], b[:, 4]) and np.array_equal(a[:, 4], b[:, 3])


def test_repeatable_bitwise():
    ops, metrics = _ops(), _metrics()
    case = ref.case_reference("w67_h70")
    runs = []
    for _ in range(2):
        hist = _hist_of(case)
        st = ops.hist_order_stats(hist, (-1, 0, 1, 2), q=(95000, 100000), group=2)
        runs.append((hist.cpu().numpy(), st.cpu().numpy(),
                     metrics.region_metrics(case["pred"], case["gt"], extra=True)))
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
