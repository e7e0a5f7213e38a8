"""CPU: the host half of waveformer_amd.metrics (percentile from two order statistics, the
region table, argument validation of the new C-ABI entries) and the numpy brute-force oracle
against the recorded scipy/medpy-restatement fixture."""
import ctypes

import numpy as np
import pytest
import torch

from tests import metrics_ref as ref
from waveformer_amd import _lib, metrics


def test_percentile_from_order_stats_is_numpy_percentile():
    rng = np.random.default_rng(20240917)
    for it in range(200):
        n = int(rng.integers(1, 401)) if it >= 4 else (1, 2, 3, 400)[it]
        d2 = rng.integers(0, (3, 40, 5000)[it % 3], size=n)
        srt = np.sort(d2)
        for q in (50, 95, 100):
            k = metrics.percentile_rank(n, q)
            assert 0 <= k <= n - 1
            got = metrics.percentile_from_order_stats(n, int(srt[k]), int(srt[min(k + 1, n - 1)]), q)
            want = np.percentile(np.sqrt(d2.astype(np.float64)), q)
            assert got == want, (n, q, got, want)


def test_device_rank_window_covers_the_float_rank():
    # the device derives base = 95000 (n - 1) // 100000 in integers and returns the ranks
    # base - 1 .. base + 2; the float64 rank k and k + 1 must always be among them
    for n in list(range(1, 5000)) + [10 ** 6 + i for i in range(50)] + [2 ** 31 - 1]:
        base = 95000 * (n - 1) // 100000
        k = metrics.percentile_rank(n, 95.0)
        assert base - 1 <= k <= base, (n, k, base)


@pytest.mark.parametrize("name", ref.CASES + ref.EXTRA_CASES)
def test_bruteforce_oracle_reproduces_the_fixture(name):
    fx = ref.fixtures()
    want_f, want_i = fx[f"{name}_float"], fx[f"{name}_int"]
    case = ref.case_reference(name)
    for r, (ints, floats, _) in enumerate(case["stats"]):
        assert [ints[c] for c in ref.INT_COLS] == list(want_i[r]), (name, r)
        if floats is None:
            assert np.isnan(want_f[r]).all()
            continue
        got = np.array([floats[c] for c in ref.FLOAT_COLS], dtype=np.float64)
        assert np.array_equal(got, want_f[r]), (name, r, got, want_f[r])
        # and the integer route to hd95 gives the same bits
        hd95 = metrics.percentile_from_order_stats(ints["n"], ints["lo_sq"], ints["hi_sq"], 95)
        assert hd95 == want_f[r, 1]
        assert np.sqrt(np.float64(ints["max_d2"])) == want_f[r, 2]


def test_fixture_has_the_cases_the_kernels_need():
    fx = ref.fixtures()
    ints = np.concatenate([fx[f"{n}_int"] for n in ref.CASES])
    assert (ints[:, 0] < 0).sum() == 1                      # exactly one empty region
    assert ((ints[:, 0] > 0) & (ints[:, 1] != ints[:, 2])).any()  # an interpolating percentile
    assert list(fx["d1_int"][0, :3]) == [80, 1, 2]
    assert fx["h1_int"][2, 0] == 2
    assert fx["w130_int"][:, 3].min() >= 3600 and fx["w130_pred"].shape[2] > 128
    assert fx["w67_h70_pred"][8, 69, 66] == 2


def test_new_entries_reject_bad_arguments_before_any_hip_call():
    fake = 256  # never dereferenced: validation fails first
    bits = (ctypes.c_int * 5)(10, 14, 8, 1, 1)
    with pytest.raises(RuntimeError, match="C <= 8"):
        _lib.call("wf_region_masks", fake, 1, 9, bits, 3, fake, fake, fake, 4, 4, 4, None)
    with pytest.raises(RuntimeError, match="R <= 4"):
        _lib.call("wf_region_masks", fake, 0, 0, bits, 5, fake, fake, fake, 4, 4, 4, None)
    with pytest.raises(RuntimeError, match="R <= 4"):
        _lib.call("wf_overlap_counts", fake, fake, 5, 4, 4, 4, fake, None)
    big = (2048, 1024, 1024)  # 2^31 voxels
    with pytest.raises(RuntimeError, match="below 2\\^31 voxels"):
        _lib.call("wf_region_masks", fake, 0, 0, bits, 3, fake, fake, fake, *big, None)
    with pytest.raises(RuntimeError, match="below 2\\^31 voxels"):
        _lib.call("wf_overlap_counts", fake, fake, 3, *big, fake, None)
    with pytest.raises(RuntimeError, match="below 2\\^31 voxels"):
        _lib.call("wf_surface_hist", fake, fake, fake, fake, 3, *big, fake, None)
    assert _lib.query("wf_surface_edt_workspace_bytes", 6, *big) < 0
    with pytest.raises(RuntimeError, match=r"D\^2 \+ H\^2 \+ W\^2"):
        _lib.call("wf_surface_hist", fake, fake, fake, fake, 1, 1, 1, 46341, fake, None)
    with pytest.raises(RuntimeError, match="masks is NULL"):
        _lib.call("wf_region_masks", fake, 0, 0, bits, 3, None, fake, fake, 4, 4, 4, None)
    with pytest.raises(RuntimeError, match="masks is NULL"):
        _lib.call("wf_surface_edt_sq", None, 6, 4, 4, 4, fake, fake, fake, 1 << 20, None)
    with pytest.raises(RuntimeError, match="labels is NULL"):
        _lib.call("wf_region_masks", fake, 2, 4, bits, 3, fake, None, fake, 4, 4, 4, None)
    with pytest.raises(RuntimeError, match="workspace smaller"):
        _lib.call("wf_surface_edt_sq", fake, 6, 4, 4, 4, fake, fake, fake, 16, None)
    with pytest.raises(RuntimeError, match="at most 4 ranks"):
        _lib.call("wf_hist_order_stats", fake, 1, 1, 10, 0, 1, None, 5, fake, None)
    with pytest.raises(RuntimeError, match="hist is NULL"):
        _lib.call("wf_hist_order_stats", None, 1, 1, 10, 0, 1, None, 0, fake, None)
    assert _lib.query("wf_surface_edt_workspace_bytes", 6, 155, 240, 240) >= 6 * 155 * 240 * 240 * 4


def test_brats_region_table_is_convert_labels():
    # the reference's definition (5_compute_metrics.py:31-37) on the four class values
    labels = torch.arange(4)
    want = torch.stack([(labels == 1) | (labels == 3),
                        (labels == 1) | (labels == 3) | (labels == 2), labels == 3])
    got = torch.tensor([[bool(b >> int(c) & 1) for c in labels] for b in metrics.BRATS_REGIONS])
    assert torch.equal(got, want)
    assert metrics.region_bits([{1, 3}, {1, 2, 3}, {3}]) == metrics.BRATS_REGIONS
    assert tuple(ref.BRATS_BITS) == metrics.BRATS_REGIONS


def test_host_side_argument_checks():
    with pytest.raises(NotImplementedError, match="isotropic"):
        metrics.region_metrics(np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8),
                               spacing=(1.0, 1.0, 2.5))
    with pytest.raises(ValueError, match="1..4 regions"):
        metrics.region_bits([1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match="classes are 0..7"):
        metrics.region_bits([{8}])
    assert metrics.result_bytes() == 3 * (3 + 8) * 8
    import waveformer_amd
    assert waveformer_amd.region_metrics is metrics.region_metrics
