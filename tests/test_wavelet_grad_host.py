"""CPU: the registration and host validation of the differentiable general-wavelet ops
(waveformer::wavedec3_level / waverec3_level, wf_dwt3d_bwd / wf_idwt3d_level_bwd).

  * the fake kernels on the meta device give the shapes of the oracle's wavedec3 / waverec3 for
    db1..db4 and odd sizes, including the level whose LL is one sample longer than the details;
  * a CPU tensor fails loudly (no CPU kernel);
  * the two backward entries validate their arguments before any HIP call.
"""
import ctypes

import pytest
import torch

from oracle import ref_waveformer as R

WAVELETS = ["db1", "db2", "db3", "db4"]
SIZES = [(11, 9, 7), (8, 13, 12), (20, 37, 70)]
B, C = 2, 3


def _ops():
    import waveformer_amd.library  # noqa: F401
    return torch.ops.waveformer


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("wav", WAVELETS)
def test_fake_shapes_match_the_oracle(wav, size):
    ops = _ops()
    ref = R.wavedec3(torch.zeros((B, C) + size), wav, 2)
    with torch.no_grad():
        cur = torch.empty((B, C) + size, device="meta")
        dets = []
        for _ in range(2):
            bands = ops.wavedec3_level(cur, wav)
            assert bands.device.type == "meta" and bands.shape[0] == 8
            dets.append(bands[1:].unbind(0))
            cur = bands[0]
        dets = dets[::-1]
        assert tuple(cur.shape) == tuple(ref[0].shape)
        for dg, dr in zip(dets, ref[1:]):
            for t, k in zip(dg, R.DETAIL_KEYS):
                assert tuple(t.shape) == tuple(dr[k].shape), k
        # synthesis, chained over the 2 levels
        x = cur
        longer = False
        for li, dg in enumerate(dets):
            longer |= li > 0 and any(a == b + 1 for a, b in zip(x.shape[2:], dg[0].shape[2:]))
            x = ops.waverec3_level(x, list(dg), wav)
            assert x.device.type == "meta"
        want = R.waverec3(ref, wav)
        assert tuple(x.shape) == tuple(want.shape)
    if size == (11, 9, 7):
        assert longer, "this size is the case whose LL is one sample longer than the details"


def test_fake_backward_shapes():
    ops = _ops()
    with torch.no_grad():
        g = torch.empty((8, B, C, 7, 6, 5), device="meta")
        dx = ops.wavedec3_level_backward(g, [11, 9, 7], "db2")
        assert tuple(dx.shape) == (B, C, 11, 9, 7)
        gout = torch.empty((B, C, 12, 10, 8), device="meta")
        gs = ops.waverec3_level_backward(gout, [8, 6, 5], [False, True] * 4, "db2")
        assert [tuple(t.shape) for t in gs] == [(B, C, 8, 6, 5)] + [(B, C, 7, 6, 5)] * 7
        assert gs[0].is_contiguous() and gs[1].stride(1) == 1


def test_cpu_tensor_fails_loudly():
    ops = _ops()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.wavedec3_level(torch.zeros(1, 2, 8, 8, 8), "db2")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.waverec3_level(torch.zeros(1, 2, 5, 5, 5), [torch.zeros(1, 2, 5, 5, 5)] * 7, "db2")


def test_backward_entries_validate_on_the_host():
    from waveformer_amd import _lib
    fake = 256  # never dereferenced: validation fails first
    filt = (ctypes.c_float * 8)()  # host filter arrays
    with pytest.raises(RuntimeError, match="filter length"):
        _lib.call("wf_dwt3d_bwd", fake, fake, 2, 8, 8, 8, filt, filt, 3, None)
    with pytest.raises(RuntimeError, match="empty tensor"):
        _lib.call("wf_dwt3d_bwd", fake, fake, 2, 8, 0, 8, filt, filt, 4, None)
    with pytest.raises(RuntimeError, match="is NULL"):
        _lib.call("wf_dwt3d_bwd", fake, None, 2, 8, 8, 8, filt, filt, 4, None)
    ptrs = (ctypes.c_void_p * 8)(*[fake] * 8)
    strides = (ctypes.c_int64 * 40)()
    with pytest.raises(RuntimeError, match="empty tensor"):
        _lib.call("wf_idwt3d_level_bwd", fake, 1000, 100, 1, 1, 0, 4, 4, 0, 0, 0, filt, filt, 4,
                  ptrs, strides, None)
    with pytest.raises(RuntimeError, match="filter length"):
        _lib.call("wf_idwt3d_level_bwd", fake, 1000, 100, 1, 1, 4, 4, 4, 0, 0, 0, filt, filt, 5,
                  ptrs, strides, None)
    with pytest.raises(RuntimeError, match="shorter than the filter"):
        _lib.call("wf_idwt3d_level_bwd", fake, 1000, 100, 1, 1, 4, 2, 4, 0, 0, 0, filt, filt, 6,
                  ptrs, strides, None)
    with pytest.raises(RuntimeError, match="one sample longer"):
        _lib.call("wf_idwt3d_level_bwd", fake, 1000, 100, 1, 1, 4, 4, 4, 0, 2, 0, filt, filt, 4,
                  ptrs, strides, None)
    with pytest.raises(RuntimeError, match="is NULL"):
        _lib.call("wf_idwt3d_level_bwd", None, 1000, 100, 1, 1, 4, 4, 4, 0, 0, 0, filt, filt, 4,
                  ptrs, strides, None)
