"""CPU: the host side of wf_window_attention_fwd_levels (all LL levels of a Block in one launch
set): the symbol is exported, its workspace is the sum of the per-level workspaces, and a bad
level list is refused before any HIP call (there is no GPU here)."""
import ctypes

import pytest

from waveformer_amd import _lib

FAKE = 256  # never dereferenced: validation fails first


def _dhw(levels):
    flat = [v for l in levels for v in l]
    return (ctypes.c_int64 * max(1, len(flat)))(*flat)


def _ptrs(n):
    return (ctypes.c_void_p * max(1, n))(*([FAKE] * n))


def _fwd(levels, B=1, C=48, heads=3, prec=1, nlev=None):
    n = len(levels) if nlev is None else nlev
    lib = _lib.load()
    rc = lib.wf_window_attention_fwd_levels(_ptrs(len(levels)), _dhw(levels), n, FAKE, FAKE, FAKE,
                                            FAKE, FAKE, FAKE, FAKE, B, C, heads, 0.25, prec, None)
    return rc, lib.wf_last_error().decode()


def test_symbols_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "wf_window_attention_fwd_levels")
    assert hasattr(lib, "wf_window_attention_levels_workspace_bytes")
    assert "wf_window_attention_fwd_levels" in _lib.SIGNATURES


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("B,C,levels", [
    (8, 48, [(32, 32, 32), (16, 16, 16), (8, 8, 8)]),
    (2, 96, [(16, 16, 16), (8, 8, 8)]),
    (2, 48, [(16, 8, 24), (8, 8, 8)]),
    (1, 48, [(8, 8, 8)]),
])
def test_workspace_is_the_sum_of_the_per_level_workspaces(B, C, levels, prec):
    got = _lib.query("wf_window_attention_levels_workspace_bytes", _dhw(levels), len(levels), B,
                     C, prec)
    want = sum(_lib.query("wf_window_attention_workspace_bytes", B, C, d, h, w, prec)
               for d, h, w in levels)
    assert got == want > 0


def test_bad_level_lists_are_refused_on_the_host():
    ok = [(16, 16, 16), (8, 8, 8)]
    rc, msg = _fwd(ok, nlev=0)
    assert rc < 0 and "1 to 4 levels" in msg
    rc, msg = _fwd(ok + ok + ok, nlev=5)
    assert rc < 0 and "1 to 4 levels" in msg
    rc, msg = _fwd([(16, 16, 16), (12, 12, 12)])
    assert rc < 0 and "8^3 windows" in msg
    rc, msg = _fwd(ok, C=48, heads=4)
    assert rc < 0 and "head_dim 16" in msg
    with pytest.raises(RuntimeError, match="is NULL"):
        _lib.call("wf_window_attention_fwd_levels", _ptrs(2), _dhw(ok), 2, None, FAKE, FAKE,
                  FAKE, FAKE, FAKE, FAKE, 1, 48, 3, 0.25, 1, None)
    for bad in ([(12, 12, 12)], ok * 3):
        assert _lib.query("wf_window_attention_levels_workspace_bytes", _dhw(bad), len(bad), 1,
                          48, 1) < 0
