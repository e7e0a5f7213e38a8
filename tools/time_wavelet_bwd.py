"""Time the four general-wavelet entries with device events:

  wf_dwt3d_fwd         x -> 8 bands           and its adjoint   wf_dwt3d_bwd
  wf_idwt3d_level      8 bands -> volume      and its adjoint   wf_idwt3d_level_bwd

wf_dwt3d_bwd runs the synthesis kernel on the bytes wf_idwt3d_level moves, and
wf_idwt3d_level_bwd the analysis kernel on the bytes of wf_dwt3d_fwd, so each backward entry is
printed next to the forward entry of the same form.  Rounds interleave the entries; one line
per entry: median and minimum microseconds, the bytes the algorithm needs (one read of the
input, one write of the output) and their fraction of the 8 TB/s HBM peak at the median.

  python tools/time_wavelet_bwd.py [--wavelet db2] [--shape 2 48 96 96 96] [--rounds 30]
                                   [--other-lib PATH]   # also time another build's forward
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformer_amd import _lib, ops  # noqa: E402

HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wavelet", default="db2")
    ap.add_argument("--shape", type=int, nargs=5, default=[2, 48, 96, 96, 96])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--other-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lib = _lib.load()
    B, C, D, H, W = a.shape
    (dlo, dhi, rlo, rhi), L = ops._filters(a.wavelet)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(a.shape, device="cuda", generator=g)
    n = tuple((s + L - 1) // 2 for s in (D, H, W))
    bands = torch.empty((8, B, C) + n, device="cuda")
    O = tuple(2 * m - L + 2 for m in n)
    vol = torch.randn((B, C) + O, device="cuda", generator=g)
    gco = torch.empty_like(bands)
    dx = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    ptrs = (ctypes.c_void_p * 8)(*[bands[k].data_ptr() for k in range(8)])
    gptrs = (ctypes.c_void_p * 8)(*[gco[k].data_ptr() for k in range(8)])
    st = (ctypes.c_int64 * 40)(*[v for k in range(8) for v in bands[k].stride()])

    def fwd_args(out):
        return (x.data_ptr(), out.data_ptr(), B * C, D, H, W, dlo, dhi, L, s)

    def inv_args(out):
        return (ptrs, st, B, C, n[0], n[1], n[2], rlo, rhi, L, out.data_ptr(), out.stride(0),
                out.stride(1), s)

    entries = [
        ("wf_dwt3d_fwd", lib.wf_dwt3d_fwd, fwd_args(bands), x.numel() + bands.numel()),
        ("wf_idwt3d_level_bwd", lib.wf_idwt3d_level_bwd,
         (vol.data_ptr(), vol.stride(0), vol.stride(1), B, C, n[0], n[1], n[2], 0, 0, 0, rlo, rhi,
          L, gptrs, st, s), vol.numel() + gco.numel()),
        ("wf_idwt3d_level", lib.wf_idwt3d_level, inv_args(vol), bands.numel() + vol.numel()),
        ("wf_dwt3d_bwd", lib.wf_dwt3d_bwd,
         (bands.data_ptr(), dx.data_ptr(), B * C, D, H, W, dlo, dhi, L, s),
         bands.numel() + dx.numel()),
    ]
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        for name in ("wf_dwt3d_fwd", "wf_idwt3d_level"):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        b2, v2 = torch.empty_like(bands), torch.empty_like(vol)
        entries += [("other:wf_dwt3d_fwd", other.wf_dwt3d_fwd, fwd_args(b2),
                     x.numel() + bands.numel()),
                    ("other:wf_idwt3d_level", other.wf_idwt3d_level, inv_args(v2),
                     bands.numel() + vol.numel())]

    def run(fn, args):
        rc = fn(*args)
        if rc != 0:
            raise RuntimeError(lib.wf_last_error().decode(errors="replace"))

    for _, fn, args, _ in entries:  # warm-up (the forward first: it fills the bands)
        for _ in range(3):
            run(fn, args)
    torch.cuda.synchronize()
    if a.other_lib:
        print("other build's outputs bit-identical:",
              bool(torch.equal(b2, bands)) and bool(torch.equal(v2, vol)))
    times = {name: [] for name, *_ in entries}
    for _ in range(a.rounds):
        for name, fn, args, _ in entries:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(fn, args)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    print(f"wavelet {a.wavelet} shape {tuple(a.shape)} bands {tuple(bands.shape)} rounds {a.rounds}")
    for name, _, _, elems in entries:
        t = times[name]
        med, mn = statistics.median(t), min(t)
        nbytes = 4 * elems
        print(f"{name:24s} median {med:8.1f} us  min {mn:8.1f} us  {nbytes / 1e6:8.1f} MB  "
              f"{nbytes / (med * 1e-6) / HBM * 100:5.1f} % of 8 TB/s")


if __name__ == "__main__":
    main()
