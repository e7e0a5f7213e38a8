"""Per-phase cycles of one workgroup of the stage-2 CCF_FFN back half, from a library built with
-DWF_DWFC2_PROBE (make ... EXTRA=-DWF_DWFC2_PROBE, loaded via WAVEFORMER_HIP_LIB): for each wave,
cycles per plane iteration in each phase between the barriers (work, then wait).  Prints the
table of whichever kernel ran: ffn_dwfc2_tb (16 waves, two barriers per plane; its role, 0..11 D
and 12..15 E, in the last column; "vm wait" is the D waves' wait for the first input row of the
plane and is part of the phase work beside it: phase 1 on the slot-2 waves, roles 2, 5, 8, 11,
phase 2 on the others) or ffn_dwfc2_kernel (12 waves, three barriers; WAVEFORMER_PRECISION=bf16,
or a library without ffn_dwfc2_tb)."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import waveformer_amd.network_models as NM  # noqa: E402
from waveformer_amd import _lib, ops  # noqa: E402

B, C, S = 8, 96, 32
ops.set_precision(os.environ.get("WAVEFORMER_PRECISION", "bf16x3"))
torch.manual_seed(0)
mlp = NM.CCF_FFN(C, 4 * C, img_size=(S, S, S)).cuda().eval()
norm2 = torch.nn.LayerNorm(C, eps=1e-6).cuda()
x = torch.randn(B, S, S, S, C, device="cuda")
xh, stats = ops.msfuse([], x, 1e-6)
for _ in range(3):
    ops.ccf_ffn(xh, stats, norm2, mlp)
torch.cuda.synchronize()
lib = _lib.load()
NAMES12 = ["C-A work", "A wait", "A-B work", "B wait", "B-C work", "C wait"]
# ffn_dwfc2_tb: phase 1 (LN2 | slot-2 scatter | fc), barrier 1, phase 2 (scatter, h2 tile |
# straddled tile), barrier 2; slot 4 the D waves' vmcnt wait, slot 7 the iterations of the march
NAMES16 = ["ph1 work", "bar1 wait", "ph2 work", "bar2 wait", "vm wait"]
for sym, waves in (("wf_debug_dwfc2tb_probe", 16), ("wf_debug_dwfc2_probe", 12)):
    if not hasattr(lib, sym):
        continue
    buf = (ctypes.c_longlong * (waves * 8))()
    assert getattr(lib, sym)(buf) == 0
    if not any(buf[w * 8 + i] for w in range(waves) for i in range(6)):
        continue
    names, slots = (NAMES16, (0, 1, 2, 3, 4)) if waves == 16 else (NAMES12, range(6))
    print(sym)
    print("wave  " + "  ".join(f"{n:>9}" for n in names) + "   total  (cycles per plane)  role")
    for w in range(waves):
        planes = buf[w * 8 + 7] if waves == 16 else S + 2
        v = [buf[w * 8 + i] / planes for i in slots]
        print(f"{w:4d}  " + "  ".join(f"{c:9.0f}" for c in v) + f"  {sum(v):7.0f}  {buf[w * 8 + 6]:4d}",
              flush=True)
