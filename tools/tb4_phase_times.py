"""Per-phase cycles of one workgroup of the stage-1 CCF_FFN back half (ffn_dwfc_tb4), from a
library built with -DWF_DWFC2_PROBE (make ... EXTRA=-DWF_DWFC2_PROBE, loaded via
WAVEFORMER_HIP_LIB), at B = 8, 64^3 (the encoder step's stage-1 shape): for each wave, cycles per
plane iteration of its work and its barrier wait in each of the two phases and, for the E waves,
the LDS-DMA issue and the vmcnt wait for the staged plane.  The role (0..11 D waves, slot =
role % 3; 12..15 E waves) is in the last column; WAVEFORMER_PRECISION=fp16 probes the <2> kernel."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import waveformer_amd.network_models as NM  # noqa: E402
from waveformer_amd import _lib, ops  # noqa: E402

B, C, S = 8, 48, 64
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
if not hasattr(lib, "wf_debug_dwfctb4_probe"):
    sys.exit("the loaded library has no tb4 probe: build it with EXTRA=-DWF_DWFC2_PROBE")
buf = (ctypes.c_longlong * (16 * 8))()
assert lib.wf_debug_dwfctb4_probe(buf) == 0
# probe slots in the order they run within an iteration
NAMES = ["ph1 work", "DMA issue", "bar1 wait", "ph2 work", "DMA wait", "bar2 wait"]
SLOTS = (0, 4, 1, 2, 5, 3)
rows = sorted((buf[w * 8 + 6], w) for w in range(16))
print(f"wf_debug_dwfctb4_probe: {buf[rows[0][1] * 8 + 7]} plane iterations")
print("role  " + "  ".join(f"{n:>9}" for n in NAMES) + "   total  (cycles per plane iteration)  wave")
for role, w in rows:
    n = max(buf[w * 8 + 7], 1)
    v = [buf[w * 8 + i] / n for i in SLOTS]
    kind = "E" if role >= 12 else "D%d" % (role % 3)
    print(f"{role:3d} {kind:2s} " + "  ".join(f"{c:9.0f}" for c in v) + f"  {sum(v):7.0f}  {w:4d}",
          flush=True)
