"""IDWT decoder block.

Mirrors network_models/idwt_upsample.py (HFRefinementRes :12-50, UnetrIDWTBlock :53-166):
same constructor and state_dict keys.  HFRefinementRes runs as one fused HIP call per level:
ops.hf_refine at inference, waveformer::hf_refine with its fused HIP backward under autograd
(the per-tensor module forward remains for CPU tensors, unsupported shapes and direct calls).
The wavelet synthesis (ptwt.waverec3, :160) and the
concatenation with the skip (:163) run as one wf_idwt3d_haar launch that writes straight into
the first half of the concatenated buffer (with the skip in the same kernel,
wf_idwt3d_haar_cl_cat); the surrounding convolutions run on the HIP conv3d_k3 kernel and the
fused InstanceNorm + LeakyReLU passes (blocks.py).  Wavelets other than Haar (db2..db4) run
one wf_idwt3d_level launch per level; under autograd both take their registered ops
(waveformer::idwt3d, waveformer::waverec3_level) and torch.cat.
"""
from __future__ import annotations

from typing import Any, Dict, Sequence, Tuple, Union

import torch
import torch.nn as nn

from .. import autograd as wfa
from .. import ops
from ..blocks import UnetBasicBlock, UnetResBlock, get_conv_layer


class HFRefinementRes(nn.Module):
    """x * sigmoid(conv1(relu(IN(dwconv3(x)))))  -- filters high-frequency coefficients."""

    def __init__(self, in_channels, init_alpha=0.3, network_config=None):
        super().__init__()
        self.network_config = network_config or {}
        hf_config = self.network_config.get('hf_refinement', {})
        self.conv1 = nn.Conv3d(in_channels, in_channels, kernel_size=3, padding=1,
                               groups=in_channels, bias=True)
        self.norm = nn.InstanceNorm3d(in_channels, affine=True)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv3d(in_channels, in_channels, kernel_size=1, bias=True)
        self.sigmoid = nn.Sigmoid() if hf_config.get('use_sigmoid', True) else None

    def train_ok(self, x) -> bool:
        """The fused HIP kernels (wf_hf_refine_fwd / _bwd) cover this module: depthwise 3^3
        conv with bias, InstanceNorm3d(affine, no running stats), 1x1 conv with bias."""
        c1, n, c2 = self.conv1, self.norm, self.conv2
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 5
                and x.shape[1] % 4 == 0 and x.shape[1] <= 256
                and c1.kernel_size == (3, 3, 3) and c1.padding == (1, 1, 1)
                and c1.groups == c1.in_channels and c1.bias is not None
                and n.affine and not n.track_running_stats
                and c2.kernel_size == (1, 1, 1) and c2.bias is not None)

    def fast_ok(self, x) -> bool:
        """train_ok with nothing to differentiate: the inference path (ops.hf_refine)."""
        return (not (torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad for p in self.parameters())))
                and self.train_ok(x))

    def forward(self, x):
        # the convs through wfa.conv_train (HIP depthwise, GEMM 1x1; modules for CPU tensors)
        cv = wfa.conv_train
        r = cv(self.conv2, self.relu(self.norm(cv(self.conv1, x))))
        if self.sigmoid is not None:
            r = self.sigmoid(r)
        return x * r


class UnetrIDWTBlock(nn.Module):
    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, stage: int,
                 hf_refinement: bool, wavelet: str, kernel_size: Union[Sequence[int], int],
                 norm_name: Union[Tuple, str], res_block: bool = False,
                 network_config: Dict[str, Any] = None) -> None:
        super().__init__()
        self.network_config = network_config or {}
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.wavelet = wavelet
        self.hf_refinement = hf_refinement
        if self.hf_refinement:
            self.hf_ref = nn.ModuleList([
                HFRefinementRes(in_channels // pow(2, stage), network_config=self.network_config)
                for _ in range(stage)])
        self.conv_lf_block = get_conv_layer(spatial_dims, in_channels, out_channels,
                                            kernel_size=kernel_size, stride=1, conv_only=True)
        cls = UnetResBlock if res_block else UnetBasicBlock
        self.conv_block = cls(spatial_dims, out_channels * 2, out_channels,
                              kernel_size=kernel_size, stride=1, norm_name=norm_name)

    def forward(self, inp, skip, hf_coeffs):
        inp = self.conv_lf_block(inp)
        if self.hf_refinement:
            # the 7 details of a level in one fused HIP call: ops.hf_refine at inference,
            # waveformer::hf_refine (fused backward) under autograd
            hf_coeffs = tuple(
                ops.hf_refine(d, self.hf_ref[i]) if self.hf_ref[i].fast_ok(d["aad"])
                else wfa.hf_refine(d, self.hf_ref[i])
                if torch.is_grad_enabled() and self.hf_ref[i].train_ok(d["aad"])
                else {k: self.hf_ref[i](d[k]) for k in d}
                for i, d in enumerate(hf_coeffs))
        wname = str(getattr(self.wavelet, "name", self.wavelet))
        if wname not in ("db1", "haar"):
            # longer filters (config 5): one wf_idwt3d_level launch per level, the finest
            # written into the concatenation buffer
            shp = hf_coeffs[-1]["aad"].shape
            size = tuple(2 * n - len(ops.WAVELETS[wname][0]) + 2 for n in shp[2:])
            B, C = inp.shape[:2]
            if skip.shape[0] != B or tuple(skip.shape[2:]) != size:
                raise ValueError(f"skip {tuple(skip.shape)} does not match the IDWT output "
                                 f"{(B, C) + size}")
            if torch.is_grad_enabled() and (inp.requires_grad or any(
                    t.requires_grad for d in hf_coeffs for t in d.values())):
                # training: a chain of waveformer::waverec3_level ops (HIP backward)
                out = wfa.waverec3((inp,) + tuple(hf_coeffs), wname)
                return self.conv_block(torch.cat((out, skip), dim=1))
            buf = torch.empty((B, C + skip.shape[1]) + size, dtype=inp.dtype, device=inp.device)
            ops.waverec3((inp,) + tuple(hf_coeffs), self.wavelet, out=buf[:, :C])
            buf[:, C:].copy_(skip)
            return self.conv_block(buf)
        B, C = inp.shape[:2]
        L = len(hf_coeffs)
        size = tuple(s * 2 ** L for s in inp.shape[2:])
        if skip.shape[0] != B or tuple(skip.shape[2:]) != size:
            raise ValueError(f"skip {tuple(skip.shape)} does not match the IDWT output {(B, C) + size}")
        if torch.is_grad_enabled() and (inp.requires_grad or skip.requires_grad or any(
                t.requires_grad for d in hf_coeffs for t in d.values())):
            out = wfa.idwt3d_haar(inp, hf_coeffs)
            return self.conv_block(torch.cat((out, skip), dim=1))
        # channel-last: the layout the conv_block's kernels read, so neither the IDWT output nor
        # the concatenation is converted again (round 2 built it NCDHW: two full-resolution
        # layout copies per decoder level)
        buf = ops.empty_cl(B, C + skip.shape[1], *size, inp.device)
        if skip.shape[1] == C:  # IDWT into [0, C) and torch.cat((out, skip), 1) in one pass
            ops.idwt3d_haar(inp, hf_coeffs, out=buf, skip=skip)
        else:
            ops.idwt3d_haar(inp, hf_coeffs, out=buf)   # channels [0, C)
            ops.copy_cl(skip, buf[:, C:])               # torch.cat((out, skip), 1)
        return self.conv_block(buf)
