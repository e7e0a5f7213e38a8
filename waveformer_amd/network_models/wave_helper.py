"""Block, wavelet transform, CCF_FFN, PatchMerging and helpers.

Mirrors network_models/wave_helper.py of the reference: class names, constructor arguments,
submodule names and state_dict keys are identical.  The hot-path classes (WaveletTransform3D,
Block, CCF_FFN, PatchMerging/PatchMergingV2) run on the waveformer_amd HIP kernels; the
decoder helper ProjectionUpsample and the unused 2D helpers (DWConv, Mlp, OverlapPatchEmbed,
PosCNN, PatchEmbed) are kept as plain PyTorch modules so the reference import surface works.
"""
from __future__ import annotations

import math
import threading
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import autograd as wfa
from .. import library  # noqa: F401  (registers the torch.ops.waveformer ops)
from .. import ops
from .attention import Attention

_OPS = torch.ops.waveformer


def _conv_fan_out_init(m: nn.Module) -> None:
    if isinstance(m, (nn.Conv2d, nn.Conv3d)):
        fan_out = math.prod(m.kernel_size) * m.out_channels // m.groups
        m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
        if m.bias is not None:
            m.bias.data.zero_()


def _std_init(m: nn.Module) -> None:
    """trunc_normal(0.02) Linear, LN = (1, 0), fan-out normal conv (the reference's
    _init_weights, e.g. wave_helper.py:435-448)."""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)
    else:
        _conv_fan_out_init(m)


class DropPath(nn.Module):
    """Per-sample stochastic depth (timm semantics).  Block never calls forward(): it asks for
    the per-sample factors and hands them to the fused kernels (branch_scale)."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def sample_scale(self, batch: int, device) -> Optional[torch.Tensor]:
        if self.drop_prob == 0.0 or not self.training:
            return None
        keep = 1.0 - self.drop_prob
        return torch.empty(batch, device=device).bernoulli_(keep).div_(keep)

    def forward(self, x):
        s = self.sample_scale(x.shape[0], x.device)
        return x if s is None else x * s.view((-1,) + (1,) * (x.ndim - 1))


class ProjectionUpsample(nn.Module):
    """Decoder upsampler (wave_helper.py:33-81): trilinear x`stride` (align_corners=True, Q6) +
    depthwise 3^3 conv, GroupNorm(C, C), 1x1 conv C->2C + GELU, 1x1 projection (double conv
    with GELU for large reductions), plus an upsampled 1x1-conv residual.  Inference: HIP
    kernels (upsample_cl, dwconv3d, GroupNorm folded into the 1x1 GEMMs); training: the
    autograd Functions of autograd.py."""

    def __init__(self, in_channels, out_channels, stride=2, residual=True, use_double_conv=False):
        super().__init__()
        self.do_res = residual
        self.stride = stride
        self.use_double_conv = use_double_conv
        self.conv1 = nn.Sequential(
            nn.Upsample(scale_factor=stride, mode='trilinear', align_corners=True),
            nn.Conv3d(in_channels, in_channels, kernel_size=3, padding=1, groups=in_channels))
        self.conv2 = nn.Conv3d(in_channels, in_channels * 2, kernel_size=1)
        if use_double_conv:
            self.conv3 = nn.Sequential(nn.Conv3d(in_channels * 2, in_channels, kernel_size=1),
                                       nn.GELU(),
                                       nn.Conv3d(in_channels, out_channels, kernel_size=1))
        else:
            self.conv3 = nn.Conv3d(in_channels * 2, out_channels, kernel_size=1)
        self.norm = nn.GroupNorm(num_groups=in_channels, num_channels=in_channels)
        if residual:
            self.res_conv = nn.Sequential(
                nn.Upsample(scale_factor=stride, mode='trilinear', align_corners=True),
                nn.Conv3d(in_channels, out_channels, kernel_size=1))
        self.act = nn.GELU()

    def _wf_split_params(self):
        c3 = self.conv3
        return [c3[0].weight, c3[2].weight] if self.use_double_conv else [c3.weight]

    def _fast(self, x) -> bool:
        dw = self.conv1[1]
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 5
                and not (torch.is_grad_enabled() and (
                    x.requires_grad or any(p.requires_grad for p in self.parameters())))
                and x.shape[1] % 4 == 0 and dw.kernel_size == (3, 3, 3) and dw.padding == (1, 1, 1)
                and self.norm.num_groups == self.norm.num_channels and self.norm.affine
                and type(self.act) is nn.GELU and self.act.approximate == "none")

    def forward(self, x):
        if self._fast(x):
            return self._forward_hip(x)
        if x.is_cuda and x.dtype == torch.float32 and x.dim() == 5:
            # training on the GPU: the trilinear up-sampling (and its adjoint) on HIP, the convs
            # through wfa.conv_train (HIP depthwise, GEMM 1x1s); the residual's 1x1 conv runs
            # before its up-sampling (linear, interpolation weights sum to 1: the same function
            # and gradients)
            size = tuple(s * self.stride for s in x.shape[2:])
            cv = wfa.conv_train
            y = cv(self.conv2, wfa.group_norm_cl(self.norm,
                                                 cv(self.conv1[1], wfa.upsample_cl(x, size))))
            y = self.act(y)
            if self.use_double_conv:
                y = cv(self.conv3[2], self.conv3[1](cv(self.conv3[0], y)))
            else:
                y = cv(self.conv3, y)
            if not self.do_res:
                return y
            return y + wfa.upsample_cl(cv(self.res_conv[1], x), size)
        y = self.conv3(self.act(self.conv2(self.norm(self.conv1(x)))))
        return y + self.res_conv(x) if self.do_res else y

    def _forward_hip(self, x):
        """Inference path, channel-last: HIP trilinear upsample (align_corners=True) + HIP
        depthwise conv + HIP per-channel GroupNorm statistics; GroupNorm's normalisation and
        affine are folded into conv2's weights per sample, so conv2 / conv3 are MFMA GEMMs
        over the position rows (bf16x3) with each GELU fused into the next GEMM's loader.  The residual's 1x1 conv runs BEFORE the
        upsample (both are linear and the trilinear weights sum to 1, so W.Up(x) + b =
        Up(W.x + b)): the GEMM is 8x / 64x smaller and only Cout channels are resampled."""
        B, C, d, h, w = x.shape
        size = (d * self.stride, h * self.stride, w * self.stride)
        P = size[0] * size[1] * size[2]
        xc = ops.to_cl(x)
        dw = self.conv1[1]
        # up-sampling fused into the depthwise conv's plane staging (the 8x / 64x larger
        # up-sampled tensor is never written and re-read), GroupNorm statistics in its epilogue
        r = ops.upsample_dwconv3d_cl(xc, size, dw.weight, dw.bias, self.norm.eps)
        if r is not None:
            y, st = r
        elif dw.bias is not None and C % 32 == 0:
            up = ops.upsample_cl(xc, size, True)
            # GroupNorm(C, C) statistics accumulated in the depthwise conv's epilogue
            y, st = ops.dwconv3d_cl(up, dw.weight, dw.bias, norm_eps=self.norm.eps)
        else:
            up = ops.upsample_cl(xc, size, True)
            y = ops.dwconv3d_cl(up, dw.weight, dw.bias)
            st = ops.instnorm_stats(y, self.norm.eps)                   # (B, 2, C)
        scale = st[:, 1] * self.norm.weight                              # (B, C)
        shift = self.norm.bias - st[:, 0] * scale
        w2 = self.conv2.weight.reshape(2 * C, C)
        w2s = w2.unsqueeze(0) * scale.unsqueeze(1)                       # (B, 2C, C)
        b2s = torch.addmm(self.conv2.bias.unsqueeze(0), shift, w2.t())   # (B, 2C)
        rows = y.permute(0, 2, 3, 4, 1).reshape(B, P, C)
        # the 1x1 convs are MFMA GEMMs (wf_linear_fwd); each GELU is applied in the NEXT
        # GEMM's operand loader, so no activation tensor is written twice
        # one GEMM per sample (GroupNorm folded per sample), each into its rows of one buffer
        hid = torch.empty((B * P, 2 * C), dtype=torch.float32, device=x.device)
        for i in range(B):
            ops.linear_rows(rows[i], w2s[i], b2s[i].contiguous(), cache=False,
                            out=hid[i * P:(i + 1) * P])
        if self.use_double_conv:
            c3a, c3b = self.conv3[0], self.conv3[2]
            hid = ops.linear_rows(hid, c3a.weight, c3a.bias, gelu_in=True)
            out = ops.linear_rows(hid, c3b.weight, c3b.bias, gelu_in=True)
        else:
            c3 = self.conv3
            out = ops.linear_rows(hid, c3.weight, c3.bias, gelu_in=True)
        Cout = out.shape[1]
        out = out.view(B, size[0], size[1], size[2], Cout).permute(0, 4, 1, 2, 3)
        if self.do_res:
            rc = self.res_conv[1]
            r = ops.conv1x1_cl(xc, rc.weight, rc.bias)
            ops.upsample_add_cl(r, out, True)  # out += Up(r), in the upsample kernel
        return out


class DWConv(nn.Module):
    """2D depthwise conv on (B, N, C) tokens (wave_helper.py:86-102); unused by WaveFormer."""

    def __init__(self, dim=768):
        super().__init__()
        self.dim = dim
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)

    def forward(self, x, H, W):
        B, N, C = x.shape
        y = self.dwconv(x.transpose(1, 2).reshape(B, C, H, W))
        return y.flatten(2).transpose(1, 2)


class PatchMergingV2(nn.Module):
    """Swin patch merging (wave_helper.py:122-167): 2x2x2 gather in itertools.product order,
    LayerNorm(8C), Linear(8C -> 2C, no bias).  3D path on the HIP GEMM."""

    def __init__(self, dim: int, norm_layer=nn.LayerNorm, spatial_dims: int = 3) -> None:
        super().__init__()
        self.dim = dim
        if spatial_dims == 3:
            self.reduction = nn.Linear(8 * dim, 2 * dim, bias=False)
            self.norm = norm_layer(8 * dim)
        elif spatial_dims == 2:
            self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
            self.norm = norm_layer(4 * dim)
        self._v2 = True

    def _merge_2d(self, x):
        b, h, w, c = x.shape
        if h % 2 or w % 2:
            x = F.pad(x, (0, 0, 0, w % 2, 0, h % 2))
        x = torch.cat([x[:, j::2, i::2, :] for i in range(2) for j in range(2)], -1)
        return self.reduction(self.norm(x))

    def forward(self, x):
        if x.dim() == 4:
            return self._merge_2d(x)
        if x.dim() != 5:
            raise ValueError(f"expecting 5D x, got {tuple(x.shape)}.")
        b, d, h, w, c = x.shape
        if d % 2 or h % 2 or w % 2:  # F.pad branch of the reference (never hit by WaveFormer)
            x = F.pad(x, (0, 0, 0, w % 2, 0, h % 2, 0, d % 2))
        x = x.contiguous()
        prec = wfa.prec_for(x, *self.parameters())
        return _OPS.patch_merging(x, self.norm.weight, self.norm.bias, float(self.norm.eps),
                                  self.reduction.weight, self._v2, prec)

    def _wf_split_params(self):
        return [self.reduction.weight]


class PatchMerging(PatchMergingV2):
    """The v0.9.0 PatchMerging (wave_helper.py:170-194) with its duplicated sub-lattices
    x5 == x2 and x6 == x3 (quirk Q3) -- reproduced by the GEMM loader's gather table."""

    def __init__(self, dim: int, norm_layer=nn.LayerNorm, spatial_dims: int = 3) -> None:
        super().__init__(dim, norm_layer, spatial_dims)
        self._v2 = False


class CCF_FFN(nn.Module):
    """Convolutional channel-fusion FFN (wave_helper.py:196-294):
    x + fc(GELU(LN(dw3(GELU(LN(pw1(x))))))) on a (B, D, H, W, C) volume."""

    def __init__(self, in_features, hidden_features=None, out_features=None,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, drop=0., img_size=(48, 48, 48)):
        super().__init__()
        self.D, self.H, self.W = img_size[0], img_size[1], img_size[2]
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.C_hid = hidden_features
        self.pwconv = nn.Conv3d(in_features, hidden_features, 1, 1, 0, bias=True)
        self.dwconv = nn.Conv3d(hidden_features, hidden_features, 3, 1, 1, bias=True,
                                groups=hidden_features)
        self.fc = nn.Linear(hidden_features, in_features)
        self.act = act_layer()
        self.norm1 = norm_layer(hidden_features)
        self.norm2 = norm_layer(hidden_features)
        if not (isinstance(self.act, nn.GELU) and self.act.approximate == "none"):
            raise NotImplementedError("CCF_FFN: only nn.GELU() (erf) is implemented")
        self.apply(self._init_weights)

    def _init_weights(self, m):
        _std_init(m)

    def forward(self, x):
        B, D, H, W, C = x.shape
        assert D * H * W == self.D * self.H * self.W
        x = x.contiguous()
        return ffn_op(x, None, None, self, None)

    def _wf_split_params(self):
        return [self.pwconv.weight, self.fc.weight]

    def flops(self):
        n = self.D * self.H * self.W
        c, h = self.fc.out_features, self.C_hid
        return n * (2 * c * h + 54 * h + 2 * h * c)


def ffn_op(xh, stats, norm2, mlp: CCF_FFN, s_mlp):
    """waveformer::ccf_ffn over a Block's norm2 (stats given) or a bare CCF_FFN (stats None)."""
    n2w = n2b = None
    n2eps = 0.0
    if stats is not None:
        n2w, n2b, n2eps = norm2.weight, norm2.bias, float(norm2.eps)
    train = wfa.needs_grad(xh, *mlp.parameters(), n2w, n2b)
    prec = wfa.SPLIT if train else ops.prec_id()
    out, _ = _OPS.ccf_ffn(xh, stats, n2w, n2b, mlp.pwconv.weight, mlp.pwconv.bias,
                          mlp.norm1.weight, mlp.norm1.bias, mlp.dwconv.weight, mlp.dwconv.bias,
                          mlp.norm2.weight, mlp.norm2.bias, mlp.fc.weight, mlp.fc.bias, s_mlp,
                          n2eps, float(mlp.norm1.eps), float(mlp.norm2.eps), prec, train)
    return out


class Mlp(nn.Module):
    """Token MLP (wave_helper.py:302-341); unused by WaveFormer, plain PyTorch."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU,
                 drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        self.apply(_std_init)

    def forward(self, x, H, W):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class WaveletTransform3D(nn.Module):
    """ptwt.wavedec3 wrapper (wave_helper.py:343-353).  forward(x NCDHW, level) returns
    (LL, [dict_coarsest, ..., dict_finest]) like ptwt; Haar ('db1'/'haar', mode 'zero') runs on
    the wf_dwt3d_haar_fwd kernel.  The returned tensors have NCDHW shape and channel-last
    strides (views of the kernel's band buffers).  db2..db4 run on the NCDHW kernels of
    csrc/wavelet.hip (contiguous band views), differentiable like the Haar path."""

    def __init__(self, wavelet='db1', level=5, mode='zero'):
        super().__init__()
        self.wavelet = wavelet
        self.mode = mode

    def _check(self):
        if str(self.wavelet) not in ("db1", "haar") or self.mode != "zero":
            raise NotImplementedError(
                f"waveformer_amd: the fused channel-last path is Haar only (got {self.wavelet!r}, "
                f"mode {self.mode!r}); forward() takes db2..db4")

    def decompose_cl(self, x_cl: torch.Tensor, level: int, ln=None):
        """Channel-last variant used by Block: returns (LL (B,d,h,w,C), [band buffers] fine->coarse)."""
        self._check()
        bands = []
        cur = x_cl
        for i in range(level):
            b = ops.dwt3d_haar(cur, ln if i == 0 else None)
            bands.append(b)
            cur = b[0]
        return cur, bands

    def forward(self, x, level):
        if self.mode != "zero":
            raise NotImplementedError(f"waveformer_amd: wavelet mode {self.mode!r} not implemented")
        if str(getattr(self.wavelet, "name", self.wavelet)) not in ("db1", "haar"):
            # longer filters (config 5: db2 3-level): NCDHW per-op kernels; under autograd (or
            # a compiler's trace) a chain of waveformer::wavedec3_level ops, the same kernel
            if wfa.needs_grad(x) or torch.compiler.is_compiling():
                co = wfa.wavedec3(x, self.wavelet, level)
            else:
                co = ops.wavedec3(x, self.wavelet, level)
            return co[0], co[1:]
        self._check()
        cur = x.permute(0, 2, 3, 4, 1).contiguous()
        yh = []
        for _ in range(level):
            bands = _OPS.dwt3d(cur, None, None, 0.0).unbind(0)  # one stack in backward
            cur = bands[0]
            yh.append(ops.bands_to_coeffs(bands)[1])
        return cur.permute(0, 4, 1, 2, 3), list(reversed(yh))


# per-thread {id(Block): level-1 LL or None} of the Blocks whose hf the running encoder
# forward discards (see Block._hf_unused)
HF_SKIP = threading.local()


class Block(nn.Module):
    """Transformer block with multi-scale DWT attention (wave_helper.py:357-569)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm,
                 level=0, ms_attention=True, img_size=(48, 48, 48), network_config=None):
        super().__init__()
        self.network_config = network_config or {}
        self.dim = dim
        self.img_size = img_size
        self.mlp_ratio = mlp_ratio
        self.level = level
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.ms_attention = ms_attention
        if self.level > 0:
            self.dwt_downsamples = WaveletTransform3D(wavelet='db1', mode='zero')
        if self.ms_attention:
            self.attn_computation_level = max(self.level, 1)
        self.window_size = self.img_size[0] // pow(2, level)
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                              attn_drop=attn_drop, proj_drop=drop, window_size=self.window_size,
                              img_size=img_size)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = CCF_FFN(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer,
                           norm_layer=lambda c: nn.LayerNorm(c), drop=drop, img_size=img_size)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def window_partition(self, x, window_size):
        """(B, D, H, W, C) -> (B*nW, ws, ws, ws, C) window-major (wave_helper.py:450-461)."""
        B, D, H, W, C = x.shape
        ws = window_size
        x = x.view(B, D // ws, ws, H // ws, ws, W // ws, ws, C)
        return x.permute(0, 1, 3, 5, 2, 4, 6, 7).contiguous().view(-1, ws, ws, ws, C)

    def _branch_scales(self, B, device):
        if isinstance(self.drop_path, DropPath):
            return (self.drop_path.sample_scale(B, device), self.drop_path.sample_scale(B, device))
        return None, None

    def _prep(self, x):
        D, H, W = self.img_size
        if x.dim() != 5 or tuple(x.shape[1:4]) != (D, H, W):
            raise AssertionError(f"Block expects (B, {D}, {H}, {W}, C), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError("waveformer_amd Block computes in float32 (bf16 inside the kernels)")
        return x.contiguous()

    def forward(self, x):
        if self.ms_attention:
            return self.multi_scale_forward(x)
        return self.single_scale_forward(x)

    # MultiscaleTransformer.forward_features marks, for the duration of one call and in this
    # thread only (HF_SKIP), a Block whose detail bands it discards (every Block of a stage but
    # the last keeps none: waveformer.py:288-292): inference then runs the LL-only DWT
    # (wf_dwt3d_haar_fwd_ll) and returns no hf dicts -- and the first Block of stage 1 takes
    # its level-1 LL from the fused PatchEmbed kernel (wf_patch_embed_ll_fwd).
    @property
    def _hf_unused(self):
        return id(self) in getattr(HF_SKIP, "blocks", {})

    @property
    def _ll_given(self):
        return getattr(HF_SKIP, "blocks", {}).get(id(self))

    def _ll_levels(self, x, ln1, n):
        """n LL-only Haar levels (norm1 fused into the first): [LL], fine -> coarse."""
        lls, cur = [], x
        for i in range(n):
            if i == 0 and self._ll_given is not None:
                cur = self._ll_given
            else:
                cur = ops.dwt3d_haar_ll(cur, (ln1[0], ln1[1], float(ln1[2])) if i == 0 else None)
            lls.append(cur)
        return lls

    def _levels(self, x, ln1, n):
        """n one-level Haar DWTs (norm1 fused into the first): per level the 8 band views
        (LL first) of its band buffer, fine -> coarse.  The buffer is unbound once, so its
        gradient is assembled by one stack in backward instead of eight select-backward
        zero-fills, copies and full-buffer accumulations."""
        bands, cur = [], x
        for i in range(n):
            b = _OPS.dwt3d(cur, ln1[0] if i == 0 else None, ln1[1] if i == 0 else None,
                           float(ln1[2]) if i == 0 else 0.0).unbind(0)
            bands.append(b)
            cur = b[0]
        return bands

    def multi_scale_forward(self, x):
        """wave_helper.py:470-512.  norm1 is fused into the first DWT (or, at level 0, into
        the qkv loader); the interpolations, their sum, the shortcut and norm2's statistics
        are one msfuse kernel; norm2 + CCF_FFN + the double residual (Q4) are the FFN
        kernels' loader/epilogues.  Inference and training run the same torch.ops.waveformer
        ops (their autograd is the HIP backward), except that inference attends all LL levels
        in one launch set (Attention.forward_rasters; bitwise the per-level calls)."""
        x = self._prep(x)
        s_attn, s_mlp = self._branch_scales(x.shape[0], x.device)
        ln1 = (self.norm1.weight, self.norm1.bias, self.norm1.eps)
        hfs = None
        if self.level > 0:
            self.dwt_downsamples._check()
            n = self.attn_computation_level
            if (self._hf_unused and x.is_cuda and not torch.is_grad_enabled()
                    and not torch.compiler.is_compiling()):
                srcs = self.attn.forward_rasters(self._ll_levels(x, ln1, n))
                xh, stats = _OPS.msfuse(srcs, x, s_attn, float(self.norm2.eps), True)
                return ffn_op(xh, stats, self.norm2, self.mlp, s_mlp), ()
            bands = self._levels(x, ln1, n)
            srcs = self.attn.forward_rasters([b[0] for b in bands])
            hfs = [ops.bands_to_coeffs(b)[1] for b in bands]
        else:
            srcs = [self.attn.forward_raster(x, ln1)]
        xh, stats = _OPS.msfuse(srcs, x, s_attn, float(self.norm2.eps), True)
        out = ffn_op(xh, stats, self.norm2, self.mlp, s_mlp)
        if self.level > 0:
            return out, tuple(reversed(hfs))
        return out

    def single_scale_forward(self, x):
        """wave_helper.py:515-549: one L-level DWT, one attention pass, one interpolation."""
        x = self._prep(x)
        s_attn, s_mlp = self._branch_scales(x.shape[0], x.device)
        ln1 = (self.norm1.weight, self.norm1.bias, self.norm1.eps)
        x_h = None
        if self.level > 0:
            self.dwt_downsamples._check()
            bands = self._levels(x, ln1, self.level)
            a = self.attn.forward_raster(bands[-1][0])
            x_h = [ops.bands_to_coeffs(b)[1] for b in reversed(bands)]
        else:
            a = self.attn.forward_raster(x, ln1)
        xh, stats = _OPS.msfuse([a], x, s_attn, float(self.norm2.eps), True)
        out = ffn_op(xh, stats, self.norm2, self.mlp, s_mlp)
        if self.level > 0:
            return out, x_h
        return out

    def flops(self):
        return self.attn.flops() + self.mlp.flops()


class OverlapPatchEmbed(nn.Module):
    """2D overlapping patch embedding (wave_helper.py:571-613); unused by WaveFormer."""

    def __init__(self, patch_size=7, stride=4, in_chans=3, embed_dim=768):
        super().__init__()
        ps = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.patch_size = ps
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=ps, stride=stride,
                              padding=(ps[0] // 2, ps[1] // 2))
        self.norm = nn.LayerNorm(embed_dim)
        self.apply(_std_init)

    def forward(self, x):
        x = self.proj(x)
        _, _, H, W = x.shape
        return self.norm(x.flatten(2).transpose(1, 2)), H, W


class PatchEmbed(nn.Module):
    """Token patch embedding (wave_helper.py:615-688); unused by WaveFormer (which uses the
    MONAI PatchEmbed), plain PyTorch."""

    def __init__(self, img_size=(96, 96, 96), patch_size=2, in_chans=1, embed_dim=48,
                 use_conv_embed=False, norm_layer=None, use_pre_norm=False, is_stem=False):
        super().__init__()
        self.img_size, self.patch_size = img_size, patch_size
        self.patches_resolution = [s // patch_size for s in img_size]
        self.num_patches = math.prod(self.patches_resolution)
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.use_pre_norm, self.use_conv_embed = use_pre_norm, use_conv_embed
        if use_conv_embed:
            k, p, s = (7, 2, 4) if is_stem else (3, 1, 2)
            self.kernel_size = k
            self.proj = nn.Conv3d(in_chans, embed_dim, kernel_size=k, stride=s, padding=p)
        else:
            self.proj = nn.Conv3d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        if use_pre_norm:
            self.pre_norm = nn.GroupNorm(1, in_chans) if norm_layer is not None else None
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        if self.use_pre_norm and self.pre_norm is not None:
            x = self.pre_norm(x)
        x = self.proj(x)
        _, _, D, H, W = x.shape
        x = x.flatten(2).transpose(1, 2).contiguous()
        if self.norm is not None:
            x = self.norm(x)
        return x, D, H, W


class PosCNN(nn.Module):
    """2D conditional position encoding (wave_helper.py:690-709); unused by WaveFormer."""

    def __init__(self, in_chans, embed_dim=768, s=1):
        super().__init__()
        self.proj = nn.Sequential(nn.Conv2d(in_chans, embed_dim, 3, s, 1, groups=embed_dim),
                                  nn.GELU(), nn.Conv2d(embed_dim, embed_dim, 1, 1, 0))
        self.s = s

    def forward(self, x, H, W):
        B, N, C = x.shape
        feat = x.transpose(1, 2).view(B, C, H, W)
        y = self.proj(feat) + feat if self.s == 1 else self.proj(feat)
        return y.flatten(2).transpose(1, 2)

    def no_weight_decay(self):
        return ['proj.%d.weight' % i for i in range(4)]
