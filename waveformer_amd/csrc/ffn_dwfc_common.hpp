// ffn_dwfc_common.hpp -- what the CCF_FFN back-half kernels share (ffn_dwfc.hip: ffn_dwfc_sb,
// ffn_dwfc2; ffn_dwfc_tb.hip: ffn_dwfc_tb4; ffn_dwfc2_tb.hip: ffn_dwfc2_tb; ffn_dwfc3_tb.hip:
// ffn_dwfc3_tb; ffn_fused.hip):
// the argument block and launchers, the tile decode, the wave roles, the LN2 row, the bf16x3
// MFMA step, the staging of the small vectors, the epilogue expression and the buffer
// descriptors.  The helpers are parameterised by geometry only.  Not here, on purpose: the
// depthwise scatter chains, the plane loaders, the barrier sequences and the ZS pickers --
// those ARE the kernels (each file reads as its schedule), and they differ where it was measured.
#pragma once
#include "kernels.hpp"

namespace wf {

// ---- CCF_FFN back half fused: dwconv + bias + LN2 + GELU + fc + bias + the Block's Q4
// residual, for C = 48, hidden = 192, C = 96, hidden = 384 and C = 192, hidden = 768 (h1 fp32
// for PREC_SPLIT / PREC_FP16, bf16 for PREC_BF16)
struct DwFcArgs {
  const void* h1;        // (B, D, H, W, HID) fp32 (SPLIT) or bf16
  const float* dw_w;     // (HID, 27)
  const float* dw_b;     // (HID)
  const float* ln2_w;    // (HID)
  const float* ln2_b;
  float eps2;
  const uint16_t* fc;    // [2][C][HID] bf16 {hi, lo}
  const float* fc_b;     // (C) or NULL
  const float* x;        // (B, D, H, W, C) residual rows
  const float* stats;    // (M, 2) {mean, rstd} of x for norm2, or NULL
  const float* n2_w;
  const float* n2_b;
  const float* bscale;   // (B) or NULL
  float* out;            // (B, D, H, W, C)
  int B, D, H, W, ZS;
  // whole-FFN kernel (ffn_fused.hip) only: the front half, recomputed on chip from x
  const uint16_t* pw;    // [2][HID][C] bf16 {hi, lo}
  const float* pw_b;     // (HID) or NULL
  const float* ln1_w;    // (HID)
  const float* ln1_b;
  float eps1;
  int dbg;               // timing experiments only (builds with WF_FFN_DBG=1): phases skipped
  // ffn_dwfc3_tb only: DWFC3_FCS_BYTES of workspace (FfnWorkspace::fcs, ffn_plan.hpp) for the
  // fc weight in stream order
  uint16_t* fcs;
};
#ifndef WF_FFN_DBG  // 1: timing-experiment build (DwFcArgs::dbg phase skips; never the shipped library)
#define WF_FFN_DBG 0
#endif
// the phases a kernel skips: none unless the build has WF_FFN_DBG=1 (results are then invalid)
__device__ __forceinline__ int ffn_dbg(const DwFcArgs& a) { return WF_FFN_DBG ? a.dbg : 0; }
inline int ffn_dbg_env() {
  return WF_FFN_DBG && getenv("WF_FFN_DBG") ? atoi(getenv("WF_FFN_DBG")) : 0;
}

// ---- launchers.  Which of them a call takes is ffn_plan's decision (ffn_plan.hpp, FfnBack):
// the tb kernels read fp32 h1 within their 32-bit offsets (ffn_dwfc*_tb_fits, there), and
// their launchers refuse anything else.
// stage-1 shape, three VALU waves per SIMD on 4 x 8 tiles, two barriers per plane
// (ffn_dwfc_tb.hip)
int launch_ffn_dwfc_tb4(const DwFcArgs& a, int prec, hipStream_t s);
// stage-1 shape, SIMD-balanced roles (ffn_dwfc.hip): any precision, no size limit
int launch_ffn_dwfc_sb(const DwFcArgs& a, int prec, hipStream_t s);
// C = 96, hidden = 384 on 4 x 4 tiles; picks ZS.  tb: ffn_dwfc2_tb (three depthwise waves + one
// fc wave per SIMD, depthwise inputs loaded straight into registers, two h2 tiles and the fc
// weight hi in LDS), else ffn_dwfc2_kernel (any precision, no size limit)
int launch_ffn_dwfc2(const DwFcArgs& a, int prec, bool tb, hipStream_t s);
// ffn_dwfc2_tb.hip; ZS set by the caller
int launch_ffn_dwfc2_tb(const DwFcArgs& a, int prec, hipStream_t s);
// the stage-3 shape, C = 192, hidden = 768, fp32 h1 (ffn_dwfc3_tb.hip): 4 x 4 tiles, direct
// depthwise loads, three h2 tiles in LDS, the fc weight streamed from L2 into registers; sets
// ZS.  Only where ffn_dwfc3_tb_fits: the plan keeps the staged path for the rest
int launch_ffn_dwfc3(const DwFcArgs& a, int prec, hipStream_t s);
// ---- the whole CCF_FFN + norm2 + Q4 residual in one kernel for C = 48, hidden = 192: the
// haloed h1 plane is computed in LDS from the x rows (pw MFMA + LN1 + GELU), never stored
int launch_ffn_fused(const DwFcArgs& a, int prec, hipStream_t s);

// h1 plane staging: fp32 (SPLIT / FP16 workspaces) or bf16 (BF16) rows widened to fp32
template <typename T>
struct H1Load;
template <>
struct H1Load<float> {
  typedef f32x4 raw;
  static __device__ __forceinline__ raw load(const float* p, int64_t i) {
    return *reinterpret_cast<const f32x4*>(p + i);
  }
  static __device__ __forceinline__ f32x4 up(raw u) { return u; }
};
template <>
struct H1Load<uint16_t> {
  typedef bf16x4 raw;
  static __device__ __forceinline__ raw load(const uint16_t* p, int64_t i) {
    return *reinterpret_cast<const bf16x4*>(p + i);
  }
  static __device__ __forceinline__ f32x4 up(raw u) {
    return f32x4{bf2f((uint16_t)u[0]), bf2f((uint16_t)u[1]), bf2f((uint16_t)u[2]),
                 bf2f((uint16_t)u[3])};
  }
};

// ---- diagnostic builds only (-DWF_DWFC2_PROBE; ffn_dwfc_sb, ffn_dwfc2, ffn_dwfc_tb4 and
// ffn_dwfc2_tb): per-wave cycles of workgroup 0 by phase between the kernel's barriers, 8 slots
// per wave
#ifdef WF_DWFC2_PROBE
#define PROBE_DECL                                                              \
  const bool probe_on = blockIdx.x == 0;                                         \
  long long pr_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pr_last = __builtin_amdgcn_s_memtime();
#define PROBE(i)                                                                \
  if (probe_on) {                                                               \
    const long long t_ = __builtin_amdgcn_s_memtime();                          \
    pr_acc[i] += t_ - pr_last;                                                  \
    pr_last = t_;                                                               \
  }
#define PROBE_DUMP_TO(arr)                                                      \
  if (probe_on && (tid & 63) == 0)                                              \
    for (int i_ = 0; i_ < 8; ++i_) arr[wid * 8 + i_] = pr_acc[i_];
#else
#define PROBE_DECL
#define PROBE(i)
#define PROBE_DUMP_TO(arr)
#endif

// ---- buffer descriptors: raw (untyped, stride 0) buffers of `bytes` bytes at p; loads from
// byte offsets at or beyond `bytes` return zeros, stores there are dropped.  BUF_OOR is the
// offset the kernels use for "outside": beyond every descriptor the launchers admit.
constexpr int BUF_OOR = (int)0x80000000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// ---- the workgroup's tile: (y0, x0) corner of its TY x TX tile, z segment [z0, z1) of ZS
// planes, sample b.  XCD-contiguous order (xcd_block_id): each XCD gets a contiguous run of
// (z, y, x) tiles -- neighbouring tiles share halo rows and meet in that XCD's L2.
struct DwFcTile {
  int b, x0, y0, z0, z1;
};
template <int TY, int TX>
__device__ __forceinline__ DwFcTile dwfc_tile(const DwFcArgs& a) {
  const int ntx = (a.W + TX - 1) / TX, nty = (a.H + TY - 1) / TY, nzs = (a.D + a.ZS - 1) / a.ZS;
  int t = xcd_block_id();
  const int xt = t % ntx;
  t /= ntx;
  const int yt = t % nty;
  t /= nty;
  const int zt = t % nzs;
  DwFcTile o;
  o.b = t / nzs;
  o.x0 = xt * TX;
  o.y0 = yt * TY;
  o.z0 = zt * a.ZS;
  o.z1 = min(o.z0 + a.ZS, a.D);
  return o;
}

// HW_ID (hwreg 4) bits [5:4]: the SIMD the wave runs on
__device__ __forceinline__ int tb_simd_id() {
  return (int)((__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4)) & 3);
}
// ---- wave roles by SIMD arrival slot, for workgroups of 4 * WPS waves: the waves of a SIMD
// take its slots 0 .. WPS - 1 first come first served, so every SIMD carries the same mix of
// roles wherever the dispatcher placed the waves.  Slots 0 .. WPS - 2 are the worker (D) waves
// (WPS - 1) * simd + slot, slot WPS - 1 is the special (E) wave 4 * (WPS - 1) + simd.  If a SIMD
// did not get exactly WPS waves the roles fall back to wave-id order (still correct, just
// unbalanced).  simd_cnt[4] (LDS) must have been zeroed behind a barrier; the one barrier
// between the atomics and the reads of simd_cnt is in here.  The result is wave-uniform.
template <int WPS>
__device__ __forceinline__ int dwfc_wave_role(int* simd_cnt, int wid, int lane) {
  const int simd = tb_simd_id();
  int slot = 0;
  if (lane == 0) slot = atomicAdd(&simd_cnt[simd], 1);
  slot = __builtin_amdgcn_readfirstlane(__shfl(slot, 0, 64));
  __syncthreads();
  const bool even = simd_cnt[0] == WPS && simd_cnt[1] == WPS && simd_cnt[2] == WPS && simd_cnt[3] == WPS;
  const int role = even ? (slot < WPS - 1 ? (WPS - 1) * simd + slot : 4 * (WPS - 1) + simd) : wid;
  return __builtin_amdgcn_readfirstlane(role);
}

// ---- staging of the small vectors into LDS by the whole workgroup (nthreads threads)
// LN2 affine, halved: GELU is evaluated from x / 2 (gelu_half4)
template <int HID>
__device__ __forceinline__ void dwfc_stage_ln2(float* lnw, float* lnb, const DwFcArgs& a,
                                               int nthreads) {
  for (int i = threadIdx.x; i < HID; i += nthreads) {
    lnw[i] = 0.5f * a.ln2_w[i];
    lnb[i] = 0.5f * a.ln2_b[i];
  }
}
// fc bias and norm2 affine (identity without norm2 statistics): dwfc_epilogue's vectors
template <int C>
__device__ __forceinline__ void dwfc_stage_epi(float* fcb, float* n2w, float* n2b,
                                               const DwFcArgs& a, int nthreads) {
  for (int i = threadIdx.x; i < C; i += nthreads) {
    fcb[i] = a.fc_b ? a.fc_b[i] : 0.f;
    n2w[i] = a.stats ? a.n2_w[i] : 1.f;
    n2b[i] = a.stats ? a.n2_b[i] : 0.f;
  }
}

// ---- LN2 + GELU + operand split of one h2 row of HID fp32 channels, by LANES consecutive
// lanes of 12 channels each: the lane's channel quads lie at q0 + STRIDE * j (j = 0, 1, 2).
// The row is rewritten in place as bf16 (or fp16) {hi[HID], lo[HID]} (lo for PREC_SPLIT only):
// the lanes of a row are one group of one wave, so all its reads precede its writes.
// Short dependency chains: three-way column sums (depth 3 + 2 instead of 12), four variance
// partials.  RAW_RSQ: the raw v_rsq_f32 (var + eps >= eps is a normal number) instead of
// rsqrtf -- an arithmetic difference between the kernels that is kept as it is.
template <int P, int HID, int LANES, int STRIDE, bool RAW_RSQ>
__device__ __forceinline__ void dwfc_ln2_row(float* row, int q0, const float* lnw,
                                             const float* lnb, float eps) {
  static_assert(HID == 12 * LANES, "12 channels per lane");
  float v[12];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(row + q0 + STRIDE * j);
    v[4 * j] = u.x;
    v[4 * j + 1] = u.y;
    v[4 * j + 2] = u.z;
    v[4 * j + 3] = u.w;
  }
  float s4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) s4[j] = (v[j] + v[j + 4]) + v[j + 8];
  const float mean = group_sum<LANES>((s4[0] + s4[1]) + (s4[2] + s4[3])) * (1.f / HID);
  float q4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float d0 = v[j] - mean, d1 = v[j + 4] - mean, d2 = v[j + 8] - mean;
    q4[j] = d2 * d2 + (d1 * d1 + d0 * d0);
  }
  const float var = group_sum<LANES>((q4[0] + q4[1]) + (q4[2] + q4[3])) * (1.f / HID) + eps;
  const float rstd = RAW_RSQ ? __builtin_amdgcn_rsqf(var) : rsqrtf(var);
  const float nmr = -mean * rstd;
  uint16_t* rowh = reinterpret_cast<uint16_t*>(row);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int cc = q0 + STRIDE * j;
    const f32x4 lw4 = *reinterpret_cast<const f32x4*>(lnw + cc);
    const f32x4 lb4 = *reinterpret_cast<const f32x4*>(lnb + cc);
    const f32x4 y = gelu_half4((f32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]} *
                                rstd + nmr) * lw4 + lb4);
    uint32_t h0, h1, l0, l1;
    split_pair<P>(y[0], y[1], h0, l0);
    split_pair<P>(y[2], y[3], h1, l1);
    *reinterpret_cast<u32x2*>(rowh + cc) = u32x2{h0, h1};
    if (P == PREC_SPLIT) *reinterpret_cast<u32x2*>(rowh + HID + cc) = u32x2{l0, l1};
  }
}

// ---- the epilogue of four output channels col .. col + 3 of one position:
//   out = x + (n2 + fc + fc_b) * bs,  n2 = (x - mean) * rstd * n2_w + n2_b  (the Block form:
// norm2 + quirk Q4's double residual), or out = x + (fc + fc_b) * bs for a bare CCF_FFN.
// fcb, n2w, n2b: the vectors dwfc_stage_epi staged; ev = norm2's {mean, rstd} of the row.
__device__ __forceinline__ f32x4 dwfc_epilogue(f32x4 acc, const float* fcb, const float* n2w,
                                               const float* n2b, int col, f32x4 xv, f32x2 ev,
                                               float bs, bool has_stats) {
  const f32x4 v = acc + *reinterpret_cast<const f32x4*>(fcb + col);
  if (!has_stats) return xv + v * bs;
  const f32x4 nw = *reinterpret_cast<const f32x4*>(n2w + col);
  const f32x4 nb = *reinterpret_cast<const f32x4*>(n2b + col);
  const f32x4 n2 = (xv - ev.x) * ev.y * nw + nb;
  return xv + (n2 + v) * bs;
}

}  // namespace wf
