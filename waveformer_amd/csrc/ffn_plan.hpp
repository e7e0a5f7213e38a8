// ffn_plan.hpp -- host side of wf_ccf_ffn_stage: the workspace layout and the dispatch plan
// (which form the LN1 + GELU takes and which kernels run the back half).  Plain C++ (no HIP),
// so a stand-alone host program can include it (tools/ffn_plan_check.cpp).
#pragma once
#include <stdint.h>

namespace wf {

constexpr int kFfnPrecBf16 = 0;  // = PREC_BF16 (kernels.hpp): the one mode with bf16 h1 / h2
constexpr bool ffn_store32(int prec) { return prec != kFfnPrecBf16; }
// the depthwise conv writes LN2 {mean, M2} partials per this many channels of every position
constexpr int DW_STAT_GROUP = 32;
// the stage-3 fc weight (192 x 768 bf16 hi + lo) rewritten per call as the 1-KB fragments the E
// waves of ffn_dwfc3_tb stream
constexpr int64_t DWFC3_FCS_BYTES = 2 * 192 * 768 * 2;

// ---- the workspace of one call over M = B * D * H * W positions: byte offsets of its areas,
// each 256-B aligned, in this order
struct FfnWorkspace {
  int64_t h1;       // (M, hidden) pwconv output, fp32 or bf16
  int64_t h2;       // (M, hidden) depthwise conv output
  int64_t ln2_pst;  // (M, hidden / 32, 2) the dwconv's {mean, M2} partials (LN2 in the fc loader)
  int64_t ln1_pst;  // the same size: the pwconv's per-column-chunk LN1 partials (<= hidden / 32)
  int64_t ln1_st;   // (M, 2) per-row LN1 {mean, rstd} (LN1 + GELU in the dwconv staging)
  int64_t fcs;      // DWFC3_FCS_BYTES at the stage-3 shape with fp32 storage, else -1 (absent)
  int64_t bytes;
};
inline int64_t ffn_align256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline bool ffn_has_fcs(int64_t C, int64_t hidden, int prec) {
  return C == 192 && hidden == 768 && ffn_store32(prec);
}
inline FfnWorkspace ffn_workspace(int64_t M, int64_t C, int64_t hidden, int prec) {
  const int64_t one = ffn_align256(M * hidden * (ffn_store32(prec) ? 4 : 2));
  const int64_t st = ffn_align256(M * (hidden / DW_STAT_GROUP) * 2 * 4);
  FfnWorkspace w;
  w.h1 = 0;
  w.h2 = one;
  w.ln2_pst = 2 * one;
  w.ln1_pst = w.ln2_pst + st;
  w.ln1_st = w.ln1_pst + st;
  const int64_t end = w.ln1_st + ffn_align256(M * 2 * 4);
  const bool fcs = ffn_has_fcs(C, hidden, prec);
  w.fcs = fcs ? end : -1;
  w.bytes = end + (fcs ? DWFC3_FCS_BYTES : 0);
  return w;
}

// ---- shape predicates
// the stage-3/4 wide-row pwconv shapes gemm_lnw takes (LayerNorm + GELU in its epilogue)
inline bool gemm_lnw_wide_shape(int64_t N, int64_t K) { return N == 768 && (K + 31) / 32 == 6; }
// The tb kernels address x, out and one h1 plane through 32-bit buffer byte offsets, and mark
// halo positions outside the volume with the offset BUF_OOR = 2^31, which must lie beyond the
// plane descriptor's range: x / out (C channels) and one haloed plane (HID channels) stay
// below 2 GiB.  (ffn_dwfc2_tb's D waves load the plane directly through such a descriptor and
// mark "outside" with a descriptor range of 0 instead.)  Larger shapes take ffn_dwfc_sb /
// ffn_dwfc2_kernel, which have no such limit, or the staged path (stage 3).
inline bool ffn_dwfc_tb4_fits(int64_t B, int64_t D, int64_t H, int64_t W) {
  return B * D * H * W * 48 * 4 < ((int64_t)1 << 31) && H * W * 192 * 4 < ((int64_t)1 << 31);
}
inline bool ffn_dwfc2_tb_fits(int64_t B, int64_t D, int64_t H, int64_t W) {
  return B * D * H * W * 96 * 4 < ((int64_t)1 << 31) && (H * W + 8) * 384 * 4 < ((int64_t)1 << 31);
}
inline bool ffn_dwfc3_tb_fits(int64_t B, int64_t D, int64_t H, int64_t W) {
  return B * D * H * W * 192 * 4 < ((int64_t)1 << 31) && (H * W + 8) * 768 * 4 < ((int64_t)1 << 31);
}

// ---- the plan
// how h1 = GELU(LN1(pwconv)) is formed
enum FfnFront {
  FFN_FRONT_EPILOGUE = 0,  // LN1 + GELU in the pwconv GEMM's epilogue
  FFN_FRONT_PASS = 1,      // plain store, then wf_ln_act_fwd in place over h1
  FFN_FRONT_PARTIALS = 2,  // LN1 partials from the epilogue + finalize; applied in the dwconv staging
  FFN_FRONT_NONE = 3,      // nothing launched: the whole-FFN kernel computes h1 on chip
};
// what runs dwconv + LN2 + GELU + fc + residual
enum FfnBack {
  FFN_BACK_FUSED = 0,         // ffn_fused: the whole FFN in one kernel (C = 48)
  FFN_BACK_DWFC_TB4 = 1,      // stage 1
  FFN_BACK_DWFC_SB = 2,       // stage 1: bf16 h1, tensors of 2 GiB and above
  FFN_BACK_DWFC2_TB = 3,      // stage 2
  FFN_BACK_DWFC2_KERNEL = 4,  // stage 2: bf16 h1, tensors of 2 GiB and above
  FFN_BACK_DWFC3_TB = 5,      // stage 3
  FFN_BACK_STAGED = 6,        // dwconv3d, then the fc GEMM with LN2 + GELU in its loader
  FFN_BACK_STAGED_DWLN = 7,   // dwconv_ln_gelu (hidden % 32 != 0), then the plain fc GEMM
};
// the environment switches as this call sees them (read in ffn.hip)
struct FfnSwitches {
  bool whole;     // WF_FFN_FUSED: the whole-FFN kernel at the stage-1 shape
  bool no_dwfc;   // WF_FFN_NO_DWFC: the staged path even where a fused back half exists
  bool ln1_fuse;  // WF_FFN_LN1_FUSE: the partials form instead of the pass
};
struct FfnPlan {
  int front, back;
  int ln1_np;  // FFN_FRONT_PARTIALS: LN1 partials per row (ffn_plan_set_kc_chunk)
};
inline bool ffn_back_fused(int back) { return back <= FFN_BACK_DWFC3_TB; }  // one kernel, no h2

// Fills p.  Returns NULL, or what is wrong.  train: the workspace keeps h1 = GELU(LN1(pwconv))
// and h2 = dwconv (pre-LN2) for the backward, so the staged path runs even where a fused back
// half exists, and LN1 + GELU is never left to the dwconv staging.
inline const char* ffn_plan(int64_t B, int64_t C, int64_t hidden, int64_t D, int64_t H, int64_t W,
                            int prec, bool train, const FfnSwitches& sw, FfnPlan& p) {
  const bool s32 = ffn_store32(prec);
  p.ln1_np = 0;
  // C = 48 / hidden = 192 (stage 1), opt-in: the whole FFN in one kernel (ffn_fused.hip), h1 and
  // h2 stay on chip.  Off by default: recomputing the 4 x 8 tile's haloed h1 plane (1.875x the
  // pw GEMM, LN1 and GELU) costs more VALU time than the h1 round trip through HBM it saves
  // 
  if (!train && sw.whole && C == 48 && hidden == 192) {
    p.front = FFN_FRONT_NONE;
    p.back = FFN_BACK_FUSED;
    return nullptr;
  }
  // wide hidden rows (stages 3 / 4: 4C = 768, 1536): a LayerNorm epilogue needs the whole row
  // in one workgroup.  gemm_lnw with 8-wave workgroups holds the 768-wide row (the columns
  // split over the waves); the 1536-wide one takes the K-chunked GEMM with a plain bias
  // epilogue, then one in-place LayerNorm + GELU row pass.
  // Opt-in instead of the pass (inference only): the pwconv epilogue writes LN1 partials, a
  // finalize pass makes the per-row {mean, rstd}, and the dwconv applies LN1 + GELU while
  // staging its planes.  It measured slower than the pass -- the depthwise conv 64 -> 130 us
  // (stage 3) and 36 -> 82 us (stage 4) against 44 / 21 us for ln_act_fwd (round 4): the
  // halo-redundant GELU on the staging lanes costs more than the h1 round trip through HBM
  const bool split_ln1 = s32 && hidden >= 768 && hidden <= 1536 && !gemm_lnw_wide_shape(hidden, C);
  p.front = !split_ln1 ? FFN_FRONT_EPILOGUE
            : !train && sw.ln1_fuse && hidden % DW_STAT_GROUP == 0 ? FFN_FRONT_PARTIALS
                                                                  : FFN_FRONT_PASS;
  // the stage-1, stage-2 and stage-3 shapes run the fused back half (h2 stays on chip); the tb
  // kernels read fp32 h1 within their 32-bit offsets.  Stage 3 has the one fused kernel.
  if (!train && !sw.no_dwfc) {
    if (C == 48 && hidden == 192) {
      p.back = s32 && ffn_dwfc_tb4_fits(B, D, H, W) ? FFN_BACK_DWFC_TB4 : FFN_BACK_DWFC_SB;
      return nullptr;
    }
    if (C == 96 && hidden == 384) {
      p.back = s32 && ffn_dwfc2_tb_fits(B, D, H, W) ? FFN_BACK_DWFC2_TB : FFN_BACK_DWFC2_KERNEL;
      return nullptr;
    }
    if (ffn_has_fcs(C, hidden, prec) && ffn_dwfc3_tb_fits(B, D, H, W)) {
      p.back = FFN_BACK_DWFC3_TB;
      return nullptr;
    }
  }
  // other shapes: the z-marching depthwise conv with LN2 + GELU moved into the fc loader, or
  // (hidden % 32 != 0) dwconv + LN fused over the full 4C row in LDS
  p.back = hidden % DW_STAT_GROUP == 0 ? FFN_BACK_STAGED : FFN_BACK_STAGED_DWLN;
  if (train && p.back != FFN_BACK_STAGED)
    return "training needs hidden % 32 == 0 (h2 kept pre-LayerNorm)";
  return nullptr;
}

// FFN_FRONT_PARTIALS: the pwconv's LN1 partials are per column chunk of gemm_kc, nt tiles of 16
// columns each (gemm_kc_pick_nt for the plain-store pwconv; 0: it does not take the shape).
// Without whole chunks per row the pass form stays.
inline void ffn_plan_set_kc_chunk(FfnPlan& p, int64_t hidden, int nt) {
  if (p.front != FFN_FRONT_PARTIALS) return;
  if (nt > 0 && hidden % (16 * nt) == 0) p.ln1_np = (int)(hidden / (16 * nt));
  else p.front = FFN_FRONT_PASS;
}

}  // namespace wf
