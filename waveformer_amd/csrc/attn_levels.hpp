// attn_levels.hpp -- host side of wf_window_attention_fwd_levels: validation of the level list
// and the prefix of logical rows.  Plain C++ (no HIP), so a stand-alone host program can
// include it.
#pragma once
#include <stdint.h>

namespace wf {

constexpr int kAttnMaxLevels = 4;  // = WF_MAX_LEVELS (kernels.hpp)
constexpr int kAttnLevelsWs = 8;   // the table-bias core: window 8, head_dim 16

struct AttnLevels {
  int nlev;
  int64_t row0[kAttnMaxLevels + 1];  // first logical row of each level; row0[nlev] = all rows
  int D[kAttnMaxLevels], H[kAttnMaxLevels], W[kAttnMaxLevels];
};

// Fills L from the nlev (D, H, W) triples of dhw.  Returns NULL, or what is wrong.
inline const char* attn_levels_plan(const int64_t* dhw, int nlev, int64_t B, int64_t C,
                                    int64_t heads, AttnLevels& L) {
  if (nlev < 1 || nlev > kAttnMaxLevels) return "1 to 4 levels";
  if (dhw == nullptr) return "dhw is NULL";
  if (B < 1) return "B must be positive";
  if (heads < 1 || C != 16 * heads) return "table-bias attention needs head_dim 16 (C == 16 * heads)";
  L.nlev = nlev;
  L.row0[0] = 0;
  for (int l = 0; l < nlev; ++l) {
    const int64_t d = dhw[3 * l], h = dhw[3 * l + 1], w = dhw[3 * l + 2];
    if (d < kAttnLevelsWs || h < kAttnLevelsWs || w < kAttnLevelsWs || d % kAttnLevelsWs != 0 ||
        h % kAttnLevelsWs != 0 || w % kAttnLevelsWs != 0)
      return "every raster must tile into 8^3 windows (window_partition, wave_helper.py:459)";
    if (d > 0x7fffffff / h || d * h > 0x7fffffff / w || d * h * w > 0x7fffffff / B)
      return "a level has 2^31 rows or more";
    L.D[l] = (int)d;
    L.H[l] = (int)h;
    L.W[l] = (int)w;
    L.row0[l + 1] = L.row0[l] + B * d * h * w;
    if (L.row0[l + 1] > 0x7fffffff) return "2^31 rows or more";
  }
  return nullptr;
}

// A core launch over wh (window, head)s takes the query-pair loop, and splits the queries of a
// (window, head) over at most two workgroups, from this many on (attn_tbl_pair_loop).
constexpr int64_t kAttnPairLoopWH = 256;

// How a table-bias launch gets its q / k / v (the qkv_mode of wf_window_attention_fwd_levels_mode)
enum AttnQkvMode { ATTN_QKV_RULE = -1, ATTN_QKV_STAGED = 0, ATTN_QKV_FUSED = 1 };

// the widths the core computes q / k / v for itself (attn_tbl_kernel_fused's instantiations)
inline bool attn_qkv_fused_width(int64_t C) { return C == 48 || C == 96; }

// The rule: a table-bias inference launch over `windows` windows computes q / k / v in the core,
// without the qkv GEMM launch and its (rows, 3 C) round trip, at C = 48 when the queries of a
// (window, head) are split over at most two workgroups: each of them projects all of the window's
// K / V rows, so at a split of four (small grids) the staged GEMM stays.  C = 96 stays staged as
// well: its 6 heads x 2 query halves read every x row twelve times and the B = 8 stage-2 launch
// measured 123 us fused against 101 us for GEMM + core; the instantiation is
// there for qkv_mode 1.  The two forms are bitwise equal, so launches on either side of the rule
// agree.
inline bool attn_qkv_fused(int64_t windows, int64_t heads, int64_t C) {
  return C == 48 && windows * heads >= kAttnPairLoopWH;
}

}  // namespace wf
