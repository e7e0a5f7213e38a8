// attn_plan.hpp -- host side of the window attention (wf_window_attention_fwd*): the level list
// and its row prefix, the workspace layout, the thresholds of the dispatch and the plan of a call
// (DESIGN.md 6.26).  Plain C++ (no HIP), so a stand-alone host program can include it
// (tools/attn_plan_check.cpp).
#pragma once
#include <stdint.h>

namespace wf {

constexpr int kAttnMaxLevels = 4;  // = WF_MAX_LEVELS (kernels.hpp)
constexpr int kAttnLevelsWs = 8;   // the table-bias core: window 8, head_dim 16
constexpr int kQB = 64;            // the dense-bias core: queries per workgroup (16 per wave)

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

// ---- the workspace of a forward over `rows` tokens: byte offsets of qkv (rows, 3 C) and of the
// core's output (rows, C), both in the precision's activation storage (fp32 but for precision 0,
// PREC_BF16) and 256-B aligned
struct AttnWorkspace {
  int64_t qkv, ao, bytes;
};
inline int64_t attn_align256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline AttnWorkspace attn_workspace(int64_t rows, int64_t C, int prec) {
  const int64_t e = prec != 0 ? 4 : 2;
  const int64_t ao = attn_align256(rows * 3 * C * e);
  return {0, ao, ao + attn_align256(rows * C * e)};
}

// ---- the thresholds of the dispatch
// The table-bias core splits the queries of one (window, head) over 1, 2 or 4 workgroups: enough
// workgroups for two per CU, each staging the window's K / V once.  A launch over wh (window,
// head)s splits them over at most two from kAttnPairLoopWH on and not at all from kAttnNoSplitWH
// on.  A workgroup with kAttnPairNsub or more 16-query sub-tiles (a split of at most two) walks
// them two at a time (the query-pair loop, NQ = 2), the others one at a time (NQ = 1); the two
// loops differ in fp32 rounding (attn_tbl_tiles).
constexpr int64_t kAttnPairLoopWH = 256;
constexpr int64_t kAttnNoSplitWH = 512;
constexpr int kAttnPairNsub = 16;
// the widths the core computes q / k / v for itself (attn_tbl_kernel_fused's instantiations)
constexpr int kAttnFusedWidths[2] = {48, 96};

// How a table-bias launch gets its q / k / v (the qkv_mode of wf_window_attention_fwd_levels_mode)
enum AttnQkvMode { ATTN_QKV_RULE = -1, ATTN_QKV_STAGED = 0, ATTN_QKV_FUSED = 1 };

// The rule: a table-bias inference launch over `windows` windows computes q / k / v in the core,
// without the qkv GEMM launch and its (rows, 3 C) round trip, at C = 48 when the queries of a
// (window, head) are split over at most two workgroups: each of them projects all of the window's
// K / V rows, so at a split of four (small grids) the staged GEMM stays.  C = 96 stays staged as
// well: its 6 heads x 2 query halves read every x row twelve times and the B = 8 stage-2 launch
// measured 123 us fused against 101 us for GEMM + core; the instantiation is
// there for qkv_mode 1.  The two forms are bitwise equal, so launches on either side of the rule
// agree.
inline bool attn_qkv_fused(int64_t windows, int64_t heads, int64_t C) {
  return C == kAttnFusedWidths[0] && windows * heads >= kAttnPairLoopWH;
}

// ---- the plan
// what a call is (the flags of wf_window_attention_plan, and ATTN_ALIGNED)
enum AttnFlags {
  ATTN_TABLE = 1,     // the bias is the (T, heads) table, else the dense (heads, N, N) one
  ATTN_LN = 2,        // a LayerNorm in the qkv loader
  ATTN_LSE = 4,       // training: the core also writes the log-sum-exp
  ATTN_RASTER = 8,    // one raster of any window and head_dim (_fwd, _fwd_table, _fwd_train)
  ATTN_ALIGNED = 16,  // every source is 16-byte aligned
};
// how the levels are grouped into launch sets (qkv GEMM or nothing, core, proj GEMM)
enum AttnGrouping {
  ATTN_MERGED = 0,  // one set over all levels, their rows gathered by MAP_LEVELS
  // a set per level (rows gathered by MAP_WINDOW) into the same output and workspace, because:
  ATTN_PER_LEVEL_NO_GEMM = 1,  // no multi-level GEMM instantiation takes this width
  ATTN_PER_LEVEL_PREFIX = 2,   // a level on the one-sub-tile loop ahead of one on the pair loop
  ATTN_PER_LEVEL_RASTER = 3,   // the call is one raster, not a level list
};
struct AttnSet {
  int64_t rows;          // its logical rows, from L.row0 of its first level on
  int64_t ao;            // byte offset of its core output in the workspace (its qkv: offset 0)
  bool fused;            // q / k / v computed in the core: no qkv GEMM launch and no qkv write
  int64_t wh;            // its (window, head)s
  int qsplit;            // table core: workgroups per (window, head), 1 / 2 / 4 (dense: 0)
  int64_t pair_windows;  // table core: its first windows that may take the query-pair loop
  int64_t grid;          // workgroups of the core launch
};
struct AttnPlan {
  AttnLevels L;
  int64_t B, C, heads, ws;
  int prec;
  bool table;  // the core: table bias, else dense bias at head_dim
  int head_dim;
  int grouping;  // AttnGrouping
  int nsets;     // 1 (merged), or nlev: set i is level i
  AttnSet set[kAttnMaxLevels];
  int nq[kAttnMaxLevels];  // table core: the tile loop each level takes, NQ = 1 or 2 (dense: 0)
  AttnWorkspace work;      // of the whole call
};

// Fills p.  Returns NULL, or what is wrong.  levels_gemm(rows): whether gemm_rows or gemm_kc takes
// the merged qkv GEMM (MAP_LEVELS) over that many rows -- the one input this header cannot
// compute; asked only where the answer decides.
template <class LevelsGemm>
inline const char* attn_plan(const int64_t* dhw, int nlev, int64_t B, int64_t C, int64_t heads,
                             int64_t ws, int prec, int flags, int qkv_mode,
                             LevelsGemm&& levels_gemm, AttnPlan& p) {
  const bool table = flags & ATTN_TABLE, raster = flags & ATTN_RASTER;
  if (qkv_mode < ATTN_QKV_RULE || qkv_mode > ATTN_QKV_FUSED)
    return "qkv_mode: -1 (the rule), 0 (staged) or 1 (q/k/v in the core)";
  AttnLevels& L = p.L;
  if (!raster) {
    if (flags != (ATTN_TABLE | ATTN_ALIGNED) && flags != ATTN_TABLE)
      return "a level list takes the table bias, no LayerNorm, inference";
    if (ws != kAttnLevelsWs) return "table-bias attention is implemented for window 8 and head_dim 16";
    if (const char* why = attn_levels_plan(dhw, nlev, B, C, heads, L)) return why;
    if (!(flags & ATTN_ALIGNED)) return "level sources must be 16-byte aligned";
  } else {
    if (nlev != 1 || dhw == nullptr) return "one raster is one (D, H, W)";
    const int64_t d = dhw[0], h = dhw[1], w = dhw[2];
    if (!(B >= 1 && C >= 8 && C % 8 == 0)) return "C must be a positive multiple of 8";
    if (!(ws >= 1 && d % ws == 0 && h % ws == 0 && w % ws == 0))
      return "the raster must tile into ws^3 windows (window_partition, wave_helper.py:459)";
    if (!(heads >= 1 && C % heads == 0)) return "dim must be divisible by num_heads";
    if (table && (ws != kAttnLevelsWs || C != 16 * heads))
      return "table-bias attention is implemented for window 8 and head_dim 16";
    if (table && (flags & ATTN_LSE)) return "attention (table bias): inference only, no log-sum-exp";
    L = AttnLevels{1, {0, B * d * h * w}, {(int)d}, {(int)h}, {(int)w}};
  }
  const int64_t N = ws * ws * ws, rows = L.row0[L.nlev];
  p.B = B, p.C = C, p.heads = heads, p.ws = ws, p.prec = prec;
  p.table = table;
  p.head_dim = (int)(C / heads);
  p.work = attn_workspace(rows, C, prec);
  // the table-bias core without a LayerNorm in the loader may compute q / k / v itself
  const bool can_fuse = (flags & ~ATTN_RASTER) == (ATTN_TABLE | ATTN_ALIGNED) && rows > 0 && rows <= 0x7fffffff;
  if (qkv_mode == ATTN_QKV_FUSED && !can_fuse)
    return "window attention: q/k/v in the core needs the table bias (ws 8, head_dim 16), "
           "inference, no LayerNorm in the loader";
  if (qkv_mode == ATTN_QKV_FUSED && C != kAttnFusedWidths[0] && C != kAttnFusedWidths[1])
    return "window attention: q/k/v in the core is instantiated for C = 48 and 96";
  auto fused = [&](int64_t r) {
    return can_fuse && (qkv_mode == ATTN_QKV_FUSED ||
                        (qkv_mode == ATTN_QKV_RULE && attn_qkv_fused(r / N, heads, C)));
  };
  // the loop each level's own launch takes: a merged launch keeps it per level (pair_windows), so
  // the levels on the query-pair loop must come first
  int64_t pair_windows = 0;
  bool prefix = true;
  for (int l = 0; l < L.nlev; ++l)
    if ((L.row0[l + 1] - L.row0[l]) / N * heads >= kAttnPairLoopWH) {
      prefix = prefix && pair_windows == L.row0[l] / N;
      pair_windows = L.row0[l + 1] / N;
    }
  p.grouping = raster                                ? ATTN_PER_LEVEL_RASTER
               : !prefix                             ? ATTN_PER_LEVEL_PREFIX
               : !fused(rows) && !levels_gemm(rows)  ? ATTN_PER_LEVEL_NO_GEMM
                                                     : ATTN_MERGED;
  const bool merged = p.grouping == ATTN_MERGED;
  p.nsets = merged ? 1 : L.nlev;
  for (int i = 0; i < p.nsets; ++i) {
    AttnSet& s = p.set[i];
    const int n = merged ? L.nlev : 1;  // its levels: i .. i + n - 1
    s.rows = L.row0[i + n] - L.row0[i];
    s.ao = attn_workspace(s.rows, C, prec).ao;
    s.fused = fused(s.rows);
    s.wh = s.rows / N * heads;
    const int64_t tiles = (N + kQB - 1) / kQB * s.wh;  // of the dense core
    if (tiles > 0x7fffffff) return "attention: too many (window, head) tiles";
    s.qsplit = !table ? 0 : s.wh >= kAttnNoSplitWH ? 1 : s.wh >= kAttnPairLoopWH ? 2 : 4;
    s.grid = table ? s.wh * s.qsplit : tiles;
    // a launch of its own: every window may take the pair loop
    s.pair_windows = !table ? 0 : merged ? pair_windows : s.rows / N;
    const bool pairs = table && N / 16 / s.qsplit >= kAttnPairNsub;
    for (int l = i; l < i + n; ++l)
      p.nq[l] = !table ? 0 : pairs && (L.row0[l] - L.row0[i]) / N < s.pair_windows ? 2 : 1;
  }
  return nullptr;
}

}  // namespace wf
