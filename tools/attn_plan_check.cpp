// Stand-alone host check of csrc/attn_plan.hpp (the level list validation and row prefix, the
// workspace layout and the plan of a window attention call), meant for a sanitizer build on the
// CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I waveformer_amd/csrc tools/attn_plan_check.cpp -o /tmp/attn_plan_check && /tmp/attn_plan_check
// The plan cases are those of tests/test_attn_plan_host.py; the answer of the GEMM predicates
// (HIP translation units) is given here as what they are documented to take: C = 48 and 96.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attn_plan.hpp"

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++fails;                                                     \
    }                                                              \
  } while (0)

using namespace wf;

struct Want {
  int fused;
  int64_t wh;
  int qsplit;
  int64_t pair_windows;
};

// plans one call (exactly-sized heap list: an over-read is caught) and checks it
static void check_plan(int line, int64_t B, int64_t C, std::vector<int64_t> dhw, int flags,
                       int grouping, std::vector<Want> sets, std::vector<int> nq) {
  const int nlev = (int)dhw.size() / 3;
  for (int prec = 0; prec < 3; ++prec) {
    AttnPlan p;
    const char* why = attn_plan(dhw.data(), nlev, B, C, C / 16, 8, prec, flags | ATTN_ALIGNED,
                                ATTN_QKV_RULE, [&](int64_t) { return C == 48 || C == 96; }, p);
    bool ok = !why && p.table && p.head_dim == 16 && p.grouping == grouping &&
              p.nsets == (int)sets.size() && p.L.nlev == nlev;
    int64_t rows = 0;
    for (int i = 0; ok && i < p.nsets; ++i) {
      const AttnSet& s = p.set[i];
      ok = s.fused == (sets[i].fused != 0) && s.wh == sets[i].wh && s.qsplit == sets[i].qsplit &&
           s.pair_windows == sets[i].pair_windows && s.grid == s.wh * s.qsplit &&
           s.ao == attn_workspace(s.rows, C, prec).ao && s.ao + s.rows * C * (prec ? 4 : 2) <= p.work.bytes;
      rows += s.rows;
    }
    for (int l = 0; ok && l < nlev; ++l) ok = p.nq[l] == nq[l];
    // the layout: qkv, then the core's output, 256-B aligned, not overlapping
    const int64_t e = prec ? 4 : 2;
    ok = ok && rows == p.L.row0[nlev] && p.work.qkv == 0 && p.work.ao % 256 == 0 &&
         p.work.bytes % 256 == 0 && p.work.ao >= rows * 3 * C * e &&
         p.work.ao < rows * 3 * C * e + 256 && p.work.bytes >= p.work.ao + rows * C * e;
    if (!ok) {
      std::printf("FAIL plan case at line %d, precision %d: %s\n", line, prec, why ? why : "fields");
      ++fails;
    }
  }
}

int main() {
  AttnLevels L;
  {  // stage 1 at B = 8: 32^3, 16^3, 8^3 (exactly-sized heap array: an over-read is caught)
    std::vector<int64_t> dhw = {32, 32, 32, 16, 16, 16, 8, 8, 8};
    CHECK(attn_levels_plan(dhw.data(), 3, 8, 48, 3, L) == nullptr);
    CHECK(L.nlev == 3 && L.row0[0] == 0 && L.row0[1] == 262144 && L.row0[2] == 294912 &&
          L.row0[3] == 299008);
    CHECK(L.D[1] == 16 && L.H[2] == 8 && L.W[0] == 32);
    for (int l = 0; l <= 3; ++l) CHECK(L.row0[l] % 512 == 0);
  }
  {  // non-cubic, four levels
    std::vector<int64_t> dhw = {16, 8, 24, 8, 8, 8, 8, 16, 8, 8, 8, 8};
    CHECK(attn_levels_plan(dhw.data(), 4, 2, 96, 6, L) == nullptr);
    CHECK(L.row0[4] == 2 * (16 * 8 * 24 + 512 + 1024 + 512));
    CHECK(L.D[0] == 16 && L.H[0] == 8 && L.W[0] == 24);
  }
  {  // refused: level count (the list is not read), raster, head_dim, NULL list, row overflow
    std::vector<int64_t> one = {8, 8, 8};
    CHECK(attn_levels_plan(one.data(), 0, 1, 48, 3, L) != nullptr);
    CHECK(attn_levels_plan(one.data(), 5, 1, 48, 3, L) != nullptr);
    CHECK(attn_levels_plan(nullptr, 1, 1, 48, 3, L) != nullptr);
    CHECK(attn_levels_plan(one.data(), 1, 0, 48, 3, L) != nullptr);
    CHECK(attn_levels_plan(one.data(), 1, 1, 48, 4, L) != nullptr);
    CHECK(attn_levels_plan(one.data(), 1, 1, 40, 0, L) != nullptr);
    std::vector<int64_t> bad = {16, 16, 16, 12, 12, 12};
    CHECK(attn_levels_plan(bad.data(), 2, 1, 48, 3, L) != nullptr);
    std::vector<int64_t> zero = {8, 0, 8};
    CHECK(attn_levels_plan(zero.data(), 1, 1, 48, 3, L) != nullptr);
    std::vector<int64_t> huge = {2048, 2048, 2048};
    CHECK(attn_levels_plan(huge.data(), 1, 1, 48, 3, L) != nullptr);
    std::vector<int64_t> big2 = {1024, 1024, 1024, 1024, 1024, 1024};  // each fits, the sum does not
    CHECK(attn_levels_plan(big2.data(), 2, 1, 48, 3, L) != nullptr);
    std::vector<int64_t> wide = {int64_t(1) << 40, 8, 8};
    CHECK(attn_levels_plan(wide.data(), 1, int64_t(1) << 40, 48, 3, L) != nullptr);
  }
  // ---- the plan: the rows of tests/test_attn_plan_host.py (the reasoning is written there)
  const std::vector<int64_t> L3 = {32, 32, 32, 16, 16, 16, 8, 8, 8}, L2 = {16, 16, 16, 8, 8, 8},
                             ONE = {8, 8, 8};
  const int LEVELS = ATTN_TABLE, RASTER = ATTN_TABLE | ATTN_RASTER;
  check_plan(__LINE__, 8, 48, L3, LEVELS, ATTN_MERGED, {{1, 1752, 1, 512}}, {2, 1, 1});
  check_plan(__LINE__, 1, 48, L3, LEVELS, ATTN_MERGED, {{0, 219, 4, 0}}, {1, 1, 1});
  check_plan(__LINE__, 8, 96, L2, LEVELS, ATTN_MERGED, {{0, 432, 2, 64}}, {2, 1});
  check_plan(__LINE__, 1, 96, L2, LEVELS, ATTN_MERGED, {{0, 54, 4, 0}}, {1, 1});
  check_plan(__LINE__, 8, 192, ONE, RASTER, ATTN_PER_LEVEL_RASTER, {{0, 96, 4, 8}}, {1});
  check_plan(__LINE__, 1, 192, ONE, RASTER, ATTN_PER_LEVEL_RASTER, {{0, 12, 4, 1}}, {1});
  check_plan(__LINE__, 8, 384, ONE, RASTER | ATTN_LN, ATTN_PER_LEVEL_RASTER, {{0, 192, 4, 8}}, {1});
  check_plan(__LINE__, 1, 384, ONE, RASTER | ATTN_LN, ATTN_PER_LEVEL_RASTER, {{0, 24, 4, 1}}, {1});
  check_plan(__LINE__, 1, 48, ONE, LEVELS, ATTN_MERGED, {{0, 3, 4, 0}}, {1});
  check_plan(__LINE__, 1, 192, L2, LEVELS, ATTN_PER_LEVEL_NO_GEMM, {{0, 96, 4, 8}, {0, 12, 4, 1}},
             {1, 1});
  check_plan(__LINE__, 11, 48, {8, 8, 8, 16, 16, 16}, LEVELS, ATTN_PER_LEVEL_PREFIX,
             {{0, 33, 4, 11}, {1, 264, 2, 88}}, {1, 2});
  check_plan(__LINE__, 11, 48, L2, LEVELS, ATTN_MERGED, {{1, 297, 2, 88}}, {2, 1});
  {  // refused by the plan: a bad mode, a fused width that is not instantiated, a misaligned list
    AttnPlan p;
    auto no = [](int64_t) { return false; };
    CHECK(attn_plan(ONE.data(), 1, 1, 48, 3, 8, 1, ATTN_TABLE | ATTN_ALIGNED, 2, no, p) != nullptr);
    CHECK(attn_plan(ONE.data(), 1, 1, 192, 12, 8, 1, ATTN_TABLE | ATTN_ALIGNED, 1, no, p) != nullptr);
    CHECK(attn_plan(ONE.data(), 1, 1, 48, 3, 8, 1, ATTN_TABLE, -1, no, p) != nullptr);
    CHECK(attn_plan(ONE.data(), 5, 1, 48, 3, 8, 1, ATTN_TABLE | ATTN_ALIGNED, -1, no, p) != nullptr);
    // one raster, misaligned: staged, not refused
    CHECK(attn_plan(ONE.data(), 1, 86, 48, 3, 8, 1, RASTER, -1, no, p) == nullptr && !p.set[0].fused);
    CHECK(attn_plan(ONE.data(), 1, 86, 48, 3, 8, 1, RASTER | ATTN_ALIGNED, -1, no, p) == nullptr &&
          p.set[0].fused);
  }
  std::printf(fails ? "%d checks failed\n" : "attn_plan ok\n", fails);
  return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
