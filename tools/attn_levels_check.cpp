// Stand-alone host check of csrc/attn_levels.hpp (the level list validation and row prefix of
// wf_window_attention_fwd_levels), meant for a sanitizer build on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I waveformer_amd/csrc tools/attn_levels_check.cpp -o /tmp/attn_levels_check && /tmp/attn_levels_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attn_levels.hpp"

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++fails;                                                     \
    }                                                              \
  } while (0)

int main() {
  using namespace wf;
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
  std::printf(fails ? "%d checks failed\n" : "attn_levels ok\n", fails);
  return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
