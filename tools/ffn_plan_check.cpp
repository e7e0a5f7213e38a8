// Stand-alone host check of csrc/ffn_plan.hpp (the workspace layout and the dispatch plan of
// wf_ccf_ffn_stage), meant for a sanitizer build on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I waveformer_amd/csrc tools/ffn_plan_check.cpp -o /tmp/ffn_plan_check && /tmp/ffn_plan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ffn_plan.hpp"

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++fails;                                                     \
    }                                                              \
  } while (0)

using namespace wf;

// one row of the dispatch table: precisions as a bit mask (1 bf16, 2 bf16x3, 4 fp16)
struct Row {
  int64_t C, hidden;
  int precs, train;
  int64_t B, D, H, W;
  int front, back;  // back < 0: an error replaces the plan
};
constexpr int FP32 = 2 | 4, BF16 = 1, ANY = 7;
constexpr int EPI = FFN_FRONT_EPILOGUE, PASS = FFN_FRONT_PASS;
static const Row kTable[] = {
    {48, 192, FP32, 0, 8, 64, 64, 64, EPI, FFN_BACK_DWFC_TB4},
    {48, 192, FP32, 0, 42, 64, 64, 64, EPI, FFN_BACK_DWFC_TB4},
    {48, 192, FP32, 0, 43, 64, 64, 64, EPI, FFN_BACK_DWFC_SB},   // x / out reach 2 GiB
    {48, 192, FP32, 0, 1, 1, 1672, 1672, EPI, FFN_BACK_DWFC_TB4},
    {48, 192, FP32, 0, 1, 1, 1673, 1673, EPI, FFN_BACK_DWFC_SB},  // one h1 plane reaches 2 GiB
    {48, 192, BF16, 0, 8, 64, 64, 64, EPI, FFN_BACK_DWFC_SB},
    {48, 192, ANY, 1, 2, 8, 8, 8, EPI, FFN_BACK_STAGED},
    {96, 384, FP32, 0, 170, 32, 32, 32, EPI, FFN_BACK_DWFC2_TB},
    {96, 384, FP32, 0, 171, 32, 32, 32, EPI, FFN_BACK_DWFC2_KERNEL},
    {96, 384, BF16, 0, 8, 32, 32, 32, EPI, FFN_BACK_DWFC2_KERNEL},
    {192, 768, FP32, 0, 682, 16, 16, 16, EPI, FFN_BACK_DWFC3_TB},  // gemm_lnw takes the wide row
    {192, 768, FP32, 0, 683, 16, 16, 16, EPI, FFN_BACK_STAGED},
    {192, 768, BF16, 0, 8, 16, 16, 16, EPI, FFN_BACK_STAGED},
    {192, 768, FP32, 1, 2, 16, 16, 16, EPI, FFN_BACK_STAGED},
    {384, 1536, FP32, 0, 8, 8, 8, 8, PASS, FFN_BACK_STAGED},
    {384, 1536, FP32, 1, 8, 8, 8, 8, PASS, FFN_BACK_STAGED},
    {384, 1536, BF16, 0, 8, 8, 8, 8, EPI, FFN_BACK_STAGED},
    {48, 96, FP32, 0, 1, 4, 4, 4, EPI, FFN_BACK_STAGED},       // not 4C
    {8, 40, FP32, 0, 1, 4, 4, 4, EPI, FFN_BACK_STAGED_DWLN},  // hidden % 32 != 0
    {8, 40, FP32, 1, 1, 4, 4, 4, -1, -1},
};

static void check_table() {
  const int n = (int)(sizeof(kTable) / sizeof(kTable[0]));
  for (int mode = 0; mode < 3; ++mode) {  // default switches, WF_FFN_NO_DWFC, WF_FFN_FUSED
    FfnSwitches sw{};
    sw.no_dwfc = mode == 1;
    sw.whole = mode == 2;
    for (int r = 0; r < n; ++r) {
      const Row& t = kTable[r];
      int front = t.front, back = t.back;
      if (mode == 1 && back >= 0 && ffn_back_fused(back)) back = FFN_BACK_STAGED;
      if (mode == 2 && t.C == 48 && t.hidden == 192 && !t.train) {
        front = FFN_FRONT_NONE;
        back = FFN_BACK_FUSED;
      }
      for (int prec = 0; prec < 3; ++prec) {
        if (!(t.precs >> prec & 1)) continue;
        FfnPlan p;
        const char* why = ffn_plan(t.B, t.C, t.hidden, t.D, t.H, t.W, prec, t.train != 0, sw, p);
        const bool ok = back < 0 ? why != nullptr && std::strstr(why, "hidden % 32") != nullptr
                                 : why == nullptr && p.front == front && p.back == back;
        if (!ok) {
          std::printf("FAIL table row %d, prec %d, switches %d: got %s front %d back %d\n", r + 1,
                      prec, mode, why ? why : "a plan,", p.front, p.back);
          ++fails;
        }
      }
    }
  }
}

static void check_ln1_fuse() {  // WF_FFN_LN1_FUSE: the partials form, if gemm_kc chunks the row
  FfnSwitches sw{};
  sw.ln1_fuse = true;
  FfnPlan p;
  CHECK(ffn_plan(8, 384, 1536, 8, 8, 8, 1, false, sw, p) == nullptr);
  CHECK(p.front == FFN_FRONT_PARTIALS && p.back == FFN_BACK_STAGED && p.ln1_np == 0);
  FfnPlan q = p;
  ffn_plan_set_kc_chunk(q, 1536, 6);  // 96-column chunks
  CHECK(q.front == FFN_FRONT_PARTIALS && q.ln1_np == 16);
  q = p;
  ffn_plan_set_kc_chunk(q, 1536, 0);  // gemm_kc does not take the shape
  CHECK(q.front == FFN_FRONT_PASS && q.ln1_np == 0);
  q = p;
  ffn_plan_set_kc_chunk(q, 1536, 5);  // no whole chunks per row
  CHECK(q.front == FFN_FRONT_PASS);
  CHECK(ffn_plan(8, 384, 1536, 8, 8, 8, 1, true, sw, p) == nullptr);  // training keeps h1
  CHECK(p.front == FFN_FRONT_PASS);
  CHECK(ffn_plan(8, 384, 1536, 8, 8, 8, 0, false, sw, p) == nullptr);  // bf16 h1
  CHECK(p.front == FFN_FRONT_EPILOGUE);
  CHECK(ffn_plan(8, 192, 768, 16, 16, 16, 1, false, sw, p) == nullptr);  // gemm_lnw's row
  CHECK(p.front == FFN_FRONT_EPILOGUE && p.back == FFN_BACK_DWFC3_TB);
  ffn_plan_set_kc_chunk(p, 768, 6);  // not the partials form: left alone
  CHECK(p.front == FFN_FRONT_EPILOGUE && p.ln1_np == 0);
}

static int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

static void check_layout() {
  const int64_t shapes[][3] = {{48, 192, 2 * 3 * 5 * 7}, {96, 384, 8 * 16 * 16 * 16},
                               {192, 768, 2 * 8 * 8 * 8}, {384, 1536, 1}, {192, 768, 210},
                               {8, 40, 64}};
  for (const auto& sh : shapes) {
    for (int prec = 0; prec < 3; ++prec) {
      const int64_t C = sh[0], hid = sh[1], M = sh[2], e = prec == 0 ? 2 : 4;
      const FfnWorkspace w = ffn_workspace(M, C, hid, prec);
      const bool fcs = C == 192 && hid == 768 && prec != 0;
      // the sizes of the areas, in order; each starts where the one before ends (rounded up)
      const int64_t size[6] = {M * hid * e, M * hid * e, M * (hid / 32) * 8, M * (hid / 32) * 8,
                               M * 8, fcs ? DWFC3_FCS_BYTES : 0};
      const int64_t off[6] = {w.h1, w.h2, w.ln2_pst, w.ln1_pst, w.ln1_st, fcs ? w.fcs : w.bytes};
      int64_t at = 0;
      for (int i = 0; i < 6; ++i) {
        CHECK(off[i] % 256 == 0);
        CHECK(off[i] == at);  // no gap beyond the alignment, no overlap
        at += round256(size[i]);
      }
      CHECK(w.bytes == at);
      CHECK((w.fcs >= 0) == fcs);
      if (fcs) CHECK(w.fcs + DWFC3_FCS_BYTES == w.bytes);  // the last area
      CHECK(w.h1 == 0 && w.h2 == round256(M * hid * e));
    }
  }
  CHECK(DWFC3_FCS_BYTES % 256 == 0);
}

int main() {
  check_table();
  check_ln1_fuse();
  check_layout();
  std::printf(fails ? "%d checks failed\n" : "ffn_plan ok\n", fails);
  return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
