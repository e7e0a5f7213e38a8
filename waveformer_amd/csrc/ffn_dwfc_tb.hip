// ffn_dwfc_tb.hip -- ffn_dwfc_tb4, the default stage-1 CCF_FFN back half (C = 48, hidden = 192;
// SURVEY 8a a8, 8f row 1) with three VALU waves per SIMD (round 4).
//
//   h2  = dwconv3x3x3(h1) + b          (wave_helper.py:285, groups = hidden, pad 1)
//   g   = GELU(LN_eps2(h2))            (:286-287)
//   ffn = fc(g) + fc_b                 (:289)
//   out = x + (n2 + ffn) * bs          (Block residual + CCF_FFN residual, quirk Q4, :293/:509)
//
// Why this kernel (tools/ubench_valu.hip, profiles/r4_ubench_valu.txt): on gfx950 one wave
// issues a VALU instruction only every ~12 cycles, two waves of a SIMD together every ~3
// (v_fma_f32) to ~5.3 (v_fmac_f32 fed by ds_read_b32), and only three or more reach the
// SIMD-32 rate of 2 cycles.  ffn_dwfc_sb ran two VALU waves per SIMD (its 27 weights x 3
// channels per lane held 160 VGPRs): its D waves issued at ~4.4 cycles per instruction.
// Here every lane owns ONE channel, so a VALU wave fits 128 VGPRs and a SIMD holds three of
// them plus the staging / fc wave (16 waves, 1024 threads):
//
//   tile 4 (y) x 8 (x) positions (the tile of ffn_dwfc_sb), z-marching through ZS planes;
//   D waves (12 = 3 per SIMD): lane = (channel c, column pair cp = the SIMD): the 27 taps of
//        channel c in VGPRs, per input row 4 ds_read_b32 (consecutive lanes = consecutive
//        channels: conflict-free) feed 2 columns x up to 3 output rows x 3 output planes;
//   E waves (4 = 1 per SIMD, s_setprio 3):
//        E0..E2: the fc of one 16-channel output column tile each over the 32 positions on
//        v_mfma_f32_16x16x32 (x3 for bf16x3; weight hi in VGPRs, lo in LDS in fragment order),
//        bias + Q4 residual + 16-B stores;
//        E3 (no fc tile): the loader -- the haloed 6 x 10 x 192 h1 plane staged by LDS-DMA
//        (buffer_load_dwordx4 ... lds through a per-plane buffer descriptor, up to two planes
//        ahead; out-of-volume positions and planes come back as zeros).
// Staging on the D waves through registers cost them 800-1400 cycles of a ~5600-cycle plane
// and needed 112 VGPRs; on the E waves by registers it needed > 128 VGPRs (spills).  LDS-DMA
// needs neither.  fp32 h1 only (bf16x3, fp16 modes); the bf16 mode keeps ffn_dwfc_sb.
//
// The tile leaves room for only two h2 tiles, so two barriers per plane as in ffn_dwfc_sb:
//   phase 1: D slots 0, 1: LN2 of h2 tile (p-2), 16 lanes x 12 channels per position, 4
//            positions per wave (8 per SIMD); D slot 2: scatter rows [0, S2) of plane p
//            E0..E2: fc of tile (p-3) + epilogue + store; residual rows of p-2
//            E3: LDS-DMA pieces [FA, 45) of plane p+1 into the buffer plane p-1 left
//   phase 2: D slots 0, 1: scatter rows [0, 6); slot 2: rows [S2, 6); all D: h2 tile p-1
//            E3: LDS-DMA pieces [0, FA) of plane p+2 into the buffer plane p left; wait for
//            plane p+1 (vmcnt(FA))
// The phase probe (tools/tb4_phase_times.py, -DWF_DWFC2_PROBE) decides this placement: the
// depthwise waves bound both phases (LN2 of slot 1 in phase 1, the scatter in phase 2), never
// the plane fill, and whatever else runs on a SIMD beside them in phase 2 lengthens it.  So the
// fc runs half an iteration late, in phase 1, where the E waves used to wait for the LN2, slot
// 2 scatters its whole plane there (S2 = 6) beside the two LN2 waves, and the loader's pieces
// go out in both phases without any wave waiting for them in the iteration of their issue.
// LDS: 2 x 46,080 B planes + 2 x 25,600 B h2 tiles + 18,432 B fc lo fragments + 1,920 B
// vectors = 163,712 B (+ 16 B of role counters).
// (The 3 x 8 one-barrier predecessor, the first E-wave memory pipeline and the round-4..8
// schedule -- every E wave staging a quarter plane in phase 1, fc in phase 2 -- are in git
// history.)
#include "ffn_dwfc_common.hpp"

namespace wf {

#ifdef WF_DWFC2_PROBE
// diagnostic builds only: per-wave cycles of workgroup 0 by phase (tools/tb4_phase_times.py):
// slot 0 phase-1 work (E: residual loads), 1 wait at barrier 1, 2 phase-2 work (E: fc + stores),
// 3 wait at barrier 2, 4 DMA issue, 5 the DMA wait (vmcnt) that ends phase 2, 6 role, 7 iterations
__device__ long long g_dwfctb4_probe[16 * 8];
extern "C" int wf_debug_dwfctb4_probe(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dwfctb4_probe), sizeof(g_dwfctb4_probe));
}
#endif

namespace tb4 {
constexpr int EPRIO = 3;  // s_setprio of the fc (E) waves
constexpr int S2 = 6;  // input rows the third D wave of a SIMD scatters in phase 1
constexpr int C = 48, HID = 192, TY = 4, TX = 8;
constexpr int PY = TY + 2, PX = TX + 2, PP = PY * PX;  // 6 x 10
constexpr int NPOS = TY * TX;                          // 32
// h2 rows are HID + 8 floats apart (50 16-B quads, 2 mod 16): the fc's B-fragment reads (16
// rows x 4 k-quads per ds_read_b128) then meet 16 distinct 4-bank groups in every lane group,
// and LN2 lane lg of row r takes the channel quads m, m + 16, m + 32 with m = (lg - 2 r) & 15,
// which cancels the row's bank offset, so its reads (and its bf16 hi / lo writes) are
// conflict-free as well.  Round 5's HID + 4 rows with 12 contiguous channels per LN2 lane had
// 0.95 bank-conflict cycles per LDS instruction.
constexpr int HS = HID + 8;
constexpr int PLANE_F = PP * HID;
constexpr int H2F = NPOS * HS;
constexpr int NV = HID / 4;
constexpr int NPC = (PP * NV + 63) / 64;               // 45 LDS-DMA pieces
static_assert(NPC * 64 == PP * NV, "whole pieces only: the loader issues no partial piece");
// pieces of a plane the loader issues half an iteration early (part A, see the loader)
constexpr int FA = 16;
static_assert(FA >= 0 && NPC + FA <= 63, "outstanding pieces must fit the 6-bit vmcnt");
constexpr int KS = HID / 32;
constexpr int FWL_BYTES = (C / 16) * KS * 64 * 16;
// vectors: LN2 affine (HID each), fc bias + norm2 bias folded into one (C), norm2 weight (C)
constexpr size_t LDS_BYTES = (size_t)(2 * PLANE_F + 2 * H2F + 2 * HID + 2 * C) * 4 + FWL_BYTES;
static_assert(LDS_BYTES <= 160 * 1024, "LDS");
}  // namespace tb4

template <int P>
__global__ __launch_bounds__(1024, 1) void ffn_dwfc_tb4_kernel(DwFcArgs a) {
  using namespace tb4;
  constexpr bool SPLIT = P == PREC_SPLIT;
  // separate static LDS objects (not one dynamic array carved by offsets): the compiler's
  // wait insertion can then tell the planes the LDS-DMA writes from the h2 tiles and fc
  // fragments the E waves read, instead of waiting for every DMA before any LDS read
  __shared__ __attribute__((aligned(16))) float planes[2 * PLANE_F];  // [2][PP][HID]
  __shared__ __attribute__((aligned(16))) float h2b[2 * H2F];         // [2][NPOS][HS]
  __shared__ __attribute__((aligned(16))) float vecs[2 * HID + 2 * C];
  __shared__ bf16x8 fwlo[FWL_BYTES / 16];
  float* lnw = vecs;                       // [HID] (halved: GELU from x / 2)
  float* lnb = lnw + HID;
  float* fcl = lnb + HID;                  // [C] fc bias (+ norm2 bias when stats are given)
  float* n2w = fcl + C;                    // [C]
  __shared__ int simd_cnt[4];

  const int tid = threadIdx.x;
  const int wid = tid >> 6, lane = tid & 63;
  const int D = a.D, H = a.H, W = a.W;
  const DwFcTile tl = dwfc_tile<TY, TX>(a);
  const int b = tl.b, x0 = tl.x0, y0 = tl.y0, z0 = tl.z0, z1 = tl.z1;
  const int64_t plane_sz = (int64_t)H * W;

  if (tid < 4) simd_cnt[tid] = 0;
  dwfc_stage_ln2<HID>(lnw, lnb, a, 1024);
  // not dwfc_stage_epi: this kernel folds norm2's bias into the fc bias (one LDS read and one
  // add less per output quad in the epilogue), a different association of the same sum
  for (int i = tid; i < C; i += 1024) {
    fcl[i] = (a.fc_b ? a.fc_b[i] : 0.f) + (a.stats ? a.n2_b[i] : 0.f);
    n2w[i] = a.stats ? a.n2_w[i] : 1.f;
  }
  if (SPLIT) {
    for (int i = tid; i < (C / 16) * KS * 64; i += 1024) {
      const int l = i & 63, ks = (i >> 6) % KS, ct = (i >> 6) / KS;
      fwlo[i] = *reinterpret_cast<const bf16x8*>(a.fc + (size_t)C * HID +
                                                 (size_t)(ct * 16 + (l & 15)) * HID + ks * 32 + 8 * (l >> 4));
    }
  }
  for (int i = tid; i < HID * 27; i += 1024) planes[i] = a.dw_w[i];
  for (int i = tid; i < HID; i += 1024) planes[HID * 27 + i] = a.dw_b[i];
  __syncthreads();
  const int role = dwfc_wave_role<4>(simd_cnt, wid, lane);  // 0..11 D, 12..15 E
  PROBE_DECL
#ifdef WF_DWFC2_PROBE
  pr_acc[6] = role;
  pr_acc[7] = z1 + 3 - z0;
#endif

  if (role < 12) {
    // ================================ D waves ===========================================
    const int cp = role / 3, kslot = role % 3, c = kslot * 64 + lane;
    float w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = planes[c * 27 + k];
    const float bias = planes[HID * 27 + c];
    float acc[3][TY][2];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int o = 0; o < TY; ++o) acc[s][o][0] = acc[s][o][1] = 0.f;
    // LN2 (slots 0, 1): position 8 cp + 4 kslot + (lane >> 4), channel quads m, m + 16, m + 32
    // of its row, m = (lg - 2 lpos) & 15 (conflict-free banks, see HS)
    const int lpos = 8 * cp + 4 * kslot + (lane >> 4), lg = lane & 15;
    const int cm = 4 * ((lg - 2 * lpos) & 15);
    __syncthreads();  // (prologue) weights read out of the plane buffer
    __syncthreads();  // (prologue) plane z0-1 staged

    auto ln2_rows = [&](float* h2t) {
      dwfc_ln2_row<P, HID, 16, 64, true>(h2t + lpos * HS, cm, lnw, lnb, a.eps2);
    };
    auto rows = [&](const float (&vin)[PY][4], auto SAc, auto SBc, auto SCc, auto LOc, auto HIc) {
      constexpr int SA = decltype(SAc)::value, SB = decltype(SBc)::value,
                    SC = decltype(SCc)::value, LO = decltype(LOc)::value, HI = decltype(HIc)::value;
#pragma unroll
      for (int r = LO; r < HI; ++r) {
        const float* v = vin[r];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int o = r - ky;
          if (o < 0 || o >= TY) continue;
          const float* w0 = w + ky * 3;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            if (ky == 0)
              acc[SC][o][j] = w0[2] * v[j + 2] + (w0[1] * v[j + 1] + w0[0] * v[j]);
            else
              acc[SC][o][j] = w0[2] * v[j + 2] + (w0[1] * v[j + 1] + (w0[0] * v[j] + acc[SC][o][j]));
            acc[SB][o][j] = w0[11] * v[j + 2] + (w0[10] * v[j + 1] + (w0[9] * v[j] + acc[SB][o][j]));
            acc[SA][o][j] = w0[20] * v[j + 2] + (w0[19] * v[j + 1] + (w0[18] * v[j] + acc[SA][o][j]));
          }
        }
      }
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, S2> IS;
    typedef std::integral_constant<int, PY> IP;
    auto step = [&](int p, auto Rc) {
      constexpr int R = decltype(Rc)::value;
      typedef std::integral_constant<int, R> SA;
      typedef std::integral_constant<int, (R + 1) % 3> SB;
      typedef std::integral_constant<int, (R + 2) % 3> SC;
      const bool live = p <= z1 && !(ffn_dbg(a) & 1);
      const bool ln = p - 2 >= z0 && p - 2 < z1 && !(ffn_dbg(a) & 2);
      float vin[PY][4];
      const float* q0 = planes + ((p - z0 + 1) & 1) * PLANE_F + 2 * cp * HID + c;
      auto load_plane = [&]() {
#pragma unroll
        for (int r = 0; r < PY; ++r)
#pragma unroll
          for (int k = 0; k < 4; ++k) vin[r][k] = q0[(r * PX + k) * HID];
      };
      // ---- phase 1.  The LN2 slots read their plane inputs after the LN2 (issued before the
      // barrier, consumed after it), so the 24 input registers are not live beside LN2's
      if (kslot < 2) {
        if (ln) ln2_rows(h2b + ((p - 2 - z0) & 1) * H2F);
        if (live) load_plane();
      } else if (live) {
        load_plane();
        rows(vin, SA(), SB(), SC(), I0(), IS());
      }
      PROBE(0)
      __syncthreads();  // 1 -> 2: LN2'd tile (p-2) visible to the fc
      PROBE(1)
      // ---- phase 2
      if (live) {
        if (kslot < 2) rows(vin, SA(), SB(), SC(), I0(), IP());
        else rows(vin, SA(), SB(), SC(), IS(), IP());
        if (p - 1 >= z0) {
          float* h2t = h2b + ((p - 1 - z0) & 1) * H2F;
#pragma unroll
          for (int o = 0; o < TY; ++o)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              h2t[(o * TX + 2 * cp + j) * HS + c] = acc[R][o][j] + bias;
        }
      }
      PROBE(2)
      __syncthreads();  // 2 -> next 1
      PROBE(3)
    };
    for (int p = z0 - 1; p <= z1 + 1; p += 3) {
      step(p, std::integral_constant<int, 0>());
      if (p + 1 <= z1 + 1) step(p + 1, std::integral_constant<int, 1>());
      if (p + 2 <= z1 + 1) step(p + 2, std::integral_constant<int, 2>());
    }
    PROBE_DUMP_TO(g_dwfctb4_probe)
    return;
  }

  // ================================== E waves ============================================
  const int e = role - 12;
  if (e == C / 16) {
    __builtin_amdgcn_s_setprio(3);
    // ============================ E3: the plane loader ====================================
    // The fourth E wave has no fc tile, no residual loads and no stores: its VM queue holds
    // LDS-DMA pieces only, in issue order, so a counted vmcnt on it is exact.  It stages every
    // plane alone, 45 pieces of 1 KiB, split in two parts that go out in different phases:
    //   part A = pieces [0, FA) of plane p + 2 in phase 2 of iteration p,
    //   part B = pieces [FA, 45) of plane p + 1 in phase 1 of iteration p,
    // so pieces are in flight through both phases and the wait that ends phase 2, vmcnt(FA),
    // retires plane p + 1 (everything older than part A of p + 2) without draining the queue.
    // * Buffer reuse: plane q lives in buffer (q - z0 + 1) & 1.  Every D wave reads plane p out
    //   into registers in phase 1 of iteration p, and its barrier 1 (__syncthreads: lgkmcnt(0)
    //   first) follows those reads.  Part A of p + 2 (the buffer of p) is issued after barrier 1
    //   of iteration p; part B of p + 1 (the buffer of p - 1) after barrier 2 of iteration p - 1,
    //   i.e. after barrier 1 of iteration p - 1.  The prologue's pieces follow the barrier behind
    //   the weight reads (the weights lie in buffer 0).
    // * Visibility: plane p + 1 is read in phase 1 of iteration p + 1, behind barrier 2 of
    //   iteration p, which this wave enters only after vmcnt(FA) (vmcnt(0) when no part A was
    //   issued) has retired every piece of plane p + 1.  Wait, barrier, read: one barrier between
    //   the covering wait and the first ds_read, as before.  The barriers here are bare
    //   s_barriers: __syncthreads()' fence would drain the pieces left in flight.
    // * Segments: planes z0 - 1 .. z1 are staged (ZS + 2 >= 3 of them), every iteration
    //   p = z0 - 1 .. z1 + 1 tests p + 1 <= z1 and p + 2 <= z1 itself, so a segment of any length
    //   (the last, ragged one included) takes this one loop; no piece beyond 45 per plane, no
    //   padding.  Out-of-volume planes go through a zero-size descriptor and out-of-volume
    //   positions through offset BUF_OOR: both land as zeros.
    // * At most 45 + FA pieces are outstanding (a whole plane and the next one's part A), within
    //   the 6-bit vmcnt.
    const float* src = reinterpret_cast<const float*>(a.h1) + (int64_t)b * D * H * W * HID;
    const int64_t plane_elems = (int64_t)H * W * HID;
    // the pieces' source offsets within a plane, once per tile (this wave has the registers)
    uint32_t off[NPC];
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int i = j * 64 + lane;
      const int pos = i / NV, v = i - pos * NV;
      const int yy = y0 - 1 + pos / PX, xx = x0 - 1 + pos % PX;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      off[j] = ok ? (uint32_t)(((yy * W + xx) * HID + 4 * v) * 4) : (uint32_t)BUF_OOR;
    }
    auto fill = [&](int p, auto LOc, auto HIc) {
      constexpr int LO = decltype(LOc)::value, HI = decltype(HIc)::value;
      float* dst = planes + ((p - z0 + 1) & 1) * PLANE_F;
      const bool pz = p >= 0 && p < D;
      const float* base = src + (int64_t)min(max(p, 0), D - 1) * plane_elems;
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(base, pz ? (int)(plane_elems * 4) : 0);
#pragma unroll
      for (int j = LO; j < HI; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs, (__attribute__((address_space(3))) void*)(dst + j * 256), 16, off[j], 0, 0, 0);
    };
    typedef std::integral_constant<int, 0> F0;
    typedef std::integral_constant<int, FA> FAc;
    typedef std::integral_constant<int, NPC> FN;
    const bool fetch = !(ffn_dbg(a) & 8);
    __syncthreads();  // (prologue) weights read out of the plane buffer
    fill(z0 - 1, F0(), FN());
    fill(z0, F0(), FAc());
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FA) : "memory");
    __builtin_amdgcn_s_barrier();  // (prologue) plane z0-1 staged
    for (int p = z0 - 1; p <= z1 + 1; ++p) {
      // ---- phase 1: the rest of plane p + 1
      if (p + 1 <= z1 && fetch) fill(p + 1, FAc(), FN());
      PROBE(4)
      __builtin_amdgcn_s_barrier();  // 1 -> 2: every D wave holds plane p in registers
      PROBE(1)
      // ---- phase 2: the head of plane p + 2 into the buffer plane p just left, then the wait
      // for plane p + 1
      if (p + 2 <= z1 && fetch) {
        fill(p + 2, F0(), FAc());
        PROBE(2)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FA) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      PROBE(5)
      __builtin_amdgcn_s_barrier();  // 2 -> next 1
      PROBE(3)
    }
    PROBE_DUMP_TO(g_dwfctb4_probe)
    return;
  }
  // =============================== E0..E2: the fc waves ===================================
  __builtin_amdgcn_s_setprio(EPRIO);
  const int l15 = lane & 15, g4 = lane >> 4;
  const int ct = e;
  const float bs = a.bscale ? a.bscale[b] : 1.f;
  bf16x8 fwh[KS];
  {
    const uint16_t* wr = a.fc + (size_t)(ct * 16 + l15) * HID + 8 * g4;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fwh[ks] = *reinterpret_cast<const bf16x8*>(wr + ks * 32);
  }
  const bf16x8* fwl = fwlo + ct * KS * 64 + lane;
  const int col = ct * 16 + 4 * g4;
  const float* sbase = a.stats ? a.stats : a.x;
  auto gpos_of = [&](int zo, int rt, bool clamp) {
    const int lp = rt * 16 + l15;
    int yo = y0 + lp / TX, xo = x0 + lp % TX;
    if (clamp) {
      yo = min(yo, H - 1);
      xo = min(xo, W - 1);
    }
    return (int64_t)b * D * plane_sz + (int64_t)zo * plane_sz + (int64_t)yo * W + xo;
  };
  auto row_ok = [&](int rt) {
    const int lp = rt * 16 + l15;
    return y0 + lp / TX < H && x0 + lp % TX < W;
  };
  // The fc waves' memory pipeline:
  //   * the residual rows of output plane zo + 1 are loaded in iteration p, into the register
  //     set of zo + 1's parity, and used by the fc one iteration later: the fc does not wait
  //     for a memory round trip;
  //   * the output rows go out as range-checked buffer stores (rows outside the volume get an
  //     out-of-range offset and are dropped) and are never waited for.
  // These waves issue no LDS-DMA (the loader above does), so nothing of theirs has to land
  // before a barrier.  (Until round 9 every E wave staged a quarter of the plane in phase 1 and
  // ended phase 2 on vmcnt(2), the wait for its pieces; that version is in git history.)
  // residual / statistics rows through 32-bit buffer offsets (64-bit pointer pairs for the two
  // register sets spilled: the host keeps the tensors under 2 GiB)
  f32x4 xr[2][2];
  f32x2 es[2][2];
  const int64_t npos = (int64_t)a.B * D * plane_sz;
  const __amdgpu_buffer_rsrc_t xrsrc = buf_rsrc(a.x, (int)(npos * C * 4));
  const __amdgpu_buffer_rsrc_t srsrc = buf_rsrc(sbase, (int)(npos * 2 * 4));
  auto load_resid = [&](int zo, f32x4 (&xv)[2], f32x2 (&ev)[2]) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int g = (int)gpos_of(zo, rt, true);
      xv[rt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (g * C + col) * 4, 0, 0));
      ev[rt] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(srsrc, g * 8, 0, 0));
    }
  };
  const __amdgpu_buffer_rsrc_t orsrc = buf_rsrc(a.out, (int)(npos * C * 4));
  auto fc_store = [&](const float* h2t, int zo, int rt, const f32x4& xv, const f32x2& ev) {
    const int lp = rt * 16 + l15;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint16_t* Bh = reinterpret_cast<const uint16_t*>(h2t) + (size_t)lp * (2 * HS);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = ks * 32 + 8 * g4;
      acc = mma3<P>(acc, fwh[ks], fwl[ks * 64], *reinterpret_cast<const bf16x8*>(Bh + k),
                         *reinterpret_cast<const bf16x8*>(Bh + HID + k));
    }
    // fc + bias (+ norm2's bias, folded) and, with stats, norm2's normalised x * weight
    f32x4 v = acc + *reinterpret_cast<const f32x4*>(fcl + col);
    if (a.stats) {
      const f32x4 lw = *reinterpret_cast<const f32x4*>(n2w + col);
      v = xv + ((xv - ev.x) * ev.y * lw + v) * bs;
    } else {
      v = xv + v * bs;
    }
    const int voff = row_ok(rt) ? (int)((gpos_of(zo, rt, false) * C + col) * 4) : BUF_OOR;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), orsrc, voff, 0, 0);
  };

  __syncthreads();  // (prologue) weights read out of the plane buffer
  __syncthreads();  // (prologue) plane z0-1 staged
  // iteration p: the fc of tile zo = p - 3 in PHASE 1, half an iteration after the phase 2 in
  // which it could first run.  Tile zo was LN2'd in phase 1 of iteration p - 1 and its buffer is
  // next written (h2 tile zo + 2) in phase 2 of iteration p, behind barrier 1, which this wave
  // enters with its LDS reads complete (lgkmcnt(0)); phase 1's LN2 works on the other buffer.
  // Register set of output plane z: (z - z0) & 1, a compile-time S for the fc (zo) and S ^ 1
  // for the prefetch (zo + 1, used one iteration later) with the loop unrolled by two.
  auto fc_tile = [&](int zo, auto Sc) {
    constexpr int S = decltype(Sc)::value;
    if (zo >= z0 && zo < z1 && !(ffn_dbg(a) & 4)) {
      const float* h2t = h2b + ((zo - z0) & 1) * H2F;
      fc_store(h2t, zo, 0, xr[S][0], es[S][0]);
      fc_store(h2t, zo, 1, xr[S][1], es[S][1]);
    }
  };
  auto iter = [&](int p, auto Sc) {
    constexpr int S = decltype(Sc)::value;
    const int zo = p - 3;
    // ---- phase 1: fc of tile zo + epilogue (the two stores stay in flight), then the residual
    // rows of zo + 1
    fc_tile(zo, Sc);
    PROBE(2)
    if (zo + 1 >= z0 && zo + 1 < z1) load_resid(zo + 1, xr[S ^ 1], es[S ^ 1]);
    PROBE(0)
    // bare s_barriers: __syncthreads()' workgroup release fence would drain vmcnt(0), i.e. the
    // stores and the residual rows just requested.  This wave writes no LDS.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // 1 -> 2
    PROBE(1)
    // ---- phase 2: nothing
    __builtin_amdgcn_s_barrier();  // 2 -> next 1
    PROBE(3)
  };
  // (zo - z0) & 1 at p = z0 - 1 + i is i & 1: even i -> S = 0
  for (int p = z0 - 1; p <= z1 + 1; p += 2) {
    iter(p, std::integral_constant<int, 0>());
    if (p + 1 <= z1 + 1) iter(p + 1, std::integral_constant<int, 1>());
  }
  // the last tile, z1 - 1 (LN2'd in phase 1 of the last iteration), behind the last barrier
  if ((z1 - 1 - z0) & 1) fc_tile(z1 - 1, std::integral_constant<int, 1>());
  else fc_tile(z1 - 1, std::integral_constant<int, 0>());
  PROBE_DUMP_TO(g_dwfctb4_probe)
}

int launch_ffn_dwfc_tb4(const DwFcArgs& a, int prec, hipStream_t s) {
  using namespace tb4;
  DwFcArgs g = a;
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  const int64_t base = (int64_t)g.B * cdiv(g.H, TY) * cdiv(g.W, TX);
  int best_zs = g.D;
  int64_t best = -1;
  for (int nz = 1; nz <= 8 && nz <= g.D; ++nz) {
    const int zs = (int)cdiv(g.D, nz);
    const int64_t cost = cdiv(base * cdiv(g.D, zs), cus) * (zs + 3);
    if (best < 0 || cost < best) {
      best = cost;
      best_zs = zs;
    }
  }
  g.ZS = best_zs;
  g.dbg = ffn_dbg_env();
  const int64_t blocks = base * cdiv(g.D, g.ZS);
  if (prec != PREC_SPLIT && prec != PREC_FP16) return fail(WF_E_SHAPE, "ffn_dwfc_tb4: fp32 h1 only");
  if (!ffn_dwfc_tb4_fits(g.B, g.D, g.H, g.W))
    return fail(WF_E_SHAPE, "ffn_dwfc_tb4: tensor beyond the 2 GiB buffer-offset range");
  void (*kern)(DwFcArgs) = prec == PREC_SPLIT ? ffn_dwfc_tb4_kernel<PREC_SPLIT>
                                              : ffn_dwfc_tb4_kernel<PREC_FP16>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), 0, s, g);  // static LDS
  return check_launch("ffn_dwfc_tb4");
}

}  // namespace wf
