// ffn_dwfc2_tb.hip -- ffn_dwfc2_tb, the default stage-2 CCF_FFN back half (C = 96, hidden = 384;
// SURVEY 8a a8) on the wave layout of ffn_dwfc_tb4 (ffn_dwfc_tb.hip): three depthwise waves per
// SIMD that own nothing else, and one E wave per SIMD for staging, fc and epilogue.
//
//   h2  = dwconv3x3x3(h1) + b          (wave_helper.py:285, groups = hidden, pad 1)
//   g   = GELU(LN_eps2(h2))            (:286-287)
//   ffn = fc(g) + fc_b                 (:289)
//   out = x + (n2 + ffn) * bs          (Block residual + CCF_FFN residual, quirk Q4, :293/:509)
//
// Why: in ffn_dwfc2_kernel (ffn_dwfc.hip) every one of the 12 waves owns depthwise lanes, so
// LN2 (4 waves, 24 channels per lane), the fc (6 waves), the plane staging through registers
// and its commit all sit on top of a full scatter share, and each of the three barrier
// intervals of a plane is bound by one role while the others wait 2-3 k cycles
// (profiles/r3_dwfc2/phase_times_split27.txt).  Here, per 4 x 4 tile and plane:
//
//   D waves (12 = 3 per SIMD): lane = (channel c, column pair xp); the 27 taps in VGPRs; the
//        6 x 4 plane inputs read into 24 VGPRs right after the barrier that makes the plane
//        visible, so the one LDS plane buffer is only a landing zone; the depthwise fmaf chain
//        of ffn_dwfc2_kernel on rolling (renamed, not moved) accumulators.  The slot-0 / slot-1
//        waves of each SIMD (8 waves) run LN2 + GELU + split of the 16-position h2 tile, 32
//        lanes x 12 channels per position; the slot-2 wave scatters its first S2 rows meanwhile.
//   E waves (4 = 1 per SIMD, s_setprio 3): the haloed 6 x 6 x 384 fp32 plane staged by LDS-DMA
//        (buffer_load_dwordx4 ... lds through a per-plane descriptor; out-of-volume positions
//        and planes come back as zeros), the fc on v_mfma_f32_16x16x32 (x3 for bf16x3) + bias +
//        Q4 residual + range-checked 16-B buffer stores.
//
// The fc on four waves: the 6 column tiles x 12 k-steps are dealt tile-major, 18 units per E
// wave, so each wave keeps 72 VGPRs of weight-lo fragments for the whole march (hi from LDS as
// in ffn_dwfc2_kernel).  E wave 2 q owns tile 3 q and k-steps 0..5 of tile 3 q + 1; E wave
// 2 q + 1 owns k-steps 6..11 of tile 3 q + 1 and tile 3 q + 2.  The odd wave writes its 16 x 16
// partial of the straddled tile to a 1 KB LDS scratch; the even wave adds it (lower k half +
// upper k half, a fixed order) after the next barrier C and stores that tile then -- a barrier
// orders the scratch, there is no spin loop.  (The alternative, 3 k-steps per wave over all six
// tiles, needs a 24 KB reduction scratch LDS does not have.)
//
// LDS: 55,296 plane + 25,088 h2 tile (16 x 392 fp32, rewritten in place as bf16 {hi, lo}) +
// 75,264 fc weight hi (96 x 392 bf16) + 4,224 vectors + 2,048 scratch = 161,936 B: one plane
// buffer and one h2 tile, hence the barriers C, A, B per plane.  Iteration p (zo = p - 1):
//   C | D: fp32 h2 tile (zo) from the completed accumulators
//     | E: the straddled tile of zo - 1 (scratch + epilogue + store), its next residual rows;
//          wait until DMA(p + 1) has landed
//   A | D: load_plane(p + 1) into registers
//   A'| D: slots 0, 1: LN2 (zo); slot 2: scatter rows [0, S2)
//     | E: DMA(p + 2) into the plane buffer every D wave has read out
//   B | E: fc (zo) + epilogue + store of the whole tile; residual rows of zo + 1
//     | D: scatter plane p + 1 from registers
// (A' is a fourth barrier the LDS budget does not force: with three, the DMA could only be
// issued after B, in front of the fc, and the E waves' B -> C -- 14 DMA pieces, then 54
// dependent MFMAs -- took 4.7 k cycles per plane while they idled 3.4 k cycles between A and B:
// profiles/r8/.  The D waves reach A' a few hundred cycles after A.)
// The E waves' vector-memory counter retires in issue order and counts stores, so every E wave
// issues the same operations in every iteration (padded DMA pieces repeat the last piece,
// rows a wave does not own and planes outside the segment get an out-of-range offset): the
// one wait that matters, for the landed DMA before barrier A, is then the constant vmcnt(6).
// fp32 h1 only (bf16x3, fp16 modes) and outputs below 2 GiB (32-bit buffer offsets); the
// launcher keeps ffn_dwfc2_kernel for the rest.
#include "ffn_dwfc_common.hpp"

namespace wf {

#ifdef WF_DWFC2_PROBE
// diagnostic builds only: per-wave cycles of workgroup 0 by phase between the kernel's
// barriers (work, then wait), read back by wf_debug_dwfc2tb_probe
__device__ long long g_dwfc2tb_probe[16 * 8];
extern "C" int wf_debug_dwfc2tb_probe(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dwfc2tb_probe), sizeof(g_dwfc2tb_probe));
}
#endif

namespace tb2 {
constexpr int S2 = 4;  // input rows the third D wave of a SIMD scatters between A' and B
constexpr int C = 96, HID = 384, TY = 4, TX = 4;
constexpr int PY = TY + 2, PX = TX + 2, PP = PY * PX;  // 6 x 6
constexpr int NPOS = TY * TX;                          // 16
// h2 rows are HID + 8 floats apart (98 16-B quads, 2 mod 16): the fc's B-fragment
// ds_read_b128 (16 rows x 4 k-quads) meets 16 distinct 4-bank groups in each of its 16-lane
// groups {0-3, 12-15, 20-27}, ... (as tb4's HS).  LN2 lane lg of a row (32 lanes, one half
// wave) takes the channel quads lg, lg + 32, lg + 64: each 16-lane group of a ds_read_b128
// covers 16 consecutive quads modulo 16 whatever the row's offset, and the bf16 hi / lo
// ds_write_b64 of consecutive lanes are consecutive 8-byte words -- all conflict-free.
constexpr int HS = HID + 8, WKP = HID + 8;
constexpr int PLANE_F = PP * HID;
constexpr int H2F = NPOS * HS;
constexpr int NV = HID / 4;
constexpr int NPC = PP * NV / 64;                      // 54 LDS-DMA pieces of 1 KB
constexpr int NPCE = (NPC + 3) / 4;                    // 14 per E wave (two of them repeats)
constexpr int KS = HID / 32, KH = KS / 2;
constexpr int NVEC = 2 * HID + 3 * C;
constexpr size_t LDS_BYTES = (size_t)(PLANE_F + H2F + NVEC) * 4 + (size_t)C * WKP * 2 + 2 * 1024 + 16;
static_assert(PP * NV == NPC * 64 && PX * NV == 9 * 64, "whole pieces, 9 per haloed row");
static_assert(LDS_BYTES <= 160 * 1024, "LDS");
static_assert(HID * 28 <= PLANE_F, "depthwise weights and bias staged in the plane buffer");
}  // namespace tb2

template <int P>
__global__ __launch_bounds__(1024, 1) void ffn_dwfc2_tb_kernel(DwFcArgs a) {
  using namespace tb2;
  constexpr bool SPLIT = P == PREC_SPLIT;
  // separate static LDS objects, as in ffn_dwfc_tb4: the compiler's wait insertion can then
  // tell the plane the LDS-DMA writes from the h2 tile, weights and scratch the E waves read
  __shared__ __attribute__((aligned(16))) float plane[PLANE_F];   // [PP][HID]
  __shared__ __attribute__((aligned(16))) float h2t[H2F];         // [NPOS][HS]
  __shared__ __attribute__((aligned(16))) uint16_t wf[C * WKP];   // fc weight hi
  __shared__ __attribute__((aligned(16))) float vecs[NVEC];
  __shared__ f32x4 fcpart[2 * 64];                                // straddled-tile partials
  __shared__ int simd_cnt[4];
  float* lnw = vecs;                       // [HID] (halved: GELU from x / 2)
  float* lnb = lnw + HID;
  float* fcb = lnb + HID;                  // [C]
  float* n2w = fcb + C;
  float* n2b = n2w + C;

  const int tid = threadIdx.x;
  const int wid = tid >> 6, lane = tid & 63;
  const int D = a.D, H = a.H, W = a.W;
  const DwFcTile tl = dwfc_tile<TY, TX>(a);
  const int b = tl.b, x0 = tl.x0, y0 = tl.y0, z0 = tl.z0, z1 = tl.z1;
  const int plane_sz = H * W;

  if (tid < 4) simd_cnt[tid] = 0;
  for (int i = tid; i < C * (HID / 8); i += 1024) {
    const int n = i / (HID / 8), k8 = i % (HID / 8);
    *reinterpret_cast<bf16x8*>(wf + n * WKP + 8 * k8) =
        *reinterpret_cast<const bf16x8*>(a.fc + (size_t)n * HID + 8 * k8);
  }
  dwfc_stage_ln2<HID>(lnw, lnb, a, 1024);
  dwfc_stage_epi<C>(fcb, n2w, n2b, a, 1024);
  for (int i = tid; i < HID * 27; i += 1024) plane[i] = a.dw_w[i];
  for (int i = tid; i < HID; i += 1024) plane[HID * 27 + i] = a.dw_b[i];
  __syncthreads();
  const int role = dwfc_wave_role<4>(simd_cnt, wid, lane);  // 0..11 D, 12..15 E
  PROBE_DECL
#ifdef WF_DWFC2_PROBE
  pr_acc[6] = role;
#endif

  if (role < 12) {
    // ================================ D waves ===========================================
    const int xp = role / 6, kslot = role % 3, c = (role % 6) * 64 + lane;
    float w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = plane[c * 27 + k];
    const float bias = plane[HID * 27 + c];
    float acc[3][TY][2];  // output-plane accumulators, renamed every plane
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int o = 0; o < TY; ++o) acc[s][o][0] = acc[s][o][1] = 0.f;
    // LN2 (slots 0, 1): position 2 (2 simd' + kslot) + (lane >> 5), channel quads lg + 32 j
    const int lpos = 2 * (2 * (role / 3) + kslot) + (lane >> 5), lg = lane & 31;
    const float* q0 = plane + 2 * xp * HID + c;
    const int dbg = ffn_dbg(a);  // WF_FFN_DBG builds only

    // the 32 lanes of a row are one half of this wave
    auto ln2_rows = [&]() {
      dwfc_ln2_row<P, HID, 32, 128, false>(h2t + lpos * HS, 4 * lg, lnw, lnb, a.eps2);
    };
    auto load_plane = [&](float (&vin)[PY][4]) {
#pragma unroll
      for (int r = 0; r < PY; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) vin[r][k] = q0[(r * PX + k) * HID];
    };
    // input rows [LO, HI) into the output planes -1 (SA), 0 (SB), +1 (SC): the fmaf chain and
    // row order of ffn_dwfc2_kernel
    auto rows = [&](const float (&vin)[PY][4], auto SAc, auto SBc, auto SCc, auto LOc, auto HIc) {
      constexpr int SA = decltype(SAc)::value, SB = decltype(SBc)::value,
                    SC = decltype(SCc)::value, LO = decltype(LOc)::value, HI = decltype(HIc)::value;
      if (dbg & 1) return;
#pragma unroll
      for (int r = LO; r < HI; ++r) {
        const float u0 = vin[r][0], u1 = vin[r][1], u2 = vin[r][2], u3 = vin[r][3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int o = r - ky;
          if (o < 0 || o >= TY) continue;
          const float* w0 = w + ky * 3;
          acc[SC][o][0] = fmaf(w0[2], u2, fmaf(w0[1], u1, fmaf(w0[0], u0, acc[SC][o][0])));
          acc[SC][o][1] = fmaf(w0[2], u3, fmaf(w0[1], u2, fmaf(w0[0], u1, acc[SC][o][1])));
          acc[SB][o][0] = fmaf(w0[11], u2, fmaf(w0[10], u1, fmaf(w0[9], u0, acc[SB][o][0])));
          acc[SB][o][1] = fmaf(w0[11], u3, fmaf(w0[10], u2, fmaf(w0[9], u1, acc[SB][o][1])));
          acc[SA][o][0] = fmaf(w0[20], u2, fmaf(w0[19], u1, fmaf(w0[18], u0, acc[SA][o][0])));
          acc[SA][o][1] = fmaf(w0[20], u3, fmaf(w0[19], u2, fmaf(w0[18], u1, acc[SA][o][1])));
        }
      }
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    typedef std::integral_constant<int, S2> IS;
    typedef std::integral_constant<int, PY> IP;
    // iteration p: acc[R] holds output plane zo = p - 1, complete since scatter(p); plane p + 1
    // then goes into SA = R + 1, SB = R + 2 and SC = R (cleared)
    auto step = [&](int p, auto Rc) {
      constexpr int R = decltype(Rc)::value;
      typedef std::integral_constant<int, (R + 1) % 3> SA;
      typedef std::integral_constant<int, (R + 2) % 3> SB;
      typedef std::integral_constant<int, R> SC;
      const bool valid = p - 1 >= z0, more = p + 1 <= z1;
      __syncthreads();  // C: scatter(p) done everywhere, fc (zo - 1) done
      PROBE(5)
      if (valid) {
#pragma unroll
        for (int o = 0; o < TY; ++o)
#pragma unroll
          for (int q = 0; q < 2; ++q) h2t[(o * TX + 2 * xp + q) * HS + c] = acc[R][o][q] + bias;
      }
#pragma unroll
      for (int o = 0; o < TY; ++o) acc[R][o][0] = acc[R][o][1] = 0.f;
      PROBE(0)
      __syncthreads();  // A: fp32 h2 tile (zo) and plane p + 1 visible
      PROBE(1)
      float vin[PY][4];
      if (more) load_plane(vin);
      __syncthreads();  // A': plane p + 1 read out (the LDS reads have returned)
      PROBE(7)
      if (kslot < 2) {
        if (valid && !(dbg & 2)) ln2_rows();
      } else if (more) {
        rows(vin, SA(), SB(), SC(), I0(), IS());
      }
      PROBE(2)
      __syncthreads();  // B: bf16 {hi, lo} tile visible
      PROBE(3)
      if (more) {
        if (kslot < 2) rows(vin, SA(), SB(), SC(), I0(), IP());
        else rows(vin, SA(), SB(), SC(), IS(), IP());
      }
      PROBE(4)
    };
    __syncthreads();  // S1: weights read out of the plane buffer
    __syncthreads();  // S2: plane z0 - 1 staged
    {
      float vin[PY][4];
      load_plane(vin);
      __syncthreads();  // S3: plane z0 - 1 read out
      rows(vin, I0(), I1(), I2(), I0(), IP());
    }
    for (int p = z0 - 1; p <= z1; p += 3) {
      step(p, I0());
      if (p + 1 <= z1) step(p + 1, I1());
      if (p + 2 <= z1) step(p + 2, I2());
    }
    __syncthreads();  // C': the last straddled partial visible to its owner
    PROBE_DUMP_TO(g_dwfc2tb_probe)
    return;
  }

  // ================================== E waves ============================================
  __builtin_amdgcn_s_setprio(3);
  const int e = role - 12;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int pair = e >> 1;
  const bool upper = e & 1;                       // holds k-steps KH.. of the straddled tile
  const int tf = 3 * pair + (upper ? 2 : 0);      // this wave's whole column tile
  const int th = 3 * pair + 1;                    // the straddled tile
  const int kh0 = upper ? KH : 0;
  const int colf = tf * 16 + 4 * g4, colh = th * 16 + 4 * g4;
  const float bs = __builtin_bit_cast(
      float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.bscale ? a.bscale[b] : 1.f)));
  const int dbg = ffn_dbg(a);
  // weight lo fragments (18 units, 72 VGPRs) for the whole march
  bf16x8 fwf[KS], fwh[KH];
  {
    const uint16_t* wr = a.fc + (size_t)(C + tf * 16 + l15) * HID + 8 * g4;
    const uint16_t* wh = a.fc + (size_t)(C + th * 16 + l15) * HID + 8 * g4 + kh0 * 32;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      fwf[ks] = SPLIT ? *reinterpret_cast<const bf16x8*>(wr + ks * 32) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < KH; ++ks)
      fwh[ks] = SPLIT ? *reinterpret_cast<const bf16x8*>(wh + ks * 32) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const float* src = reinterpret_cast<const float*>(a.h1) + (int64_t)b * D * plane_sz * HID;
  const int64_t plane_elems = (int64_t)plane_sz * HID;
  // plane p into the plane buffer: NPCE pieces per wave whatever e is (the padded ones repeat
  // the last piece: same bytes to the same place); planes outside the volume or past the
  // segment's halo get a zero-range descriptor, positions outside the volume an out-of-range
  // offset.  A haloed row of the plane is 6 x 384 floats = 9 pieces, contiguous in h1: piece j
  // is part q = j % 9 of row j / 9, and its 32-lane halves lie in x positions 2 (q / 3) +
  // (q % 3 == 2) and 2 (q / 3) + (q % 3 >= 1) of the row.  All of that is scalar: the row's
  // byte offset goes into the instruction's scalar offset (the descriptor starts one position
  // before the plane so it is never negative) and a lane's offset is 16 lane or out of range --
  // three VALU instructions per piece instead of ~25 for per-lane offsets (the launch time is the
  // same; this form needs no SGPR spills).  `ln` and `es` are opaque so nothing
  // per piece is hoisted out of the plane loop into VGPRs the fc needs.
  auto stage = [&](int p) {
    const bool pz = p >= 0 && p < D && p <= z1 && !(dbg & 8);
    const float* base = src + (int64_t)min(max(p, 0), D - 1) * plane_elems - HID;
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(base, pz ? (int)((plane_elems + HID) * 4) : 0);
    int ln = lane, es = e;
    asm volatile("" : "+v"(ln), "+s"(es));
    const int l16 = ln * 16, hbit = ln >= 32 ? 2 : 1;
#pragma unroll
    for (int k = 0; k < NPCE; ++k) {
      const int j = min(4 * k + es, NPC - 1);
      const int r = j / 9, q = j - 9 * r, m = q / 3, q3 = q - 3 * m;
      const int yy = y0 - 1 + r;
      const int xlo = x0 - 1 + 2 * m + (q3 == 2), xhi = x0 - 1 + 2 * m + (q3 >= 1);
      const bool rowok = yy >= 0 && yy < H;
      // bit 0 / 1: the lower / upper 32 lanes are inside the volume (a scalar)
      const int okbits = (rowok && xlo >= 0 && xlo < W ? 1 : 0) | (rowok && xhi >= 0 && xhi < W ? 2 : 0);
      const int voff = (okbits & hbit) ? l16 : BUF_OOR;
      const int soff = (max(yy, 0) * W + x0) * (HID * 4) + q * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs, (__attribute__((address_space(3))) void*)(plane + j * 256), 16, voff, soff, 0, 0);
    }
  };
  // this lane's fc row: tile position l15; everything through 32-bit buffer offsets (the
  // launcher keeps the tensors under 2 GiB)
  const int yo = y0 + l15 / TX, xo = x0 + l15 % TX;
  const bool rv = yo < H && xo < W;
  const int gpos0 = b * D * plane_sz + min(yo, H - 1) * W + min(xo, W - 1);
  const float* sbase = a.stats ? a.stats : a.x;
  const int64_t npos = (int64_t)a.B * D * plane_sz;
  const __amdgpu_buffer_rsrc_t xrsrc = buf_rsrc(a.x, (int)(npos * C * 4));
  const __amdgpu_buffer_rsrc_t srsrc = buf_rsrc(sbase, (int)(npos * 2 * 4));
  const __amdgpu_buffer_rsrc_t orsrc = buf_rsrc(a.out, (int)(npos * C * 4));
  f32x4 xrf = f32x4{0.f, 0.f, 0.f, 0.f}, xrh = xrf;  // residual rows: whole / straddled tile
  f32x2 esf = f32x2{0.f, 1.f}, esh = esf;
  // residual + statistics rows of output plane z (clamped: a plane outside the segment is
  // never used); `own` false -> out-of-range offsets, zeros come back without a memory access
  auto load_resid = [&](int z, int col, bool own, f32x4& xv, f32x2& ev) {
    const int g = gpos0 + min(max(z, 0), D - 1) * plane_sz;
    xv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                       xrsrc, own ? (g * C + col) * 4 : BUF_OOR, 0, 0));
    ev = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(srsrc, own ? g * 8 : BUF_OOR, 0, 0));
  };
  // the epilogue + a range-checked store (dropped when !ok)
  auto epi_store = [&](f32x4 acc, int z, int col, bool ok, const f32x4& xv, const f32x2& ev) {
    const f32x4 v = dwfc_epilogue(acc, fcb, n2w, n2b, col, xv, ev, bs, a.stats != nullptr);
    const int voff = ok ? ((gpos0 + z * plane_sz) * C + col) * 4 : BUF_OOR;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), orsrc, voff, 0, 0);
  };
  f32x4 acch = f32x4{0.f, 0.f, 0.f, 0.f};  // this wave's k half of the straddled tile
  // the straddled tile of output plane z: lower k half + upper k half, epilogue, store, then
  // its residual rows for z + 1 (one store + two loads on every E wave)
  auto finish_half = [&](int z) {
    const f32x4 part = fcpart[pair * 64 + lane];
    epi_store(acch + part, z, colh, !upper && rv && z >= z0, xrh, esh);
    load_resid(z + 1, colh, !upper, xrh, esh);
  };
  const uint16_t* Bh = reinterpret_cast<const uint16_t*>(h2t) + (size_t)l15 * (2 * HS) + 8 * g4;
  const uint16_t* Wf = wf + (size_t)(tf * 16 + l15) * WKP + 8 * g4;
  const uint16_t* Wh = wf + (size_t)(th * 16 + l15) * WKP + 8 * g4;
  auto lds8 = [](const uint16_t* q) { return *reinterpret_cast<const bf16x8*>(q); };
  // both tiles of this wave over the LN2'd h2 tile.  The straddled tile's k-steps are the whole
  // tile's steps 0..5 (even E waves) or 6..11 (odd) and use the lo fragments 0..5 either way.
  // The two accumulator chains are independent (each keeps its own k order): interleaved, one's
  // MFMA latency hides the other's.
  auto fc = [&](f32x4& accf) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      {
        const bf16x8 bh = lds8(Bh + ks * 32), bl = lds8(Bh + (SPLIT ? HID : 0) + ks * 32);
        accf = mma3<P>(accf, lds8(Wf + ks * 32), fwf[ks], bh, bl);
      }
      if (ks < KH) {
        const int k = (kh0 + ks) * 32;
        const bf16x8 bh = lds8(Bh + k), bl = lds8(Bh + (SPLIT ? HID : 0) + k);
        acch = mma3<P>(acch, lds8(Wh + k), fwh[ks], bh, bl);
      }
    }
  };

  __syncthreads();  // S1: weights read out of the plane buffer
  stage(z0 - 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // S2: plane z0 - 1 staged
  // the loop's issue order from the start: (1 store, 2 loads), the plane DMA, (1 store, 2
  // loads); nothing of these first sets is used
  finish_half(z0 - 3);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // S3: plane z0 - 1 read out
  stage(z0);
  asm volatile("" ::: "memory");
  epi_store(acch, z0 - 2, colf, false, xrf, esf);
  load_resid(z0 - 2, colf, true, xrf, esf);
  for (int p = z0 - 1; p <= z1; ++p) {
    const int zo = p - 1;
    const bool valid = zo >= z0;
    __builtin_amdgcn_s_barrier();  // C (bare, as in tb4: a fence here would drain vmcnt)
    PROBE(5)
    finish_half(zo - 1);
    // outstanding, oldest first: DMA(p + 1) x 14 | store, 2 loads | store, 2 loads
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PROBE(0)
    __builtin_amdgcn_s_barrier();  // A: plane p + 1 landed
    PROBE(1)
    __builtin_amdgcn_s_barrier();  // A': every D wave has read the plane out
    PROBE(7)
    stage(p + 2);
    asm volatile("" ::: "memory");  // the DMA stays ahead of the store and loads below
    PROBE(2)
    __builtin_amdgcn_s_barrier();  // B: LN2'd tile (zo) visible
    PROBE(3)
    f32x4 accf = f32x4{0.f, 0.f, 0.f, 0.f};
    acch = accf;
    if (!(dbg & 4)) {
      fc(accf);
      if (upper) fcpart[pair * 64 + lane] = acch;
    }
    asm volatile("" ::: "memory");
    epi_store(accf, zo, colf, rv && valid, xrf, esf);
    load_resid(zo + 1, colf, true, xrf, esf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PROBE(4)
  }
  __builtin_amdgcn_s_barrier();  // C'
  finish_half(z1 - 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PROBE_DUMP_TO(g_dwfc2tb_probe)
}

int launch_ffn_dwfc2_tb(const DwFcArgs& g, int prec, hipStream_t s) {
  using namespace tb2;
  if (prec != PREC_SPLIT && prec != PREC_FP16) return fail(WF_E_SHAPE, "ffn_dwfc2_tb: fp32 h1 only");
  if (!ffn_dwfc2_tb_fits(g))
    return fail(WF_E_SHAPE, "ffn_dwfc2_tb: tensor beyond the 2 GiB buffer-offset range");
  const int64_t blocks =
      (int64_t)g.B * cdiv(g.H, TY) * cdiv(g.W, TX) * cdiv(g.D, g.ZS);
  void (*kern)(DwFcArgs) = prec == PREC_SPLIT ? ffn_dwfc2_tb_kernel<PREC_SPLIT>
                                              : ffn_dwfc2_tb_kernel<PREC_FP16>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), 0, s, g);  // static LDS
  return check_launch("ffn_dwfc2_tb");
}

}  // namespace wf
