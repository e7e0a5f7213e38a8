// ffn_dwfc2_tb.hip -- ffn_dwfc2_tb, the default stage-2 CCF_FFN back half (C = 96, hidden = 384;
// SURVEY 8a a8) on the wave layout and the two-barrier schedule of ffn_dwfc_tb4
// (ffn_dwfc_tb.hip): three depthwise waves per SIMD that own nothing else, and one E wave per
// SIMD for the fc and the epilogue.
//
//   h2  = dwconv3x3x3(h1) + b          (wave_helper.py:285, groups = hidden, pad 1)
//   g   = GELU(LN_eps2(h2))            (:286-287)
//   ffn = fc(g) + fc_b                 (:289)
//   out = x + (n2 + ffn) * bs          (Block residual + CCF_FFN residual, quirk Q4, :293/:509)
//
// Per 4 x 4 tile, z-marching through ZS planes:
//
//   D waves (12 = 3 per SIMD): lane = (channel c, column pair xp); the 27 taps in VGPRs; the
//        6 x 4 haloed inputs of a plane come STRAIGHT FROM h1 INTO 24 VGPRs, one
//        buffer_load_dword per (row, column): 64 consecutive channels, one 256-B wave access.
//        No LDS plane, no LDS-DMA.  Everything but the channel is scalar: the plane's
//        descriptor starts one position before the plane (never a negative offset), the row /
//        column byte offset is the instruction's scalar offset, the lane's offset is 4 c, and a
//        (row, column) outside the volume, or a plane outside the volume or past the segment's
//        halo, is loaded through the same descriptor with range 0, so zeros come back without a
//        memory access (one s_bitcmp + s_cselect per load, no VALU, no extra VGPR).
//        Row r of plane p + 1 is requested right behind the fmaf block that consumed row r of
//        plane p, into the same four registers, so every row is a whole plane iteration in
//        flight: 24 loads outstanding per wave, and the waits in front of a row's four inputs
//        are vmcnt(23) .. vmcnt(20) -- the compiler's own counts, exact because the D waves
//        issue no other vector memory and the LN2 slots and the slot-2 waves run separate
//        loops (no merged wait state).
//        The depthwise fmaf chain is ffn_dwfc2_kernel's, on rolling (renamed, not moved)
//        accumulators.  The slot-0 / slot-1 waves of each SIMD (8 waves) run LN2 + GELU + split
//        of the 16-position h2 tile, 32 lanes x 12 channels per position.
//   E waves (4 = 1 per SIMD, s_setprio 3): the fc on v_mfma_f32_16x16x32 (x3 for bf16x3) + bias
//        + Q4 residual + range-checked 16-B buffer stores, the residual rows one plane ahead.
//
// The fc on four waves: the 6 column tiles x 12 k-steps are dealt tile-major, 18 units per E
// wave, so each wave keeps 72 VGPRs of weight-lo fragments for the whole march (hi from LDS as
// in ffn_dwfc2_kernel).  E wave 2 q owns tile 3 q and k-steps 0..5 of tile 3 q + 1; E wave
// 2 q + 1 owns k-steps 6..11 of tile 3 q + 1 and tile 3 q + 2.  The odd wave writes its 16 x 16
// partial of the straddled tile to a 1 KB LDS scratch in phase 1; the even wave adds it (lower
// k half + upper k half, a fixed order) in phase 2 and stores that tile then -- the two barriers
// order the scratch, there is no spin loop.
//
// LDS: 2 x 25,088 h2 tiles (16 x 392 fp32, rewritten in place as bf16 {hi, lo}) + 75,264 fc
// weight hi (96 x 392 bf16) + 4,224 vectors + 2,048 scratch = 131,728 B.  Two h2 tiles, two
// barriers per plane.  Iteration p (p = z0 - 1 .. z1 + 1), tile t in buffer (t - z0) & 1:
//   phase 1 | D slots 0, 1: LN2 of tile p - 2
//           | D slot 2: scatter rows [0, S2) of plane p (and request those rows of p + 1)
//           | E: fc of tile p - 3, epilogue + store of the whole column tile, the odd wave's
//           |    partial to the scratch, residual rows of p - 2
//   phase 2 | D: scatter the other rows of plane p (request them of p + 1); fp32 h2 tile p - 1
//           |    from the completed accumulators into the buffer the fc has just left
//           | E: the straddled tile of p - 3 (scratch + epilogue + store), its next residual rows
// and the fc of the last tile behind the loop.  The fc of tile t thus runs beside LN2 of tile
// t + 1 (tb4's "fc half an iteration late").  All barriers are bare s_barriers behind
// lgkmcnt(0): __syncthreads()' fence would drain the loads and stores in flight.
// fp32 h1 only (bf16x3, fp16 modes) and tensors below 2 GiB (32-bit buffer offsets: x, out and
// one haloed h1 plane); the launcher keeps ffn_dwfc2_kernel for the rest.
#include "ffn_dwfc_common.hpp"

namespace wf {

#ifdef WF_DWFC2_PROBE
// diagnostic builds only: per-wave cycles of workgroup 0 by phase (tools/dwfc2_phase_times.py):
// slot 0 phase-1 work, 1 wait at barrier 1, 2 phase-2 work, 3 wait at barrier 2, 4 (D) the wait
// for the first input row of the plane (vmcnt), 6 role, 7 iterations; read back by
// wf_debug_dwfc2tb_probe
__device__ long long g_dwfc2tb_probe[16 * 8];
extern "C" int wf_debug_dwfc2tb_probe(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dwfc2tb_probe), sizeof(g_dwfc2tb_probe));
}
// the first row's inputs have landed: separates the wait for memory from the scatter
#define PROBE_VMWAIT asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); PROBE(4)
#else
#define PROBE_VMWAIT
#endif

namespace tb2 {
constexpr int S2 = 6;  // input rows the third D wave of a SIMD scatters in phase 1
constexpr int C = 96, HID = 384, TY = 4, TX = 4;
constexpr int PY = TY + 2;                             // 6 haloed rows, 4 columns per column pair
constexpr int NPOS = TY * TX;                          // 16
// h2 rows are HID + 8 floats apart (98 16-B quads, 2 mod 16): the fc's B-fragment
// ds_read_b128 (16 rows x 4 k-quads) meets 16 distinct 4-bank groups in each of its 16-lane
// groups {0-3, 12-15, 20-27}, ... (as tb4's HS).  LN2 lane lg of a row (32 lanes, one half
// wave) takes the channel quads lg, lg + 32, lg + 64: each 16-lane group of a ds_read_b128
// covers 16 consecutive quads modulo 16 whatever the row's offset, and the bf16 hi / lo
// ds_write_b64 of consecutive lanes are consecutive 8-byte words -- all conflict-free.
constexpr int HS = HID + 8, WKP = HID + 8;
constexpr int H2F = NPOS * HS;
constexpr int KS = HID / 32, KH = KS / 2;
constexpr int NVEC = 2 * HID + 3 * C;
constexpr size_t LDS_BYTES = (size_t)(2 * H2F + NVEC) * 4 + (size_t)C * WKP * 2 + 2 * 1024 + 16;
static_assert(LDS_BYTES <= 160 * 1024, "LDS");
static_assert(HID * 28 <= 2 * H2F, "depthwise weights and bias staged in the h2 tiles");
static_assert(S2 >= 0 && S2 <= PY, "S2");
}  // namespace tb2

template <int P>
__global__ __launch_bounds__(1024, 1) void ffn_dwfc2_tb_kernel(DwFcArgs a) {
  using namespace tb2;
  constexpr bool SPLIT = P == PREC_SPLIT;
  __shared__ __attribute__((aligned(16))) float h2b[2 * H2F];     // [2][NPOS][HS]
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
  for (int i = tid; i < HID * 27; i += 1024) h2b[i] = a.dw_w[i];
  for (int i = tid; i < HID; i += 1024) h2b[HID * 27 + i] = a.dw_b[i];
  __syncthreads();
  const int role = dwfc_wave_role<4>(simd_cnt, wid, lane);  // 0..11 D, 12..15 E
  PROBE_DECL
#ifdef WF_DWFC2_PROBE
  pr_acc[6] = role;
  pr_acc[7] = z1 + 3 - z0;
#endif
  // every barrier of the march: this wave's LDS accesses complete, nothing else drained
  auto bar = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  if (role < 12) {
    // ================================ D waves ===========================================
    const int xp = role / 6, kslot = role % 3, c = (role % 6) * 64 + lane;
    float w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = h2b[c * 27 + k];
    const float bias = h2b[HID * 27 + c];
    float acc[3][TY][2];  // output-plane accumulators, renamed every plane
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int o = 0; o < TY; ++o) acc[s][o][0] = acc[s][o][1] = 0.f;
    // LN2 (slots 0, 1): position 2 (2 simd' + kslot) + (lane >> 5), channel quads lg + 32 j
    const int lpos = 2 * (2 * (role / 3) + kslot) + (lane >> 5), lg = lane & 31;
    const int dbg = ffn_dbg(a);  // WF_FFN_DBG builds only

    // ---- the direct loads.  Input (r, k) of plane p is h1[b, p, y0 - 1 + r, x0 - 1 + 2 xp + k,
    // c]; the descriptor of plane p starts one position (HID floats) before the plane.
    const float* src = reinterpret_cast<const float*>(a.h1) + (int64_t)b * D * plane_sz * HID;
    const int64_t plane_elems = (int64_t)plane_sz * HID;
    const int plane_bytes = (int)((plane_elems + HID) * 4);
    const int c4 = 4 * c;
    int rowoff[PY], okmask = 0;  // scalar: a row's byte offset; bit 4 r + k: (r, k) inside
#pragma unroll
    for (int r = 0; r < PY; ++r) {
      const int yy = y0 - 1 + r;
      rowoff[r] = (min(max(yy, 0), H - 1) * W + x0 + 2 * xp) * (HID * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xx = x0 - 1 + 2 * xp + k;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) okmask |= 1 << (4 * r + k);
      }
    }
    // what selects plane p's descriptor: its base and the (r, k) it may read (none for a plane
    // outside the volume or past the segment's halo plane z1).  `mk` is opaque so the per-load
    // ranges are made where they are used, not hoisted out of the plane loop into 24 registers.
    struct PlaneSel {
      const float* base;
      int mk;
    };
    auto plane_sel = [&](int p) {
      PlaneSel s;
      s.base = src + (int64_t)min(max(p, 0), D - 1) * plane_elems - HID;
      s.mk = (p >= 0 && p < D && p <= z1 && !(dbg & 8)) ? okmask : 0;
      asm volatile("" : "+s"(s.mk));
      return s;
    };
    auto load_row = [&](float (&v)[4], int r, const PlaneSel& s) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rng = (s.mk >> (4 * r + k)) & 1 ? plane_bytes : 0;
        v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                             buf_rsrc(s.base, rng), c4, rowoff[r] + k * (HID * 4), 0));
      }
    };
    // input rows [LO, HI) of the plane in vin into the output planes -1 (SA), 0 (SB), +1 (SC):
    // the fmaf chain and row order of ffn_dwfc2_kernel; behind each row, that row of the next
    // plane is requested into the registers just consumed
    auto rows = [&](float (&vin)[PY][4], const PlaneSel& nx, auto SAc, auto SBc, auto SCc, auto LOc,
                    auto HIc) {
      constexpr int SA = decltype(SAc)::value, SB = decltype(SBc)::value,
                    SC = decltype(SCc)::value, LO = decltype(LOc)::value, HI = decltype(HIc)::value;
#pragma unroll
      for (int r = LO; r < HI; ++r) {
        if (!(dbg & 1)) {
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
        // pinned between the row's fmaf block and the next row's: the chain is pure arithmetic
        // the compiler may otherwise sink past the barrier into the other phase, or past the
        // loads, which then need a second set of input registers
#pragma unroll
        for (int o = 0; o < TY; ++o)
          if (o <= r && o >= r - 2)
            asm volatile(""
                         : "+v"(acc[SA][o][0]), "+v"(acc[SA][o][1]), "+v"(acc[SB][o][0]),
                           "+v"(acc[SB][o][1]), "+v"(acc[SC][o][0]), "+v"(acc[SC][o][1])
                         :
                         : "memory");
        __builtin_amdgcn_sched_barrier(0);
        load_row(vin[r], r, nx);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    typedef std::integral_constant<int, S2> IS;
    typedef std::integral_constant<int, PY> IP;
    float vin[PY][4];
    // Every iteration runs the same instructions (the plane behind the halo plane z1 is loaded
    // through range 0 and scattered as zeros into accumulators nobody reads), so a loaded
    // register is never merged with an older value and nothing is moved or waited for between
    // iterations.
    // iteration p scatters plane p into SA = R (output plane p - 1, complete with it), SB =
    // R + 1 (plane p) and SC = R + 2 (plane p + 1, cleared one iteration ago); then acc[R] + bias
    // is the fp32 h2 tile p - 1.  LN: this wave runs LN2 in phase 1 and its scatter in phase 2
    // (slots 0, 1); else it scatters rows [0, S2) in phase 1 (slot 2).
    auto step = [&](int p, auto Rc, auto LNc) {
      constexpr int R = decltype(Rc)::value;
      constexpr bool LN = decltype(LNc)::value;
      typedef std::integral_constant<int, R> SA;
      typedef std::integral_constant<int, (R + 1) % 3> SB;
      typedef std::integral_constant<int, (R + 2) % 3> SC;
      const PlaneSel nx = plane_sel(p + 1);
      // ---- phase 1
      if (LN) {
        if (p - 2 >= z0 && p - 2 < z1 && !(dbg & 2))
          dwfc_ln2_row<P, HID, 32, 128, false>(h2b + ((p - 2 - z0) & 1) * H2F + lpos * HS, 4 * lg,
                                               lnw, lnb, a.eps2);
      } else {
        PROBE_VMWAIT
        rows(vin, nx, SA(), SB(), SC(), I0(), IS());
      }
      PROBE(0)
      bar();  // 1 -> 2: LN2'd tile (p - 2) visible; the fc has left the buffer of tile p - 1
      PROBE(1)
      // ---- phase 2
      if (LN) {
        PROBE_VMWAIT
        rows(vin, nx, SA(), SB(), SC(), I0(), IP());
      } else {
        rows(vin, nx, SA(), SB(), SC(), IS(), IP());
      }
      if (p - 1 >= z0 && p - 1 < z1) {
        float* h2t = h2b + ((p - 1 - z0) & 1) * H2F;
#pragma unroll
        for (int o = 0; o < TY; ++o)
#pragma unroll
          for (int q = 0; q < 2; ++q) h2t[(o * TX + 2 * xp + q) * HS + c] = acc[R][o][q] + bias;
      }
#pragma unroll
      for (int o = 0; o < TY; ++o) acc[R][o][0] = acc[R][o][1] = 0.f;
      PROBE(2)
      bar();  // 2 -> next 1: fp32 h2 tile (p - 1) visible
      PROBE(3)
    };
    auto march = [&](auto LNc) {
      for (int p = z0 - 1; p <= z1 + 1; p += 3) {
        step(p, I0(), LNc);
        if (p + 1 <= z1 + 1) step(p + 1, I1(), LNc);
        if (p + 2 <= z1 + 1) step(p + 2, I2(), LNc);
      }
    };
    __syncthreads();  // (prologue) weights read out of the h2 tiles
    {
      const PlaneSel first = plane_sel(z0 - 1);
#pragma unroll
      for (int r = 0; r < PY; ++r) load_row(vin[r], r, first);
    }
    if (kslot < 2) march(std::true_type());
    else march(std::false_type());
    bar();  // (tail) the last straddled partial visible to its owner
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
  const uint16_t* Wf = wf + (size_t)(tf * 16 + l15) * WKP + 8 * g4;
  const uint16_t* Wh = wf + (size_t)(th * 16 + l15) * WKP + 8 * g4;
  auto lds8 = [](const uint16_t* q) { return *reinterpret_cast<const bf16x8*>(q); };
  // both tiles of this wave over the LN2'd h2 tile of output plane z.  The straddled tile's
  // k-steps are the whole tile's steps 0..5 (even E waves) or 6..11 (odd) and use the lo
  // fragments 0..5 either way.  The two accumulator chains are independent (each keeps its own
  // k order): interleaved, one's MFMA latency hides the other's.  Then the whole tile's
  // epilogue + store and its residual rows for z + 1; the odd wave's partial to the scratch.
  auto fc_tile = [&](int z) {
    const uint16_t* Bh = reinterpret_cast<const uint16_t*>(h2b + ((z - z0) & 1) * H2F) +
                         (size_t)l15 * (2 * HS) + 8 * g4;
    f32x4 accf = f32x4{0.f, 0.f, 0.f, 0.f};
    acch = accf;
    if (!(dbg & 4)) {
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
      if (upper) fcpart[pair * 64 + lane] = acch;
    }
    asm volatile("" ::: "memory");
    epi_store(accf, z, colf, rv && z >= z0, xrf, esf);
    load_resid(z + 1, colf, true, xrf, esf);
  };

  // the lo fragments have landed before the march: its waits then count only its own loads
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(fwf[ks]));
#pragma unroll
  for (int ks = 0; ks < KH; ++ks) asm volatile("" : "+v"(fwh[ks]));
  __syncthreads();  // (prologue) weights read out of the h2 tiles
  // iteration p: tile zo = p - 3 (LN2'd in phase 1 of iteration p - 1; its buffer is next
  // written, with the fp32 tile zo + 2, in phase 2 of this iteration, behind barrier 1).  The
  // tiles before z0 are computed from whatever the buffers hold and never stored, so every E
  // wave issues the same vector-memory operations in every iteration and the waits for the
  // residual rows (the compiler's) never wait for more than those rows.
  for (int p = z0 - 1; p <= z1 + 1; ++p) {
    const int zo = p - 3;
    fc_tile(zo);
    PROBE(0)
    bar();  // 1 -> 2
    PROBE(1)
    finish_half(zo);
    PROBE(2)
    bar();  // 2 -> next 1
    PROBE(3)
  }
  // the last tile, z1 - 1 (LN2'd in phase 1 of the last iteration), behind the last barrier
  fc_tile(z1 - 1);
  bar();  // (tail)
  finish_half(z1 - 1);
  PROBE_DUMP_TO(g_dwfc2tb_probe)
}

int launch_ffn_dwfc2_tb(const DwFcArgs& g, int prec, hipStream_t s) {
  using namespace tb2;
  if (prec != PREC_SPLIT && prec != PREC_FP16) return fail(WF_E_SHAPE, "ffn_dwfc2_tb: fp32 h1 only");
  if (!ffn_dwfc2_tb_fits(g.B, g.D, g.H, g.W))
    return fail(WF_E_SHAPE, "ffn_dwfc2_tb: tensor beyond the 2 GiB buffer-offset range");
  const int64_t blocks =
      (int64_t)g.B * cdiv(g.H, TY) * cdiv(g.W, TX) * cdiv(g.D, g.ZS);
  void (*kern)(DwFcArgs) = prec == PREC_SPLIT ? ffn_dwfc2_tb_kernel<PREC_SPLIT>
                                              : ffn_dwfc2_tb_kernel<PREC_FP16>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), 0, s, g);  // static LDS
  return check_launch("ffn_dwfc2_tb");
}

}  // namespace wf
