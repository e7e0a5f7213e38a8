// ffn_dwfc3_tb.hip -- ffn_dwfc3_tb, the stage-3 CCF_FFN back half (C = 192, hidden = 768) in one
// kernel, on the wave layout of ffn_dwfc2_tb (ffn_dwfc2_tb.hip): three depthwise waves per SIMD
// that own nothing else, and one E wave per SIMD for the fc and the epilogue.
//
//   h2  = dwconv3x3x3(h1) + b          (wave_helper.py:285, groups = hidden, pad 1)
//   g   = GELU(LN_eps2(h2))            (:286-287)
//   ffn = fc(g) + fc_b                 (:289)
//   out = x + (n2 + ffn) * bs          (Block residual + CCF_FFN residual, quirk Q4, :293/:509)
//
// What differs from stage 2 is the fc weight: 768 x 192 bf16 hi + lo = 590 KB does not fit in
// LDS, so it never touches it.  As in gemm_lnw (gemm_lnw.hip) each E wave streams its own
// columns from L2 straight into registers, ahead of the MFMAs that use them, with no barrier in
// the k loop; the whole weight is streamed once per tile-plane.  It is streamed from a copy in
// fragment order (dwfc3_fc_stream_kernel below, one small launch in front of this kernel), so
// that every load of a wave is 1 KB of consecutive bytes.
//
// Per 4 x 4 tile, z-marching through ZS planes:
//
//   D waves (12 = 3 per SIMD): wave d owns the hidden channels 64 d .. 64 d + 63, one per lane,
//        and the whole 4 x 4 tile: the 27 taps in VGPRs, three rolling (renamed, not moved)
//        accumulator sets of 16.  The 6 x 6 haloed inputs of a plane come STRAIGHT FROM h1, one
//        buffer_load_dword per (row, column): 64 consecutive channels, one 256-B wave access.
//        Everything but the channel is scalar, as in ffn_dwfc2_tb: the plane's descriptor starts
//        one position before the plane, the row / column byte offset is the instruction's scalar
//        offset, the lane's offset is 4 c, and a (row, column) outside the volume, or a plane
//        outside the volume or past the segment's halo, is loaded through the same descriptor
//        with range 0 (zeros come back without a memory access).  The inputs live in a ring of
//        three rows (18 VGPRs, not the plane's 36: with 48 accumulators and 27 taps a whole
//        plane does not fit beside LN2 in 128 registers): row r + 3 is requested right behind the
//        fmaf block that consumed row r, into the same six registers, so 18 loads (4.6 KB) are
//        outstanding per wave, 55 KB per CU.  Every iteration issues the same loads (the plane
//        behind the halo plane z1 goes through range 0), so the waits in front of a row are the
//        compiler's own counts.  The slot-0 / slot-1 waves of each SIMD (8 waves) run LN2 + GELU
//        + split of two rows of the 16-position h2 tile each, 64 lanes x 12 channels per row.
//        The accumulator set that becomes plane p + 1 is cleared behind LN2, so it is dead across
//        it: LN2's registers overlay it.
//   E waves (4 = 1 per SIMD, s_setprio 3): M = 16 positions, N = 48 columns (3 column tiles) each,
//        K = 768 in 24 k-steps of v_mfma_f32_16x16x32 (x3 for bf16x3, mma3's order).  The weight
//        fragments of a k-step (3 tiles x {hi, lo} = 24 VGPRs, 6 KB of consecutive bytes) come
//        through one buffer descriptor with 16 lane as the per-lane offset; a ring of three
//        k-steps keeps two steps (12 loads) in flight, and a step's registers are refilled one
//        step after its MFMAs issued.  The ring runs on across tiles (24 = 0 mod 3: steps 22 and
//        23 request steps 0 and 1 of the next tile).  The A fragments (the LN2'd h2 rows in LDS)
//        of a step are read behind the MFMAs of the step before (one pair: two would spill).
//        Then bias + Q4 residual (dwfc_epilogue) + range-checked 16-B buffer stores, the
//        residual rows one plane ahead.  Tiles before z0 are skipped, not computed: the weight
//        stream is what the E waves cost.
//
// LDS: 3 x 49,664 h2 tiles (16 x 776 fp32, rewritten in place as bf16 {hi, lo}) + 8,448 vectors
// = 157,456 B.  Three h2 tiles, two barriers per plane, so the fc of a tile has the whole
// iteration.  Iteration p (p = z0 - 1 .. z1 + 1), tile t in buffer (t - z0) mod 3:
//   phase 1 | D slots 0, 1: LN2 of tile p - 2
//           | D slot 2: scatter rows [0, S2) of plane p
//           | E: k-steps 0..11 of the fc of tile p - 3
//   phase 2 | D: scatter the other rows of plane p; fp32 h2 tile p - 1 from the completed
//           |    accumulators into the buffer of tile p - 4
//           | E: k-steps 12..23 of tile p - 3, epilogue + store, residual rows of p - 2
// and the fc of the last tile behind the loop.  All barriers are bare s_barriers behind
// lgkmcnt(0): __syncthreads()' fence would drain the loads and stores in flight.
// fp32 h1 only (bf16x3, fp16 modes) and tensors below 2 GiB (32-bit buffer offsets: x, out and
// one haloed h1 plane); wf_ccf_ffn_stage keeps the staged path for the rest.
//
// The z segment (launch_ffn_dwfc3): whole columns where that gives a workgroup per CU, halved
// while longer than 8 planes otherwise (B = 8 at 16^3: 16 tiles x 8 samples x 2 segments of 8).
// A plane's result does not depend on the segment: seam planes are loaded, not zero-filled.
#include "ffn_dwfc_common.hpp"

namespace wf {

namespace tb3 {
constexpr int S2 = 3;  // input rows the third D wave of a SIMD scatters in phase 1
constexpr int C = 192, HID = 768, TY = 4, TX = 4;
constexpr int PY = TY + 2, PX = TX + 2;                // 6 x 6 haloed inputs
constexpr int NPOS = TY * TX;                          // 16
constexpr int NR = 3;                                  // input rows in flight
// h2 rows are HID + 8 floats apart (194 16-B quads, 2 mod 16): the fc's A-fragment
// ds_read_b128 (16 rows x 4 k-quads) meets distinct 4-bank groups in each of its 16-lane
// groups, as in ffn_dwfc2_tb.  LN2 lane l of a row takes the channel quads l, l + 64, l + 128.
constexpr int HS = HID + 8;
constexpr int H2F = NPOS * HS;
constexpr int NT = 3;                                  // h2 tiles
constexpr int KS = HID / 32, KH = KS / 2;              // 24 k-steps, 12 per phase
constexpr int NTW = C / 64;                            // 3 column tiles per E wave
constexpr int NVEC = 2 * HID + 3 * C;
constexpr size_t LDS_BYTES = (size_t)(NT * H2F + NVEC) * 4 + 16;
static_assert(LDS_BYTES <= 160 * 1024, "LDS");
static_assert(HID * 28 <= NT * H2F, "depthwise weights and bias staged in the h2 tiles");
static_assert(S2 >= 0 && S2 <= PY, "S2");
static_assert(KS % NR == 0 && KH % NR == 0, "the weight ring keeps its phase across tiles and halves");
}  // namespace tb3

// The fc weight [NPL][C][HID] (bf16 / fp16 hi, and lo for bf16x3) in the order the E waves
// stream it: [E wave e][k-step ks][column tile t][plane pl][lane] fragments of 16 B, the lane's
// MFMA operand (row 48 e + 16 t + l15, k = 32 ks + 8 g4 .. + 7).  Read in place, a fragment
// load touches 16 rows 1,536 B apart, 64 B of each: measured at 2,000 cycles per k-step on the
// E waves (a fifth of the L2 -> CU rate).  In this order every load is 1 KB of
// consecutive bytes.  One thread per fragment; runs in front of every launch (the weight may
// change between calls), 0.6 MB.
template <int NPL>
__global__ __launch_bounds__(256) void dwfc3_fc_stream_kernel(const uint16_t* __restrict__ fc,
                                                               uint16_t* __restrict__ out) {
  using namespace tb3;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * KS * NTW * NPL * 64) return;
  const int lane = i & 63;
  int r = i >> 6;
  const int pl = r % NPL;
  r /= NPL;
  const int t = r % NTW;
  r /= NTW;
  const int ks = r % KS, e = r / KS;
  const int l15 = lane & 15, g4 = lane >> 4;
  const uint16_t* src = fc + (size_t)pl * C * HID + (size_t)(e * (16 * NTW) + 16 * t + l15) * HID + ks * 32 + 8 * g4;
  *reinterpret_cast<bf16x8*>(out + (size_t)i * 8) = *reinterpret_cast<const bf16x8*>(src);
}

template <int P>
__global__ __launch_bounds__(1024, 1) void ffn_dwfc3_tb_kernel(DwFcArgs a) {
  using namespace tb3;
  constexpr bool SPLIT = P == PREC_SPLIT;
  __shared__ __attribute__((aligned(16))) float h2b[NT * H2F];    // [NT][NPOS][HS]
  __shared__ __attribute__((aligned(16))) float vecs[NVEC];
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
  dwfc_stage_ln2<HID>(lnw, lnb, a, 1024);
  dwfc_stage_epi<C>(fcb, n2w, n2b, a, 1024);
  {
    // the depthwise weights and bias through the h2 tiles: all of a thread's loads in flight at
    // once (as a load + store loop the 21 round trips ran one after the other: 15 us of a launch)
    constexpr int NW = HID * 27, PER = (NW + 1023) / 1024;
    float t[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) t[j] = tid + 1024 * j < NW ? a.dw_w[tid + 1024 * j] : 0.f;
    const float tb = tid < HID ? a.dw_b[tid] : 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (tid + 1024 * j < NW) h2b[tid + 1024 * j] = t[j];
    if (tid < HID) h2b[NW + tid] = tb;
  }
  __syncthreads();
  const int role = dwfc_wave_role<4>(simd_cnt, wid, lane);  // 0..11 D, 12..15 E
  const int dbg = ffn_dbg(a);  // WF_FFN_DBG builds only
  // every barrier of the march: this wave's LDS accesses complete, nothing else drained
  auto bar = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // the buffer of tile t (t >= z0 - 6)
  auto tile_buf = [&](int t) { return h2b + ((t - z0 + 6) % NT) * H2F; };

  if (role < 12) {
    // ================================ D waves ===========================================
    const int kslot = role % 3, c = role * 64 + lane;
    float w[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = h2b[c * 27 + k];
    const float bias = h2b[HID * 27 + c];
    float acc[3][TY][TX];  // output-plane accumulators, renamed every plane
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int o = 0; o < TY; ++o)
#pragma unroll
        for (int q = 0; q < TX; ++q) acc[s][o][q] = 0.f;
    // LN2 (slots 0, 1): rows lrow, lrow + 1 of the tile, channel quads lane + 64 j
    const int lrow = 2 * (2 * (role / 3) + kslot);

    // ---- the direct loads.  Input (r, k) of plane p is h1[b, p, y0 - 1 + r, x0 - 1 + k, c];
    // the descriptor of plane p starts one position (HID floats) before the plane.
    const float* src = reinterpret_cast<const float*>(a.h1) + (int64_t)b * D * plane_sz * HID;
    const int64_t plane_elems = (int64_t)plane_sz * HID;
    const int plane_bytes = (int)((plane_elems + HID) * 4);
    const int c4 = 4 * c;
    int rowoff[PY], okmask = 0;  // scalar: a row's byte offset; bit r: row inside, bit 8 + k: column
#pragma unroll
    for (int r = 0; r < PY; ++r) {
      const int yy = y0 - 1 + r;
      rowoff[r] = (min(max(yy, 0), H - 1) * W + x0) * (HID * 4);
      if (yy >= 0 && yy < H) okmask |= 1 << r;
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int xx = x0 - 1 + k;
      if (xx >= 0 && xx < W) okmask |= 1 << (8 + k);
    }
    // what selects plane p's descriptor: its base and the rows / columns it may read (none for
    // a plane outside the volume or past the segment's halo plane z1).  `mk` is opaque so the
    // per-load ranges are made where they are used, not hoisted out of the plane loop.
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
    auto load_row = [&](float (&v)[PX], int r, const PlaneSel& s) {
#pragma unroll
      for (int k = 0; k < PX; ++k) {
        const int rng = ((s.mk >> r) & (s.mk >> (8 + k)) & 1) ? plane_bytes : 0;
        v[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                             buf_rsrc(s.base, rng), c4, rowoff[r] + k * (HID * 4), 0));
      }
    };
    float vin[NR][PX];  // input row r of the plane at hand is in vin[r % NR]
    // input rows [LO, HI) of plane p into the output planes -1 (SA), 0 (SB), +1 (SC); behind
    // each row, the row three further on (of this plane `cur`, then of the next one `nx`) is
    // requested into the registers just consumed
    auto rows = [&](const PlaneSel& cur, const PlaneSel& nx, auto SAc, auto SBc, auto SCc, auto LOc,
                    auto HIc) {
      constexpr int SA = decltype(SAc)::value, SB = decltype(SBc)::value,
                    SC = decltype(SCc)::value, LO = decltype(LOc)::value, HI = decltype(HIc)::value;
#pragma unroll
      for (int r = LO; r < HI; ++r) {
        float(&u)[PX] = vin[r % NR];
        if (!(dbg & 1)) {
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) {
            const int o = r - ky;
            if (o < 0 || o >= TY) continue;
            const float* w0 = w + ky * 3;
#pragma unroll
            for (int q = 0; q < TX; ++q) {
              acc[SC][o][q] = fmaf(w0[2], u[q + 2], fmaf(w0[1], u[q + 1], fmaf(w0[0], u[q], acc[SC][o][q])));
              acc[SB][o][q] = fmaf(w0[11], u[q + 2], fmaf(w0[10], u[q + 1], fmaf(w0[9], u[q], acc[SB][o][q])));
              acc[SA][o][q] = fmaf(w0[20], u[q + 2], fmaf(w0[19], u[q + 1], fmaf(w0[18], u[q], acc[SA][o][q])));
            }
          }
        }
        // pinned between the row's fmaf block and the next row's: the chain is pure arithmetic
        // the compiler may otherwise sink past the barrier into the other phase, or past the
        // loads, which then need a second set of input registers
#pragma unroll
        for (int o = 0; o < TY; ++o)
          if (o <= r && o >= r - 2) {
            asm volatile("" : "+v"(acc[SA][o][0]), "+v"(acc[SA][o][1]), "+v"(acc[SA][o][2]),
                              "+v"(acc[SA][o][3]) : : "memory");
            asm volatile("" : "+v"(acc[SB][o][0]), "+v"(acc[SB][o][1]), "+v"(acc[SB][o][2]),
                              "+v"(acc[SB][o][3]) : : "memory");
            asm volatile("" : "+v"(acc[SC][o][0]), "+v"(acc[SC][o][1]), "+v"(acc[SC][o][2]),
                              "+v"(acc[SC][o][3]) : : "memory");
          }
        __builtin_amdgcn_sched_barrier(0);
        if (r + NR < PY) load_row(u, r + NR, cur);
        else load_row(u, r + NR - PY, nx);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    typedef std::integral_constant<int, S2> IS;
    typedef std::integral_constant<int, PY> IP;
    // iteration p scatters plane p into SA = R (output plane p - 1, complete with it), SB =
    // R + 1 (plane p) and SC = R + 2 (plane p + 1, cleared in front of the scatter and dead
    // before that); then acc[R] + bias is the fp32 h2 tile p - 1.  LN: this wave runs LN2 in
    // phase 1 and its scatter in phase 2 (slots 0, 1); else it scatters rows [0, S2) in phase 1
    // (slot 2).
    auto step = [&](int p, const PlaneSel& cur, const PlaneSel& nx, auto Rc, auto LNc) {
      constexpr int R = decltype(Rc)::value;
      constexpr bool LN = decltype(LNc)::value;
      typedef std::integral_constant<int, R> SA;
      typedef std::integral_constant<int, (R + 1) % 3> SB;
      typedef std::integral_constant<int, (R + 2) % 3> SC;
      // ---- phase 1
      if (LN) {
        if (p - 2 >= z0 && p - 2 < z1 && !(dbg & 2)) {
          float* t2 = tile_buf(p - 2) + lrow * HS;
          dwfc_ln2_row<P, HID, 64, 256, false>(t2, 4 * lane, lnw, lnb, a.eps2);
          __builtin_amdgcn_sched_barrier(0);  // one row at a time: interleaved, the two spill
          dwfc_ln2_row<P, HID, 64, 256, false>(t2 + HS, 4 * lane, lnw, lnb, a.eps2);
        }
      }
#pragma unroll
      for (int o = 0; o < TY; ++o)
#pragma unroll
        for (int q = 0; q < TX; ++q) acc[SC::value][o][q] = 0.f;
      if (!LN) rows(cur, nx, SA(), SB(), SC(), I0(), IS());
      bar();  // 1 -> 2: LN2'd tile (p - 2) visible
      // ---- phase 2
      if (LN) rows(cur, nx, SA(), SB(), SC(), I0(), IP());
      else rows(cur, nx, SA(), SB(), SC(), IS(), IP());
      if (p - 1 >= z0 && p - 1 < z1) {
        float* h2t = tile_buf(p - 1);
#pragma unroll
        for (int o = 0; o < TY; ++o)
#pragma unroll
          for (int q = 0; q < TX; ++q) h2t[(o * TX + q) * HS + c] = acc[R][o][q] + bias;
      }
      bar();  // 2 -> next 1: fp32 h2 tile (p - 1) visible
    };
    auto march = [&](auto LNc) {
      PlaneSel cur = plane_sel(z0 - 1);
#pragma unroll
      for (int r = 0; r < NR; ++r) load_row(vin[r], r, cur);
      for (int p = z0 - 1; p <= z1 + 1; p += 3) {
        PlaneSel nx = plane_sel(p + 1);
        step(p, cur, nx, I0(), LNc);
        cur = nx;
        if (p + 1 <= z1 + 1) {
          nx = plane_sel(p + 2);
          step(p + 1, cur, nx, I1(), LNc);
          cur = nx;
        }
        if (p + 2 <= z1 + 1) {
          nx = plane_sel(p + 3);
          step(p + 2, cur, nx, I2(), LNc);
          cur = nx;
        }
      }
    };
    __syncthreads();  // (prologue) weights read out of the h2 tiles
    if (kslot < 2) march(std::true_type());
    else march(std::false_type());
    return;
  }

  // ================================== E waves ============================================
  __builtin_amdgcn_s_setprio(3);
  const int e = role - 12;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int col0 = e * (16 * NTW) + 4 * g4;      // this lane's four columns of column tile 0
  const float bs = __builtin_bit_cast(
      float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.bscale ? a.bscale[b] : 1.f)));
  // ---- the weight stream: fragment (k-step ks, tile t, plane pl) of this wave is 1 KB of
  // a.fcs (dwfc3_fc_stream_kernel), 16 B per lane; everything but the lane is the instruction's
  // scalar offset
  constexpr int NPL = SPLIT ? 2 : 1;
  const __amdgpu_buffer_rsrc_t wrsrc = buf_rsrc(a.fcs, NPL * C * HID * 2);
  const int wvoff = e * (KS * NTW * NPL * 1024) + 16 * lane;
  const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 wh[NR][NTW], wl[NR][NTW];
  auto wload = [&](int ks) {  // k-step ks (mod KS) into its ring slot
    const int k = ks % KS, sl = ks % NR;
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int so = (k * NTW + t) * NPL * 1024;
      wh[sl][t] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wvoff, so, 0));
      wl[sl][t] = SPLIT ? __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                                         wrsrc, wvoff, so + 1024, 0))
                        : z8;
    }
  };
  // this lane's fc row: tile position l15; everything through 32-bit buffer offsets (the
  // dispatch keeps the tensors under 2 GiB)
  const int yo = y0 + l15 / TX, xo = x0 + l15 % TX;
  const bool rv = yo < H && xo < W;
  const int gpos0 = b * D * plane_sz + min(yo, H - 1) * W + min(xo, W - 1);
  const float* sbase = a.stats ? a.stats : a.x;
  const int64_t npos = (int64_t)a.B * D * plane_sz;
  const __amdgpu_buffer_rsrc_t xrsrc = buf_rsrc(a.x, (int)(npos * C * 4));
  const __amdgpu_buffer_rsrc_t srsrc = buf_rsrc(sbase, (int)(npos * 2 * 4));
  const __amdgpu_buffer_rsrc_t orsrc = buf_rsrc(a.out, (int)(npos * C * 4));
  f32x4 xr[NTW];
  f32x2 es = f32x2{0.f, 1.f};
  // residual + statistics rows of output plane z (clamped: a plane outside the segment is
  // never used)
  auto load_resid = [&](int z) {
    const int g = gpos0 + min(max(z, 0), D - 1) * plane_sz;
#pragma unroll
    for (int t = 0; t < NTW; ++t)
      xr[t] = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (g * C + col0 + 16 * t) * 4, 0, 0));
    es = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(srsrc, g * 8, 0, 0));
  };
  f32x4 acc[NTW];
  bf16x8 ah, al;  // the A fragments of the k-step at hand, read one step ahead
  auto lds8 = [](const uint16_t* q) { return *reinterpret_cast<const bf16x8*>(q); };
  // k-steps [HALF KH, HALF KH + KH) of the fc of tile z
  auto fc_half = [&](int z, auto HALFc) {
    constexpr int HALF = decltype(HALFc)::value;
    const uint16_t* Bh = reinterpret_cast<const uint16_t*>(tile_buf(z)) + (size_t)l15 * (2 * HS) + 8 * g4;
    if (HALF == 0) {
#pragma unroll
      for (int t = 0; t < NTW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      ah = lds8(Bh);
      al = SPLIT ? lds8(Bh + HID) : z8;
    }
#pragma unroll
    for (int i = 0; i < KH; ++i) {
      const int ks = HALF * KH + i;
      // two steps ahead, into the registers of step ks - 1 (its MFMAs are a whole step old)
      wload(ks + 2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NTW; ++t) acc[t] = mma3<P>(acc[t], wh[ks % NR][t], wl[ks % NR][t], ah, al);
      __builtin_amdgcn_sched_barrier(0);
      // the next step's A fragments, behind the MFMAs that read this step's (all issued): the
      // LDS latency lies under the wait for the weights (a second fragment pair would spill)
      if (ks + 1 < KS) {
        ah = lds8(Bh + (ks + 1) * 32);
        al = SPLIT ? lds8(Bh + HID + (ks + 1) * 32) : z8;
      }
    }
  };
  // the epilogue + range-checked stores of tile z, then the residual rows of z + 1
  auto finish = [&](int z) {
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      const int col = col0 + 16 * t;
      const f32x4 v = dwfc_epilogue(acc[t], fcb, n2w, n2b, col, xr[t], es, bs, a.stats != nullptr);
      const int voff = rv ? ((gpos0 + z * plane_sz) * C + col) * 4 : BUF_OOR;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), orsrc, voff, 0, 0);
    }
    load_resid(z + 1);
  };

  wload(0);
  wload(1);
  load_resid(z0);
  __syncthreads();  // (prologue) weights read out of the h2 tiles
  // iteration p: tile zo = p - 3 (LN2'd in phase 1 of iteration p - 1; its buffer is next
  // written, with the fp32 tile zo + 3, in phase 2 of iteration p + 1)
  // written, with the fp32 tile zo + 3, in phase 2 of iteration p + 1).  The four iterations
  // before tile z0 is ready are barriers only -- a loop of their own, so the march carries no
  // condition around the fc (with one, the weight ring was spilled around it).
  if (dbg & 4) {  // WF_FFN_DBG builds only: no fc at all
    for (int p = z0 - 1; p <= z1 + 1; ++p) {
      bar();
      bar();
    }
    return;
  }
  for (int p = z0 - 1; p < z0 + 3; ++p) {
    bar();
    bar();
  }
  // The last tile, z1 - 1 (LN2'd in phase 1 of the last iteration), runs behind the last
  // barrier: the same loop body without its two barriers (the D waves have left).
  for (int zo = z0; zo < z1; ++zo) {
    const bool more = zo < z1 - 1;
    fc_half(zo, std::integral_constant<int, 0>());
    if (more) bar();  // 1 -> 2
    fc_half(zo, std::integral_constant<int, 1>());
    finish(zo);
    if (more) bar();  // 2 -> next 1
  }
}

int launch_ffn_dwfc3(const DwFcArgs& a, int prec, hipStream_t s) {
  using namespace tb3;
  if (prec != PREC_SPLIT && prec != PREC_FP16) return fail(WF_E_SHAPE, "ffn_dwfc3_tb: fp32 h1 only");
  if (!ffn_dwfc3_tb_fits(a.B, a.D, a.H, a.W))
    return fail(WF_E_SHAPE, "ffn_dwfc3_tb: tensor beyond the 2 GiB buffer-offset range");
  if (!a.fcs) return fail(WF_E_SHAPE, "ffn_dwfc3_tb: no workspace for the streamed fc weight");
  DwFcArgs g = a;
  // z segment: whole columns where that gives a workgroup per CU, shorter segments otherwise
  // (B = 8 at 16^3: 128 tiles x 2 segments of 8)
  const int64_t base = (int64_t)g.B * cdiv(g.H, TY) * cdiv(g.W, TX);
  int ZS = g.D;
  while (ZS > 8 && base * cdiv(g.D, ZS) < 256) ZS = (ZS + 1) / 2;
  g.ZS = ZS;
  g.dbg = ffn_dbg_env();
  const int64_t blocks = base * cdiv(g.D, ZS);
  const int nfrag = 4 * KS * NTW * 64 * (prec == PREC_SPLIT ? 2 : 1);
  if (prec == PREC_SPLIT)
    hipLaunchKernelGGL(dwfc3_fc_stream_kernel<2>, dim3(cdiv(nfrag, 256)), dim3(256), 0, s, g.fc, g.fcs);
  else
    hipLaunchKernelGGL(dwfc3_fc_stream_kernel<1>, dim3(cdiv(nfrag, 256)), dim3(256), 0, s, g.fc, g.fcs);
  void (*kern)(DwFcArgs) = prec == PREC_SPLIT ? ffn_dwfc3_tb_kernel<PREC_SPLIT>
                                              : ffn_dwfc3_tb_kernel<PREC_FP16>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(1024), 0, s, g);  // static LDS
  return check_launch("ffn_dwfc3_tb");
}

}  // namespace wf
