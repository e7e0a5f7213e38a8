// attention.hip -- windowed multi-head self-attention.
//
// Reference: network_models/attention.py:83-104 (Attention.forward), driven by
// Block.multi_scale_forward (wave_helper.py:482-499): window_partition -> qkv -> q*scale ->
// q@k^T + relative_position_bias -> softmax -> @v -> proj, then the window "reverse" that is
// a plain reshape (quirk Q1).  Here:
//   qkv  : gemm_ares with the window gather (and norm1 for level-0 blocks) in its loader; or no
//          launch at all: the table-bias core computes q / k / v itself from x and the weight
//          where attn_qkv_fused says so (attn_tbl_kernel_fused)
//   core : one workgroup = (window b_, head h, 64 queries); flash-style loop over key tiles
//          staged in LDS.  S^T = K.Q^T is computed "swapped" (keys on the MFMA rows, queries
//          on the lanes) so the fp32 accumulator of S^T is, register for register, the B
//          operand of O^T = V^T.P^T after bf16 rounding -- P never leaves registers and the
//          softmax column reductions are 2 lane shuffles.  v_mfma_f32_16x16x16_bf16 covers
//          head_dim in 16-wide steps (head_dim is 16 at the default widths).  PREC_SPLIT
//          carries Q, K, V and P as bf16 hi + lo pairs (3 MFMAs per product).
//   proj : gemm_ares; rows stay in window-major order, which is exactly the reference's
//          reshaped raster (Q1).
//   host : what a call launches is decided in attn_plan.hpp (AttnPlan) and run
//          by run_window_attention below.
#include "attn_plan.hpp"
#include "gemm_common.hpp"

namespace wf {

// XCD-contiguous decode of the 1-D grid: the query tiles of one (window, head), which all stage
// the same K / V rows, run on one XCD instead of fetching those rows into 8 L2s
__device__ __forceinline__ void attn_block(int gx, int heads, int& qb, int& h, int64_t& bw) {
  int64_t t = xcd_block_id<int64_t>();
  qb = (int)(t % gx);
  t /= gx;
  h = (int)(t % heads);
  bw = t / heads;
}

// 8 consecutive values of an activation row as MFMA operands: fp32 storage (PREC_SPLIT,
// PREC_FP16) converted to the operand kind (+ the split's lo part), or bf16 storage as-is
template <int P>
__device__ __forceinline__ void load8_split(const void* base, int64_t off, bf16x8& hi,
                                            bf16x8& lo) {
  if (store32(P)) {
    const f32x4* p = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
    const f32x4 a = p[0], b = p[1];
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint16_t h = op_cvt<P>(v[j]);
      hi[j] = (short)h;
      lo[j] = op_lo<P>(v[j], h);
    }
  } else {
    hi = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const uint16_t*>(base) + off);
  }
}

// The tiled core for any window and head_dim; `bias` is the dense (heads, N, N)
// relative-position bias.  It also serves training: with `lse` it writes the row log-sum-exp
// the backward recomputes P from.  (The table-bias form of the default window is
// attn_tbl_kernel, inference only.)
template <int HD, int KT, int P>
__global__ __launch_bounds__(256) void attn_core_kernel(const void* __restrict__ qkv,
                                                        const float* __restrict__ bias,
                                                        void* __restrict__ out,
                                                        float* __restrict__ lse, int N,
                                                        int heads, float scale_log2) {
  constexpr bool SPLIT = P == PREC_SPLIT;  // P: Prec (operand kind)
  constexpr int NC = HD / 16;  // 16-wide head_dim chunks
  constexpr int NKT = KT / 16; // 16-key sub-tiles per tile
  constexpr int KS = HD + 4, VS = KT + 4;
  constexpr int NB = SPLIT ? 2 : 1;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[NB][KT * KS];  // [key][hd]
  __shared__ __attribute__((aligned(16))) uint16_t Vt[NB][HD * VS];  // [hd][key]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int qb, h;
  int64_t bw;
  attn_block((N + kQB - 1) / kQB, heads, qb, h, bw);
  const int C = heads * HD;
  const int64_t row0 = bw * N;  // first token row of this window
  const int ld = 3 * C;
  const int q = qb * kQB + wid * 16 + (lane & 15);  // this lane's query (column)
  const bool qv = q < N;
  const int g4 = 4 * (lane >> 4);

  // Q^T fragments (B operand): lane holds Q[q][c*16 + g4 + j], j < 4
  bf16x4 qf[NC], qfl[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    qf[c] = bf16x4{0, 0, 0, 0};
    qfl[c] = bf16x4{0, 0, 0, 0};
    if (!qv) continue;
    const int64_t off = (row0 + q) * ld + h * HD + c * 16 + g4;
    if (store32(P)) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(qkv) + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint16_t hh = op_cvt<P>(v[j]);
        qf[c][j] = (short)hh;
        qfl[c][j] = op_lo<P>(v[j], hh);
      }
    } else {
      qf[c] = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const uint16_t*>(qkv) + off);
    }
  }
  f32x4 o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = f32x4{0, 0, 0, 0};
  float mrun = -INFINITY, lrun = 0.f;
  const float* brow = bias + ((int64_t)h * N + (qv ? q : 0)) * N;

  for (int k0 = 0; k0 < N; k0 += KT) {
    __syncthreads();
    // stage K rows and V^T for keys k0..k0+KT-1 (chunks of 8 head_dim values)
    for (int it = tid; it < KT * (HD / 8); it += 256) {
      const int kr = it / (HD / 8), ch = it % (HD / 8);
      const int key = k0 + kr;
      bf16x8 kh = {0, 0, 0, 0, 0, 0, 0, 0}, kl = kh, vh = kh, vl = kh;
      if (key < N) {
        const int64_t off = (row0 + key) * ld + h * HD + ch * 8;
        load8_split<P>(qkv, off + C, kh, kl);
        load8_split<P>(qkv, off + 2 * C, vh, vl);
      }
      *reinterpret_cast<bf16x8*>(&Ks[0][kr * KS + ch * 8]) = kh;
      if (SPLIT) *reinterpret_cast<bf16x8*>(&Ks[NB - 1][kr * KS + ch * 8]) = kl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        Vt[0][(ch * 8 + j) * VS + kr] = (uint16_t)vh[j];
        if (SPLIT) Vt[NB - 1][(ch * 8 + j) * VS + kr] = (uint16_t)vl[j];
      }
    }
    __syncthreads();

    // S^T for NKT sub-tiles of 16 keys: rows key = k0 + kt*16 + g4 + i, column = query
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      s[kt] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int ko = (kt * 16 + (lane & 15)) * KS + c * 16 + g4;
        const bf16x4 a = *reinterpret_cast<const bf16x4*>(&Ks[0][ko]);
        if (SPLIT) {
          const bf16x4 al = *reinterpret_cast<const bf16x4*>(&Ks[NB - 1][ko]);
          s[kt] = mma16<P>(al, qf[c], s[kt]);
          s[kt] = mma16<P>(a, qfl[c], s[kt]);
        }
        s[kt] = mma16<P>(a, qf[c], s[kt]);
      }
    }
    // scale + relative-position bias (log2 domain), key mask
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const int kb = k0 + kt * 16 + g4;
      f32x4 bv;
      if (kb + 3 < N) {
        bv = *reinterpret_cast<const f32x4*>(brow + kb) * 1.4426950408889634f;
      } else {
        bv.x = kb + 0 < N ? brow[kb + 0] : 0.f;
        bv.y = kb + 1 < N ? brow[kb + 1] : 0.f;
        bv.z = kb + 2 < N ? brow[kb + 2] : 0.f;
        bv.w = kb + 3 < N ? brow[kb + 3] : 0.f;
        bv *= 1.4426950408889634f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float t = s[kt][i] * scale_log2 + bv[i];
        t = (kb + i < N) ? t : -INFINITY;
        s[kt][i] = t;
        tmax = fmaxf(tmax, t);
      }
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mnew = fmaxf(mrun, tmax);
    const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);  // mrun = -inf on the first tile -> 0
    mrun = mnew;
    float psum = 0.f;
    bf16x4 pf[NKT], pfl[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(s[kt][i] - mnew);
        psum += p;
        const uint16_t ph = op_cvt<P>(p);
        pf[kt][i] = (short)ph;
        pfl[kt][i] = op_lo<P>(p, ph);
      }
    }
    lrun = lrun * alpha + psum;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      o[c] *= alpha;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int vo = (c * 16 + (lane & 15)) * VS + kt * 16 + g4;
        const bf16x4 a = *reinterpret_cast<const bf16x4*>(&Vt[0][vo]);
        if (SPLIT) {
          const bf16x4 al = *reinterpret_cast<const bf16x4*>(&Vt[NB - 1][vo]);
          o[c] = mma16<P>(al, pf[kt], o[c]);
          o[c] = mma16<P>(a, pfl[kt], o[c]);
        }
        o[c] = mma16<P>(a, pf[kt], o[c]);
      }
    }
  }
  // full column sums: the 4 lane groups hold disjoint key subsets
  lrun = xsum16(lrun);
  lrun = xsum32(lrun);
  // training: the row log-sum-exp (log2 domain) that the backward recomputes P from
  if (lse && qv && lane < 16) lse[(bw * heads + h) * N + q] = mrun + __log2f(lrun);
  if (qv) {
    const float inv = 1.f / lrun;
    const int64_t off = (row0 + q) * C + h * HD + g4;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (store32(P)) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + off + c * 16) = o[c] * inv;
      } else {
        bf16x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (short)f2bf(o[c][i] * inv);
        *reinterpret_cast<bf16x4*>(reinterpret_cast<uint16_t*>(out) + off + c * 16) = r;
      }
    }
  }
}

// Table-bias attention for the default window (ws 8: N = 512 tokens, head_dim 16), one
// workgroup per (window, head) -- or per 1/2 or 1/4 of its queries when there are too few
// windows to fill the chip.  K and V are split into bf16 hi / lo ONCE per (window, head) and
// staged in LDS (68 KB: two workgroups per CU), instead of once per 64-query workgroup.  Every
// product runs on v_mfma_f32_16x16x32_bf16:
//   S^T = K Q'^T + B : the K = 32 reduction packs [Kh | Kl] against [Q'h | Q'h] (Kh Q'h + Kl Q'h
//                 in one MFMA), a second MFMA adds Kh Q'l ([Kh | Kl] against [Q'l | 0]).  Q' is
//                 Q pre-scaled by scale * log2 e, and the accumulator STARTS at the bias
//                 (log2 e-scaled table entries), so the MFMA output is already the exp2-domain
//                 logit: no scale / bias pass on the VALU;
//   O^T = V^T P^T : 32 keys per MFMA, the B operand is the lane's two 4-key score quads of two
//                 16-key sub-tiles as they come out of the S MFMAs (the K-slot order is matched
//                 by reading V at the same keys), x3 for the split;
//   l   = 1^T P^T : bf16 / fp16 operands: the softmax row sums on the same B operands (a ones A
//                 operand), instead of an add per score on the VALU; every accumulator row
//                 holds the sum.  Split operands add the fp32 exponentials (attn_tbl_tiles).
// The bias index is the reference's formula (attention.py:40-56, Q2 depth stride 3 ws - 1)
// with the key part reduced to per-tile constants: a 64-key tile is one z slice of the window.
// The table is staged REVERSED, so a lane's 16 bias values of a tile are 4 ascending runs of 4
// at one per-tile base + compile-time offsets 30 kt + i (ds_read2_b32 immediate offsets).
// K rows are 64 B (hi 16 | lo 16) with the four 16-B chunks XOR-swizzled by (row / 4) & 3
// through {0, 2, 3, 1}: every 16-lane group of a ds_read_b128 (gfx950 groups lanes
// {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...) then hits 16 distinct 4-bank sets -- the
// round-2 80-B padded rows were 2-way conflicted (SQ_LDS_BANK_CONFLICT ~ SQ_INSTS_LDS).
template <int P>
__device__ __forceinline__ void load8_split_scaled(const void* base, int64_t off, float sc,
                                                   bf16x8& hi, bf16x8& lo) {
  if (store32(P)) {
    const f32x4* p = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
    const f32x4 a = p[0] * sc, b = p[1] * sc;
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint16_t h = op_cvt<P>(v[j]);
      hi[j] = (short)h;
      lo[j] = op_lo<P>(v[j], h);
    }
  } else {
    const bf16x8 r = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const uint16_t*>(base) + off);
#pragma unroll
    for (int j = 0; j < 8; ++j) hi[j] = (short)f2bf(bf2f((uint16_t)r[j]) * sc);
  }
}

__device__ __forceinline__ int kswz(int row) {  // 16-B chunk XOR of a K row (see above)
  return (0x78 >> (2 * ((row >> 2) & 3))) & 3;  // {0, 2, 3, 1}[(row >> 2) & 3]
}

namespace tbl {
constexpr int N = 512, HD = 16;
constexpr int TBLN = 547;  // reachable rows of the (15^3, heads) table under Q2
constexpr int KS = 32;     // K row: hi[16] | lo[16], chunks swizzled (kswz)
// V: [hi, lo][key/4][hd][4 keys], each key-quad block padded to 136 B so the staging
// stores (lanes 64 / 128 B apart) spread over the banks; the loop's 16-lane reads stay
// contiguous inside one block
constexpr int VB = HD * 4 + 4;
constexpr int VQ = (N / 4) * VB;
// the reversed table as overlapping quads: tq[i] = {tbr[i], tbr[i+1], tbr[i+2], tbr[i+3]},
// so a lane's 4 consecutive bias values are one aligned ds_read_b128
constexpr int TQ_BYTES = TBLN * 16;
// Lazy rescale: the running max is kept while no score of a 64-key tile exceeds it by more
// than 2^kTau in the exp2 domain (a lane-local max + one wave ballot); only then does the tile
// pay the cross-group max exchange (two ds_bpermute round trips on the critical path), the
// alpha exponential and the o / l rescale.  The exponentials of a kept tile are at most
// 2^kTau; the normalisation o / l is the same quotient, so this changes only fp32 rounding.
// The exponentials become MFMA operands, so 2^tau must be finite in the operand kind: bf16 has
// fp32's range, but fp16 ends at 65504 and a kept score in (mrun + 15.99965, mrun + 16] gave an
// inf probability and a NaN row.  fp16 operands therefore keep a tile only up to 2^15
// (tests/test_gpu_attention_softmax.py, f16_band).
constexpr float kTau = 16.0f;
constexpr float kTauFp16 = 15.0f;
template <int P>
constexpr float tau = P == PREC_FP16 ? kTauFp16 : kTau;
}  // namespace tbl

// ---- q / k / v computed in the core (attn_tbl_kernel_fused) -----------------------------------
// The fused form takes x and the qkv weight instead of a staged (rows, 3 C) tensor: g is the qkv
// GEMM's own argument block (MAP_LEVELS rows, K = C = CW, N = 3 C, the [2][3C][C] weight planes,
// the bias), and every value is formed exactly as gemm_rows / gemm_kc form it -- the weight rows
// as the MFMA's A operand, the activation octets through a_fragment as B, 32-deep k steps in
// ascending order through mma3, the tail of K = 48 as gemm_kc's (load clamped at K - 8, the
// activation octet zeroed), the bias added after the last step -- and then rounded as the staged
// store + load8_split pair rounds it (split4: op_cvt / op_lo; bf16 storage is op_cvt itself).
// So the two forms are bitwise equal and a launch may take either (attn_qkv_fused).
template <int CW>
struct FusedQkv {
  static constexpr int NKS = (CW + 31) / 32;
};

// one 16 x 16 tile: 16 weight rows (fragments wh / wl: row l15) against 16 x rows (octets v:
// row l15).  The lane ends with x row l15 against weight rows 4 g4 .. + 3, as the GEMMs' lanes do
template <int P, int CW>
__device__ __forceinline__ f32x4 fused_tile(const float (&v)[FusedQkv<CW>::NKS][8],
                                            const bf16x8 (&wh)[FusedQkv<CW>::NKS],
                                            const bf16x8 (&wl)[FusedQkv<CW>::NKS], int g4) {
  f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < FusedQkv<CW>::NKS; ++ks) {
    const int k = ks * 32 + 8 * g4;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = v[ks][j];
    bf16x8 ah, al;
    a_fragment<P>(x, 0.f, 1.f, nullptr, nullptr, k, k < CW, false, false, ah, al);
    acc = mma3<P>(acc, wh[ks], wl[ks], ah, al);
  }
  return acc;
}
template <int P, int CW>
__device__ __forceinline__ void fused_load_w(const GemmArgs& g, int wo, int g4,
                                             bf16x8 (&wh)[FusedQkv<CW>::NKS],
                                             bf16x8 (&wl)[FusedQkv<CW>::NKS]) {
#pragma unroll
  for (int ks = 0; ks < FusedQkv<CW>::NKS; ++ks) {
    const int off = wo + min(ks * 32 + 8 * g4, CW - 8);  // past K: a finite re-read x a zeroed octet
    wh[ks] = *reinterpret_cast<const bf16x8*>(g.w + off);
    wl[ks] = P == PREC_SPLIT ? *reinterpret_cast<const bf16x8*>(g.w + 3 * CW * CW + off) : wh[ks];
  }
}
// The x rows of one window: RowMapper<MAP_LEVELS>'s map (gemm_common.hpp) with what a workgroup's
// 512 rows share taken once -- they are one window of one level, so the level's raster and the
// window's corner are wave-uniform (scalar registers, three divisions per workgroup) and a row is
// the corner plus its token's (z, y, x) offset.  Through RowMapper itself every 16-row tile paid a
// per-lane fetch of the level's geometry and the divisions in front of its loads.
struct WindowRows {
  const float* corner;  // channel 0 of the window's token 0
  int H, W;             // the level's raster
  __device__ __forceinline__ WindowRows() : corner(nullptr), H(0), W(0) {}
  __device__ __forceinline__ WindowRows(const GemmArgs& g, int row0) {
    row0 = __builtin_amdgcn_readfirstlane(row0);
    const int l = (row0 >= g.lv_row0[1]) + (row0 >= g.lv_row0[2]) + (row0 >= g.lv_row0[3]);
    const int r0 = l == 0 ? g.lv_row0[0] : l == 1 ? g.lv_row0[1] : l == 2 ? g.lv_row0[2] : g.lv_row0[3];
    const int mD = l == 0 ? g.lv_D[0] : l == 1 ? g.lv_D[1] : l == 2 ? g.lv_D[2] : g.lv_D[3];
    const int mH = l == 0 ? g.lv_H[0] : l == 1 ? g.lv_H[1] : l == 2 ? g.lv_H[2] : g.lv_H[3];
    const int mW = l == 0 ? g.lv_W[0] : l == 1 ? g.lv_W[1] : l == 2 ? g.lv_W[2] : g.lv_W[3];
    const float* src = l == 0 ? g.lv_src[0] : l == 1 ? g.lv_src[1] : l == 2 ? g.lv_src[2] : g.lv_src[3];
    H = mH;
    W = mW;
    corner = src + (int64_t)window_row_pos(row0 - r0, 8, mD, mH, mW) * g.K;
  }
  // element offset of token t's row from the corner
  __device__ __forceinline__ int64_t row(int t, int K) const {
    return (int64_t)(((t >> 6) * H + ((t >> 3) & 7)) * W + (t & 7)) * K;
  }
};
template <int CW>
__device__ __forceinline__ void fused_load_x(const WindowRows& w, int t, int g4,
                                             float (&v)[FusedQkv<CW>::NKS][8]) {
  const int64_t off = w.row(t, CW);
#pragma unroll
  for (int ks = 0; ks < FusedQkv<CW>::NKS; ++ks)
    load8f<false>(w.corner, off + min(ks * 32 + 8 * g4, CW - 8), v[ks]);
}

// K and V of the window's 512 rows into Ks / Vq (their staged layouts): wave wid takes rows
// 64 wid .. + 63 as four 16-row tiles against this head's 16 K and 16 V weight rows.  One pass
// with both weight sets at C = 48; at C = 96 they and the rows in flight do not fit the 128
// registers of four waves per SIMD together, so K and V are a pass each (the second pass reads
// the rows again, from L2).
template <int P, int CW, bool DOK, bool DOV>
__device__ __forceinline__ void fused_stage_pass(const GemmArgs& g, const WindowRows& w, int h,
                                                 uint16_t* Ks, uint16_t* Vq) {
  using namespace tbl;
  constexpr int NKS = FusedQkv<CW>::NKS;
  constexpr bool SPLIT = P == PREC_SPLIT;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  bf16x8 kwh[NKS], kwl[NKS], vwh[NKS], vwl[NKS];
  if (DOK) fused_load_w<P, CW>(g, (CW + h * HD + l15) * CW, g4, kwh, kwl);
  if (DOV) fused_load_w<P, CW>(g, (2 * CW + h * HD + l15) * CW, g4, vwh, vwl);
  f32x4 kb = f32x4{0, 0, 0, 0}, vb = kb;
  if (g.bias) {
    if (DOK) kb = *reinterpret_cast<const f32x4*>(g.bias + CW + h * HD + 4 * g4);
    if (DOV) vb = *reinterpret_cast<const f32x4*>(g.bias + 2 * CW + h * HD + 4 * g4);
  }
  // DEPTH tiles' rows in flight: all four at C = 48 (64 registers), two at C = 96
  constexpr int DEPTH = CW <= 48 ? 4 : 2;
  float v[DEPTH][NKS][8];
#pragma unroll
  for (int tt = 0; tt < DEPTH; ++tt) fused_load_x<CW>(w, wid * 64 + tt * 16 + l15, g4, v[tt]);
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    const int key = wid * 64 + tt * 16 + l15;
    f32x4 ka = f32x4{0, 0, 0, 0}, va = ka;
    if (DOK) ka = fused_tile<P, CW>(v[tt % DEPTH], kwh, kwl, g4);
    if (DOV) va = fused_tile<P, CW>(v[tt % DEPTH], vwh, vwl, g4);
    if (tt + DEPTH < 4) fused_load_x<CW>(w, key + 16 * DEPTH, g4, v[tt % DEPTH]);
    if (g.bias) {
      ka += kb;
      va += vb;
    }
    if (DOK) {
      bf16x4 kh, kl;
      split4<P>(ka, kh, kl);
      const int sw = kswz(key), hc = g4 >> 1, ho = 4 * (g4 & 1);
      *reinterpret_cast<bf16x4*>(&Ks[key * KS + 8 * (hc ^ sw) + ho]) = kh;
      *reinterpret_cast<bf16x4*>(&Ks[key * KS + 8 * ((2 + hc) ^ sw) + ho]) =
          SPLIT ? kl : bf16x4{0, 0, 0, 0};
    }
    if (DOV) {
      bf16x4 vh, vl;
      split4<P>(va, vh, vl);
      const int vo = (key >> 2) * VB + (4 * g4) * 4 + (key & 3);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Vq[vo + 4 * i] = (uint16_t)vh[i];
        if (SPLIT) Vq[VQ + vo + 4 * i] = (uint16_t)vl[i];
      }
    }
  }
}
template <int P, int CW>
__device__ __forceinline__ void fused_stage_kv(const GemmArgs& g, int row0, int h, uint16_t* Ks,
                                               uint16_t* Vq) {
  const WindowRows w(g, row0);
  if constexpr (CW <= 48) {
    fused_stage_pass<P, CW, true, true>(g, w, h, Ks, Vq);
  } else {
    fused_stage_pass<P, CW, true, false>(g, w, h, Ks, Vq);
    fused_stage_pass<P, CW, false, true>(g, w, h, Ks, Vq);
  }
}

// The S operands of 16 queries (lane: token t of the window w): Q' = Q * sc rounded as
// load8_split_scaled rounds the staged Q, then moved from the accumulator layout (channels
// 4 g4 .. + 3) to the operand slots (8 values 8 (g4 & 1) .. + 7: two lanes' quads)
template <int P, int CW>
__device__ __forceinline__ void fused_q_operands(const GemmArgs& g, const WindowRows& w, int t,
                                                 int h, float sc, bf16x8& hi, bf16x8& lo) {
  using namespace tbl;
  constexpr int NKS = FusedQkv<CW>::NKS;
  const int lane = threadIdx.x & 63, l15 = lane & 15, g4 = lane >> 4;
  // the weight fragments are loaded per sub-tile (L2 hits): held across the tile loop they would
  // not fit its registers, so the loads hang on a value the compiler cannot hoist
  int wo = (h * HD + l15) * CW;
  asm volatile("" : "+v"(wo));
  bf16x8 wh[NKS], wl[NKS];
  fused_load_w<P, CW>(g, wo, g4, wh, wl);
  float v[NKS][8];
  fused_load_x<CW>(w, t, g4, v);
  f32x4 q = fused_tile<P, CW>(v, wh, wl, g4);
  if (g.bias) q += *reinterpret_cast<const f32x4*>(g.bias + h * HD + 4 * g4);
  bf16x4 qh, ql;
  if (store32(P)) {
    // load8_split_scaled's text: with FMA contraction the lo part is bf16(fma(q, sc, -hi)), the
    // product unrounded, and only the same expression gives the same bits
    const f32x4 a = q * sc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint16_t hh = op_cvt<P>(a[i]);
      qh[i] = (short)hh;
      ql[i] = op_lo<P>(a[i], hh);
    }
  } else {  // bf16 storage of the staged Q, then the scale
#pragma unroll
    for (int i = 0; i < 4; ++i) qh[i] = (short)f2bf(bf2f(f2bf(q[i])) * sc);
    ql = bf16x4{0, 0, 0, 0};
  }
  const u32x2 hw = __builtin_bit_cast(u32x2, qh), lw = __builtin_bit_cast(u32x2, ql);
  const int sa = l15 + 32 * (g4 & 1), sb = sa + 16;
  hi = __builtin_bit_cast(bf16x8, u32x4{(uint32_t)__shfl((int)hw[0], sa, 64), (uint32_t)__shfl((int)hw[1], sa, 64),
                                        (uint32_t)__shfl((int)hw[0], sb, 64), (uint32_t)__shfl((int)hw[1], sb, 64)});
  if (P == PREC_SPLIT)
    lo = __builtin_bit_cast(bf16x8, u32x4{(uint32_t)__shfl((int)lw[0], sa, 64), (uint32_t)__shfl((int)lw[1], sa, 64),
                                          (uint32_t)__shfl((int)lw[0], sb, 64), (uint32_t)__shfl((int)lw[1], sb, 64)});
}

// The tile loop of attn_tbl_kernel over this wave's 16-query sub-tiles, NQ at a time (sub-tiles
// st, st + 8, ...; q0 = the workgroup's first query).  NQ = 2: every K / V fragment read from
// LDS feeds both sub-tiles, and their dependency chains (scores -> max -> exp -> PV)
// interleave -- with one sub-tile the SIMDs wait on those chains with four waves each (LDS
// caps the workgroups at two per CU).  The two forms differ in fp32 rounding when a tile after
// the first raises the running max: NQ = 2 rescales BOTH its sub-tiles when either asks for it.
// What the loop does, each against alternatives that were built and measured (they and their
// measurements are in the history before this commit and in DESIGN 6):
//  * the max exchange across the 4 key groups of a query column is __shfl_xor (ds_bpermute, LDS
//    crossbar), not v_permlane16/32_swap: the kernel's VALU is its tighter resource
//    (profiles/r5_attention_ab.txt);
//  * bf16 / fp16 operands take the softmax row sums as ones-operand MFMAs (4 of the 18 per
//    64-key tile), not VALU adds (profiles/r4_attention_rowsum_ab.txt): their l must be the sum
//    of the same rounded P the numerator uses;
//  * split operands sum the fp32 exponentials on the VALU (each lane's partial over its 4 keys
//    per 16-key block, the 4 lanes of a query reduced once at the end): 157.0 vs 159.6 us per
//    B = 8 stage-1 launch, interleaved (profiles/r6/r6n_attn_vsum_ab.txt), and closer to exact
//    by the split's 2^-16 residual.  The order is the same for NQ = 1 and 2: a volume's result
//    must not depend on the batch (the qsplit = 4 launches of small grids run NQ = 1);
//  * the split's lo part of a pair of probabilities comes from split_pair (v_dot2c_f32_bf16
//    against the packed hi pair), bitwise the unpack-and-subtract form.
// CW != 0: the fused form -- Q' of a sub-tile comes from x and the weight (g; fused_q_operands)
// where the staged form reads it from qkv.
template <int P, int NQ, int CW = 0>
__device__ __forceinline__ void attn_tbl_tiles(const void* __restrict__ qkv,
                                               const GemmArgs* __restrict__ g, void* __restrict__ out,
                                               const f32x4* tq, const uint16_t* Ks,
                                               const uint16_t* Vq, int64_t row0, int q0, int h,
                                               int heads, int nsub, float scale_log2) {
  using namespace tbl;
  constexpr bool SPLIT = P == PREC_SPLIT;
  constexpr bool VSUM = SPLIT;  // row sums on the VALU (see above)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int C = heads * HD, ld = 3 * C;
  const int kch = 8 * (g4 ^ kswz(l15));  // this lane's K chunk (rows t*64 + kt*16 + l15)
  const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const short one = (short)op_cvt<P>(1.0f);
  const bf16x8 ones = bf16x8{one, one, one, one, one, one, one, one};
  // fused: the window's x rows (scalars; the staged form never reads g)
  const WindowRows wrows = CW != 0 ? WindowRows(*g, (int)row0) : WindowRows();
  for (int st = wid; st < nsub; st += 8 * NQ) {
    int qq[NQ], rbq[NQ];
    bf16x8 b1[NQ], b2[NQ];
    f32x4 o[NQ], l4[NQ];
    float mrun[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int q = q0 + (st + 8 * u) * 16 + l15;
      qq[u] = q;
      // B operands of S: slots 8 g4 .. +7 <- Q'[q][8 (g4 & 1) ..]: [Q'h | Q'h] and [Q'l | 0]
      bf16x8 hi = z8, lo = z8;
      if constexpr (CW != 0)
        fused_q_operands<P, CW>(*g, wrows, q, h, scale_log2, hi, lo);
      else
        load8_split_scaled<P>(qkv, (row0 + q) * ld + h * HD + 8 * (g4 & 1), scale_log2, hi, lo);
      b1[u] = hi;
      b2[u] = (SPLIT && g4 < 2) ? lo : z8;
      const int qz = q >> 6, qy = (q >> 3) & 7, qx = q & 7;
      // reversed-table base of tile 0: (TBLN - 1) - index(q, key (0, 2 (g4 >> 1), 4 (g4 & 1)))
      rbq[u] = (TBLN - 1) - ((qz + 7) * 23 + (qy + 7) * 15 + (qx + 7)) +
               ((g4 >> 1) * 15 + 4 * (g4 & 1));
      o[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      l4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      mrun[u] = -INFINITY;
    }
#pragma clang loop unroll_count(NQ == 1 ? 2 : 1)
    for (int t = 0; t < 8; ++t) {  // 64-key tiles (one z slice of the window each)
      // S^T of tile t: 4 sub-tiles of 16 keys, the accumulator starting at the bias
      f32x4 s[NQ][4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&Ks[(t * 64 + kt * 16 + l15) * KS + kch]);
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          s[u][kt] = mma32<P>(a, b1[u], tq[rbq[u] + 23 * t + 30 * kt]);
          if (SPLIT) s[u][kt] = mma32<P>(a, b2[u], s[u][kt]);
        }
      }
      float lmax[NQ];
      bool big = false;
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        lmax[u] = s[u][0][0];  // a chain, so the compiler pairs it into v_max3_f32
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = (kt == 0 ? 1 : 0); i < 4; ++i) lmax[u] = fmaxf(lmax[u], s[u][kt][i]);
        big = big || lmax[u] > mrun[u] + tau<P>;
      }
      if (__builtin_amdgcn_ballot_w64(big) != 0) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          float tmax = fmaxf(mrun[u], lmax[u]);
          tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
          tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
          const float alpha = __builtin_amdgcn_exp2f(mrun[u] - tmax);  // 0 on the first tile
          mrun[u] = tmax;
          o[u] *= alpha;
          l4[u] *= alpha;
        }
      }
      // P^T operand words: pairs of 16-bit values, hi and (bf16x3) lo parts
      uint32_t ph[NQ][4][2], pl[NQ][4][2];
#pragma unroll
      for (int u = 0; u < NQ; ++u)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = 0; i < 4; i += 2) {
            const float e0 = __builtin_amdgcn_exp2f(s[u][kt][i] - mrun[u]);
            const float e1 = __builtin_amdgcn_exp2f(s[u][kt][i + 1] - mrun[u]);
            if (VSUM) l4[u][0] += e0 + e1;
            split_pair<P>(e0, e1, ph[u][kt][i >> 1], pl[u][kt][i >> 1]);
          }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int o1 = (16 * t + 8 * j + g4) * VB + l15 * 4;
        const int o2 = (16 * t + 8 * j + 4 + g4) * VB + l15 * 4;
        const bf16x4 v1 = *reinterpret_cast<const bf16x4*>(&Vq[o1]);
        const bf16x4 v2 = *reinterpret_cast<const bf16x4*>(&Vq[o2]);
        const bf16x8 vh = bf16x8{v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
        bf16x8 vl = z8;
        if (SPLIT) {
          const bf16x4 w1 = *reinterpret_cast<const bf16x4*>(&Vq[VQ + o1]);
          const bf16x4 w2 = *reinterpret_cast<const bf16x4*>(&Vq[VQ + o2]);
          vl = bf16x8{w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          const bf16x8 pb = __builtin_bit_cast(
              bf16x8, u32x4{ph[u][2 * j][0], ph[u][2 * j][1], ph[u][2 * j + 1][0], ph[u][2 * j + 1][1]});
          if (SPLIT) {
            const bf16x8 plb = __builtin_bit_cast(
                bf16x8, u32x4{pl[u][2 * j][0], pl[u][2 * j][1], pl[u][2 * j + 1][0], pl[u][2 * j + 1][1]});
            o[u] = mma32<P>(vl, pb, o[u]);
            o[u] = mma32<P>(vh, plb, o[u]);
            if (!VSUM) l4[u] = mma32<P>(ones, plb, l4[u]);
          }
          o[u] = mma32<P>(vh, pb, o[u]);
          if (!VSUM) l4[u] = mma32<P>(ones, pb, l4[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      if (VSUM) {  // the 4 lanes (g4) of query l15
        l4[u][0] += __shfl_xor(l4[u][0], 16, 64);
        l4[u][0] += __shfl_xor(l4[u][0], 32, 64);
      }
      const float inv = 1.f / l4[u][0];
      const int64_t off = (row0 + qq[u]) * C + h * HD + 4 * g4;
      if (store32(P)) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + off) = o[u] * inv;
      } else {
        bf16x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (short)f2bf(o[u][i] * inv);
        *reinterpret_cast<bf16x4*>(reinterpret_cast<uint16_t*>(out) + off) = r;
      }
    }
  }
}

// head h's column of the table, log2 e-scaled, as the reversed overlapping quads (tbl::TQ_BYTES)
__device__ __forceinline__ void attn_tbl_stage_table(f32x4* tq, const float* __restrict__ table,
                                                     int heads, int h) {
  using namespace tbl;
  for (int i = threadIdx.x; i < TBLN; i += 512) {
    // tq[j].c = tbr[j + c] = table[TBLN - 1 - j - c] (0 past the end: never read)
    const float v = table[(int64_t)i * heads + h] * 1.4426950408889634f;
    const int j = TBLN - 1 - i;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (j - c >= 0) reinterpret_cast<float*>(&tq[j - c])[c] = v;
    if (j >= TBLN - 3)
      for (int c = TBLN - j; c < 4; ++c) reinterpret_cast<float*>(&tq[j])[c] = 0.f;
  }
}

template <int P>
__global__ __launch_bounds__(512, 2) void attn_tbl_kernel(const void* __restrict__ qkv,
                                                          const float* __restrict__ table,
                                                          void* __restrict__ out, int heads,
                                                          int qsplit, float scale_log2,
                                                          int64_t pair_end) {
  // pair_end: windows [0, pair_end) may take the tile loop two sub-tiles at a time, the others
  // take one at a time whatever the split (the two differ in fp32 rounding: attn_tbl_tiles).  A
  // launch over several levels (wf_window_attention_fwd_levels) gives each level the form its
  // own launch would have taken, so its bits do not move.
  using namespace tbl;
  constexpr bool SPLIT = P == PREC_SPLIT;  // P: Prec (operand kind)
  // one LDS block, the table first: its quads then sit below the 64-KiB reach of the ds_read
  // offset field, so a tile's 4 bias reads are one base register + immediates (separate
  // __shared__ arrays were placed table-last, 72 KB up: one address add per read)
  __shared__ __attribute__((aligned(16))) uint8_t lds_tbl[TQ_BYTES + N * KS * 2 + 2 * VQ * 2];
  f32x4* tq = reinterpret_cast<f32x4*>(lds_tbl);
  uint16_t* Ks = reinterpret_cast<uint16_t*>(lds_tbl + TQ_BYTES);
  uint16_t* Vq = Ks + N * KS;
  const int tid = threadIdx.x;
  int qs, h;
  int64_t bw;
  attn_block(qsplit, heads, qs, h, bw);
  const int C = heads * HD, ld = 3 * C;
  const int64_t row0 = bw * N;
  const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};

  attn_tbl_stage_table(tq, table, heads, h);
  for (int it = tid; it < N * 2; it += 512) {  // K: (key, 8-value chunk)
    const int key = it >> 1, ch = it & 1, sw = kswz(key);
    bf16x8 hi = z8, lo = z8;
    load8_split<P>(qkv, (row0 + key) * ld + C + h * HD + ch * 8, hi, lo);
    *reinterpret_cast<bf16x8*>(&Ks[key * KS + 8 * (ch ^ sw)]) = hi;
    *reinterpret_cast<bf16x8*>(&Ks[key * KS + 8 * ((2 + ch) ^ sw)]) = SPLIT ? lo : z8;
  }
  for (int it = tid; it < (N / 4) * 2; it += 512) {  // V: (key quad, 8-value chunk)
    const int k4 = it >> 1, ch = it & 1;
    bf16x8 vh[4], vl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      vh[r] = z8;
      vl[r] = z8;
      load8_split<P>(qkv, (row0 + 4 * k4 + r) * ld + 2 * C + h * HD + ch * 8, vh[r], vl[r]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = k4 * VB + (ch * 8 + j) * 4;
      *reinterpret_cast<bf16x4*>(&Vq[o]) = bf16x4{vh[0][j], vh[1][j], vh[2][j], vh[3][j]};
      if (SPLIT) *reinterpret_cast<bf16x4*>(&Vq[VQ + o]) = bf16x4{vl[0][j], vl[1][j], vl[2][j], vl[3][j]};
    }
  }
  __syncthreads();

  const int nsub = N / 16 / qsplit;  // 16-query sub-tiles of this workgroup
  const int q0 = qs * (N / qsplit);
  if (nsub >= kAttnPairNsub && bw < pair_end)
    attn_tbl_tiles<P, 2>(qkv, nullptr, out, tq, Ks, Vq, row0, q0, h, heads, nsub, scale_log2);
  else
    attn_tbl_tiles<P, 1>(qkv, nullptr, out, tq, Ks, Vq, row0, q0, h, heads, nsub, scale_log2);
}

// attn_tbl_kernel with q / k / v computed here from x and the qkv weight (g: the qkv GEMM's
// arguments, MAP_LEVELS rows of width CW) instead of read from a tensor the GEMM stored: the
// prologue fills Ks / Vq through fused_stage_kv, the tile loop forms each sub-tile's Q' itself.
// With qsplit > 1 every workgroup of a (window, head) projects all 512 K / V rows again, so the
// host takes this form at qsplit <= 2 only (attn_qkv_fused).  Same LDS block, same tile loops,
// bitwise the staged kernel's output.
template <int P, int CW>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_tbl_kernel_fused(const GemmArgs g,
                                                                const float* __restrict__ table,
                                                                void* __restrict__ out, int heads,
                                                                int qsplit, float scale_log2,
                                                                int64_t pair_end) {
  using namespace tbl;
  __shared__ __attribute__((aligned(16))) uint8_t lds_tbl[TQ_BYTES + N * KS * 2 + 2 * VQ * 2];
  f32x4* tq = reinterpret_cast<f32x4*>(lds_tbl);
  uint16_t* Ks = reinterpret_cast<uint16_t*>(lds_tbl + TQ_BYTES);
  uint16_t* Vq = Ks + N * KS;
  int qs, h;
  int64_t bw;
  attn_block(qsplit, heads, qs, h, bw);
  const int64_t row0 = bw * N;
  attn_tbl_stage_table(tq, table, heads, h);
  fused_stage_kv<P, CW>(g, (int)row0, h, Ks, Vq);
  __syncthreads();

  const int nsub = N / 16 / qsplit;  // 16-query sub-tiles of this workgroup
  const int q0 = qs * (N / qsplit);
  if (nsub >= kAttnPairNsub && bw < pair_end)
    attn_tbl_tiles<P, 2, CW>(nullptr, &g, out, tq, Ks, Vq, row0, q0, h, heads, nsub, scale_log2);
  else
    attn_tbl_tiles<P, 1, CW>(nullptr, &g, out, tq, Ks, Vq, row0, q0, h, heads, nsub, scale_log2);
}

// The core launch of launch set t of p over a (rows, 3C) qkv buffer (bf16, or fp32 when the
// precision stores fp32).  fused: the qkv GEMM's argument block (MAP_LEVELS rows); the table
// core then computes q / k / v itself from x and the weight and `qkv` is not read.
static int launch_attn_core(const AttnPlan& p, const AttnSet& t, const void* qkv, const float* bias,
                            void* out, float* lse, float scale, hipStream_t s,
                            const GemmArgs* fused) {
  if (t.grid <= 0) return WF_OK;
  const dim3 grid((unsigned)t.grid);  // 1-D, decoded XCD-aware by attn_block
  const float sl2 = scale * 1.4426950408889634f;
  const bool split = p.prec == PREC_SPLIT;
  const bool f16 = p.prec == PREC_FP16;
  const int heads = (int)p.heads;
  if (p.table) {  // bias = the (T, heads) table; index from the coordinates
    auto k = split ? attn_tbl_kernel<PREC_SPLIT>
                   : (f16 ? attn_tbl_kernel<PREC_FP16> : attn_tbl_kernel<PREC_BF16>);
    if (fused) {  // q / k / v from x and the weight
      void (*kf)(GemmArgs, const float*, void*, int, int, float, int64_t) = nullptr;
#define ATTN_FUSED_CASE(CWV)                                                               \
  if (fused->K == CWV)                                                                     \
    kf = split ? attn_tbl_kernel_fused<PREC_SPLIT, CWV>                                    \
               : (f16 ? attn_tbl_kernel_fused<PREC_FP16, CWV> : attn_tbl_kernel_fused<PREC_BF16, CWV>);
      ATTN_FUSED_CASE(kAttnFusedWidths[0])
      ATTN_FUSED_CASE(kAttnFusedWidths[1])
#undef ATTN_FUSED_CASE
      if (!kf || !gemm_levels_callsite(*fused) || fused->N != 3 * fused->K || heads * 16 != fused->K)
        return fail(WF_E_SHAPE, "attention core (q/k/v in the core): instantiated for C = 48 and 96");
      hipLaunchKernelGGL(kf, grid, dim3(512), 0, s, *fused, bias, out, heads, t.qsplit, sl2,
                         t.pair_windows);
      return check_launch("attention core (table bias, q/k/v in the core)");
    }
    hipLaunchKernelGGL(k, grid, dim3(512), 0, s, qkv, bias, out, heads, t.qsplit, sl2,
                       t.pair_windows);
    return check_launch("attention core (table bias, window per workgroup)");
  }
  const int N = (int)(p.ws * p.ws * p.ws);
#define ATTN_HD_CASE(HDV)                                                                  \
  case HDV: {                                                                              \
    auto k = split ? attn_core_kernel<HDV, (HDV >= 192 ? 32 : 64), PREC_SPLIT>             \
                   : (f16 ? attn_core_kernel<HDV, 64, PREC_FP16>                           \
                          : attn_core_kernel<HDV, 64, PREC_BF16>);                         \
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, qkv, bias, out, lse, N, heads, sl2);      \
    break;                                                                                 \
  }
  switch (p.head_dim) {
    ATTN_HD_CASE(16)
    ATTN_HD_CASE(32)
    ATTN_HD_CASE(48)
    ATTN_HD_CASE(64)
    ATTN_HD_CASE(96)
    ATTN_HD_CASE(128)
    ATTN_HD_CASE(192)
    ATTN_HD_CASE(384)
    default:
      return fail(WF_E_SHAPE, "attention: head_dim must be one of 16,32,48,64,96,128,192,384");
  }
#undef ATTN_HD_CASE
  return check_launch("attention core");
}

__global__ void rel_pos_bias_kernel(const float* __restrict__ table, const int64_t* __restrict__ index,
                                    float* __restrict__ bias, int64_t NN, int heads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NN) return;
  const int64_t r = index[i];
  for (int h = 0; h < heads; ++h) bias[h * NN + i] = table[r * heads + h];
}

// qkv = Linear(window_partition(norm1?(x))) of a (B, D1, H1, W1, C) raster into (rows, 3 C)
static GemmArgs qkv_gemm_args(const float* x, const float* ln_w, const float* ln_b, float ln_eps,
                              const uint16_t* wqkv, const float* bqkv, void* qkv, int64_t rows,
                              int64_t B, int64_t C, int64_t D1, int64_t H1, int64_t W1,
                              int64_t ws, int prec) {
  GemmArgs g{};
  g.prec = prec;
  g.a_src = x;
  g.a_bf16 = 0;
  g.a_C = (int)C;
  g.a_nseg = 1;
  g.a_map = MAP_WINDOW;
  g.mB = (int)B;
  g.mD = (int)D1;
  g.mH = (int)H1;
  g.mW = (int)W1;
  g.mws = (int)ws;
  g.a_ln = ln_w ? LN_COMPUTE : LN_NONE;
  g.a_ln_w = ln_w;
  g.a_ln_b = ln_b;
  g.a_eps = ln_eps;
  g.w = wqkv;
  g.M = rows;
  g.N = (int)(3 * C);
  g.K = (int)C;
  g.epi = EPI_STORE;
  g.bias = bqkv;
  g.out = qkv;
  g.out_bf16 = !store32(prec);
  g.ldo = 3 * C;
  return g;
}

// the rows of g come from the n levels of L from level l0 on (MAP_LEVELS), x[0] being level l0's
static void set_level_sources(GemmArgs& g, const float* const* x, const AttnLevels& L, int l0,
                              int n) {
  g.a_map = MAP_LEVELS;
  g.mD = g.mH = g.mW = 0;
  g.a_eps = 0.f;
  for (int l = 0; l < WF_MAX_LEVELS; ++l) {
    const bool on = l < n;
    g.lv_src[l] = on ? x[l] : x[0];
    g.lv_row0[l] = on ? (int)(L.row0[l0 + l] - L.row0[l0]) : 0x7fffffff;
    g.lv_D[l] = on ? L.D[l0 + l] : kAttnLevelsWs;
    g.lv_H[l] = on ? L.H[l0 + l] : kAttnLevelsWs;
    g.lv_W[l] = on ? L.W[l0 + l] : kAttnLevelsWs;
  }
}

// out = Linear(core output); window-major rows == the reshaped raster (Q1)
static GemmArgs proj_gemm_args(const void* ao, const uint16_t* wproj, const float* bproj,
                               float* out, int64_t rows, int64_t C, int prec) {
  GemmArgs p{};
  p.prec = prec;
  p.a_src = ao;
  p.a_bf16 = !store32(prec);
  p.a_C = (int)C;
  p.a_nseg = 1;
  p.a_map = MAP_IDENTITY;
  p.a_ln = LN_NONE;
  p.w = wproj;
  p.M = rows;
  p.N = (int)C;
  p.K = (int)C;
  p.epi = EPI_STORE;
  p.bias = bproj;
  p.out = out;
  p.out_bf16 = 0;
  p.ldo = C;
  return p;
}

// The plan of a call, or what is wrong with it: attn_plan, then the one input the plain header
// cannot compute -- whether a streaming GEMM takes the merged qkv GEMM (only its shape is read)
static const char* attn_plan_call(const int64_t* dhw, int nlev, int64_t B, int64_t C, int64_t heads,
                                  int64_t ws, int prec, int flags, int qkv_mode, AttnPlan& p) {
  if (!valid_prec(prec)) return "unknown precision";
  auto levels_gemm = [&](int64_t rows) {
    GemmArgs g = qkv_gemm_args(nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, rows, B,
                               C, 0, 0, 0, ws, prec);
    g.a_map = MAP_LEVELS;
    GemmRowsPick r;
    return gemm_rows_pick(g, true, r) || gemm_kc_pick_nt(g) > 0;
  };
  return attn_plan(dhw, nlev, B, C, heads, ws, prec, flags, qkv_mode, levels_gemm, p);
}

// the pointers of a call; x: one source per level
struct AttnPtrs {
  const float* const* x;
  const float *ln_w, *ln_b;
  float ln_eps;
  const uint16_t* wqkv_bf16x2;
  const float *bqkv, *bias;
  const uint16_t* wproj_bf16x2;
  const float* bproj;
  float* out;
  void* workspace;
  float* lse;
  float scale;
};

// The launch sets of p, one after the other: qkv GEMM (or nothing: q / k / v in the core), core,
// proj GEMM.  The levels share the weights, the window and head_dim and do not depend on one
// another, so a merged set is one problem of sum(rows) logical rows: the qkv GEMM gathers each
// row from its level (MAP_LEVELS), the core runs over sum(windows), the proj GEMM is the
// identity-map one.  Every row's arithmetic is what its level's own set does, so the two
// groupings are bitwise equal: a GEMM row does not depend on the rows it shares a launch with,
// and the core's result depends on its grid only through which of its two loops a window takes,
// which the merged launch keeps per level (pair_windows).  A fused set computes q / k / v from
// the rasters and the weight, bitwise the GEMM's values, and leaves the qkv area untouched.
static int run_window_attention(const AttnPlan& p, const AttnPtrs& a, hipStream_t s) {
  const AttnLevels& L = p.L;
  const bool merged = p.grouping == ATTN_MERGED;
  for (int l = 0; l < p.nsets; ++l) {  // the set's first level
    const AttnSet& t = p.set[l];
    void* qkv = a.workspace;
    void* ao = reinterpret_cast<char*>(a.workspace) + t.ao;
    // 1. qkv = Linear(window_partition(norm1?(x))): a launch, or the argument block the core
    //    computes q / k / v from
    GemmArgs g = qkv_gemm_args(a.x[l], a.ln_w, a.ln_b, a.ln_eps, a.wqkv_bf16x2, a.bqkv, qkv, t.rows,
                               p.B, p.C, L.D[l], L.H[l], L.W[l], p.ws, p.prec);
    if (merged || t.fused) set_level_sources(g, a.x + l, L, l, merged ? L.nlev : 1);
    int rc = WF_OK;
    if (!t.fused && merged) {  // the plan asked the two launchers' predicates
      if (!try_launch_gemm_rows(g, s, true) && !try_launch_gemm_kc(g, s))
        return fail(WF_E_LAUNCH, "window attention: no GEMM took the planned multi-level qkv");
      rc = check_launch("wf_window_attention_fwd(qkv)");
    } else if (!t.fused) {
      rc = launch_gemm(g, s, "wf_window_attention_fwd(qkv)");
    }
    if (rc) return rc;
    // 2. softmax(q k^T * scale + bias) v
    rc = launch_attn_core(p, t, qkv, a.bias, ao, a.lse, a.scale, s, t.fused ? &g : nullptr);
    if (rc) return rc;
    // 3. proj; window-major rows == the reshaped raster (Q1), level after level
    rc = launch_gemm(proj_gemm_args(ao, a.wproj_bf16x2, a.bproj, a.out + L.row0[l] * p.C, t.rows,
                                    p.C, p.prec),
                     s, "wf_window_attention_fwd(proj)");
    if (rc) return rc;
  }
  return WF_OK;
}

// every forward entry point: validate the pointers, build the plan, run it
static int window_attention_call(const char* who, const int64_t* dhw, int nlev, int64_t B,
                                 int64_t C, int64_t heads, int64_t ws, int prec, int flags,
                                 int qkv_mode, const AttnPtrs& a, void* stream) {
#define ATTN_REQUIRE_PTR(ptr, name) \
  if ((ptr) == nullptr) return fail(WF_E_NULLPTR, std::string(who) + ": " name " is NULL")
  ATTN_REQUIRE_PTR(a.x, "x");
  flags |= ATTN_ALIGNED;
  for (int l = 0; l < nlev && l < kAttnMaxLevels; ++l)
    if (reinterpret_cast<uintptr_t>(a.x[l]) % 16 != 0) flags &= ~ATTN_ALIGNED;
  AttnPlan p;
  if (const char* why = attn_plan_call(dhw, nlev, B, C, heads, ws, prec, flags, qkv_mode, p))
    return fail(WF_E_SHAPE, std::string(who) + ": " + why);
  for (int l = 0; l < nlev; ++l) ATTN_REQUIRE_PTR(a.x[l], "x");
  ATTN_REQUIRE_PTR(a.wqkv_bf16x2, "wqkv_bf16x2");
  ATTN_REQUIRE_PTR(a.bias, "bias");
  ATTN_REQUIRE_PTR(a.wproj_bf16x2, "wproj_bf16x2");
  ATTN_REQUIRE_PTR(a.out, "out");
  ATTN_REQUIRE_PTR(a.workspace, "workspace");
  if (a.ln_w) ATTN_REQUIRE_PTR(a.ln_b, "ln_b");
#undef ATTN_REQUIRE_PTR
  return run_window_attention(p, a, (hipStream_t)stream);
}

}  // namespace wf

using namespace wf;

extern "C" int wf_rel_pos_bias(const float* table, const int64_t* index, float* bias, int64_t N,
                               int64_t heads, int64_t table_rows, void* stream) {
  WF_REQUIRE(N >= 1 && heads >= 1 && table_rows >= 1, "empty bias");
  WF_REQUIRE_PTR(table);
  WF_REQUIRE_PTR(index);
  WF_REQUIRE_PTR(bias);
  const int64_t NN = N * N;
  hipLaunchKernelGGL(rel_pos_bias_kernel, dim3((unsigned)cdiv(NN, 256)), dim3(256), 0,
                     (hipStream_t)stream, table, index, bias, NN, (int)heads);
  return check_launch("wf_rel_pos_bias");
}

extern "C" int64_t wf_window_attention_workspace_bytes(int64_t B, int64_t C, int64_t D1,
                                                       int64_t H1, int64_t W1, int precision) {
  return attn_workspace(B * D1 * H1 * W1, C, precision).bytes;
}

extern "C" int64_t wf_window_attention_levels_workspace_bytes(const int64_t* dhw, int nlev,
                                                              int64_t B, int64_t C,
                                                              int precision) {
  AttnLevels L;
  if (attn_levels_plan(dhw, nlev, B, C, C / 16, L)) return WF_E_SHAPE;
  return attn_workspace(L.row0[nlev], C, precision).bytes;
}

extern "C" int wf_window_attention_plan(const int64_t* dhw, int nlev, int64_t B, int64_t C,
                                        int64_t heads, int64_t ws, int precision, int flags,
                                        int qkv_mode, int64_t* fields) {
  WF_REQUIRE(flags >= 0 && flags < ATTN_ALIGNED, "flags: 1 table bias | 2 LayerNorm | 4 lse | 8 one raster");
  WF_REQUIRE_PTR(fields);
  AttnPlan p{};  // the sets and levels a plan does not use read as 0
  if (const char* why = attn_plan_call(dhw, nlev, B, C, heads, ws, precision, flags | ATTN_ALIGNED,
                                       qkv_mode, p))
    return fail(WF_E_SHAPE, std::string(__func__) + ": " + why);
  int64_t* f = fields;
  for (int64_t v : {(int64_t)p.table, (int64_t)p.head_dim, (int64_t)p.grouping, (int64_t)p.nsets,
                    p.work.qkv, p.work.ao, p.work.bytes, (int64_t)0})
    *f++ = v;
  for (int i = 0; i < kAttnMaxLevels; ++i)
    for (int64_t v : {(int64_t)p.set[i].fused, p.set[i].wh, (int64_t)p.set[i].qsplit,
                      p.set[i].pair_windows, p.set[i].grid})
      *f++ = i < p.nsets ? v : 0;
  for (int l = 0; l < kAttnMaxLevels; ++l) *f++ = l < p.L.nlev ? p.nq[l] : 0;
  return WF_OK;
}

extern "C" int wf_window_attention_fwd_train(const float* x, const float* ln_w,
                                             const float* ln_b, float ln_eps,
                                             const uint16_t* wqkv_bf16x2, const float* bqkv,
                                             const float* bias, const uint16_t* wproj_bf16x2,
                                             const float* bproj, float* out, void* workspace,
                                             float* lse, int64_t B, int64_t C, int64_t D1,
                                             int64_t H1, int64_t W1, int64_t ws, int64_t heads,
                                             float scale, int precision, void* stream) {
  const int64_t dhw[3] = {D1, H1, W1};
  return window_attention_call(
      __func__, dhw, 1, B, C, heads, ws, precision,
      ATTN_RASTER | (ln_w ? ATTN_LN : 0) | (lse ? ATTN_LSE : 0), ATTN_QKV_RULE,
      {&x, ln_w, ln_b, ln_eps, wqkv_bf16x2, bqkv, bias, wproj_bf16x2, bproj, out, workspace, lse, scale},
      stream);
}

extern "C" int wf_window_attention_fwd_table(const float* x, const float* ln_w,
                                             const float* ln_b, float ln_eps,
                                             const uint16_t* wqkv_bf16x2, const float* bqkv,
                                             const float* table, const uint16_t* wproj_bf16x2,
                                             const float* bproj, float* out, void* workspace,
                                             int64_t B, int64_t C, int64_t D1, int64_t H1,
                                             int64_t W1, int64_t ws, int64_t heads, float scale,
                                             int precision, void* stream) {
  const int64_t dhw[3] = {D1, H1, W1};
  return window_attention_call(
      __func__, dhw, 1, B, C, heads, ws, precision, ATTN_RASTER | ATTN_TABLE | (ln_w ? ATTN_LN : 0),
      ATTN_QKV_RULE,
      {&x, ln_w, ln_b, ln_eps, wqkv_bf16x2, bqkv, table, wproj_bf16x2, bproj, out, workspace, nullptr, scale},
      stream);
}

extern "C" int wf_window_attention_fwd(const float* x, const float* ln_w, const float* ln_b,
                                       float ln_eps, const uint16_t* wqkv_bf16x2,
                                       const float* bqkv, const float* bias,
                                       const uint16_t* wproj_bf16x2, const float* bproj,
                                       float* out, void* workspace, int64_t B, int64_t C,
                                       int64_t D1, int64_t H1, int64_t W1, int64_t ws,
                                       int64_t heads, float scale, int precision, void* stream) {
  return wf_window_attention_fwd_train(x, ln_w, ln_b, ln_eps, wqkv_bf16x2, bqkv, bias,
                                       wproj_bf16x2, bproj, out, workspace, nullptr, B, C, D1,
                                       H1, W1, ws, heads, scale, precision, stream);
}

extern "C" int wf_window_attention_fwd_levels(const float* const* x, const int64_t* dhw, int nlev,
                                              const uint16_t* wqkv_bf16x2, const float* bqkv,
                                              const float* table, const uint16_t* wproj_bf16x2,
                                              const float* bproj, float* out, void* workspace,
                                              int64_t B, int64_t C, int64_t heads, float scale,
                                              int precision, void* stream) {
  return wf_window_attention_fwd_levels_mode(x, dhw, nlev, wqkv_bf16x2, bqkv, table, wproj_bf16x2,
                                             bproj, out, workspace, B, C, heads, scale, precision,
                                             stream, ATTN_QKV_RULE);
}

extern "C" int wf_window_attention_fwd_levels_mode(const float* const* x, const int64_t* dhw,
                                                   int nlev, const uint16_t* wqkv_bf16x2,
                                                   const float* bqkv, const float* table,
                                                   const uint16_t* wproj_bf16x2,
                                                   const float* bproj, float* out, void* workspace,
                                                   int64_t B, int64_t C, int64_t heads, float scale,
                                                   int precision, void* stream, int qkv_mode) {
  return window_attention_call(
      __func__, dhw, nlev, B, C, heads, kAttnLevelsWs, precision, ATTN_TABLE, qkv_mode,
      {x, nullptr, nullptr, 0.f, wqkv_bf16x2, bqkv, table, wproj_bf16x2, bproj, out, workspace, nullptr, scale},
      stream);
}
