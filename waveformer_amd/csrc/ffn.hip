// ffn.hip -- CCF_FFN with the Block's norm2 + double residual (a7, quirk Q4),
// and PatchMerging (a9, quirk Q3).
//
// CCF_FFN.forward (network_models/wave_helper.py:260-294), for input n (B,D,H,W,C):
//   h1 = GELU(LN_eps1(pwconv(n)))              pwconv = Conv3d(C, 4C, 1) (+bias)    :278-279
//   h2 = GELU(LN_eps2(dwconv(h1)))             dwconv = Conv3d(4C, 4C, 3, pad 1, groups=4C) :285-286
//   return n + fc(h2)                          fc = Linear(4C, C)                    :289-293
// and the Block adds it to attn_fused again: out = x + (n + fc(h2)), n = norm2(x)   :509
// Launches: gemm(pw, LN2 of x in the loader, LN+GELU epilogue) -> dwconv_ln_gelu ->
//           gemm(fc, residual epilogue).  h1/h2 live in the caller's workspace (bf16 for
//           PREC_BF16, fp32 for PREC_SPLIT).  That is the general form; which kernels a
//           call takes and where its workspace areas lie is ffn_plan.hpp's decision.
#include "kernels.hpp"

namespace wf {

template <typename T>
struct Store4;
template <>
struct Store4<uint16_t> {  // bf16 storage
  typedef bf16x4 vec;
  static __device__ __forceinline__ f32x4 up(vec u) {
    return f32x4{bf2f((uint16_t)u[0]), bf2f((uint16_t)u[1]), bf2f((uint16_t)u[2]),
                 bf2f((uint16_t)u[3])};
  }
  static __device__ __forceinline__ uint16_t down(float v) { return f2bf(v); }
  static __device__ __forceinline__ vec zero() { return vec{0, 0, 0, 0}; }
  static __device__ __forceinline__ void store4(uint16_t* p, f32x4 v) {
    bf16x4 o;
    o[0] = (short)f2bf(v.x);
    o[1] = (short)f2bf(v.y);
    o[2] = (short)f2bf(v.z);
    o[3] = (short)f2bf(v.w);
    *reinterpret_cast<bf16x4*>(p) = o;
  }
};
template <>
struct Store4<float> {  // fp32 storage
  typedef f32x4 vec;
  static __device__ __forceinline__ f32x4 up(vec u) { return u; }
  static __device__ __forceinline__ float down(float v) { return v; }
  static __device__ __forceinline__ vec zero() { return vec{0, 0, 0, 0}; }
  static __device__ __forceinline__ void store4(float* p, f32x4 v) {
    *reinterpret_cast<f32x4*>(p) = v;
  }
};

// Depthwise 3x3x3 conv + bias, then LayerNorm over the Hd channels of each position and
// GELU.  Workgroup = R rows (y) x TW columns (x) of one (b, z) plane, all channels; a thread
// owns 4 channels of one row and slides a 3x3x3 register window along x (9 new loads per
// output).  Outputs are staged in LDS for the per-position LayerNorm.
template <int TW, typename T>
__global__ __launch_bounds__(512) void dwconv_ln_gelu_kernel(
    const T* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps,
    T* __restrict__ out, int B, int Hd, int D, int H, int W, int R) {
  typedef Store4<T> S;
  typedef typename S::vec vec;
  extern __shared__ __attribute__((aligned(16))) float rb[];  // [R*TW][Hd+4], then stats
  const int HP = Hd + 4;
  const int nchunk = Hd >> 2;
  const int ntx = (W + TW - 1) / TW, nty = (H + R - 1) / R;
  // XCD-contiguous (z, y, x) tile order: neighbouring tiles re-read the same input rows and
  // find them in their XCD's L2
  int t = xcd_block_id();
  const int xt = t % ntx;
  t /= ntx;
  const int yt = t % nty;
  t /= nty;
  const int z = t % D;
  const int b = t / D;
  const int tid = threadIdx.x;
  const int chunk = tid % nchunk, rr = tid / nchunk;
  const int y = yt * R + rr;
  const int xb = xt * TW;
  const bool act = rr < R && y < H;

  if (act) {
    f32x4 wt[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      wt[k].x = w[(4 * chunk + 0) * 27 + k];
      wt[k].y = w[(4 * chunk + 1) * 27 + k];
      wt[k].z = w[(4 * chunk + 2) * 27 + k];
      wt[k].w = w[(4 * chunk + 3) * 27 + k];
    }
    const f32x4 bv = reinterpret_cast<const f32x4*>(bias)[chunk];
    // The 9 (dz, dy) input rows: clamped base pointers + a validity mask.  Loads are always
    // issued (clamped in-bounds addresses) and zeroed by a select afterwards: a branch around
    // each load would make hipcc wait vmcnt(0) per load and serialise the 9-load batch.
    const T* rowp[9];
    unsigned rvalid = 0;
#pragma unroll
    for (int r9 = 0; r9 < 9; ++r9) {
      const int zz = z + r9 / 3 - 1, yy = y + r9 % 3 - 1;
      const bool ok = zz >= 0 && zz < D && yy >= 0 && yy < H;
      rvalid |= (ok ? 1u : 0u) << r9;
      const int zc = min(max(zz, 0), D - 1), yc = min(max(yy, 0), H - 1);
      rowp[r9] = in + (((int64_t)b * D + zc) * H + yc) * (int64_t)W * Hd + 4 * chunk;
    }
    auto ld = [&](int r9, int xx) -> vec {
      const int xc = min(max(xx, 0), W - 1);
      const vec v = *reinterpret_cast<const vec*>(rowp[r9] + (int64_t)xc * Hd);
      const bool ok = ((rvalid >> r9) & 1u) && xx >= 0 && xx < W;
      return ok ? v : S::zero();
    };
    vec win[9][3];
#pragma unroll
    for (int r9 = 0; r9 < 9; ++r9) {
      win[r9][0] = ld(r9, xb - 1);
      win[r9][1] = ld(r9, xb);
    }
#pragma unroll 1
    for (int xi = 0; xi < TW; ++xi) {
      const int x = xb + xi;
#pragma unroll
      for (int r9 = 0; r9 < 9; ++r9) win[r9][2] = ld(r9, x + 1);
      f32x4 acc = bv;
#pragma unroll
      for (int r9 = 0; r9 < 9; ++r9)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) acc += wt[r9 * 3 + dx] * S::up(win[r9][dx]);
      *reinterpret_cast<f32x4*>(rb + (size_t)(rr * TW + xi) * HP + 4 * chunk) = acc;
#pragma unroll
      for (int r9 = 0; r9 < 9; ++r9) {
        win[r9][0] = win[r9][1];
        win[r9][1] = win[r9][2];
      }
    }
  }
  __syncthreads();
  // LayerNorm statistics: one lane per position walks its row in LDS (no cross-lane traffic)
  const int P = R * TW;
  float* st = rb + (size_t)P * HP;  // [P][2]
  for (int p = tid; p < P; p += blockDim.x) {
    const f32x4* row = reinterpret_cast<const f32x4*>(rb + (size_t)p * HP);
    f32x4 s4 = {0, 0, 0, 0};
    for (int c = 0; c < nchunk; ++c) s4 += row[c];
    const float mean = ((s4.x + s4.y) + (s4.z + s4.w)) / (float)Hd;
    f32x4 q4 = {0, 0, 0, 0};
    for (int c = 0; c < nchunk; ++c) {
      const f32x4 d = row[c] - mean;
      q4 += d * d;
    }
    st[2 * p] = mean;
    st[2 * p + 1] = rsqrtf(((q4.x + q4.y) + (q4.z + q4.w)) / (float)Hd + eps);
  }
  __syncthreads();
  // normalise + GELU + store: consecutive threads own consecutive 4-channel chunks of a row,
  // so every store instruction writes whole contiguous rows
  for (int it = tid; it < P * nchunk; it += blockDim.x) {
    const int p = it / nchunk, c = it - p * nchunk;
    const int yy = yt * R + p / TW, xx = xb + p % TW;
    if (yy >= H || xx >= W) continue;
    const f32x4 lw = reinterpret_cast<const f32x4*>(ln_w)[c];
    const f32x4 lb = reinterpret_cast<const f32x4*>(ln_b)[c];
    f32x4 v = (reinterpret_cast<const f32x4*>(rb + (size_t)p * HP)[c] - st[2 * p]) * st[2 * p + 1] *
                  lw + lb;
    T* dst = out + ((((int64_t)b * D + z) * H + yy) * W + xx) * Hd + 4 * c;
    v = gelu_erf4(v);
    S::store4(dst, v);
  }
}

// Depthwise 3x3x3 conv + bias, no normalisation (CCF_FFN's LN2 + GELU run in the fc GEMM's
// A loader).  Workgroup = (b, z segment of ZS output planes, TY x TX tile of (y, x), CH = 32
// channels); 256 threads = TX columns x CH channels, each thread owning the TY outputs of its
// (x, channel) column.  The workgroup marches z through the input planes z0-1 .. z0+ZS: each
// plane's (TY+2) x (TX+2) x CH halo tile is staged once into LDS (double buffered; the next
// plane's loads are issued before the current plane's arithmetic), and every input value is
// read from LDS once per thread row and scattered into the three output planes it feeds
// (rolling accumulators accA/accB/accC = planes p-1, p, p+1): 3.75 LDS reads and 27 FMAs per
// output.  Global traffic is one read of the input (+ the halo, shared through L2 by the
// neighbouring tiles that the XCD-contiguous order runs on the same XCD) and one write.
template <typename T>
struct Vec16;  // one 16-byte global vector of T, widened to fp32
template <>
struct Vec16<float> {
  typedef f32x4 raw;
  static constexpr int N = 4;
  static __device__ __forceinline__ raw zero() { return raw{0, 0, 0, 0}; }
  static __device__ __forceinline__ void put(float* d, raw u) {
    *reinterpret_cast<f32x4*>(d) = u;
  }
};
template <>
struct Vec16<uint16_t> {
  typedef bf16x8 raw;
  static constexpr int N = 8;
  static __device__ __forceinline__ raw zero() { return raw{0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ void put(float* d, raw u) {
    reinterpret_cast<f32x4*>(d)[0] = f32x4{bf2f((uint16_t)u[0]), bf2f((uint16_t)u[1]),
                                           bf2f((uint16_t)u[2]), bf2f((uint16_t)u[3])};
    reinterpret_cast<f32x4*>(d)[1] = f32x4{bf2f((uint16_t)u[4]), bf2f((uint16_t)u[5]),
                                           bf2f((uint16_t)u[6]), bf2f((uint16_t)u[7])};
  }
};

constexpr int DW_CH = 32, DW_TX = 16, DW_TY = 8;

template <typename T>
struct Store2;
template <>
struct Store2<float> {
  static __device__ __forceinline__ void put(float* p, f32x2 v) {
    *reinterpret_cast<f32x2*>(p) = v;
  }
  static __device__ __forceinline__ f32x2 round(f32x2 v) { return v; }
};
template <>
struct Store2<uint16_t> {
  static __device__ __forceinline__ void put(uint16_t* p, f32x2 v) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
  }
  static __device__ __forceinline__ f32x2 round(f32x2 v) {  // statistics of the stored values
    return f32x2{bf2f(f2bf(v.x)), bf2f(f2bf(v.y))};
  }
};

// 256 threads = DW_TX columns x 16 channel PAIRS: each thread owns two adjacent channels of
// one x column and the TY outputs of that column, so the 27-tap accumulation runs on f32x2
// channel pairs (one 8-B LDS read per tap feeds both; the build has no packed-FP32
// instructions, DESIGN.md 6.1, so each pair FMA is two v_fma_f32), and the per-position
// 32-channel statistics reduce over 16 lanes.
// LN1 (fp32 only): the input is the pwconv's raw output and h1 = GELU(LN1(.)) is formed in
// the plane staging -- ln1_stats (M, 2) {mean, rstd} per position, ln1_w / ln1_b (Hd) -- so
// the separate LayerNorm + GELU pass over h1 (read + write of the whole tensor) is gone
// (stages 3 / 4 of the encoder); halo positions outside the volume stay zero.
// CH_ / TX_: the channel chunk and tile width -- 32 x 16 by default; narrow volumes (W <= 8:
// the stage-4 8^3 shapes, where half of a 16-wide tile's threads had no column) take 64 x 8
// (two 32-channel statistics groups per workgroup)
template <typename T, bool LN1, bool FLIP = false, int CH_ = DW_CH, int TX_ = DW_TX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void dwconv3d_kernel(
    const T* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
    T* __restrict__ out, float* __restrict__ pstats, int B, int Hd, int D, int H, int W, int ZS,
    double* __restrict__ cstats, const float* __restrict__ ln1_stats,
    const float* __restrict__ ln1_w, const float* __restrict__ ln1_b) {
  static_assert(!LN1 || sizeof(T) == 4, "LN1 staging: fp32 h1");
  constexpr int CH = CH_, TX = TX_, TY = DW_TY;
  static_assert(CH % DW_STAT_GROUP == 0, "whole statistics groups per workgroup channel chunk");
  constexpr int NG = CH / DW_STAT_GROUP;  // statistics groups per channel chunk
  static_assert(TX * (CH / 2) == 256, "one thread per (column, channel pair)");
  constexpr int PY = TY + 2, PX = TX + 2;
  typedef Vec16<T> V;
  constexpr int NV = CH / V::N;                  // 16-byte vectors per tile position
  constexpr int NLD = (PY * PX * NV + 255) / 256;
  __shared__ __attribute__((aligned(16))) float pl[2][PY * PX * CH];
  __shared__ __attribute__((aligned(16))) float l1w[LN1 ? CH : 1], l1b[LN1 ? CH : 1];

  const int ncc = Hd / CH, ntx = (W + TX - 1) / TX, nty = (H + TY - 1) / TY;
  const int nzs = (D + ZS - 1) / ZS;
  // XCD-contiguous tile order, channel chunk fastest, then x: the ncc workgroups that split
  // one spatial tile's Hd-wide rows run together (whole rows leave DRAM together), and
  // neighbouring tiles, which share halo rows, run on the same XCD and meet in its L2
  int t = xcd_block_id();
  const int cc = t % ncc;
  t /= ncc;
  const int xt = t % ntx;
  t /= ntx;
  const int yt = t % nty;
  t /= nty;
  const int zt = t % nzs;
  const int b = t / nzs;
  const int x0 = xt * TX, y0 = yt * TY, z0 = zt * ZS, z1 = min(z0 + ZS, D);
  const int c0 = cc * CH;
  const int tid = threadIdx.x;
  const int cp = tid % (CH / 2), xi = tid / (CH / 2);

  // FLIP: the taps mirrored (w[26 - k]) -- the input gradient of the same conv (training)
  f32x2 w2[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const int kk = FLIP ? 26 - k : k;
    w2[k] = f32x2{w[(c0 + 2 * cp) * 27 + kk], w[(c0 + 2 * cp + 1) * 27 + kk]};
  }
  const f32x2 bv = bias ? f32x2{bias[c0 + 2 * cp], bias[c0 + 2 * cp + 1]} : f32x2{0.f, 0.f};

  if (LN1) {
    for (int i = tid; i < CH; i += 256) {
      l1w[i] = ln1_w[c0 + i];
      l1b[i] = ln1_b[c0 + i];
    }
    __syncthreads();
  }
  // staging of one input plane: item i -> (tile position i / NV, vector i % NV)
  typename V::raw stg[NLD];
  f32x2 st1[LN1 ? NLD : 1];
  bool ok1[LN1 ? NLD : 1];
  const T* src = in + (int64_t)b * D * H * W * Hd + c0;
  auto fetch = [&](int p) {
    const bool pz = p >= 0 && p < D;
    const int pc = min(max(p, 0), D - 1);
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int i = min(j * 256 + tid, PY * PX * NV - 1);
      const int pos = i / NV, v = i - pos * NV;
      const int yy = y0 - 1 + pos / PX, xx = x0 - 1 + pos % PX;
      const bool ok = pz && yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int yc = min(max(yy, 0), H - 1), xc = min(max(xx, 0), W - 1);
      const int64_t gp = ((int64_t)pc * H + yc) * W + xc;
      const typename V::raw u = *reinterpret_cast<const typename V::raw*>(src + gp * Hd + V::N * v);
      stg[j] = ok ? u : V::zero();
      if constexpr (LN1) {
        st1[j] = *reinterpret_cast<const f32x2*>(ln1_stats + ((int64_t)b * D * H * W + gp) * 2);
        ok1[j] = ok;
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int i = j * 256 + tid;
      if (i < PY * PX * NV) {
        if constexpr (LN1) {
          const int v = i % NV;
          const f32x4 lw = *reinterpret_cast<const f32x4*>(l1w + 4 * v);
          const f32x4 lb = *reinterpret_cast<const f32x4*>(l1b + 4 * v);
          const f32x4 y = gelu_erf4((stg[j] - st1[j].x) * st1[j].y * lw + lb);
          stg[j] = ok1[j] ? y : V::zero();
        }
        V::put(pl[buf] + (size_t)i * V::N, stg[j]);
      }
    }
  };

  f32x2 accA[TY], accB[TY], accC[TY];
#pragma unroll
  for (int o = 0; o < TY; ++o) accA[o] = accB[o] = accC[o] = f32x2{0.f, 0.f};
  const int xo = x0 + xi;
  // cstats: per-(sample, channel) sum and sum of squares of the stored outputs (InstanceNorm /
  // GroupNorm(C, C) statistics of the next layer), fp64 per thread
  double cs0 = 0.0, cs1 = 0.0, cq0 = 0.0, cq1 = 0.0;
  fetch(z0 - 1);
  commit(0);
  __syncthreads();
  int buf = 0;
  for (int p = z0 - 1; p <= z1; ++p) {
    fetch(p + 1);  // next plane in flight during this plane's arithmetic (past z1: unused)
    const float* P = pl[buf] + xi * CH + 2 * cp;
    // plane p feeds output p+1 (kz = 0), p (kz = 1) and p-1 (kz = 2)
#pragma unroll
    for (int r = 0; r < PY; ++r) {
      const f32x2 v0 = *reinterpret_cast<const f32x2*>(P + (r * PX + 0) * CH);
      const f32x2 v1 = *reinterpret_cast<const f32x2*>(P + (r * PX + 1) * CH);
      const f32x2 v2 = *reinterpret_cast<const f32x2*>(P + (r * PX + 2) * CH);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int o = r - ky;  // output row fed by input row r through tap ky
        if (o < 0 || o >= TY) continue;
        const f32x2* w0 = w2 + ky * 3;
        // one pair FMA per tap into the running sum
        accC[o] = w0[2] * v2 + (w0[1] * v1 + (w0[0] * v0 + accC[o]));
        accB[o] = w0[11] * v2 + (w0[10] * v1 + (w0[9] * v0 + accB[o]));
        accA[o] = w0[20] * v2 + (w0[19] * v1 + (w0[18] * v0 + accA[o]));
      }
    }
    // output plane p-1 is complete
    const int zo = p - 1;
    if (zo >= z0) {
      f32x2 r1[TY];
#pragma unroll
      for (int o = 0; o < TY; ++o) r1[o] = Store2<T>::round(accA[o] + bv);
      float mu[TY], m2[TY];
      if (pstats) {  // {mean, M2} of this 32-channel group (16 consecutive lanes) per position
#pragma unroll
        for (int o = 0; o < TY; ++o) mu[o] = group_sum<16>(r1[o].x + r1[o].y) * (1.f / 32.f);
#pragma unroll
        for (int o = 0; o < TY; ++o) {
          const float dx = r1[o].x - mu[o], dy = r1[o].y - mu[o];
          m2[o] = group_sum<16>(dx * dx + dy * dy);
        }
      }
      if (xo < W) {
#pragma unroll
        for (int o = 0; o < TY; ++o) {
          const int yo = y0 + o;
          if (yo < H) {
            const int64_t pos = (((int64_t)b * D + zo) * H + yo) * W + xo;
            Store2<T>::put(out + pos * Hd + c0 + 2 * cp, r1[o]);
            if (cstats) {
              const double a0 = (double)r1[o].x, a1 = (double)r1[o].y;
              cs0 += a0;
              cs1 += a1;
              cq0 += a0 * a0;
              cq1 += a1 * a1;
            }
            if (pstats && cp % (DW_STAT_GROUP / 2) == 0)
              *reinterpret_cast<float2*>(pstats + (pos * (ncc * NG) + cc * NG + cp / (DW_STAT_GROUP / 2)) * 2) =
                  float2{mu[o], m2[o]};
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < TY; ++o) {
      accA[o] = accB[o];
      accB[o] = accC[o];
      accC[o] = f32x2{0.f, 0.f};
    }
    commit(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  if (cstats) {  // the 16 columns of a channel pair, then one fp64 atomic per (channel, moment)
    double* red = reinterpret_cast<double*>(&pl[0][0]);  // [TX][CH / 2][4]
    double* r = red + (xi * (CH / 2) + cp) * 4;
    r[0] = cs0;
    r[1] = cs1;
    r[2] = cq0;
    r[3] = cq1;
    __syncthreads();
    if (tid < CH * 2) {
      const int pc = tid >> 2, mom = tid & 3;  // mom: {sum c, sum c+1, sq c, sq c+1}
      double t = 0.0;
#pragma unroll
      for (int xx = 0; xx < TX; ++xx) t += red[(xx * (CH / 2) + pc) * 4 + mom];
      const int c = c0 + 2 * pc + (mom & 1);
      atomicAdd(cstats + ((int64_t)b * Hd + c) * 2 + (mom >> 1), t);
    }
  }
}

int launch_dwconv3d(const void* in, const float* w, const float* b, void* out, float* pstats,
                    int B, int Hd, int D, int H, int W, int prec, hipStream_t s, double* cstats,
                    const float* ln1_stats, const float* ln1_w, const float* ln1_b, int flip) {
  if (Hd % DW_CH != 0) return fail(WF_E_SHAPE, "dwconv3d: hidden width must be a multiple of 32");
  if (flip && (ln1_stats || !store32(prec)))
    return fail(WF_E_SHAPE, "dwconv3d: the mirrored taps are for fp32 data without LN1 staging");
  // z segment: enough workgroups to fill 256 CUs ~8 deep, but long enough that the two halo
  // planes per segment stay a small overhead
  // narrow volumes (W <= 8): 64 channels x 8 columns per workgroup, z segments down to 4
  const bool narrow = W <= 8 && Hd % 64 == 0 && store32(prec) && !flip && !ln1_stats;
  const int dch = narrow ? 64 : DW_CH, dtx = narrow ? 8 : DW_TX;
  const int64_t base = (int64_t)B * (Hd / dch) * cdiv(H, DW_TY) * cdiv(W, dtx);
  int ZS = D;
  const int zmin = narrow ? 4 : 8;
  while (ZS > zmin && base * cdiv(D, ZS) < 2048) ZS = (ZS + 1) / 2;
  const int64_t blocks = base * cdiv(D, ZS);
  if (narrow) {
    hipLaunchKernelGGL((dwconv3d_kernel<float, false, false, 64, 8>), dim3((unsigned)blocks),
                       dim3(256), 0, s, reinterpret_cast<const float*>(in), w, b,
                       reinterpret_cast<float*>(out), pstats, B, Hd, D, H, W, ZS, cstats, nullptr,
                       nullptr, nullptr);
  } else if (ln1_stats) {
    if (!store32(prec) || !ln1_w || !ln1_b)
      return fail(WF_E_SHAPE, "dwconv3d: the LN1 staging needs fp32 h1 and LN1 weights");
    hipLaunchKernelGGL((dwconv3d_kernel<float, true>), dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const float*>(in), w, b, reinterpret_cast<float*>(out),
                       pstats, B, Hd, D, H, W, ZS, cstats, ln1_stats, ln1_w, ln1_b);
  } else if (store32(prec) && flip)
    hipLaunchKernelGGL((dwconv3d_kernel<float, false, true>), dim3((unsigned)blocks), dim3(256),
                       0, s, reinterpret_cast<const float*>(in), w, b,
                       reinterpret_cast<float*>(out), pstats, B, Hd, D, H, W, ZS, cstats,
                       nullptr, nullptr, nullptr);
  else if (store32(prec))
    hipLaunchKernelGGL((dwconv3d_kernel<float, false>), dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const float*>(in), w, b, reinterpret_cast<float*>(out),
                       pstats, B, Hd, D, H, W, ZS, cstats, nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL((dwconv3d_kernel<uint16_t, false>), dim3((unsigned)blocks), dim3(256), 0,
                       s, reinterpret_cast<const uint16_t*>(in), w, b,
                       reinterpret_cast<uint16_t*>(out), pstats, B, Hd, D, H, W, ZS, cstats,
                       nullptr, nullptr, nullptr);
  return check_launch("dwconv3d");
}

__global__ __launch_bounds__(256) void ln_stats_finalize_kernel(const float* __restrict__ ps,
                                                                int np, int group, float eps,
                                                                float* __restrict__ out,
                                                                int64_t M) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  const float2* p = reinterpret_cast<const float2*>(ps) + r * np;
  float mu = 0.f;
  for (int i = 0; i < np; ++i) mu += p[i].x;
  mu *= 1.f / np;
  float m2 = 0.f;
  for (int i = 0; i < np; ++i) {
    const float d = p[i].x - mu;
    m2 += p[i].y + (float)group * d * d;
  }
  *reinterpret_cast<float2*>(out + 2 * r) = float2{mu, rsqrtf(m2 / ((float)np * group) + eps)};
}

int launch_ln_stats_finalize(const float* pstats, int np, int group, float eps, float* out,
                             int64_t M, hipStream_t s) {
  hipLaunchKernelGGL(ln_stats_finalize_kernel, dim3((unsigned)cdiv(M, 256)), dim3(256), 0, s,
                     pstats, np, group, eps, out, M);
  return check_launch("ln_stats_finalize");
}

template <typename T>
static void launch_dw(int tw, dim3 grid, dim3 block, size_t lds, hipStream_t s, const void* in,
                      const float* w, const float* b, const float* ln_w, const float* ln_b,
                      float eps, void* out, int B, int Hd, int D, int H, int W, int R) {
  const T* i = reinterpret_cast<const T*>(in);
  T* o = reinterpret_cast<T*>(out);
  switch (tw) {
    case 2: hipLaunchKernelGGL((dwconv_ln_gelu_kernel<2, T>), grid, block, lds, s, i, w, b, ln_w, ln_b, eps, o, B, Hd, D, H, W, R); break;
    case 4: hipLaunchKernelGGL((dwconv_ln_gelu_kernel<4, T>), grid, block, lds, s, i, w, b, ln_w, ln_b, eps, o, B, Hd, D, H, W, R); break;
    case 8: hipLaunchKernelGGL((dwconv_ln_gelu_kernel<8, T>), grid, block, lds, s, i, w, b, ln_w, ln_b, eps, o, B, Hd, D, H, W, R); break;
    default: hipLaunchKernelGGL((dwconv_ln_gelu_kernel<16, T>), grid, block, lds, s, i, w, b, ln_w, ln_b, eps, o, B, Hd, D, H, W, R); break;
  }
}

int launch_dwconv_ln_gelu(const void* in, const float* w, const float* b, const float* ln_w,
                          const float* ln_b, float eps, void* out, int B, int Hd, int D, int H,
                          int W, int prec, hipStream_t s) {
  if (Hd % 4 != 0) return fail(WF_E_SHAPE, "dwconv: hidden width must be a multiple of 4");
  const int nchunk = Hd / 4;
  if (nchunk > 512) return fail(WF_E_SHAPE, "dwconv: hidden width > 2048 is not supported");
  int R = 256 / nchunk;
  if (R < 1) R = 1;
  if (R > H) R = H;
  int TW = Hd >= 1536 ? 8 : 16;
  // LDS budget: R * TW * (Hd + 4) floats <= 64 KB
  while (TW > 2 && (size_t)R * TW * (Hd + 4) * 4 > 64 * 1024) TW >>= 1;
  while (R > 1 && (size_t)R * TW * (Hd + 4) * 4 > 64 * 1024) --R;
  const int threads = (int)cdiv((int64_t)nchunk * R, 64) * 64;
  const int tw_eff = TW > W ? W : TW;
  int tw_t = 16;
  if (tw_eff <= 2) tw_t = 2;
  else if (tw_eff <= 4) tw_t = 4;
  else if (tw_eff <= 8) tw_t = 8;
  const size_t lds = ((size_t)R * tw_t * (Hd + 4) + 2 * (size_t)R * tw_t) * 4;
  const int64_t blocks = (int64_t)B * D * cdiv(H, R) * cdiv(W, tw_t);
  if (store32(prec))
    launch_dw<float>(tw_t, dim3((unsigned)blocks), dim3(threads), lds, s, in, w, b, ln_w, ln_b,
                     eps, out, B, Hd, D, H, W, R);
  else
    launch_dw<uint16_t>(tw_t, dim3((unsigned)blocks), dim3(threads), lds, s, in, w, b, ln_w,
                        ln_b, eps, out, B, Hd, D, H, W, R);
  return check_launch("dwconv_ln_gelu");
}

// the back half's argument block (ZS and dbg are the launchers'; the whole-FFN kernel's front
// half is added by its caller)
static DwFcArgs dwfc_args(const void* h1, const float* dw_w, const float* dw_b, const float* ln2_w,
                          const float* ln2_b, float eps2, const uint16_t* fc, const float* fc_b,
                          const float* x, const float* stats, const float* n2_w,
                          const float* n2_b, const float* bscale, float* out, int64_t B, int64_t D,
                          int64_t H, int64_t W) {
  DwFcArgs d{};
  d.h1 = h1;
  d.dw_w = dw_w;
  d.dw_b = dw_b;
  d.ln2_w = ln2_w;
  d.ln2_b = ln2_b;
  d.eps2 = eps2;
  d.fc = fc;
  d.fc_b = fc_b;
  d.x = x;
  d.stats = stats;
  d.n2_w = n2_w;
  d.n2_b = n2_b;
  d.bscale = bscale;
  d.out = out;
  d.B = (int)B;
  d.D = (int)D;
  d.H = (int)H;
  d.W = (int)W;
  return d;
}

static_assert(kFfnPrecBf16 == PREC_BF16, "ffn_plan.hpp's storage rule is store32");

// h1 = GELU(LN1(pwconv(norm2?(x)) + bias)) into (M, hidden): the LN1 + GELU epilogue form (the
// other front forms store plainly, EPI_STORE)
static GemmArgs pwconv_gemm_args(const float* xh, const float* stats, const float* n2_w,
                                 const float* n2_b, const uint16_t* pw, const float* pw_b,
                                 const float* ln1_w, const float* ln1_b, float eps1, void* h1,
                                 int64_t M, int64_t C, int64_t hidden, int prec) {
  GemmArgs g{};
  g.prec = prec;
  g.a_src = xh;
  g.a_bf16 = 0;
  g.a_C = (int)C;
  g.a_nseg = 1;
  g.a_map = MAP_IDENTITY;
  g.a_ln = stats ? LN_GIVEN : LN_NONE;
  g.a_stats = stats;
  g.a_ln_w = n2_w;
  g.a_ln_b = n2_b;
  g.w = pw;
  g.M = M;
  g.N = (int)hidden;
  g.K = (int)C;
  g.epi = EPI_LN_GELU;
  g.bias = pw_b;
  g.e_ln_w = ln1_w;
  g.e_ln_b = ln1_b;
  g.e_eps = eps1;
  g.out = h1;
  g.out_bf16 = !store32(prec);
  g.ldo = hidden;
  return g;
}

// out = x + (norm2?(x) + fc(.) + bias) * branch_scale over the rows of h2: GELU(LN2(h2)) formed
// in the loader from the dwconv's partials ln2_pst, or (ln2_pst NULL) h2 taken as it is
static GemmArgs fc_gemm_args(const void* h2, const float* ln2_pst, const float* ln2_w,
                             const float* ln2_b, float eps2, const uint16_t* fc,
                             const float* fc_b, const float* xh, const float* stats,
                             const float* n2_w, const float* n2_b, const float* branch_scale,
                             float* out, int64_t M, int64_t C, int64_t hidden,
                             int64_t rows_per_sample, int prec) {
  GemmArgs f{};
  f.prec = prec;
  f.a_src = h2;
  f.a_bf16 = !store32(prec);
  f.a_C = (int)hidden;
  f.a_nseg = 1;
  f.a_map = MAP_IDENTITY;
  f.a_ln = ln2_pst ? LN_PARTIAL : LN_NONE;
  if (ln2_pst) {
    f.a_stats = ln2_pst;
    f.a_np = (int)(hidden / DW_STAT_GROUP);
    f.a_ln_w = ln2_w;
    f.a_ln_b = ln2_b;
    f.a_eps = eps2;
    f.a_gelu = 1;
  }
  f.w = fc;
  f.M = M;
  f.N = (int)C;
  f.K = (int)hidden;
  f.epi = EPI_RESID;
  f.bias = fc_b;
  f.r_x = xh;
  f.r_stats = stats;
  f.r_ln_w = n2_w;
  f.r_ln_b = n2_b;
  f.r_scale = branch_scale;
  f.rows_per_sample = rows_per_sample;
  f.out = out;
  f.ldo = C;
  return f;
}

// The plan of a call, or what is wrong with it: the shape, then ffn_plan under the environment
// switches as a call in this process sees them, then the one input the plain
// header cannot compute -- gemm_kc's column chunk for the plain-store pwconv of the partials form
static const char* ffn_plan_call(int64_t B, int64_t C, int64_t hidden, int64_t D, int64_t H,
                                 int64_t W, int prec, bool train, FfnPlan& p) {
  if (!(B >= 1 && D >= 1 && H >= 1 && W >= 1)) return "empty volume";
  if (!(C % 8 == 0 && hidden % 8 == 0)) return "C and hidden must be multiples of 8";
  if (!valid_prec(prec)) return "unknown precision";
  static const bool ln1_fuse = getenv("WF_FFN_LN1_FUSE") != nullptr;  // latched
  FfnSwitches sw;
  sw.whole = getenv("WF_FFN_FUSED") != nullptr;      // per call: tests switch it
  sw.no_dwfc = getenv("WF_FFN_NO_DWFC") != nullptr;  // per call: tests switch it
  sw.ln1_fuse = ln1_fuse;
  const char* why = ffn_plan(B, C, hidden, D, H, W, prec, train, sw, p);
  if (!why && p.front == FFN_FRONT_PARTIALS) {  // only the GEMM's shape is read
    GemmArgs pw = pwconv_gemm_args(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, 0.f, nullptr, B * D * H * W, C, hidden, prec);
    pw.epi = EPI_STORE;
    ffn_plan_set_kc_chunk(p, hidden, gemm_kc_pick_nt(pw));
  }
  return why;
}

}  // namespace wf

using namespace wf;

extern "C" int64_t wf_ccf_ffn_workspace_bytes(int64_t B, int64_t C, int64_t hidden, int64_t D,
                                              int64_t H, int64_t W, int precision) {
  return ffn_workspace(B * D * H * W, C, hidden, precision).bytes;
}

extern "C" int wf_ccf_ffn_plan(int64_t B, int64_t C, int64_t hidden, int64_t D, int64_t H,
                               int64_t W, int precision, int train, int64_t* offsets) {
  FfnPlan plan;
  if (const char* why = ffn_plan_call(B, C, hidden, D, H, W, precision, train != 0, plan))
    return fail(WF_E_SHAPE, std::string(__func__) + ": " + why);
  if (offsets) {
    const FfnWorkspace ws = ffn_workspace(B * D * H * W, C, hidden, precision);
    const int64_t o[7] = {ws.h1, ws.h2, ws.ln2_pst, ws.ln1_pst, ws.ln1_st, ws.fcs, ws.bytes};
    for (int i = 0; i < 7; ++i) offsets[i] = o[i];
  }
  return plan.front | plan.back << 8;
}

extern "C" int wf_ccf_ffn_stage(int stage, const float* xh, const float* stats,
                                const float* n2_w, const float* n2_b,
                                const uint16_t* pw_bf16x2, const float* pw_b,
                                const float* ln1_w, const float* ln1_b, float eps1,
                                const float* dw_w, const float* dw_b, const float* ln2_w,
                                const float* ln2_b, float eps2, const uint16_t* fc_bf16x2,
                                const float* fc_b, const float* branch_scale, float* out,
                                void* workspace, int64_t B, int64_t C, int64_t hidden,
                                int64_t D, int64_t H, int64_t W, int precision, void* stream) {
  // ---- the stage: which of the three launches run.  Bit 4: training -- the staged path even
  // where a fused back half exists, so the workspace keeps h1 = GELU(LN1(pwconv)) and h2 =
  // dwconv (pre-LN2) for the backward
  const bool train = (stage & 16) != 0;
  const int which = stage & ~16;
  WF_REQUIRE(which >= 0 && which <= 3, "stage must be 0 (all), 1 (pwconv), 2 (dwconv) or 3 (fc)");
  const bool run_pw = which == 0 || which == 1, run_dw = which == 0 || which == 2,
             run_fc = which == 0 || which == 3;
  // ---- validate, and plan
  FfnPlan plan;
  if (const char* why = ffn_plan_call(B, C, hidden, D, H, W, precision, train, plan))
    return fail(WF_E_SHAPE, std::string(__func__) + ": " + why);
  WF_REQUIRE_PTR(xh);
  WF_REQUIRE_PTR(pw_bf16x2);
  WF_REQUIRE_PTR(ln1_w);
  WF_REQUIRE_PTR(ln1_b);
  WF_REQUIRE_PTR(dw_w);
  WF_REQUIRE_PTR(dw_b);
  WF_REQUIRE_PTR(ln2_w);
  WF_REQUIRE_PTR(ln2_b);
  WF_REQUIRE_PTR(fc_bf16x2);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE_PTR(workspace);
  if (stats) {
    WF_REQUIRE_PTR(n2_w);
    WF_REQUIRE_PTR(n2_b);
  }
  // ---- workspace
  hipStream_t s = (hipStream_t)stream;
  const int64_t M = B * D * H * W;
  const FfnWorkspace ws = ffn_workspace(M, C, hidden, precision);
  char* base = reinterpret_cast<char*>(workspace);
  void* h1 = base + ws.h1;
  void* h2 = base + ws.h2;
  float* ln2_pst = reinterpret_cast<float*>(base + ws.ln2_pst);
  float* ln1_pst = reinterpret_cast<float*>(base + ws.ln1_pst);
  float* ln1_st = reinterpret_cast<float*>(base + ws.ln1_st);
  GemmArgs pw = pwconv_gemm_args(xh, stats, n2_w, n2_b, pw_bf16x2, pw_b, ln1_w, ln1_b, eps1, h1, M,
                                 C, hidden, precision);
  // ---- front: pwconv + LN1 + GELU
  int rc = 0;
  if (run_pw && plan.front != FFN_FRONT_NONE) {
    if (plan.front != FFN_FRONT_EPILOGUE) pw.epi = EPI_STORE;
    if (plan.front == FFN_FRONT_PARTIALS) pw.o_pstats = ln1_pst;
    rc = launch_gemm(pw, s, "wf_ccf_ffn_fwd(pwconv)");
    if (!rc && plan.front == FFN_FRONT_PASS)
      rc = wf_ln_act_fwd(reinterpret_cast<const float*>(h1), ln1_w, ln1_b, eps1, 1,
                         reinterpret_cast<float*>(h1), M, hidden, stream);
    if (!rc && plan.front == FFN_FRONT_PARTIALS)
      rc = launch_ln_stats_finalize(ln1_pst, plan.ln1_np, (int)(hidden / plan.ln1_np), eps1,
                                    ln1_st, M, s);
  }
  if (rc) return rc;
  // ---- back, one kernel: dwconv + LN2 + GELU + fc + residual is the dwconv stage, the fc stage
  // is part of it (and so is the pwconv stage of the whole-FFN kernel)
  if (ffn_back_fused(plan.back)) {
    if (!run_dw) return 0;
    DwFcArgs d = dwfc_args(plan.back == FFN_BACK_FUSED ? nullptr : h1, dw_w, dw_b, ln2_w, ln2_b, eps2,
                           fc_bf16x2, fc_b, xh, stats, n2_w, n2_b, branch_scale, out, B, D, H, W);
    switch (plan.back) {
      case FFN_BACK_FUSED:
        d.pw = pw_bf16x2;
        d.pw_b = pw_b;
        d.ln1_w = ln1_w;
        d.ln1_b = ln1_b;
        d.eps1 = eps1;
        return launch_ffn_fused(d, precision, s);
      case FFN_BACK_DWFC_TB4: return launch_ffn_dwfc_tb4(d, precision, s);
      case FFN_BACK_DWFC_SB: return launch_ffn_dwfc_sb(d, precision, s);
      case FFN_BACK_DWFC2_TB: return launch_ffn_dwfc2(d, precision, true, s);
      case FFN_BACK_DWFC2_KERNEL: return launch_ffn_dwfc2(d, precision, false, s);
      default:  // FFN_BACK_DWFC3_TB
        d.fcs = reinterpret_cast<uint16_t*>(base + ws.fcs);
        return launch_ffn_dwfc3(d, precision, s);
    }
  }
  // ---- back, staged: the depthwise conv into h2, then the fc GEMM
  const bool ln2_loader = plan.back == FFN_BACK_STAGED;
  if (run_dw) {
    if (ln2_loader)  // LN1 + GELU in the staging where the front left them to it
      rc = launch_dwconv3d(h1, dw_w, dw_b, h2, ln2_pst, (int)B, (int)hidden, (int)D, (int)H, (int)W,
                           precision, s, nullptr,
                           plan.front == FFN_FRONT_PARTIALS ? ln1_st : nullptr, ln1_w, ln1_b);
    else
      rc = launch_dwconv_ln_gelu(h1, dw_w, dw_b, ln2_w, ln2_b, eps2, h2, (int)B, (int)hidden,
                                 (int)D, (int)H, (int)W, precision, s);
  }
  if (rc || !run_fc) return rc;
  GemmArgs f = fc_gemm_args(h2, ln2_loader ? ln2_pst : nullptr, ln2_w, ln2_b, eps2, fc_bf16x2, fc_b,
                            xh, stats, n2_w, n2_b, branch_scale, out, M, C, hidden, D * H * W,
                            precision);
  if (!train) {  // h1 is dead once the depthwise conv has read it: the fc's split-K scratch
    f.kpart = reinterpret_cast<float*>(h1);
    f.kpart_bytes = ws.h2 - ws.h1;
  }
  return launch_gemm(f, s, "wf_ccf_ffn_fwd(fc)");
}

extern "C" int wf_ccf_ffn_fwd(const float* xh, const float* stats, const float* n2_w,
                              const float* n2_b, const uint16_t* pw_bf16x2, const float* pw_b,
                              const float* ln1_w, const float* ln1_b, float eps1,
                              const float* dw_w, const float* dw_b, const float* ln2_w,
                              const float* ln2_b, float eps2, const uint16_t* fc_bf16x2,
                              const float* fc_b, const float* branch_scale, float* out,
                              void* workspace, int64_t B, int64_t C, int64_t hidden, int64_t D,
                              int64_t H, int64_t W, int precision, void* stream) {
  return wf_ccf_ffn_stage(0, xh, stats, n2_w, n2_b, pw_bf16x2, pw_b, ln1_w, ln1_b, eps1, dw_w,
                          dw_b, ln2_w, ln2_b, eps2, fc_bf16x2, fc_b, branch_scale, out,
                          workspace, B, C, hidden, D, H, W, precision, stream);
}

extern "C" int wf_patch_merging_fwd(const float* x, const float* ln_w, const float* ln_b,
                                    float eps, const uint16_t* red_bf16x2, int v2, float* out,
                                    int64_t B, int64_t C, int64_t D, int64_t H, int64_t W,
                                    int precision, void* stream) {
  WF_REQUIRE(B >= 1 && C % 8 == 0 && C >= 8, "C must be a positive multiple of 8");
  WF_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0 && D >= 2 && H >= 2 && W >= 2,
             "odd sizes (the F.pad branch, wave_helper.py:180-182) are not supported");
  WF_REQUIRE(valid_prec(precision), "unknown precision");
  WF_REQUIRE_PTR(x);
  WF_REQUIRE_PTR(ln_w);
  WF_REQUIRE_PTR(ln_b);
  WF_REQUIRE_PTR(red_bf16x2);
  WF_REQUIRE_PTR(out);
  GemmArgs g{};
  g.prec = precision;
  g.a_src = x;
  g.a_bf16 = 0;
  g.a_C = (int)C;
  g.a_nseg = 8;
  g.a_map = MAP_MERGE;
  // (d,h,w) offsets of the 8 sub-lattices, one nibble each (bit2 d, bit1 h, bit0 w):
  //   PatchMerging (wave_helper.py:183-190, quirk Q3): 000,100,010,001,101,010,001,111
  //   PatchMergingV2 (itertools.product, :154-156):     000,001,010,011,100,101,110,111
  g.merge_code = v2 ? 0x76543210 : 0x71251240;
  g.mB = (int)B;
  g.mD = (int)D;
  g.mH = (int)H;
  g.mW = (int)W;
  g.a_ln = LN_COMPUTE;
  g.a_ln_w = ln_w;
  g.a_ln_b = ln_b;
  g.a_eps = eps;
  g.w = red_bf16x2;
  g.M = B * (D / 2) * (H / 2) * (W / 2);
  g.N = (int)(2 * C);
  g.K = (int)(8 * C);
  g.epi = EPI_STORE;
  g.bias = nullptr;
  g.out = out;
  g.out_bf16 = 0;
  g.ldo = 2 * C;
  if (try_launch_merge_resident(g, (hipStream_t)stream)) return check_launch("wf_patch_merging_fwd");
  return launch_gemm(g, (hipStream_t)stream, "wf_patch_merging_fwd");
}
