// hfref.hip -- HFRefinementRes (idwt_upsample.py:12-50) over the 7 detail tensors of one
// wavelet level, the config-5 branch the decoder applies before the IDWT (:153-156):
//
//     out = x * sigmoid( conv1x1( relu( IN_affine( dwconv3^3(x) + b1 ) ) ) + b2 )
//
// in two streaming passes over channel-last (B, D, H, W, C) fp32 tensors, nothing written in
// between:
//   hf_stats_kernel  depthwise 3^3 conv (zero padding) of each detail tensor, marching down
//                    whole z columns with a 3-plane rolling accumulator (each input plane is
//                    read once per column: 9 neighbour loads, L1/L2-resident), and the
//                    InstanceNorm moments per (detail, sample, channel): fp32 per thread,
//                    fp64 per workgroup, one fp64 atomic per channel and workgroup.
//   hf_apply_kernel  recomputes the conv for a tile of NPOS (y, x) positions x 8 planes,
//                    normalises (mean / rstd from the moments, affine), ReLU -> LDS as
//                    [channel][voxel]; then the C x C 1x1 conv in fp32 FMAs (each thread: 8
//                    voxels x 4 output channels, weights streamed from L1 once per 4 input
//                    channels), bias, sigmoid, times x, one store.
// The 1x1 conv is 2 C^2 flops per voxel (<= 74 KFLOP at C = 192), small against the HBM
// time of the three tensor passes (read x twice, write out once), so it stays exact fp32 on
// the VALU: the branch is HBM-bound.  Thread mapping in both kernels: tid -> (position, 4-
// channel group), NPOS = 256 / (C / 4) positions per workgroup.
#include <algorithm>

#include "kernels.hpp"

namespace wf {

constexpr int HF_ZS = 8;  // planes per apply tile

struct HfArgs {
  const float* x[7];  // detail tensors, channel-last, batch stride ldb
  int64_t ldb;
  float* out;         // (7, B, D, H, W, C)
  const float* dw_w;  // (C, 27)
  const float* dw_b;  // (C)
  const float* in_w;  // InstanceNorm affine weight / bias (C)
  const float* in_b;
  const float* pw_w;  // (C, C) [co][ci]
  const float* pw_b;  // (C)
  double* acc;        // (7, B, C, 2) {sum, sum of squares}
  int B, C, D, H, W;
  int npos, tiles_xy;
  float eps;
  int sigmoid;
};

// the 27 taps of channels [4 cg, 4 cg + 4) from a [27][C] LDS copy of the weights
__device__ __forceinline__ void load_taps(const float* wl, int C, int cg, f32x4 (&w)[27]) {
#pragma unroll
  for (int t = 0; t < 27; ++t) w[t] = *reinterpret_cast<const f32x4*>(wl + t * C + 4 * cg);
}

// stage the (C, 27) depthwise weights transposed to [27][C] in LDS
__device__ __forceinline__ void stage_taps(const float* __restrict__ w, float* wl, int C) {
  for (int i = threadIdx.x; i < 27 * C; i += blockDim.x) {
    const int c = i / 27, t = i - c * 27;
    wl[t * C + c] = w[i];
  }
}

// the 3 x 3 in-plane neighbourhood of (z, y, x), channels [4 cg, +4), zero outside
__device__ __forceinline__ void load_plane(const float* __restrict__ xb, int z, int y, int x,
                                           int cg, const HfArgs& a, f32x4 (&v)[9]) {
  const bool zin = z >= 0 && z < a.D;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = y + dy - 1, xx = x + dx - 1;
      const bool in = zin && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (in)
        t = *reinterpret_cast<const f32x4*>(
            xb + (((int64_t)z * a.H + yy) * a.W + xx) * a.C + 4 * cg);
      v[dy * 3 + dx] = t;
    }
}

// acc += sum over the 9 in-plane taps of depth kz
__device__ __forceinline__ f32x4 taps9(const f32x4 (&v)[9], const f32x4 (&w)[27], int kz,
                                       f32x4 acc) {
#pragma unroll
  for (int i = 0; i < 9; ++i) acc += v[i] * w[kz * 9 + i];
  return acc;
}

__global__ __launch_bounds__(256) void hf_stats_kernel(HfArgs a) {
  __shared__ float wl[27 * 256];
  __shared__ float red[2 * 256 * 4];  // [moment][thread][4]
  const int C = a.C, C4 = C >> 2;
  const int tid = threadIdx.x;
  const int pi = tid / C4, cg = tid - pi * C4;
  const int kb = blockIdx.y;  // detail * B + b
  const int k = kb / a.B, b = kb - k * a.B;
  const int p = blockIdx.x * a.npos + pi;
  const bool act = pi < a.npos && p < a.H * a.W;
  stage_taps(a.dw_w, wl, C);
  __syncthreads();
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
  if (act) {
    f32x4 w[27];
    load_taps(wl, C, cg, w);
    const f32x4 bias = *reinterpret_cast<const f32x4*>(a.dw_b + 4 * cg);
    const float* xb = a.x[k] + (int64_t)b * a.ldb;
    const int y = p / a.W, x = p - y * a.W;
    // rolling accumulators: o0 -> plane z - 1, o1 -> z, o2 -> z + 1 while reading plane z
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
    f32x4 v[9];
    for (int z = 0; z <= a.D; ++z) {
      if (z < a.D) {
        load_plane(xb, z, y, x, cg, a, v);
        o0 = taps9(v, w, 2, o0);
        o1 = taps9(v, w, 1, o1);
        o2 = taps9(v, w, 0, o2);
      }
      if (z >= 1) {  // plane z - 1 is complete
        const f32x4 yv = o0 + bias;
        s += yv;
        q += yv * yv;
      }
      o0 = o1;
      o1 = o2;
      o2 = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  *reinterpret_cast<f32x4*>(red + tid * 4) = s;
  *reinterpret_cast<f32x4*>(red + (256 + tid) * 4) = q;
  __syncthreads();
  for (int i = tid; i < 2 * C; i += blockDim.x) {
    const int c = i >> 1, mom = i & 1;
    const int g = c >> 2, j = c & 3;
    double t = 0;
    for (int r = 0; r < a.npos; ++r) t += (double)red[(mom * 256 + r * C4 + g) * 4 + j];
    atomicAdd(a.acc + ((int64_t)kb * C + c) * 2 + mom, t);
  }
}

__global__ __launch_bounds__(256) void hf_apply_kernel(HfArgs a) {
  extern __shared__ float sm[];
  const int C = a.C, C4 = C >> 2;
  const int NV = a.npos * HF_ZS;
  float* wl = sm;                    // [27][C]
  float* nsc = wl + 27 * C;          // [C] scale
  float* nsh = nsc + C;              // [C] shift
  float* zt = nsh + C;               // [C][NV] normalised, activated conv output
  const int tid = threadIdx.x;
  const int pi = tid / C4, cg = tid - pi * C4;
  const int kb = blockIdx.y;
  const int k = kb / a.B, b = kb - k * a.B;
  const int zseg = blockIdx.x / a.tiles_xy;
  const int tile = blockIdx.x - zseg * a.tiles_xy;
  const int z0 = zseg * HF_ZS;
  const int p = tile * a.npos + pi;
  const int64_t P = (int64_t)a.D * a.H * a.W;
  const bool act = pi < a.npos && p < a.H * a.W;
  stage_taps(a.dw_w, wl, C);
  for (int c = tid; c < C; c += blockDim.x) {
    const double* m = a.acc + ((int64_t)kb * C + c) * 2;
    const double mean = m[0] / (double)P;
    double var = m[1] / (double)P - mean * mean;
    if (var < 0) var = 0;
    const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    const float sc = rstd * a.in_w[c];
    nsc[c] = sc;
    nsh[c] = a.in_b[c] - (float)mean * sc;
  }
  __syncthreads();
  const float* xb = a.x[k] + (int64_t)b * a.ldb;
  const int y = act ? p / a.W : 0, x = act ? p - y * a.W : 0;
  if (pi < a.npos) {
    // rolling accumulators as in hf_stats_kernel; each completed plane is normalised,
    // activated and written to zt at once (zero outside the volume / for idle positions)
    f32x4 w[27];
    f32x4 bias = {0.f, 0.f, 0.f, 0.f}, sc = bias, sh = bias;
    if (act) {
      load_taps(wl, C, cg, w);
      bias = *reinterpret_cast<const f32x4*>(a.dw_b + 4 * cg);
      sc = *reinterpret_cast<const f32x4*>(nsc + 4 * cg);
      sh = *reinterpret_cast<const f32x4*>(nsh + 4 * cg);
    }
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
    f32x4 v[9];
    float* zc = zt + (int64_t)(4 * cg) * NV + pi * HF_ZS;
    for (int i = 0; i < HF_ZS + 2; ++i) {  // input plane z0 - 1 + i
      if (act) {
        load_plane(xb, z0 - 1 + i, y, x, cg, a, v);
        o0 = taps9(v, w, 2, o0);
        o1 = taps9(v, w, 1, o1);
        o2 = taps9(v, w, 0, o2);
      }
      if (i >= 2) {  // output plane j = i - 2 (z0 + j) is complete
        const int j = i - 2;
        f32x4 t = (o0 + bias) * sc + sh;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = fmaxf(t[e], 0.f);
        if (!act || z0 + j >= a.D) t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) zc[e * NV + j] = t[e];
      }
      o0 = o1;
      o1 = o2;
      o2 = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __syncthreads();
  if (!act) return;
  // 1x1 conv: o[j][e] = sum_ci zt[ci][pi * 8 + j] * W[4 cg + e][ci]
  f32x4 o[HF_ZS];
#pragma unroll
  for (int j = 0; j < HF_ZS; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wrow = a.pw_w + (int64_t)(4 * cg) * C;
  for (int c0 = 0; c0 < C; c0 += 4) {
    f32x4 wv[4];  // wv[e] = W[4 cg + e][c0 .. c0 + 4)
#pragma unroll
    for (int e = 0; e < 4; ++e) wv[e] = *reinterpret_cast<const f32x4*>(wrow + e * C + c0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* zr = zt + (int64_t)(c0 + u) * NV + pi * HF_ZS;
      const f32x4 za = *reinterpret_cast<const f32x4*>(zr);
      const f32x4 zb = *reinterpret_cast<const f32x4*>(zr + 4);
      const f32x4 wc = {wv[0][u], wv[1][u], wv[2][u], wv[3][u]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] += za[j] * wc;
        o[4 + j] += zb[j] * wc;
      }
    }
  }
  const f32x4 pb = *reinterpret_cast<const f32x4*>(a.pw_b + 4 * cg);
  float* ob = a.out + ((int64_t)kb * P) * C;
#pragma unroll
  for (int j = 0; j < HF_ZS; ++j) {
    const int z = z0 + j;
    if (z >= a.D) break;
    const int64_t off = (((int64_t)z * a.H + y) * a.W + x) * C + 4 * cg;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xb + off);
    f32x4 g = o[j] + pb;
    if (a.sigmoid) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = 1.f / (1.f + __expf(-g[e]));
    }
    *reinterpret_cast<f32x4*>(ob + off) = xv * g;
  }
}

}  // namespace wf

using namespace wf;

extern "C" int64_t wf_hf_refine_workspace_bytes(int64_t B, int64_t C) {
  return 7 * B * C * 2 * (int64_t)sizeof(double);
}

extern "C" int wf_hf_refine_fwd(const float* const* details, int64_t ldb, const float* dw_w,
                                const float* dw_b, const float* in_w, const float* in_b,
                                float eps, const float* pw_w, const float* pw_b, int sigmoid,
                                float* out, void* workspace, int64_t B, int64_t C, int64_t D,
                                int64_t H, int64_t W, void* stream) {
  WF_REQUIRE(B >= 1 && D >= 1 && H >= 1 && W >= 1, "empty tensor");
  WF_REQUIRE(C >= 4 && C % 4 == 0 && C <= 256, "C must be a multiple of 4 in [4, 256]");
  WF_REQUIRE(ldb >= D * H * W * C, "batch stride smaller than one channel-last sample");
  WF_REQUIRE_PTR(details);
  WF_REQUIRE_PTR(dw_w);
  WF_REQUIRE_PTR(dw_b);
  WF_REQUIRE_PTR(in_w);
  WF_REQUIRE_PTR(in_b);
  WF_REQUIRE_PTR(pw_w);
  WF_REQUIRE_PTR(pw_b);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE_PTR(workspace);
  HfArgs a{};
  for (int i = 0; i < 7; ++i) {
    WF_REQUIRE_PTR(details[i]);
    a.x[i] = details[i];
  }
  a.ldb = ldb;
  a.out = out;
  a.dw_w = dw_w;
  a.dw_b = dw_b;
  a.in_w = in_w;
  a.in_b = in_b;
  a.pw_w = pw_w;
  a.pw_b = pw_b;
  a.acc = reinterpret_cast<double*>(workspace);
  a.B = (int)B;
  a.C = (int)C;
  a.D = (int)D;
  a.H = (int)H;
  a.W = (int)W;
  a.npos = 256 / (int)(C / 4);
  a.tiles_xy = (int)cdiv(H * W, a.npos);
  a.eps = eps;
  a.sigmoid = sigmoid;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a.acc, 0, (size_t)wf_hf_refine_workspace_bytes(B, C), s) != hipSuccess)
    return check_launch("wf_hf_refine_fwd (memset)");
  hipLaunchKernelGGL(hf_stats_kernel, dim3((unsigned)a.tiles_xy, (unsigned)(7 * B)), dim3(256), 0,
                     s, a);
  int rc = check_launch("wf_hf_refine_fwd (stats)");
  if (rc) return rc;
  const int zsegs = (int)cdiv(D, HF_ZS);
  const size_t lds = (size_t)(27 * C + 2 * C + C * a.npos * HF_ZS) * sizeof(float);
  hipLaunchKernelGGL(hf_apply_kernel, dim3((unsigned)(a.tiles_xy * zsegs), (unsigned)(7 * B)),
                     dim3(256), lds, s, a);
  return check_launch("wf_hf_refine_fwd (apply)");
}

// ==========================================================================================
// Backward (training): per detail tensor and sample, P = D H W positions,
//   u = dwconv(x) + b1;  uh = (u - mean) rstd;  a = g uh + b;  h = max(a, 0);
//   v = W2 h + b2;  s = sigmoid(v) (or v);  y = x s
//   gs = gy x;  gv = gs s (1 - s) (or gs);  gh = gv W2;  ga = gh [a > 0]
//   gu = rstd g (ga - mean_P(ga) - uh mean_P(ga uh));  gx = gy s + dwconv^T(gu)
// mean / rstd come from the forward's saved moments.  Kernels, all without atomics (every
// cross-workgroup sum is per-workgroup partials added in index order):
//   hf_bwd_gate_kernel   the apply kernel's tile (NPOS positions x 8 planes, [channel][voxel]
//                        LDS): recomputes the conv, uh and h; the 1x1 conv W2 h, the gate
//                        derivative, gv W2 (both exact fp32 FMAs) down to ga; writes
//                        gx = gy s, and uh, ga, h, gv to the workspace (pass 2 reads the stored
//                        uh instead of recomputing the conv); per-tile partial sums of ga,
//                        ga uh and gv per channel.
//   hf_bwd_sums_kernel   the partials of each (detail, sample, channel) in tile order (fp64):
//                        {sum ga, sum ga uh, sum gv} and the coefficients of gu.
//   hf_bwd_gu_kernel     ga -> gu in place.
//   hf_bwd_dgrad_kernel  gx += dwconv^T(gu): the stats kernel's z march with mirrored taps.
//   hf_bwd_wgrad_kernel  per-workgroup partials of gW1[c][t] = sum_p gu[p] x[p + t], same march.
//   hf_bwd_final_kernel  gW1 from the partials; g_in_w, g_in_b, g_pw_b over the (detail,
//                        sample) sums; g_dw_b = 0 (the InstanceNorm removes the mean of u, so
//                        sum_p gu = 0 exactly; exact zeros are returned).
// gW2 = gv^T h runs on wf_gemm_tn over the 7 B P stored rows.
namespace wf {

struct HfBwdArgs {
  HfArgs f;         // the forward's arguments (f.out unused, f.acc = the saved moments)
  const float* gy;  // (7, B, D, H, W, C)
  float* gx;        // (7, B, D, H, W, C)
  float* uh;        // workspace tensors, (7, B, D, H, W, C) each
  float* ga;        //   ga, then gu in place
  float* hb;
  float* gv;
  float* part1;     // (7 B, nt1, 3, C) {ga, ga uh, gv} per gate tile
  float* stat;      // (7 B, C, 6) {sum ga, sum ga uh, sum gv, rstd g, mean ga, mean ga uh}
  float* partw;     // (7 B tiles_xy, C, 27)
  float* g_dw_w;
  float* g_dw_b;
  float* g_in_w;
  float* g_in_b;
  float* g_pw_b;
  int nt1;          // gate tiles per (detail, sample): tiles_xy * z segments
};

__global__ __launch_bounds__(256) void hf_bwd_gate_kernel(HfBwdArgs g) {
  extern __shared__ float sm[];
  const HfArgs& a = g.f;
  const int C = a.C, C4 = C >> 2;
  const int NV = a.npos * HF_ZS;
  float* wl = sm;            // [27][C]
  float* nsc = wl + 27 * C;  // [C] scale, shift (as hf_apply_kernel), mean, rstd
  float* nsh = nsc + C;
  float* nmu = nsh + C;
  float* nrs = nmu + C;
  float* zt = nrs + C;       // [C][NV]: h, then gv, then the reduction scratch
  const int tid = threadIdx.x;
  const int pi = tid / C4, cg = tid - pi * C4;
  const int kb = blockIdx.y;
  const int k = kb / a.B, b = kb - k * a.B;
  const int zseg = blockIdx.x / a.tiles_xy;
  const int tile = blockIdx.x - zseg * a.tiles_xy;
  const int z0 = zseg * HF_ZS;
  const int p = tile * a.npos + pi;
  const int64_t P = (int64_t)a.D * a.H * a.W;
  const bool act = pi < a.npos && p < a.H * a.W;
  stage_taps(a.dw_w, wl, C);
  for (int c = tid; c < C; c += blockDim.x) {
    const double* m = a.acc + ((int64_t)kb * C + c) * 2;
    const double mean = m[0] / (double)P;
    double var = m[1] / (double)P - mean * mean;
    if (var < 0) var = 0;
    const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    const float sc = rstd * a.in_w[c];
    nsc[c] = sc;
    nsh[c] = a.in_b[c] - (float)mean * sc;
    nmu[c] = (float)mean;
    nrs[c] = rstd;
  }
  __syncthreads();
  const float* xb = a.x[k] + (int64_t)b * a.ldb;
  const int y = act ? p / a.W : 0, x = act ? p - y * a.W : 0;
  const int64_t dense = (int64_t)kb * P * C;  // this (detail, sample) in the dense tensors
  unsigned mask = 0;                          // bit 4 j + e: a > 0 at plane j, channel e
  if (pi < a.npos) {
    f32x4 w[27];
    f32x4 bias = {0.f, 0.f, 0.f, 0.f}, sc = bias, sh = bias, mu = bias, rs = bias;
    if (act) {
      load_taps(wl, C, cg, w);
      bias = *reinterpret_cast<const f32x4*>(a.dw_b + 4 * cg);
      sc = *reinterpret_cast<const f32x4*>(nsc + 4 * cg);
      sh = *reinterpret_cast<const f32x4*>(nsh + 4 * cg);
      mu = *reinterpret_cast<const f32x4*>(nmu + 4 * cg);
      rs = *reinterpret_cast<const f32x4*>(nrs + 4 * cg);
    }
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
    f32x4 v[9];
    float* zc = zt + (int64_t)(4 * cg) * NV + pi * HF_ZS;
    for (int i = 0; i < HF_ZS + 2; ++i) {  // input plane z0 - 1 + i
      if (act) {
        load_plane(xb, z0 - 1 + i, y, x, cg, a, v);
        o0 = taps9(v, w, 2, o0);
        o1 = taps9(v, w, 1, o1);
        o2 = taps9(v, w, 0, o2);
      }
      if (i >= 2) {  // output plane j = i - 2 (z0 + j) is complete
        const int j = i - 2;
        const f32x4 u = o0 + bias;
        f32x4 t = u * sc + sh;
        const bool in = act && z0 + j < a.D;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (in && t[e] > 0.f) mask |= 1u << (4 * j + e);
          t[e] = fmaxf(t[e], 0.f);
        }
        if (!in) t = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) zc[e * NV + j] = t[e];
        if (in) {
          const int64_t off = dense + (((int64_t)(z0 + j) * a.H + y) * a.W + x) * C + 4 * cg;
          *reinterpret_cast<f32x4*>(g.uh + off) = (u - mu) * rs;
          *reinterpret_cast<f32x4*>(g.hb + off) = t;
        }
      }
      o0 = o1;
      o1 = o2;
      o2 = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __syncthreads();
  // 1x1 conv as in hf_apply_kernel: o[j][e] = sum_ci zt[ci][pi * 8 + j] * W[4 cg + e][ci]
  f32x4 o[HF_ZS];
#pragma unroll
  for (int j = 0; j < HF_ZS; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 sgv = {0.f, 0.f, 0.f, 0.f};
  if (act) {
    const float* wrow = a.pw_w + (int64_t)(4 * cg) * C;
    for (int c0 = 0; c0 < C; c0 += 4) {
      f32x4 wv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[e] = *reinterpret_cast<const f32x4*>(wrow + e * C + c0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* zr = zt + (int64_t)(c0 + u) * NV + pi * HF_ZS;
        const f32x4 za = *reinterpret_cast<const f32x4*>(zr);
        const f32x4 zb = *reinterpret_cast<const f32x4*>(zr + 4);
        const f32x4 wc = {wv[0][u], wv[1][u], wv[2][u], wv[3][u]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] += za[j] * wc;
          o[4 + j] += zb[j] * wc;
        }
      }
    }
    // the gate and its derivative: gx = gy s, o[j] <- gv
    const f32x4 pb = *reinterpret_cast<const f32x4*>(a.pw_b + 4 * cg);
#pragma unroll
    for (int j = 0; j < HF_ZS; ++j) {
      const int z = z0 + j;
      if (z >= a.D) {
        o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
      const int64_t sp = (((int64_t)z * a.H + y) * a.W + x) * C + 4 * cg;
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xb + sp);
      const f32x4 gyv = *reinterpret_cast<const f32x4*>(g.gy + dense + sp);
      f32x4 s = o[j] + pb;
      f32x4 gvv = gyv * xv;
      if (a.sigmoid) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[e] = 1.f / (1.f + __expf(-s[e]));
          gvv[e] *= s[e] * (1.f - s[e]);
        }
      }
      *reinterpret_cast<f32x4*>(g.gx + dense + sp) = gyv * s;
      *reinterpret_cast<f32x4*>(g.gv + dense + sp) = gvv;
      o[j] = gvv;
      sgv += gvv;
    }
  }
  __syncthreads();  // every read of h in zt is done
  if (pi < a.npos) {
    float* zc = zt + (int64_t)(4 * cg) * NV + pi * HF_ZS;
#pragma unroll
    for (int j = 0; j < HF_ZS; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) zc[e * NV + j] = o[j][e];
  }
  __syncthreads();
  // gh[j][e] = sum_co gv[co][pi * 8 + j] * W[co][4 cg + e];  ga = gh [a > 0]
  f32x4 sga = {0.f, 0.f, 0.f, 0.f}, sgu = sga;
  if (act) {
#pragma unroll
    for (int j = 0; j < HF_ZS; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wcol = a.pw_w + 4 * cg;
    for (int co = 0; co < C; ++co) {
      const f32x4 wc = *reinterpret_cast<const f32x4*>(wcol + (int64_t)co * C);
      const float* zr = zt + (int64_t)co * NV + pi * HF_ZS;
      const f32x4 za = *reinterpret_cast<const f32x4*>(zr);
      const f32x4 zb = *reinterpret_cast<const f32x4*>(zr + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] += za[j] * wc;
        o[4 + j] += zb[j] * wc;
      }
    }
#pragma unroll
    for (int j = 0; j < HF_ZS; ++j) {
      const int z = z0 + j;
      if (z >= a.D) break;
      const int64_t off = dense + (((int64_t)z * a.H + y) * a.W + x) * C + 4 * cg;
      const f32x4 uh = *reinterpret_cast<const f32x4*>(g.uh + off);
      f32x4 gav = o[j];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!((mask >> (4 * j + e)) & 1u)) gav[e] = 0.f;
      *reinterpret_cast<f32x4*>(g.ga + off) = gav;
      sga += gav;
      sgu += gav * uh;
    }
  }
  __syncthreads();  // every read of gv in zt is done: zt becomes [3][256][4]
  *reinterpret_cast<f32x4*>(zt + tid * 4) = sga;
  *reinterpret_cast<f32x4*>(zt + (256 + tid) * 4) = sgu;
  *reinterpret_cast<f32x4*>(zt + (512 + tid) * 4) = sgv;
  __syncthreads();
  float* dst = g.part1 + ((int64_t)kb * g.nt1 + blockIdx.x) * 3 * C;
  for (int i = tid; i < 3 * C; i += blockDim.x) {
    const int m = i / C, c = i - m * C;
    const int gq = c >> 2, j = c & 3;
    float t = 0.f;
    for (int r = 0; r < a.npos; ++r) t += zt[(m * 256 + r * C4 + gq) * 4 + j];
    dst[i] = t;
  }
}

__global__ __launch_bounds__(256) void hf_bwd_sums_kernel(HfBwdArgs g) {
  const HfArgs& a = g.f;
  const int C = a.C, kb = blockIdx.x;
  const double P = (double)a.D * a.H * a.W;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double s[3] = {0, 0, 0};
    const float* src = g.part1 + (int64_t)kb * g.nt1 * 3 * C + c;
    for (int t = 0; t < g.nt1; ++t)
#pragma unroll
      for (int m = 0; m < 3; ++m) s[m] += (double)src[((int64_t)t * 3 + m) * C];
    const double* mo = a.acc + ((int64_t)kb * C + c) * 2;
    const double mean = mo[0] / P;
    double var = mo[1] / P - mean * mean;
    if (var < 0) var = 0;
    const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    float* st = g.stat + ((int64_t)kb * C + c) * 6;
    st[0] = (float)s[0];
    st[1] = (float)s[1];
    st[2] = (float)s[2];
    st[3] = rstd * a.in_w[c];
    st[4] = (float)(s[0] / P);
    st[5] = (float)(s[1] / P);
  }
}

// gu = rstd g (ga - mean ga - uh mean(ga uh)), in place over ga; n4 = 7 B P C / 4
__global__ __launch_bounds__(256) void hf_bwd_gu_kernel(HfBwdArgs g, int64_t n4) {
  const HfArgs& a = g.f;
  const int C4 = a.C >> 2;
  const int64_t per = (int64_t)a.D * a.H * a.W * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kb = i / per;
    const int cg = (int)(i % C4);
    const float* st = g.stat + (kb * a.C + 4 * cg) * 6;
    const f32x4 gav = *reinterpret_cast<const f32x4*>(g.ga + i * 4);
    const f32x4 uh = *reinterpret_cast<const f32x4*>(g.uh + i * 4);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      r[e] = st[e * 6 + 3] * (gav[e] - st[e * 6 + 4] - uh[e] * st[e * 6 + 5]);
    *reinterpret_cast<f32x4*>(g.ga + i * 4) = r;
  }
}

__global__ __launch_bounds__(256) void hf_bwd_dgrad_kernel(HfBwdArgs g) {
  __shared__ float wl[27 * 256];
  const HfArgs& a = g.f;
  const int C = a.C, C4 = C >> 2;
  const int tid = threadIdx.x;
  const int pi = tid / C4, cg = tid - pi * C4;
  const int kb = blockIdx.y;
  const int p = blockIdx.x * a.npos + pi;
  const bool act = pi < a.npos && p < a.H * a.W;
  // mirrored taps: wl[t][c] = w[c][26 - t], so the forward's march computes the adjoint
  for (int i = tid; i < 27 * C; i += blockDim.x) {
    const int c = i / 27, t = i - c * 27;
    wl[(26 - t) * C + c] = a.dw_w[i];
  }
  __syncthreads();
  if (!act) return;
  f32x4 w[27];
  load_taps(wl, C, cg, w);
  const int64_t P = (int64_t)a.D * a.H * a.W;
  const float* gu = g.ga + (int64_t)kb * P * C;
  float* gx = g.gx + (int64_t)kb * P * C;
  const int y = p / a.W, x = p - y * a.W;
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
  f32x4 v[9];
  for (int z = 0; z <= a.D; ++z) {
    if (z < a.D) {
      load_plane(gu, z, y, x, cg, a, v);
      o0 = taps9(v, w, 2, o0);
      o1 = taps9(v, w, 1, o1);
      o2 = taps9(v, w, 0, o2);
    }
    if (z >= 1) {  // plane z - 1 is complete
      float* dst = gx + (((int64_t)(z - 1) * a.H + y) * a.W + x) * C + 4 * cg;
      *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(dst) + o0;
    }
    o0 = o1;
    o1 = o2;
    o2 = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// gW1[c][kz][ky][kx] = sum_q x[q] gu[q - (kz - 1, ky - 1, kx - 1)]: each thread holds x at
// its (y, x) for planes z - 1, z, z + 1 and meets the 3 x 3 neighbourhood of gu in plane z;
// gu at (y + dy - 1, x + dx - 1) is the (ky, kx) = (2 - dy, 2 - dx) partner of x at (y, x).
__global__ __launch_bounds__(256) void hf_bwd_wgrad_kernel(HfBwdArgs g) {
  __shared__ float red[9 * 256 * 4];  // [tap of one kz][thread][4]
  const HfArgs& a = g.f;
  const int C = a.C, C4 = C >> 2;
  const int tid = threadIdx.x;
  const int pi = tid / C4, cg = tid - pi * C4;
  const int kb = blockIdx.y;
  const int k = kb / a.B, b = kb - k * a.B;
  const int p = blockIdx.x * a.npos + pi;
  const bool act = pi < a.npos && p < a.H * a.W;
  f32x4 acc[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (act) {
    const int64_t P = (int64_t)a.D * a.H * a.W;
    const float* gu = g.ga + (int64_t)kb * P * C;
    const int y = p / a.W, x = p - y * a.W;
    const float* xc = a.x[k] + (int64_t)b * a.ldb + ((int64_t)y * a.W + x) * C + 4 * cg;
    const int64_t zst = (int64_t)a.H * a.W * C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 xm = zero, x0 = *reinterpret_cast<const f32x4*>(xc), xp;
    f32x4 v[9];
    for (int z = 0; z < a.D; ++z) {
      xp = z + 1 < a.D ? *reinterpret_cast<const f32x4*>(xc + (int64_t)(z + 1) * zst) : zero;
      load_plane(gu, z, y, x, cg, a, v);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        acc[8 - i] += xm * v[i];       // kz = 0: x at plane z - 1
        acc[9 + 8 - i] += x0 * v[i];   // kz = 1
        acc[18 + 8 - i] += xp * v[i];  // kz = 2: x at plane z + 1
      }
      xm = x0;
      x0 = xp;
    }
  }
  float* dst = g.partw + ((int64_t)kb * gridDim.x + blockIdx.x) * C * 27;
#pragma unroll
  for (int kz = 0; kz < 3; ++kz) {
#pragma unroll
    for (int i = 0; i < 9; ++i)
      *reinterpret_cast<f32x4*>(red + (i * 256 + tid) * 4) = acc[kz * 9 + i];
    __syncthreads();
    for (int q = tid; q < 9 * C; q += blockDim.x) {
      const int c = q / 9, i = q - c * 9;
      const int gq = c >> 2, j = c & 3;
      float t = 0.f;
      for (int r = 0; r < a.npos; ++r) t += red[(i * 256 + r * C4 + gq) * 4 + j];
      dst[c * 27 + kz * 9 + i] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void hf_bwd_final_kernel(HfBwdArgs g, int nparts) {
  const HfArgs& a = g.f;
  const int C = a.C;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 27 * C) {
    double t = 0;
    for (int n = 0; n < nparts; ++n) t += (double)g.partw[(int64_t)n * 27 * C + i];
    g.g_dw_w[i] = (float)t;
  }
  if (i < C) {
    double s0 = 0, s1 = 0, s2 = 0;
    for (int kb = 0; kb < 7 * a.B; ++kb) {
      const float* st = g.stat + ((int64_t)kb * C + i) * 6;
      s0 += (double)st[0];
      s1 += (double)st[1];
      s2 += (double)st[2];
    }
    g.g_in_b[i] = (float)s0;
    g.g_in_w[i] = (float)s1;
    g.g_pw_b[i] = (float)s2;
    g.g_dw_b[i] = 0.f;
  }
}

// sub-buffer offsets (bytes) of the backward workspace
struct HfBwdLayout {
  int64_t uh, ga, hb, gv, part1, stat, partw, tn, tn_bytes, total;
};

static HfBwdLayout hf_bwd_layout(int64_t B, int64_t C, int64_t D, int64_t H, int64_t W) {
  const int64_t P = D * H * W, M = 7 * B * P;
  const int64_t npos = 256 / (C / 4), tiles_xy = cdiv(H * W, npos), zsegs = cdiv(D, HF_ZS);
  const int64_t fl = (int64_t)sizeof(float);
  HfBwdLayout l{};
  int64_t o = 0;
  l.uh = o, o += align256(M * C * fl);
  l.ga = o, o += align256(M * C * fl);
  l.hb = o, o += align256(M * C * fl);
  l.gv = o, o += align256(M * C * fl);
  l.part1 = o, o += align256(7 * B * tiles_xy * zsegs * 3 * C * fl);
  l.stat = o, o += align256(7 * B * C * 6 * fl);
  l.partw = o, o += align256(7 * B * tiles_xy * C * 27 * fl);
  // wf_gemm_tn deals the M rows to at most min(1024 / tiles, M / 256) chunks of (C, C)
  // partials; this bound (unlike its exact query) grows with M
  const int64_t tiles = cdiv(C, 64) * cdiv(C, 64);
  const int64_t chunks = std::min(std::max<int64_t>(1, 1024 / tiles), cdiv(M, 256));
  l.tn = o, l.tn_bytes = align256(chunks * C * C * fl), o += l.tn_bytes;
  l.total = o;
  return l;
}

}  // namespace wf

extern "C" int64_t wf_hf_refine_bwd_workspace_bytes(int64_t B, int64_t C, int64_t D, int64_t H,
                                                    int64_t W) {
  if (B < 1 || D < 1 || H < 1 || W < 1 || C < 4 || C % 4 || C > 256) return 0;
  return hf_bwd_layout(B, C, D, H, W).total;
}

extern "C" int wf_hf_refine_bwd(const float* const* details, int64_t ldb, const float* dw_w,
                                const float* dw_b, const float* in_w, const float* in_b,
                                float eps, const float* pw_w, const float* pw_b, int sigmoid,
                                const double* moments, const float* gy, float* gx,
                                float* g_dw_w, float* g_dw_b, float* g_in_w, float* g_in_b,
                                float* g_pw_w, float* g_pw_b, void* workspace, int64_t B,
                                int64_t C, int64_t D, int64_t H, int64_t W, void* stream) {
  WF_REQUIRE(B >= 1 && D >= 1 && H >= 1 && W >= 1, "empty tensor");
  WF_REQUIRE(C >= 4 && C % 4 == 0 && C <= 256, "C must be a multiple of 4 in [4, 256]");
  WF_REQUIRE(D < (1 << 20) && H < (1 << 20) && W < (1 << 20) && 7 * B <= 65535 &&
                 D * H * W < ((int64_t)1 << 31) && 7 * B * D * H * W * C < ((int64_t)1 << 40),
             "tensor too large");
  WF_REQUIRE(ldb >= D * H * W * C, "batch stride smaller than one channel-last sample");
  WF_REQUIRE_PTR(details);
  WF_REQUIRE_PTR(dw_w);
  WF_REQUIRE_PTR(dw_b);
  WF_REQUIRE_PTR(in_w);
  WF_REQUIRE_PTR(in_b);
  WF_REQUIRE_PTR(pw_w);
  WF_REQUIRE_PTR(pw_b);
  WF_REQUIRE_PTR(moments);
  WF_REQUIRE_PTR(gy);
  WF_REQUIRE_PTR(gx);
  WF_REQUIRE_PTR(g_dw_w);
  WF_REQUIRE_PTR(g_dw_b);
  WF_REQUIRE_PTR(g_in_w);
  WF_REQUIRE_PTR(g_in_b);
  WF_REQUIRE_PTR(g_pw_w);
  WF_REQUIRE_PTR(g_pw_b);
  WF_REQUIRE_PTR(workspace);
  HfBwdArgs g{};
  HfArgs& a = g.f;
  for (int i = 0; i < 7; ++i) {
    WF_REQUIRE_PTR(details[i]);
    a.x[i] = details[i];
  }
  const int64_t M = 7 * B * D * H * W;
  const HfBwdLayout l = hf_bwd_layout(B, C, D, H, W);
  WF_REQUIRE(wf_gemm_tn_workspace_bytes(M, C, C) <= l.tn_bytes, "GEMM workspace bound");
  a.ldb = ldb;
  a.dw_w = dw_w;
  a.dw_b = dw_b;
  a.in_w = in_w;
  a.in_b = in_b;
  a.pw_w = pw_w;
  a.pw_b = pw_b;
  a.acc = const_cast<double*>(moments);  // read only
  a.B = (int)B;
  a.C = (int)C;
  a.D = (int)D;
  a.H = (int)H;
  a.W = (int)W;
  a.npos = 256 / (int)(C / 4);
  a.tiles_xy = (int)cdiv(H * W, a.npos);
  a.eps = eps;
  a.sigmoid = sigmoid;
  char* ws = static_cast<char*>(workspace);
  g.gy = gy;
  g.gx = gx;
  g.uh = reinterpret_cast<float*>(ws + l.uh);
  g.ga = reinterpret_cast<float*>(ws + l.ga);
  g.hb = reinterpret_cast<float*>(ws + l.hb);
  g.gv = reinterpret_cast<float*>(ws + l.gv);
  g.part1 = reinterpret_cast<float*>(ws + l.part1);
  g.stat = reinterpret_cast<float*>(ws + l.stat);
  g.partw = reinterpret_cast<float*>(ws + l.partw);
  g.g_dw_w = g_dw_w;
  g.g_dw_b = g_dw_b;
  g.g_in_w = g_in_w;
  g.g_in_b = g_in_b;
  g.g_pw_b = g_pw_b;
  const int zsegs = (int)cdiv(D, HF_ZS);
  g.nt1 = a.tiles_xy * zsegs;
  hipStream_t s = (hipStream_t)stream;
  const dim3 cols((unsigned)a.tiles_xy, (unsigned)(7 * B));
  const size_t lds = (size_t)(27 * C + 4 * C + C * a.npos * HF_ZS) * sizeof(float);
  hipLaunchKernelGGL(hf_bwd_gate_kernel, dim3((unsigned)g.nt1, (unsigned)(7 * B)), dim3(256),
                     lds, s, g);
  int rc = check_launch("wf_hf_refine_bwd (gate)");
  if (rc) return rc;
  hipLaunchKernelGGL(hf_bwd_sums_kernel, dim3((unsigned)(7 * B)), dim3(256), 0, s, g);
  if ((rc = check_launch("wf_hf_refine_bwd (sums)"))) return rc;
  const int64_t n4 = M * (C / 4);
  hipLaunchKernelGGL(hf_bwd_gu_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n4, 256), 16384)),
                     dim3(256), 0, s, g, n4);
  if ((rc = check_launch("wf_hf_refine_bwd (gu)"))) return rc;
  hipLaunchKernelGGL(hf_bwd_dgrad_kernel, cols, dim3(256), 0, s, g);
  if ((rc = check_launch("wf_hf_refine_bwd (dgrad)"))) return rc;
  hipLaunchKernelGGL(hf_bwd_wgrad_kernel, cols, dim3(256), 0, s, g);
  if ((rc = check_launch("wf_hf_refine_bwd (wgrad)"))) return rc;
  hipLaunchKernelGGL(hf_bwd_final_kernel, dim3((unsigned)cdiv(27 * C, 256)), dim3(256), 0, s, g,
                     (int)(7 * B * a.tiles_xy));
  if ((rc = check_launch("wf_hf_refine_bwd (final)"))) return rc;
  return wf_gemm_tn(g.gv, C, g.hb, C, g_pw_w, C, 0, ws + l.tn, M, C, C, stream);
}
