// wavelet.hip -- general orthogonal-wavelet 3D analysis / synthesis (ptwt 'zero' mode) for
// gfx950: db1..db4 (filter length L = 2, 4, 6, 8), any sizes (odd included), NCDHW planes.
//
// Reference arithmetic: ptwt 0.1.9 wavedec3 / waverec3 (call sites
// network_models/wave_helper.py:350 and network_models/idwt_upsample.py:160) with a wavelet
// other than 'db1' -- BASELINE config 5 ("db2 3-level DWT + HF refinement").  ptwt follows
// PyWavelets' MODE_ZERO conventions (pinned by tests/golden/pywt_dwt3.npz):
//   analysis,  per axis:  out[n] = sum_j dec[L-1-j] * x[2n + j - (L-2)],  n < (N + L - 1) / 2
//   synthesis, per axis:  y[t]   = sum_j rec[j] * c[(t - j) / 2]  over j == t (mod 2),
//                         kept for t in [L-2, 2n), i.e. 2n - L + 2 outputs,
// x and c zero outside their range.  The Haar encoder path keeps its fused channel-last
// kernels (dwt.hip); these kernels serve the NCDHW per-op API for longer filters.
//
// Both kernels stream along z: a workgroup owns a (TY x TX) output tile of one (b, c) plane
// and a chunk of output z-planes.  Each input z-plane is read once from HBM into LDS (with
// the filter halo), filtered along x then y in LDS, and parked in a ring of the last L
// (analysis) or L/2 (synthesis) filtered planes; every output plane is then one L-tap
// (resp. L/2-tap) combination of ring slots, written as contiguous TX-float rows.  HBM
// traffic is one read of the input (plus the y/x halo, served from L2 by the neighbouring
// tiles) and one write of the output: the HBM roofline bounds both.
//
// The backward entries run the same two kernels: the adjoint of an analysis
// level is the synthesis form with the taps dec[L-1-j] and an output extent that may be one
// sample short of 2n - L + 2 per axis (wf_dwt3d_bwd -> idwt3d_gen_kernel); the adjoint of a
// synthesis level is the analysis form with the taps rec[j] over the output gradient
// (wf_idwt3d_level_bwd -> dwt3d_gen_fwd_kernel, strided input, one strided output per band).
#include "wf_common.hpp"

namespace wf {

constexpr int kWaveMaxTaps = 8;

struct WaveFwdArgs {
  const float* x;       // element (b, ch, z, y, x) at b*xs0 + ch*xs1 + (z*H + y)*W + x
  int64_t xs0, xs1;
  float* out[8];        // band k bits (z, y, x) = (k>>2, k>>1 & 1, k & 1); element
  int64_t os[8][5];     //   (b, ch, z, y, x) at out[k][b*os0 + ch*os1 + z*os2 + y*os3 + x*os4]
  int64_t C;            // channels per batch entry (plane p = b*C + ch)
  int D, H, W, d, h, w;
  int ez, ey, ex;       // band 0 is (d+ez, h+ey, w+ex): the samples past (d, h, w) get 0
  int zc;               // output z-planes per workgroup
  int tiles_y, tiles_x;
  float ka[kWaveMaxTaps], kd[kWaveMaxTaps];  // out[n] = sum_j k[j] x[2n + j - (L-2)]
};

// STRIDED = false: one batch entry of C planes and the contiguous (8, C, d, h, w) band buffer
// of wf_dwt3d_fwd (ez = ey = ex = 0), addressed with one offset for the 8 bands
template <int L, bool STRIDED>
__global__ __launch_bounds__(256) void dwt3d_gen_fwd_kernel(WaveFwdArgs a) {
  constexpr int TY = 8, TX = 32, PAD = L - 2;
  constexpr int IY = 2 * TY + L - 2, IX = 2 * TX + L - 2;
  __shared__ float s_in[IY][IX + 1];
  __shared__ float s_x[2][IY][TX + 1];
  __shared__ float s_ring[L][4][TY][TX + 1];
  const int tid = threadIdx.x;

  int64_t t = blockIdx.x;
  const int tx = (int)(t % a.tiles_x);
  t /= a.tiles_x;
  const int ty = (int)(t % a.tiles_y);
  const int64_t p = t / a.tiles_y;
  const int y0 = ty * TY, x0 = tx * TX;
  const int64_t b = STRIDED ? p / a.C : 0, ch = p - b * a.C;
  const int z0 = blockIdx.y * a.zc;
  const int z1 = min(a.d + a.ez, z0 + a.zc);
  const float* xp = a.x + b * a.xs0 + ch * a.xs1;
  const int64_t band_stride = a.C * a.os[0][1];  // !STRIDED
  float* bp = a.out[0] + p * a.os[0][1];

  float ka[L], kd[L];
#pragma unroll
  for (int j = 0; j < L; ++j) { ka[j] = a.ka[j]; kd[j] = a.kd[j]; }

  const int zs = 2 * z0 - PAD, ze = 2 * (z1 - 1) - PAD + L - 1;
  for (int zi = zs; zi <= ze; ++zi) {
    const bool zin = zi >= 0 && zi < a.D;
    const float* plane = xp + (int64_t)zi * a.H * a.W;
    for (int i = tid; i < IY * IX; i += 256) {
      const int iy = i / IX, ix = i - iy * IX;
      const int gy = 2 * y0 - PAD + iy, gx = 2 * x0 - PAD + ix;
      float v = 0.f;
      if (zin && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = plane[(int64_t)gy * a.W + gx];
      s_in[iy][ix] = v;
    }
    __syncthreads();
    for (int i = tid; i < IY * TX; i += 256) {
      const int iy = i / TX, ox = i - iy * TX;
      float lo = 0.f, hi = 0.f;
#pragma unroll
      for (int j = 0; j < L; ++j) {
        const float v = s_in[iy][2 * ox + j];
        lo = fmaf(ka[j], v, lo);
        hi = fmaf(kd[j], v, hi);
      }
      s_x[0][iy][ox] = lo;
      s_x[1][iy][ox] = hi;
    }
    __syncthreads();
    const int r = zi - zs;
    const int slot = r % L;
    for (int i = tid; i < TY * TX; i += 256) {
      const int oy = i / TX, ox = i - oy * TX;
#pragma unroll
      for (int xb = 0; xb < 2; ++xb) {
        float lo = 0.f, hi = 0.f;
#pragma unroll
        for (int j = 0; j < L; ++j) {
          const float v = s_x[xb][2 * oy + j][ox];
          lo = fmaf(ka[j], v, lo);
          hi = fmaf(kd[j], v, hi);
        }
        s_ring[slot][xb][oy][ox] = lo;       // y low
        s_ring[slot][2 | xb][oy][ox] = hi;   // y high
      }
    }
    __syncthreads();
    // output plane z' is complete once its last input plane r = 2 (z' - z0) + L - 1 is in
    if (r >= L - 1 && ((r - (L - 1)) & 1) == 0) {
      const int oz = z0 + ((r - (L - 1)) >> 1);
      const int rb = r - (L - 1);  // ring position of tap j is (rb + j) % L
      for (int i = tid; i < TY * TX; i += 256) {
        const int oy = i / TX, ox = i - oy * TX;
        const int gy = y0 + oy, gx = x0 + ox;
        if (gy >= a.h + a.ey || gx >= a.w + a.ex) continue;
        // inside the 7 details' extent; outside it only band 0 has a sample, and it is 0
        const bool det = oz < a.d && gy < a.h && gx < a.w;
        const int64_t off = ((int64_t)oz * a.h + gy) * a.w + gx;  // !STRIDED
#pragma unroll
        for (int yx = 0; yx < 4; ++yx) {
          float lo = 0.f, hi = 0.f;
#pragma unroll
          for (int j = 0; j < L; ++j) {
            const float v = s_ring[(rb + j) % L][yx][oy][ox];
            lo = fmaf(ka[j], v, lo);
            hi = fmaf(kd[j], v, hi);
          }
          if (!STRIDED) {
            bp[(int64_t)yx * band_stride + off] = lo;
            bp[(int64_t)(4 | yx) * band_stride + off] = hi;
            continue;
          }
          if (yx == 0) lo = det ? lo : 0.f;
          if (yx == 0 || det)
            a.out[yx][b * a.os[yx][0] + ch * a.os[yx][1] + oz * a.os[yx][2] +
                      gy * a.os[yx][3] + gx * a.os[yx][4]] = lo;
          if (det)
            a.out[4 | yx][b * a.os[4 | yx][0] + ch * a.os[4 | yx][1] + oz * a.os[4 | yx][2] +
                          gy * a.os[4 | yx][3] + gx * a.os[4 | yx][4]] = hi;
        }
      }
    }
    // the next load writes s_in only; the ring slot this plane's taps read is rewritten
    // after two more barriers
  }
}

// ---------------------------------------------------------------------------------------
// synthesis, one level
// ---------------------------------------------------------------------------------------
struct WaveInvArgs {
  const float* c[8];      // band k = (z, y, x) bits as above; element (b, ch, z, y, x) at
  int64_t cs[8][5];       //   c[k][b*cs0 + ch*cs1 + z*cs2 + y*cs3 + x*cs4]
  float* out;             // element (b, ch, z, y, x) at b*os0 + ch*os1 + (z*Ho + y)*Wo + x
  int64_t os0, os1;
  int C, n_z, n_y, n_x, Oz, Oy, Ox;
  int zc;                 // output z-planes per workgroup (even)
  int tiles_y, tiles_x;
  float rlo[kWaveMaxTaps], rhi[kWaveMaxTaps];
};

template <int L>
__global__ __launch_bounds__(256) void idwt3d_gen_kernel(WaveInvArgs a) {
  constexpr int TY = 16, TX = 64, H2 = L / 2;
  constexpr int CY = TY / 2 + H2 - 1, CX = TX / 2 + H2 - 1;
  __shared__ float s_c[8][CY][CX + 1];
  __shared__ float s_x[4][CY][TX + 1];       // (z band, y band) after the x synthesis
  __shared__ float s_ring[H2][2][TY][TX + 1];  // z band, after the y synthesis
  const int tid = threadIdx.x;

  int64_t t = blockIdx.x;
  const int tx = (int)(t % a.tiles_x);
  t /= a.tiles_x;
  const int ty = (int)(t % a.tiles_y);
  const int64_t p = t / a.tiles_y;
  const int b = (int)(p / a.C), ch = (int)(p - (int64_t)b * a.C);
  const int y0 = ty * TY, x0 = tx * TX;
  const int cy0 = y0 / 2, cx0 = x0 / 2;
  const int z0 = blockIdx.y * a.zc;
  const int z1 = min(a.Oz, z0 + a.zc);
  float* op = a.out + b * a.os0 + ch * a.os1;

  float rl[L], rh[L];
#pragma unroll
  for (int j = 0; j < L; ++j) { rl[j] = a.rlo[j]; rh[j] = a.rhi[j]; }

  const int ns = z0 / 2, ne = (z1 - 1 + L - 2) >> 1;
  for (int n = ns; n <= ne; ++n) {
    const bool zin = n < a.n_z;
    for (int i = tid; i < 8 * CY * CX; i += 256) {
      const int k = i / (CY * CX);
      const int rem = i - k * CY * CX;
      const int iy = rem / CX, ix = rem - iy * CX;
      const int gy = cy0 + iy, gx = cx0 + ix;
      float v = 0.f;
      if (zin && gy < a.n_y && gx < a.n_x)
        v = a.c[k][b * a.cs[k][0] + ch * a.cs[k][1] + n * a.cs[k][2] + gy * a.cs[k][3] +
                   gx * a.cs[k][4]];
      s_c[k][iy][ix] = v;
    }
    __syncthreads();
    // x synthesis: (zb, yb) pairs combine bands (zb yb 0) and (zb yb 1)
    for (int i = tid; i < 4 * CY * TX; i += 256) {
      const int zy = i / (CY * TX);
      const int rem = i - zy * CY * TX;
      const int iy = rem / TX, lx = rem - iy * TX;
      const int par = lx & 1, base = (lx >> 1) + H2 - 1;
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < H2; ++q) {
        v = fmaf(rl[2 * q + par], s_c[2 * zy][iy][base - q], v);
        v = fmaf(rh[2 * q + par], s_c[2 * zy + 1][iy][base - q], v);
      }
      s_x[zy][iy][lx] = v;
    }
    __syncthreads();
    const int slot = (n - ns) % H2;
    for (int i = tid; i < 2 * TY * TX; i += 256) {
      const int zb = i / (TY * TX);
      const int rem = i - zb * TY * TX;
      const int ly = rem / TX, lx = rem - ly * TX;
      const int par = ly & 1, base = (ly >> 1) + H2 - 1;
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < H2; ++q) {
        v = fmaf(rl[2 * q + par], s_x[2 * zb][base - q][lx], v);
        v = fmaf(rh[2 * q + par], s_x[2 * zb + 1][base - q][lx], v);
      }
      s_ring[slot][zb][ly][lx] = v;
    }
    __syncthreads();
    // full-length indices 2n and 2n+1 are complete: output plane oz = t - (L - 2)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int oz = 2 * n + par - (L - 2);
      if (oz < z0 || oz >= z1) continue;
      for (int i = tid; i < TY * TX; i += 256) {
        const int ly = i / TX, lx = i - ly * TX;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= a.Oy || gx >= a.Ox) continue;
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < H2; ++q) {
          const int s = ((n - q - ns) % H2 + H2) % H2;
          v = fmaf(rl[2 * q + par], s_ring[s][0][ly][lx], v);
          v = fmaf(rh[2 * q + par], s_ring[s][1][ly][lx], v);
        }
        op[((int64_t)oz * a.Oy + gy) * a.Ox + gx] = v;
      }
    }
  }
}

}  // namespace wf

using namespace wf;

namespace {
int pick_zchunk(int64_t tiles, int planes, int multiple) {
  // enough workgroups to cover 256 CUs several times, but long z runs (the L-2 halo planes
  // are re-read per chunk)
  int zc = planes;
  while (zc > 8 && tiles * cdiv(planes, zc) < 2048) zc = (zc + 1) / 2;
  if (multiple > 1) zc = (int)cdiv(zc, multiple) * multiple;
  return zc;
}

#define WF_REQUIRE_TAPS(taps)                                      \
  WF_REQUIRE((taps) == 2 || (taps) == 4 || (taps) == 6 || (taps) == 8, \
             "filter length must be 2, 4, 6 or 8 (db1..db4)")

// dwt3d_gen_fwd_kernel<taps> over P planes of `a` (pointers, strides, extents and taps set)
template <bool STRIDED>
int launch_analysis(WaveFwdArgs& a, int64_t P, int taps, void* stream, const char* what) {
  const int dz = a.d + a.ez;
  a.tiles_y = (int)cdiv(a.h + a.ey, 8);
  a.tiles_x = (int)cdiv(a.w + a.ex, 32);
  const int64_t tiles = P * a.tiles_y * a.tiles_x;
  if (tiles >= ((int64_t)1 << 31)) return fail(WF_E_SHAPE, std::string(what) + ": too many tiles");
  a.zc = pick_zchunk(tiles, dz, 1);
  dim3 grid((unsigned)tiles, (unsigned)cdiv(dz, a.zc));
  hipStream_t s = (hipStream_t)stream;
  switch (taps) {
    case 2: hipLaunchKernelGGL((dwt3d_gen_fwd_kernel<2, STRIDED>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((dwt3d_gen_fwd_kernel<4, STRIDED>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((dwt3d_gen_fwd_kernel<6, STRIDED>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((dwt3d_gen_fwd_kernel<8, STRIDED>), grid, dim3(256), 0, s, a); break;
  }
  return check_launch(what);
}

// idwt3d_gen_kernel<taps> over P planes of `a`; (Oz, Oy, Ox) <= 2n - taps + 2 per axis
int launch_synthesis(WaveInvArgs& a, int64_t P, int taps, void* stream, const char* what) {
  a.tiles_y = (int)cdiv(a.Oy, 16);
  a.tiles_x = (int)cdiv(a.Ox, 64);
  const int64_t tiles = P * a.tiles_y * a.tiles_x;
  if (tiles >= ((int64_t)1 << 31)) return fail(WF_E_SHAPE, std::string(what) + ": too many tiles");
  a.zc = pick_zchunk(tiles, a.Oz, 2);
  dim3 grid((unsigned)tiles, (unsigned)cdiv(a.Oz, a.zc));
  hipStream_t s = (hipStream_t)stream;
  switch (taps) {
    case 2: hipLaunchKernelGGL(idwt3d_gen_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL(idwt3d_gen_kernel<4>, grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL(idwt3d_gen_kernel<6>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(idwt3d_gen_kernel<8>, grid, dim3(256), 0, s, a); break;
  }
  return check_launch(what);
}
}  // namespace

extern "C" int wf_dwt3d_fwd(const float* x, float* bands, int64_t P, int64_t D, int64_t H,
                            int64_t W, const float* dec_lo, const float* dec_hi, int taps,
                            void* stream) {
  WF_REQUIRE_TAPS(taps);
  WF_REQUIRE(P >= 1 && D >= 1 && H >= 1 && W >= 1, "empty tensor");
  WF_REQUIRE(P * D * H * W < ((int64_t)1 << 40) && D < (1 << 20) && H < (1 << 20) &&
             W < (1 << 20), "tensor too large");
  WF_REQUIRE_PTR(x);
  WF_REQUIRE_PTR(bands);
  WF_REQUIRE_PTR(dec_lo);
  WF_REQUIRE_PTR(dec_hi);
  WaveFwdArgs a{};
  a.x = x;
  a.xs0 = 0;  // one batch entry of P channels
  a.xs1 = D * H * W;
  a.C = P;
  a.D = (int)D; a.H = (int)H; a.W = (int)W;
  a.d = (int)((D + taps - 1) / 2);
  a.h = (int)((H + taps - 1) / 2);
  a.w = (int)((W + taps - 1) / 2);
  const int64_t plane = (int64_t)a.d * a.h * a.w;
  for (int k = 0; k < 8; ++k) {
    a.out[k] = bands + k * P * plane;
    a.os[k][0] = 0;
    a.os[k][1] = plane;
    a.os[k][2] = (int64_t)a.h * a.w;
    a.os[k][3] = a.w;
    a.os[k][4] = 1;
  }
  for (int j = 0; j < taps; ++j) {
    a.ka[j] = dec_lo[taps - 1 - j];
    a.kd[j] = dec_hi[taps - 1 - j];
  }
  return launch_analysis<false>(a, P, taps, stream, "wf_dwt3d_fwd");
}

extern "C" int wf_dwt3d_bwd(const float* gbands, float* dx, int64_t P, int64_t D, int64_t H,
                            int64_t W, const float* dec_lo, const float* dec_hi, int taps,
                            void* stream) {
  WF_REQUIRE_TAPS(taps);
  WF_REQUIRE(P >= 1 && D >= 1 && H >= 1 && W >= 1, "empty tensor");
  WF_REQUIRE(P * D * H * W < ((int64_t)1 << 40) && D < (1 << 20) && H < (1 << 20) &&
             W < (1 << 20), "tensor too large");
  WF_REQUIRE_PTR(gbands);
  WF_REQUIRE_PTR(dx);
  WF_REQUIRE_PTR(dec_lo);
  WF_REQUIRE_PTR(dec_hi);
  // the synthesis form over the band gradients with k[j] = dec[L-1-j], kept for o < (D, H, W):
  // n = (N + taps - 1) / 2 gives 2n - taps + 2 = N (N even) or N + 1 (N odd) full outputs
  WaveInvArgs a{};
  a.n_z = (int)((D + taps - 1) / 2);
  a.n_y = (int)((H + taps - 1) / 2);
  a.n_x = (int)((W + taps - 1) / 2);
  const int64_t plane = (int64_t)a.n_z * a.n_y * a.n_x;
  for (int k = 0; k < 8; ++k) {
    a.c[k] = gbands + k * P * plane;
    a.cs[k][0] = 0;
    a.cs[k][1] = plane;
    a.cs[k][2] = (int64_t)a.n_y * a.n_x;
    a.cs[k][3] = a.n_x;
    a.cs[k][4] = 1;
  }
  for (int j = 0; j < taps; ++j) {
    a.rlo[j] = dec_lo[taps - 1 - j];
    a.rhi[j] = dec_hi[taps - 1 - j];
  }
  a.out = dx;
  a.os0 = 0;
  a.os1 = D * H * W;
  WF_REQUIRE(P < ((int64_t)1 << 31), "too many planes");
  a.C = (int)P;
  a.Oz = (int)D; a.Oy = (int)H; a.Ox = (int)W;
  return launch_synthesis(a, P, taps, stream, "wf_dwt3d_bwd");
}

extern "C" int wf_idwt3d_level(const float* const* coef, const int64_t* coef_strides,
                               int64_t B, int64_t C, int64_t n_z, int64_t n_y, int64_t n_x,
                               const float* rec_lo, const float* rec_hi, int taps, float* out,
                               int64_t out_bstride, int64_t out_cstride, void* stream) {
  WF_REQUIRE_TAPS(taps);
  WF_REQUIRE(B >= 1 && C >= 1 && n_z >= 1 && n_y >= 1 && n_x >= 1, "empty tensor");
  const int64_t Oz = 2 * n_z - taps + 2, Oy = 2 * n_y - taps + 2, Ox = 2 * n_x - taps + 2;
  WF_REQUIRE(Oz >= 1 && Oy >= 1 && Ox >= 1, "coefficients shorter than the filter");
  WF_REQUIRE(n_z < (1 << 20) && n_y < (1 << 20) && n_x < (1 << 20), "tensor too large");
  WF_REQUIRE_PTR(coef);
  WF_REQUIRE_PTR(coef_strides);
  WF_REQUIRE_PTR(rec_lo);
  WF_REQUIRE_PTR(rec_hi);
  WF_REQUIRE_PTR(out);
  WaveInvArgs a{};
  for (int k = 0; k < 8; ++k) {
    WF_REQUIRE_PTR(coef[k]);
    a.c[k] = coef[k];
    for (int i = 0; i < 5; ++i) a.cs[k][i] = coef_strides[5 * k + i];
  }
  for (int j = 0; j < taps; ++j) {
    a.rlo[j] = rec_lo[j];
    a.rhi[j] = rec_hi[j];
  }
  a.out = out;
  a.os0 = out_bstride;
  a.os1 = out_cstride;
  a.C = (int)C;
  a.n_z = (int)n_z; a.n_y = (int)n_y; a.n_x = (int)n_x;
  a.Oz = (int)Oz; a.Oy = (int)Oy; a.Ox = (int)Ox;
  return launch_synthesis(a, B * C, taps, stream, "wf_idwt3d_level");
}

extern "C" int wf_idwt3d_level_bwd(const float* gout, int64_t gout_bstride, int64_t gout_cstride,
                                   int64_t B, int64_t C, int64_t n_z, int64_t n_y, int64_t n_x,
                                   int extra_z, int extra_y, int extra_x, const float* rec_lo,
                                   const float* rec_hi, int taps, float* const* gcoef,
                                   const int64_t* gcoef_strides, void* stream) {
  WF_REQUIRE_TAPS(taps);
  WF_REQUIRE(B >= 1 && C >= 1 && n_z >= 1 && n_y >= 1 && n_x >= 1, "empty tensor");
  const int64_t Oz = 2 * n_z - taps + 2, Oy = 2 * n_y - taps + 2, Ox = 2 * n_x - taps + 2;
  WF_REQUIRE(Oz >= 1 && Oy >= 1 && Ox >= 1, "coefficients shorter than the filter");
  WF_REQUIRE(n_z < (1 << 20) && n_y < (1 << 20) && n_x < (1 << 20) && C < ((int64_t)1 << 31),
             "tensor too large");
  WF_REQUIRE((extra_z == 0 || extra_z == 1) && (extra_y == 0 || extra_y == 1) &&
             (extra_x == 0 || extra_x == 1), "the LL is at most one sample longer per axis");
  WF_REQUIRE_PTR(gout);
  WF_REQUIRE_PTR(rec_lo);
  WF_REQUIRE_PTR(rec_hi);
  WF_REQUIRE_PTR(gcoef);
  WF_REQUIRE_PTR(gcoef_strides);
  // the analysis form over the output gradient with k[j] = rec[j]; (O + taps - 1) / 2 = n
  WaveFwdArgs a{};
  a.x = gout;
  a.xs0 = gout_bstride;
  a.xs1 = gout_cstride;
  a.C = C;
  a.D = (int)Oz; a.H = (int)Oy; a.W = (int)Ox;
  a.d = (int)n_z; a.h = (int)n_y; a.w = (int)n_x;
  a.ez = extra_z; a.ey = extra_y; a.ex = extra_x;
  for (int k = 0; k < 8; ++k) {
    WF_REQUIRE_PTR(gcoef[k]);
    a.out[k] = gcoef[k];
    for (int i = 0; i < 5; ++i) a.os[k][i] = gcoef_strides[5 * k + i];
  }
  for (int j = 0; j < taps; ++j) {
    a.ka[j] = rec_lo[j];
    a.kd[j] = rec_hi[j];
  }
  return launch_analysis<true>(a, B * C, taps, stream, "wf_idwt3d_level_bwd");
}

