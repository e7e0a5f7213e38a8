// augment.hip -- the train-time augmentation of light_training/augment/train_augment.py on the
// device (batchgenerators' SpatialTransform, GaussianBlur, BrightnessMultiplicative, Contrast,
// SimulateLowResolution and Gamma transforms): a cubic B-spline prefilter, an affine sampler
// (cubic data, per-label trilinear segmentation), the two zoom samplers of the low-resolution
// transform, a separable Gaussian blur, and a pointwise kernel that applies one intensity step
// and accumulates the statistics the next step needs.
//
// The prefilter and the blur are the same kernel: a symmetric FIR along one axis.  The cubic
// prefilter 6 / (z + 4 + 1/z) has the impulse response sqrt(3) p^|k| with the pole p = sqrt(3) - 2,
// and |p|^k is below 2^-30 after 16 samples, so the recursion scipy runs along a line is cut off
// after AUG_SPLINE_TAPS samples on either side and every output voxel becomes a tile of its own:
// it reads only the launch's input, never what another workgroup writes, and every device loop
// runs over a tap count or a grid stride.  The boundary is an index map: scipy's
// `mirror` (whole sample) for map_coordinates(mode='constant'), `reflect` (half sample) for
// gaussian_filter, and 12 virtual edge samples on either side, mirrored beyond, for
// zoom(mode='nearest', grid_mode=True), whose output keeps the padding.
//
// Statistics are fp64 partials per workgroup around the workgroup's own first value, merged in a
// fixed order by a second kernel: bitwise repeatable, no float atomics.
#include <algorithm>
#include <math.h>

#include "spline.hpp"
#include "wf_common.hpp"

namespace wf {

constexpr int AUG_MAX_C = 64;
constexpr int AUG_STAT_BLOCKS = 256;  // upper bound of statistic partials per plane
constexpr int AUG_PART = 6;           // doubles per partial: n, shift, sum, sum of squares, min, max

// out (outer, n_out, inner) = FIR along the middle axis of in (outer, n_in, inner); the taps are
// added from the outermost pair inwards, smallest first
template <int MODE>
__global__ __launch_bounds__(256) void fir_axis_kernel(const float* __restrict__ in,
                                                       float* __restrict__ out, int64_t total,
                                                       int n_in, int n_out, int64_t inner,
                                                       FirTaps t) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t q = idx / inner, r = idx - q * inner;
    const int64_t o = q / n_out;
    const int i = (int)(q - o * n_out);
    const float* line = in + o * n_in * inner + r;
    float acc = 0.f;
    for (int k = t.r; k >= 1; --k) {
      const float a = line[(int64_t)fir_src<MODE>(i - k, n_in, n_out) * inner];
      const float b = line[(int64_t)fir_src<MODE>(i + k, n_in, n_out) * inner];
      acc = fmaf(t.w[k], a + b, acc);
    }
    out[idx] = fmaf(t.w[0], line[(int64_t)fir_src<MODE>(i, n_in, n_out) * inner], acc);
  }
}

// ---------------------------------------------------------------------------------------
// cubic evaluation: the 64 taps, x innermost (weights and tap indices: spline.hpp)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float cubic_eval(const float* __restrict__ c, int H, int W,
                                            const int* iz, const int* iy, const int* ix,
                                            const float* wz, const float* wy, const float* wx) {
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float za = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float* row = c + ((int64_t)iz[a] * H + iy[b]) * W;
      float yb = 0.f;
#pragma unroll
      for (int d = 0; d < 4; ++d) yb = fmaf(wx[d], row[ix[d]], yb);
      za = fmaf(wy[b], yb, za);
    }
    acc = fmaf(wz[a], za, acc);
  }
  return acc;
}

struct Affine {
  double m[12];  // input coordinate j of an output voxel at p (zero-centred): sum_i p_i m[4j+i] + m[4j+3]
};

// One thread per output voxel.  coef (C, D, H, W): the prefiltered channels, out (C, oD, oH, oW).
// seg (D, H, W) / oseg (oD, oH, oW) may be NULL.  A point outside [0, n - 1] on any axis gives
// cval: 0 for data, and for seg the -1 that never reaches 0.5, i.e. label 0.
__global__ __launch_bounds__(256) void affine_sample_kernel(
    const float* __restrict__ coef, const float* __restrict__ seg, int C, int D, int H, int W,
    int oD, int oH, int oW, Affine A, float* __restrict__ out, float* __restrict__ oseg) {
  const int64_t S = (int64_t)D * H * W, oS = (int64_t)oD * oH * oW;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < oS;
       idx += (int64_t)gridDim.x * 256) {
    const int ox = (int)(idx % oW), oy = (int)((idx / oW) % oH), oz = (int)(idx / ((int64_t)oW * oH));
    const double p0 = oz - (oD - 1) * 0.5, p1 = oy - (oH - 1) * 0.5, p2 = ox - (oW - 1) * 0.5;
    const double z = (p0 * A.m[0] + p1 * A.m[1] + p2 * A.m[2]) + A.m[3];
    const double y = (p0 * A.m[4] + p1 * A.m[5] + p2 * A.m[6]) + A.m[7];
    const double x = (p0 * A.m[8] + p1 * A.m[9] + p2 * A.m[10]) + A.m[11];
    const bool inside = z >= 0.0 && z <= D - 1 && y >= 0.0 && y <= H - 1 && x >= 0.0 && x <= W - 1;
    if (coef) {
      if (!inside) {
        for (int c = 0; c < C; ++c) out[c * oS + idx] = 0.f;
      } else {
        int iz[4], iy[4], ix[4];
        float wz[4], wy[4], wx[4];
        cubic_taps(z, D, iz, wz);
        cubic_taps(y, H, iy, wy);
        cubic_taps(x, W, ix, wx);
        for (int c = 0; c < C; ++c)
          out[c * oS + idx] = cubic_eval(coef + c * S, H, W, iz, iy, ix, wz, wy, wx);
      }
    }
    if (seg) {
      float best = 0.f;
      if (inside) {
        // the eight trilinear taps in scipy's order (x fastest), weights (wz wy) wx in fp64; a
        // tap past the end has weight 0 and is read at the last index
        const double fz = floor(z), fy = floor(y), fx = floor(x);
        const int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
        const int zi[2] = {z0, min(z0 + 1, D - 1)}, yi[2] = {y0, min(y0 + 1, H - 1)},
                  xi[2] = {x0, min(x0 + 1, W - 1)};
        const double tz = z - fz, ty = y - fy, tx = x - fx;
        const double uz[2] = {1.0 - tz, tz}, uy[2] = {1.0 - ty, ty}, ux[2] = {1.0 - tx, tx};
        float lab[8];
        double w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int a = k >> 2, b = (k >> 1) & 1, d = k & 1;
          lab[k] = seg[((int64_t)zi[a] * H + yi[b]) * W + xi[d]];
          w[k] = (uz[a] * uy[b]) * ux[d];
        }
        best = label_vote(lab, w);
      }
      oseg[idx] = best;
    }
  }
}

// scipy.ndimage.zoom(order=0, mode='nearest', grid_mode=True) of N planes: the source index is
// floor((o + 0.5) n / on - 0.5 + 0.5) clamped, in fp64 as scipy computes it
__device__ __forceinline__ int nearest_src(int o, int n, int on) {
  const double cc = (o + 0.5) * ((double)n / (double)on) - 0.5;
  return min(max((int)floor(cc + 0.5), 0), n - 1);
}

__global__ __launch_bounds__(256) void zoom_nearest_kernel(const float* __restrict__ in, int N,
                                                           int D, int H, int W, int oD, int oH,
                                                           int oW, float* __restrict__ out) {
  const int64_t S = (int64_t)D * H * W, oS = (int64_t)oD * oH * oW, total = oS * N;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t n = idx / oS, v = idx - n * oS;
    const int ox = (int)(v % oW), oy = (int)((v / oW) % oH), oz = (int)(v / ((int64_t)oW * oH));
    const int z = nearest_src(oz, D, oD), y = nearest_src(oy, H, oH), x = nearest_src(ox, W, oW);
    out[idx] = in[n * S + ((int64_t)z * H + y) * W + x];
  }
}

// zoom(order=3, mode='nearest', grid_mode=True) after the prefilter: coef is the padded
// coefficient volume (N, D + 24, H + 24, W + 24) of a (D, H, W) input, sampled at
// (o + 0.5) n / on - 0.5 + 12
__global__ __launch_bounds__(256) void zoom_cubic_kernel(const float* __restrict__ coef, int N,
                                                         int D, int H, int W, int oD, int oH,
                                                         int oW, float* __restrict__ out) {
  const int pD = D + 2 * AUG_PAD, pH = H + 2 * AUG_PAD, pW = W + 2 * AUG_PAD;
  const int64_t pS = (int64_t)pD * pH * pW, oS = (int64_t)oD * oH * oW, total = oS * N;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t n = idx / oS, v = idx - n * oS;
    const int ox = (int)(v % oW), oy = (int)((v / oW) % oH), oz = (int)(v / ((int64_t)oW * oH));
    const double z = (oz + 0.5) * ((double)D / (double)oD) - 0.5 + AUG_PAD;
    const double y = (oy + 0.5) * ((double)H / (double)oH) - 0.5 + AUG_PAD;
    const double x = (ox + 0.5) * ((double)W / (double)oW) - 0.5 + AUG_PAD;
    int iz[4], iy[4], ix[4];
    float wz[4], wy[4], wx[4];
    cubic_taps(z, pD, iz, wz);
    cubic_taps(y, pH, iy, wy);
    cubic_taps(x, pW, ix, wx);
    out[idx] = cubic_eval(coef + n * pS, pH, pW, iz, iy, ix, wz, wy, wx);
  }
}

// ---------------------------------------------------------------------------------------
// pointwise step + statistics
// ---------------------------------------------------------------------------------------
// What a plane's step does to a value, from its parameters {active, value, sign, -} and the
// statistics {mean, std, min, max} it is given; fp32 arithmetic, constants rounded from fp64.
struct PointOp {
  int op;  // WF_AUG_NONE for a plane that is not drawn
  float a, b, c, d, e;
  __device__ __forceinline__ float operator()(float v) const {
    switch (op) {
      case WF_AUG_SCALE:
        return v * a;
      case WF_AUG_CONTRAST:  // (x - mean) f + mean clipped to [min, max]
        return fminf(fmaxf((v - b) * a + b, c), d);
      case WF_AUG_GAMMA_POW: {  // a: gamma, b: sign, c: min, d: range + 1e-7, e: range
        const float t = (b * v - c) / d;
        return powf(t, a) * e + c;
      }
      case WF_AUG_GAMMA_RESTORE:  // a: new mean, c: new std + 1e-8, d: old std, e: old mean, b: sign
        return b * ((v - a) / c * d + e);
      default:
        return v;
    }
  }
};

__device__ __forceinline__ PointOp point_op(int op, const double* __restrict__ params,
                                            const double* __restrict__ sa,
                                            const double* __restrict__ sb, int n) {
  PointOp f{WF_AUG_NONE, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (op == WF_AUG_NONE || params[n * 4] == 0.0) return f;
  f.op = op;
  const double val = params[n * 4 + 1], sgn = params[n * 4 + 2];
  if (op == WF_AUG_SCALE) {
    f.a = (float)val;
  } else if (op == WF_AUG_CONTRAST) {
    f.a = (float)val;
    f.b = (float)sa[n * 4];
    f.c = (float)sa[n * 4 + 2];
    f.d = (float)sa[n * 4 + 3];
  } else if (op == WF_AUG_GAMMA_POW) {  // on sign * x: its minimum is -max when inverted
    const double mn = sgn > 0 ? sa[n * 4 + 2] : -sa[n * 4 + 3];
    const double rng = sa[n * 4 + 3] - sa[n * 4 + 2];
    f.a = (float)val;
    f.b = (float)sgn;
    f.c = (float)mn;
    f.d = (float)(rng + 1e-7);
    f.e = (float)rng;
  } else {  // restore: sa describes x before the power step, sb the power step's output
    f.a = (float)sb[n * 4];
    f.b = (float)sgn;
    f.c = (float)(sb[n * 4 + 1] + 1e-8);
    f.d = (float)sa[n * 4 + 1];
    f.e = (float)(sgn * sa[n * 4]);
  }
  return f;
}

// grid (blocks per plane, N).  Block b owns the contiguous chunk b of its plane: it applies the
// step in place where the plane is drawn and, with partials, reduces what it wrote (or read)
// around its chunk's first value.  GAMMA_POW writes sign * x's power, RESTORE takes the sign off.
__global__ __launch_bounds__(256) void pointwise_stats_kernel(
    float* __restrict__ x, int64_t S, int64_t chunk, int op, const double* __restrict__ params,
    const double* __restrict__ sa, const double* __restrict__ sb, double* __restrict__ partials) {
  const int n = blockIdx.y;
  const PointOp f = point_op(op, params, sa, sb, n);
  float* p = x + (int64_t)n * S;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(S, lo + chunk);
  if (lo >= hi) return;  // block-uniform; the launcher sizes the grid so that it does not happen
  const float shift = f(p[lo]);
  __syncthreads();  // every thread has read p[lo] before thread 0 overwrites it
  double s1 = 0.0, s2 = 0.0;
  float mn = shift, mx = shift;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    float v = p[i];
    if (f.op != WF_AUG_NONE) {
      v = f(v);
      p[i] = v;
    }
    const double dlt = (double)v - (double)shift;
    s1 += dlt;
    s2 += dlt * dlt;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  if (partials == nullptr) return;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  __shared__ double r1[4], r2[4];
  __shared__ float rmn[4], rmx[4];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    r1[wv] = s1; r2[wv] = s2; rmn[wv] = mn; rmx[wv] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partials + ((int64_t)n * gridDim.x + blockIdx.x) * AUG_PART;
    o[0] = (double)(hi - lo);
    o[1] = (double)shift;
    o[2] = ((r1[0] + r1[1]) + r1[2]) + r1[3];
    o[3] = ((r2[0] + r2[1]) + r2[2]) + r2[3];
    o[4] = (double)fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
    o[5] = (double)fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
  }
}

// one thread per plane merges its nblk partials in index order (Chan et al.'s pairwise update):
// stats {mean, population std, min, max}
__global__ __launch_bounds__(64) void stats_finish_kernel(const double* __restrict__ partials,
                                                          int N, int nblk,
                                                          double* __restrict__ stats) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const double* p = partials + (int64_t)n * nblk * AUG_PART;
  double cnt = 0.0, mean = 0.0, m2 = 0.0, mn = p[4], mx = p[5];
  for (int b = 0; b < nblk; ++b, p += AUG_PART) {
    const double nb = p[0], mb = p[1] + p[2] / nb, m2b = fmax(p[3] - p[2] * p[2] / nb, 0.0);
    const double tot = cnt + nb, dlt = mb - mean;
    mean += dlt * (nb / tot);
    m2 += m2b + dlt * dlt * (cnt * nb / tot);
    cnt = tot;
    mn = fmin(mn, p[4]);
    mx = fmax(mx, p[5]);
  }
  stats[n * 4] = mean;
  stats[n * 4 + 1] = sqrt(m2 / cnt);
  stats[n * 4 + 2] = mn;
  stats[n * 4 + 3] = mx;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// the FIR along `axis` of N planes (D, H, W); n_out is the output's length along that axis
static int launch_fir(const char* who, int mode, const float* in, float* out, int64_t N,
                      int64_t D, int64_t H, int64_t W, int axis, int64_t n_out,
                      const FirTaps& taps, hipStream_t s) {
  const int64_t dims[3] = {D, H, W};
  const int64_t n_in = dims[axis];
  const int64_t inner = axis == 0 ? H * W : axis == 1 ? W : 1;
  const int64_t outer = axis == 0 ? N : axis == 1 ? N * D : N * D * H;
  const int64_t total = outer * n_out * inner;
  if (!(total < ((int64_t)1 << 40))) return fail(WF_E_SHAPE, std::string(who) + ": output too large");
  const dim3 grid(aug_grid(total)), block(256);
  if (mode == FIR_MIRROR)
    hipLaunchKernelGGL(fir_axis_kernel<FIR_MIRROR>, grid, block, 0, s, in, out, total, (int)n_in,
                       (int)n_out, inner, taps);
  else if (mode == FIR_REFLECT)
    hipLaunchKernelGGL(fir_axis_kernel<FIR_REFLECT>, grid, block, 0, s, in, out, total, (int)n_in,
                       (int)n_out, inner, taps);
  else
    hipLaunchKernelGGL(fir_axis_kernel<FIR_EDGEPAD>, grid, block, 0, s, in, out, total, (int)n_in,
                       (int)n_out, inner, taps);
  return check_launch(who);
}

static int64_t stat_blocks(int64_t S) {
  return std::max<int64_t>(1, std::min<int64_t>(cdiv(S, 256 * 16), AUG_STAT_BLOCKS));
}

}  // namespace wf

using namespace wf;

extern "C" int wf_spline_prefilter_axis(const float* in, float* out, int64_t N, int64_t D,
                                        int64_t H, int64_t W, int axis, int mode, void* stream) {
  if (int rc = aug_check_volume(__func__, N, D, H, W)) return rc;
  WF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0 (D), 1 (H) or 2 (W)");
  WF_REQUIRE(mode == WF_SPLINE_MIRROR || mode == WF_SPLINE_EDGE, "mode must be 0 (mirror) or 1 (edge)");
  WF_REQUIRE_PTR(in);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE(in != out, "in and out must be different buffers");
  const int64_t dims[3] = {D, H, W};
  const int64_t n = dims[axis];
  hipStream_t s = (hipStream_t)stream;
  if (mode == WF_SPLINE_MIRROR && n == 1) {  // scipy leaves an axis of length 1 alone
    if (hipMemcpyAsync(out, in, (size_t)(N * D * H * W) * sizeof(float), hipMemcpyDeviceToDevice,
                       s) != hipSuccess)
      return check_launch("wf_spline_prefilter_axis (copy)");
    return WF_OK;
  }
  const FirTaps t = spline_taps();
  const bool edge = mode == WF_SPLINE_EDGE;
  return launch_fir(__func__, edge ? FIR_EDGEPAD : FIR_MIRROR, in, out, N, D, H, W, axis,
                    edge ? n + 2 * AUG_PAD : n, t, s);
}

extern "C" int wf_gauss_blur_axis(const float* in, float* out, int64_t N, int64_t D, int64_t H,
                                  int64_t W, int axis, const float* weights, int radius,
                                  void* stream) {
  if (int rc = aug_check_volume(__func__, N, D, H, W)) return rc;
  WF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0 (D), 1 (H) or 2 (W)");
  WF_REQUIRE(radius >= 0 && radius <= AUG_MAX_R, "radius must be in [0, 20]");
  WF_REQUIRE_PTR(weights);
  WF_REQUIRE_PTR(in);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE(in != out, "in and out must be different buffers");
  FirTaps t;
  t.r = radius;
  for (int k = 0; k <= radius; ++k) t.w[k] = weights[k];
  const int64_t dims[3] = {D, H, W};
  return launch_fir(__func__, FIR_REFLECT, in, out, N, D, H, W, axis, dims[axis], t,
                    (hipStream_t)stream);
}

extern "C" int wf_affine_sample(const float* coef, const float* seg, const double* matrix,
                                int64_t C, int64_t D, int64_t H, int64_t W, int64_t oD,
                                int64_t oH, int64_t oW, float* out, float* out_seg,
                                void* stream) {
  WF_REQUIRE(coef != nullptr || seg != nullptr, "coef and seg are both NULL");
  WF_REQUIRE(!coef || (C >= 1 && C <= AUG_MAX_C), "need 1 <= C <= 64 channels");
  if (int rc = aug_check_volume(__func__, coef ? C : 1, D, H, W)) return rc;
  if (int rc = aug_check_volume(__func__, coef ? C : 1, oD, oH, oW)) return rc;
  WF_REQUIRE_PTR(matrix);
  if (coef) WF_REQUIRE_PTR(out);
  if (seg) WF_REQUIRE_PTR(out_seg);
  Affine A;
  for (int k = 0; k < 12; ++k) {
    WF_REQUIRE(std::isfinite(matrix[k]) && fabs(matrix[k]) < 1e6,
               "matrix entries must be finite and below 1e6 in magnitude");
    A.m[k] = matrix[k];
  }
  hipLaunchKernelGGL(affine_sample_kernel, dim3(aug_grid(oD * oH * oW)), dim3(256), 0,
                     (hipStream_t)stream, coef, seg, (int)C, (int)D, (int)H, (int)W, (int)oD,
                     (int)oH, (int)oW, A, out, out_seg);
  return check_launch("wf_affine_sample");
}

extern "C" int wf_zoom_nearest(const float* in, int64_t N, int64_t D, int64_t H, int64_t W,
                               int64_t oD, int64_t oH, int64_t oW, float* out, void* stream) {
  if (int rc = aug_check_volume(__func__, N, D, H, W)) return rc;
  if (int rc = aug_check_volume(__func__, N, oD, oH, oW)) return rc;
  WF_REQUIRE_PTR(in);
  WF_REQUIRE_PTR(out);
  hipLaunchKernelGGL(zoom_nearest_kernel, dim3(aug_grid(N * oD * oH * oW)), dim3(256), 0,
                     (hipStream_t)stream, in, (int)N, (int)D, (int)H, (int)W, (int)oD, (int)oH,
                     (int)oW, out);
  return check_launch("wf_zoom_nearest");
}

extern "C" int wf_zoom_cubic(const float* coef, int64_t N, int64_t D, int64_t H, int64_t W,
                             int64_t oD, int64_t oH, int64_t oW, float* out, void* stream) {
  if (int rc = aug_check_volume(__func__, N, D + 2 * AUG_PAD, H + 2 * AUG_PAD, W + 2 * AUG_PAD))
    return rc;
  if (int rc = aug_check_volume(__func__, N, D, H, W)) return rc;
  if (int rc = aug_check_volume(__func__, N, oD, oH, oW)) return rc;
  WF_REQUIRE_PTR(coef);
  WF_REQUIRE_PTR(out);
  hipLaunchKernelGGL(zoom_cubic_kernel, dim3(aug_grid(N * oD * oH * oW)), dim3(256), 0,
                     (hipStream_t)stream, coef, (int)N, (int)D, (int)H, (int)W, (int)oD, (int)oH,
                     (int)oW, out);
  return check_launch("wf_zoom_cubic");
}

extern "C" int64_t wf_augment_pointwise_workspace_bytes(int64_t N, int64_t S) {
  if (!(N >= 1 && N <= 65535 && S >= 1 && S < ((int64_t)1 << 31))) {
    fail(WF_E_SHAPE, "wf_augment_pointwise_workspace_bytes: need 1 <= N <= 65535 planes of "
                     "1 <= S < 2^31 voxels");
    return -1;
  }
  return align256(N * stat_blocks(S) * AUG_PART * (int64_t)sizeof(double));
}

extern "C" int wf_augment_pointwise(float* x, int64_t N, int64_t S, int op, const double* params,
                                    const double* stats_a, const double* stats_b,
                                    double* stats_out, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  WF_REQUIRE(N >= 1 && N <= 65535 && S >= 1 && S < ((int64_t)1 << 31),
             "need 1 <= N <= 65535 planes of 1 <= S < 2^31 voxels");
  WF_REQUIRE(op >= WF_AUG_NONE && op <= WF_AUG_GAMMA_RESTORE, "unknown op");
  WF_REQUIRE(op != WF_AUG_NONE || stats_out != nullptr, "nothing to do: no op and no stats_out");
  WF_REQUIRE_PTR(x);
  if (op != WF_AUG_NONE) WF_REQUIRE_PTR(params);
  if (op >= WF_AUG_CONTRAST) WF_REQUIRE_PTR(stats_a);
  if (op == WF_AUG_GAMMA_RESTORE) WF_REQUIRE_PTR(stats_b);
  WF_REQUIRE(stats_out == nullptr || (stats_out != stats_a && stats_out != stats_b),
             "stats_out must not be an input of the same call");
  double* partials = nullptr;
  if (stats_out) {
    WF_REQUIRE_PTR(workspace);
    WF_REQUIRE(workspace_bytes >= wf_augment_pointwise_workspace_bytes(N, S),
               "workspace smaller than wf_augment_pointwise_workspace_bytes");
    WF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
    partials = static_cast<double*>(workspace);
  }
  // chunks of whole 256-voxel rounds; the grid is the number of non-empty chunks
  const int64_t chunk = cdiv(cdiv(S, stat_blocks(S)), 256) * 256;
  const int64_t nblk = cdiv(S, chunk);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pointwise_stats_kernel, dim3((unsigned)nblk, (unsigned)N), dim3(256), 0, s, x,
                     S, chunk, op, params, stats_a, stats_b, partials);
  if (stats_out)
    hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, s, partials,
                       (int)N, (int)nblk, stats_out);
  return check_launch("wf_augment_pointwise");
}

extern "C" int wf_channel_stats(const float* x, int64_t N, int64_t S, double* stats,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  WF_REQUIRE_PTR(stats);
  return wf_augment_pointwise(const_cast<float*>(x), N, S, WF_AUG_NONE, nullptr, nullptr, nullptr,
                              stats, workspace, workspace_bytes, stream);
}
