// spline.hpp -- what augment.hip and resample.hip share: the index maps and the taps of the
// cubic B-spline prefilter as a FIR, scipy's order-3 interpolation weights, and the per-label
// vote of a segmentation's trilinear interpolation.
#pragma once
#include <algorithm>
#include <math.h>

#include "wf_common.hpp"
#include "zoom_plan.hpp"

namespace wf {

constexpr int AUG_MAX_R = 20;         // taps on either side of a FIR centre
constexpr int AUG_SPLINE_TAPS = 18;   // the cut leaves 2 sqrt(3) |p|^19 / (1 - |p|) = 6.4e-11 max|x|
constexpr int AUG_PAD = WF_SPLINE_PAD;
static_assert(AUG_SPLINE_TAPS == ZOOM_TAPS && AUG_PAD == ZOOM_PAD, "zoom_plan.hpp restates both");

struct FirTaps {
  float w[AUG_MAX_R + 1];
  int r;
};

enum { FIR_MIRROR = 0, FIR_REFLECT = 1, FIR_EDGEPAD = 2 };

// the cubic prefilter's impulse response sqrt(3) pole^|k|, pole = sqrt(3) - 2 (gain 6 times
// -p / (1 - p^2)), rounded from fp64
inline FirTaps spline_taps() {
  FirTaps t;
  const double pole = sqrt(3.0) - 2.0;
  double v = sqrt(3.0);
  t.r = AUG_SPLINE_TAPS;
  for (int k = 0; k <= t.r; ++k, v *= pole) t.w[k] = (float)v;
  return t;
}

// half-sample mirror (scipy's `reflect`): ... 1 0 | 0 1 ... n-1 | n-1 n-2 ...
__device__ __forceinline__ int reflect_index(int j, int n) {
  if ((unsigned)j < (unsigned)n) return j;
  const int P = 2 * n;
  int m = j % P;
  if (m < 0) m += P;
  return m < n ? m : P - 1 - m;
}

template <int MODE>
__device__ __forceinline__ int fir_src(int j, int n_in, int n_out) {
  if (MODE == FIR_REFLECT) return reflect_index(j, n_in);
  if (MODE == FIR_MIRROR) return mirror_index(j, n_in);
  return edgepad_src(j, n_in, n_out);
}

// ---------------------------------------------------------------------------------------
// cubic evaluation: scipy's order-3 weights
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_weights(float t, float* w) {
  const float z = 1.f - t;
  w[1] = (t * t * (t - 2.f) * 3.f + 4.f) / 6.f;
  w[2] = (z * z * (z - 2.f) * 3.f + 4.f) / 6.f;
  w[0] = z * z * z / 6.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
}

// taps floor(x) - 1 .. floor(x) + 2 mirrored onto [0, n), and the weights of x's fraction
__device__ __forceinline__ void cubic_taps(double x, int n, int* idx, float* w) {
  const double f = floor(x);
  cubic_weights((float)(x - f), w);
  const int s = (int)f - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = mirror_index(s + k, n);
}

// resize_segmentation(order=1) at one voxel: the weights of the eight trilinear taps are summed
// per distinct label, in tap order, and the largest label whose sum is >= 0.5 wins, else 0
template <typename T>
__device__ __forceinline__ T label_vote(const T* lab, const double* w) {
  T best = 0;
  bool found = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += lab[j] == lab[k] ? w[j] : 0.0;
    if (s >= 0.5 && (!found || lab[k] > best)) {
      best = lab[k];
      found = true;
    }
  }
  return best;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
inline int aug_check_volume(const char* who, int64_t N, int64_t D, int64_t H, int64_t W) {
  if (!(N >= 1 && D >= 1 && H >= 1 && W >= 1))
    return fail(WF_E_SHAPE, std::string(who) + ": empty volume");
  const int64_t lim = (int64_t)1 << 31;
  if (!(D < lim && H < lim && W < lim && D * H < lim && D * H * W < lim))
    return fail(WF_E_SHAPE, std::string(who) + ": D*H*W must be below 2^31 voxels");
  if (!(N < lim && N * D * H * W < ((int64_t)1 << 40)))
    return fail(WF_E_SHAPE, std::string(who) + ": N*D*H*W must be below 2^40");
  return WF_OK;
}

inline unsigned aug_grid(int64_t n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256), 8192));
}

}  // namespace wf
