// interp.hpp -- the source index and weights of one trilinear axis (PyTorch's
// upsample_trilinear3d: area_pixel_compute_scale / area_pixel_compute_source_index, fp32).
// A forward kernel and its adjoint, or a kernel and its host-side check, agree only if they
// form the same index and weights; each pair calls one of the two functions below.  The two
// round differently (multiply, then subtract; one FMA) and are not interchangeable.
#pragma once
#include <math.h>

#include "wf_common.hpp"

namespace wf {

struct Src1 {
  int i0, i1;
  float l0, l1;
};

// align_corners=False with an explicit output size, the product rounded before the subtraction
// (ATen's CPU order) and the results clamped.  The multi-scale fuse (misc.hip: lin_index of
// msfuse_kernel and msfuse_row_kernel) and its adjoint (train.hip: interp_adjoint_kernel<false>)
// agree through it.  Out-parameters, not a Src1: the fuse keeps one variable per axis and
// value, and through a returned struct its kernels order three v_mov differently.
__device__ __forceinline__ void src_index_rn(int dst, int in, int out, int& i0, int& i1,
                                             float& l0, float& l1) {
  const float scale = (float)in / (float)out;
  float s = __fmul_rn(scale, (float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min((int)floorf(s), in - 1);
  l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l0 = 1.f - l1;
}

// align_corners either way: True: src = dst * (in - 1) / (out - 1); False: src =
// max((dst + 0.5) * in / out - 0.5, 0) as one FMA, spelled out so that the host forms the
// device's index.  i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.  The
// decoder's up-sampling and the prediction resampling (upsample.hip, every kernel) and the host
// check of wf_upsample_dwconv3d_stats_cl against upsample_dwconv3d_kernel's staging agree
// through these.  (The align_corners=True adjoint, train.hip's lin_src_ac, clamps l1 and stays
// apart: see there.)
__host__ __device__ __forceinline__ float src_scale(int in, int out, bool ac) {
  if (ac) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}
__host__ __device__ __forceinline__ float src_coord(int dst, float scale, bool ac) {
  return ac ? scale * (float)dst : fmaxf(fmaf(scale, (float)dst + 0.5f, -0.5f), 0.f);
}
__host__ __device__ __forceinline__ Src1 src_split(float r, int in) {
  Src1 s;
  s.i0 = (int)r;
  s.i1 = s.i0 + (s.i0 < in - 1 ? 1 : 0);
  s.l1 = r - (float)s.i0;
  s.l0 = 1.f - s.l1;
  return s;
}
// the axis' scale precomputed (scale = src_scale(in, out, ac)): the fused up-sample + conv
// forms thousands of indices per plane
__host__ __device__ __forceinline__ Src1 src_index_s(int dst, int in, float scale, bool ac) {
  return src_split(src_coord(dst, scale, ac), in);
}
// scale and coordinate under one test of ac (src_index_s(dst, in, src_scale(in, out, ac), ac)
// tests it twice, and the row kernels of upsample.hip then compile to other text)
__device__ __forceinline__ Src1 src_index(int dst, int in, int out, bool ac) {
  return src_split(ac ? src_coord(dst, src_scale(in, out, true), true)
                      : src_coord(dst, src_scale(in, out, false), false), in);
}

}  // namespace wf
