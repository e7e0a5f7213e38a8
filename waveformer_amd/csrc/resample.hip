// resample.hip -- the resampling step of preprocessing (light_training/preprocessing/resampling/
// default_resampling.py, the 3-D branch of resample_data_or_seg) on the device: the cubic zoom of
// the data as three fused axis passes, and the per-label linear zoom of the segmentation.
//
// skimage.transform.resize(order=3, mode='edge', anti_aliasing=False) is scipy.ndimage.zoom(
// order=3, mode='nearest', grid_mode=True): an edge padding of 12, the cubic B-spline prefilter
// and a 64-tap interpolation at (o + 0.5) n / on - 0.5 + 12 on every axis.  The zoom is axis
// aligned, so prefilter and interpolation of one axis commute with those of the others and the
// whole operation is the product of three passes, each of which prefilters the edge-padded line
// and interpolates it with 4 taps.  A pass never materialises the padding: the
// coefficients a segment of outputs needs are computed in LDS from the input samples they need.
//
// One workgroup takes 64 lines times one segment of the axis (zoom_plan.hpp).  For the axes D
// and H the 64 lines are adjacent positions of the contiguous inner extent, for W they are 64
// adjacent rows and the threads run along W: every global access is coalesced.  The LDS footprint
// is fixed (64 lines x 156 floats = 39 KB, four workgroups per CU), whatever the axis' length.
// No launch reads what another workgroup writes, there are no atomics, and every output is a
// fixed sequence of fp32 operations: bitwise repeatable.
#include "spline.hpp"
#include "wf_common.hpp"

namespace wf {

constexpr int RS_LINES = 64;
constexpr int RS_ROW = ZOOM_SEG_SAMP + ZOOM_SEG_COEF;  // floats per line: samples, coefficients

// AW: the axis is W (unit stride), a line is a row and `lines` counts all N*D*H rows.  Otherwise
// the volume is (outer, n, lines) with the axis in the middle.  pdiv: rows resp. outer indices
// per plane, for the clamp.  grid: (outer x) tiles of 64 lines x segments, segments fastest.
template <bool AW>
__global__ __launch_bounds__(256) void spline_zoom_axis_kernel(
    const float* __restrict__ in, float* __restrict__ out, int n, int on, int64_t lines,
    int ntile, int nseg, int64_t pdiv, const double* __restrict__ clip, FirTaps t) {
  __shared__ float lds[RS_LINES * RS_ROW];
  const int64_t b = blockIdx.x;
  const int seg = (int)(b % nseg);
  const int tile = (int)((b / nseg) % ntile);
  const int64_t outer = b / nseg / ntile;
  const ZoomSeg zs = zoom_segment(n, on, seg);
  const int P = n + 2 * AUG_PAD;
  const int ns = zs.shi - zs.slo + 1, nc = zs.jhi - zs.jlo + 1, no = zs.o1 - zs.o0;
  const int64_t line0 = (int64_t)tile * RS_LINES;
  const int tid = threadIdx.x;
  auto at = [](int l, int a) { return AW ? l * RS_ROW + a : a * RS_LINES + l; };
  auto split = [](int idx, int cnt, int& l, int& a) {
    if (AW) {
      l = idx / cnt;
      a = idx - l * cnt;
    } else {
      a = idx >> 6;
      l = idx & (RS_LINES - 1);
    }
  };

  // the input samples [slo, shi] of every line
  for (int idx = tid; idx < RS_LINES * ns; idx += 256) {
    int l, a;
    split(idx, ns, l, a);
    const int64_t line = line0 + l;
    if (line >= lines) continue;
    const int64_t src = AW ? line * n + (zs.slo + a) : (outer * n + (zs.slo + a)) * lines + line;
    lds[at(l, a)] = in[src];
  }
  __syncthreads();

  // the coefficients [jlo, jhi] of the edge-padded line: the taps are added from the outermost
  // pair inwards, as fir_axis_kernel adds them
  for (int idx = tid; idx < RS_LINES * nc; idx += 256) {
    int l, j;
    split(idx, nc, l, j);
    const int J = zs.jlo + j;
    float acc = 0.f;
    for (int k = t.r; k >= 1; --k) {
      const float a = lds[at(l, fir_src<FIR_EDGEPAD>(J - k, n, P) - zs.slo)];
      const float c = lds[at(l, fir_src<FIR_EDGEPAD>(J + k, n, P) - zs.slo)];
      acc = fmaf(t.w[k], a + c, acc);
    }
    lds[at(l, ZOOM_SEG_SAMP + j)] =
        fmaf(t.w[0], lds[at(l, fir_src<FIR_EDGEPAD>(J, n, P) - zs.slo)], acc);
  }
  __syncthreads();

  // the outputs [o0, o1): 4 taps each, as the innermost axis of cubic_eval adds them
  for (int idx = tid; idx < RS_LINES * no; idx += 256) {
    int l, oi;
    split(idx, no, l, oi);
    const int64_t line = line0 + l;
    if (line >= lines) continue;
    const int o = zs.o0 + oi;
    int ix[4];
    float w[4];
    cubic_taps(zoom_coord(o, n, on), P, ix, w);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = fmaf(w[k], lds[at(l, ZOOM_SEG_SAMP + ix[k] - zs.jlo)], acc);
    if (clip) {
      const int64_t plane = (AW ? line : outer) / pdiv;
      acc = fminf(fmaxf(acc, (float)clip[plane * 4 + 2]), (float)clip[plane * 4 + 3]);
    }
    out[AW ? line * on + o : (outer * on + o) * lines + line] = acc;
  }
}

// resize_segmentation(order=1): zoom's coordinate (no padding below order 2) clamped to the
// axis, the taps floor and floor + 1, the latter read at the last index when past the end
__device__ __forceinline__ void linear_taps(int o, int n, int on, int* i, double* u) {
  double c = (o + 0.5) * ((double)n / (double)on) - 0.5;
  c = fmin(fmax(c, 0.0), (double)(n - 1));
  const double f = floor(c);
  i[0] = (int)f;
  i[1] = min(i[0] + 1, n - 1);
  u[1] = c - f;
  u[0] = 1.0 - u[1];
}

__global__ __launch_bounds__(256) void zoom_seg_linear_kernel(const int16_t* __restrict__ seg,
                                                              int D, int H, int W, int oD, int oH,
                                                              int oW, int16_t* __restrict__ out) {
  const int64_t oS = (int64_t)oD * oH * oW;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < oS;
       idx += (int64_t)gridDim.x * 256) {
    const int ox = (int)(idx % oW), oy = (int)((idx / oW) % oH), oz = (int)(idx / ((int64_t)oW * oH));
    int zi[2], yi[2], xi[2];
    double uz[2], uy[2], ux[2];
    linear_taps(oz, D, oD, zi, uz);
    linear_taps(oy, H, oH, yi, uy);
    linear_taps(ox, W, oW, xi, ux);
    int lab[8];
    double w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int a = k >> 2, b = (k >> 1) & 1, d = k & 1;
      lab[k] = seg[((int64_t)zi[a] * H + yi[b]) * W + xi[d]];
      w[k] = (uz[a] * uy[b]) * ux[d];
    }
    out[idx] = (int16_t)label_vote(lab, w);
  }
}

}  // namespace wf

using namespace wf;

extern "C" int wf_spline_zoom_axis_plan(int64_t n, int64_t on, int64_t seg, int64_t* plan) {
  const int64_t lim = ((int64_t)1 << 31) - 2 * ZOOM_PAD - 2 * ZOOM_TAPS;
  WF_REQUIRE(n >= 1 && n < lim && on >= 1 && on < lim, "need 1 <= n, on < 2^31 - 60");
  const int nseg = zoom_seg_count((int)n, (int)on);
  if (plan) {
    WF_REQUIRE(seg >= 0 && seg < nseg, "seg outside [0, segments)");
    const ZoomSeg s = zoom_segment((int)n, (int)on, (int)seg);
    const int64_t v[8] = {s.o0, s.o1, s.jlo, s.jhi, s.slo, s.shi, ZOOM_SEG_COEF, ZOOM_SEG_SAMP};
    for (int i = 0; i < 8; ++i) plan[i] = v[i];
  }
  return nseg;
}

extern "C" int wf_spline_zoom_axis(const float* in, float* out, int64_t N, int64_t D, int64_t H,
                                   int64_t W, int axis, int64_t on, const double* clip,
                                   void* stream) {
  if (int rc = aug_check_volume(__func__, N, D, H, W)) return rc;
  WF_REQUIRE(axis >= 0 && axis <= 2, "axis must be 0 (D), 1 (H) or 2 (W)");
  int64_t odims[3] = {D, H, W};
  const int64_t n = odims[axis];
  odims[axis] = on;
  if (int rc = aug_check_volume(__func__, N, odims[0], odims[1], odims[2])) return rc;
  WF_REQUIRE(n < ((int64_t)1 << 30) && on < ((int64_t)1 << 30), "axis lengths must be below 2^30");
  WF_REQUIRE_PTR(in);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE(in != out, "in and out must be different buffers");
  const int64_t nseg = zoom_seg_count((int)n, (int)on);
  // axis W: all rows are lines; else (outer, n, inner) with the inner positions as lines
  const int64_t lines = axis == 2 ? N * D * H : axis == 1 ? W : H * W;
  const int64_t outer = axis == 2 ? 1 : axis == 1 ? N * D : N;
  const int64_t pdiv = axis == 2 ? D * H : axis == 1 ? D : 1;
  const int64_t ntile = cdiv(lines, RS_LINES);
  WF_REQUIRE(ntile < ((int64_t)1 << 31) && outer * ntile * nseg < ((int64_t)1 << 31),
             "too many workgroups: outer * tiles * segments must be below 2^31");
  const dim3 grid((unsigned)(outer * ntile * nseg)), block(256);
  const FirTaps t = spline_taps();
  hipStream_t s = (hipStream_t)stream;
  if (axis == 2)
    hipLaunchKernelGGL(spline_zoom_axis_kernel<true>, grid, block, 0, s, in, out, (int)n, (int)on,
                       lines, (int)ntile, (int)nseg, pdiv, clip, t);
  else
    hipLaunchKernelGGL(spline_zoom_axis_kernel<false>, grid, block, 0, s, in, out, (int)n, (int)on,
                       lines, (int)ntile, (int)nseg, pdiv, clip, t);
  return check_launch("wf_spline_zoom_axis");
}

extern "C" int wf_zoom_seg_linear(const int16_t* seg, int64_t D, int64_t H, int64_t W, int64_t oD,
                                  int64_t oH, int64_t oW, int16_t* out, void* stream) {
  if (int rc = aug_check_volume(__func__, 1, D, H, W)) return rc;
  if (int rc = aug_check_volume(__func__, 1, oD, oH, oW)) return rc;
  WF_REQUIRE_PTR(seg);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE(seg != out, "seg and out must be different buffers");
  hipLaunchKernelGGL(zoom_seg_linear_kernel, dim3(aug_grid(oD * oH * oW)), dim3(256), 0,
                     (hipStream_t)stream, seg, (int)D, (int)H, (int)W, (int)oD, (int)oH, (int)oW,
                     out);
  return check_launch("wf_zoom_seg_linear");
}
