// zoom_plan.hpp -- the segment arithmetic of wf_spline_zoom_axis (resample.hip) in plain C++: no
// HIP type or call, so that the host reports it (wf_spline_zoom_axis_plan) and a CPU test can
// check it against brute force, while the kernel runs the very same functions.
//
// One axis of length n is zoomed to length on.  Output o reads the cubic at the padded coordinate
// x(o) = (o + 0.5) n / on - 0.5 + PAD, i.e. the coefficients floor(x) - 1 .. floor(x) + 2 of the
// padded line of n + 2 PAD, and a coefficient j reads the padded samples j - TAPS .. j + TAPS,
// each of which is an input sample after the index map of the edge padding.  A workgroup takes a
// segment of consecutive outputs [o0, o1): the coefficients [jlo, jhi] its taps span, and the
// input samples [slo, shi] those need (their halo of TAPS on either side, after the index map).
// The segment length m is chosen from n / on so that no segment spans more than ZOOM_SEG_COEF
// coefficients, whatever n: a segment of one output spans 4.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WF_HD __host__ __device__ inline
#else
#define WF_HD inline
#endif

namespace wf {

constexpr int ZOOM_PAD = 12;       // WF_SPLINE_PAD: scipy's edge padding for mode='nearest'
constexpr int ZOOM_TAPS = 18;      // AUG_SPLINE_TAPS: the prefilter's taps on either side
constexpr int ZOOM_SEG_COEF = 60;  // coefficients a segment may span (staged per line in LDS)
constexpr int ZOOM_SEG_SAMP = ZOOM_SEG_COEF + 2 * ZOOM_TAPS;  // input samples a segment may need

// whole-sample mirror of any index onto [0, n): ... 2 1 | 0 1 2 ... n-1 | n-2 ...
WF_HD int mirror_index(int j, int n) {
  if ((unsigned)j < (unsigned)n) return j;
  if (n == 1) return 0;
  const int P = 2 * (n - 1);
  int m = j % P;
  if (m < 0) m += P;
  return m < n ? m : P - m;
}

// the input sample behind index j of the padded line of n_pad = n_in + 2 PAD: PAD edge samples
// on either side, mirrored beyond them
WF_HD int edgepad_src(int j, int n_in, int n_pad) {
  const int q = mirror_index(j, n_pad) - ZOOM_PAD;
  return q < 0 ? 0 : (q > n_in - 1 ? n_in - 1 : q);
}

// zoom(mode='nearest', grid_mode=True)'s coordinate of output o on the padded line, in fp64 as
// scipy computes it.  Not contracted into an FMA, so that host and device agree on the floor.
WF_HD double zoom_coord(int o, int n, int on) {
#pragma clang fp contract(off)
  return (o + 0.5) * ((double)n / (double)on) - 0.5 + ZOOM_PAD;
}

// outputs per segment: (m - 1) n / on + 5 bounds the span in exact arithmetic; one coefficient
// is kept spare for the rounding of the coordinates
WF_HD int zoom_seg_outputs(int n, int on) {
  const double m = floor((double)(ZOOM_SEG_COEF - 6) * (double)on / (double)n) + 1.0;
  return m >= (double)on ? on : (int)m;
}

WF_HD int zoom_seg_count(int n, int on) {
  const int m = zoom_seg_outputs(n, on);
  return (on + m - 1) / m;
}

struct ZoomSeg {
  int o0, o1;    // outputs [o0, o1)
  int jlo, jhi;  // padded coefficients [jlo, jhi]
  int slo, shi;  // input samples [slo, shi]
};

WF_HD ZoomSeg zoom_segment(int n, int on, int seg) {
  const int m = zoom_seg_outputs(n, on), P = n + 2 * ZOOM_PAD;
  ZoomSeg s;
  s.o0 = seg * m;
  s.o1 = s.o0 + m < on ? s.o0 + m : on;
  s.jlo = (int)floor(zoom_coord(s.o0, n, on)) - 1;
  s.jhi = (int)floor(zoom_coord(s.o1 - 1, n, on)) + 2;
  s.slo = edgepad_src(s.jlo - ZOOM_TAPS, n, P);
  s.shi = edgepad_src(s.jhi + ZOOM_TAPS, n, P);
  return s;
}

}  // namespace wf
