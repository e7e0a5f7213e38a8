// loader_plan.hpp -- the segment arithmetic of wf_crop_pad_batch (loader.hip) in plain C++: no
// HIP type or call, so that the host reports it (wf_crop_pad_axis_plan) and a CPU test can check
// it against three lines of Python, while the launch path runs the very same function.
//
// One axis of a patch box: the box covers [lb, lb + patch) in the coordinates of a case whose axis
// has `extent` voxels, and may hang over either edge or lie wholly outside.  The part inside is
// copied, the rest of the patch is zero:
//   out[dst0 : dst0 + n] = in[src0 : src0 + n],   out elsewhere = 0.
// Where n > 0, src0 - dst0 = lb: output o reads input o + lb.  An empty overlap is {0, 0, 0}.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WF_HD __host__ __device__ inline
#else
#define WF_HD inline
#endif

namespace wf {

struct CropPadAxis {
  int64_t dst0, src0, n;
};

// 64-bit throughout: lb is the caller's and may be far outside the case
WF_HD CropPadAxis crop_pad_axis(int64_t lb, int64_t patch, int64_t extent) {
  const int64_t lo = lb > 0 ? lb : 0;
  const int64_t end = lb > extent - patch ? extent : lb + patch;  // min(lb + patch, extent)
  CropPadAxis s;
  s.n = end > lo ? end - lo : 0;
  s.dst0 = s.n ? lo - lb : 0;
  s.src0 = s.n ? lo : 0;
  return s;
}

}  // namespace wf
