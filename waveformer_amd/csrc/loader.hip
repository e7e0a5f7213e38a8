// loader.hip -- a training batch from cases that lie on the device: the slice + np.pad of
// light_training/dataloading/base_data_loader.py (generate_train_batch) for every sample of the
// batch in one launch.  Sample b is the patch box [lb, lb + patch) of case b; the part of the box
// inside the case is copied, the rest is zero, in the data and in the segmentation (the reference
// pads both with 0), and the segmentation becomes fp32 as the reference returns it.
//
// The cases of a batch are separate allocations of different shapes, so the kernel needs a table
// of them.  It gets the table by value in its argument struct, LOADER_MAX_RECORDS rows per launch:
// no device table to allocate, copy or wait for, and the launch can be captured.
//
// grid.y is the output plane (sample, channel): the record and "data or segmentation" are
// uniform over a workgroup.  grid.x strides over the plane's items, an item being 4 consecutive x
// outputs of one (z, y) row.  The per-axis overlap {dst0, n} and the shift src - dst come from
// loader_plan.hpp, computed once per record on the host.
#include <algorithm>

#include "loader_plan.hpp"
#include "wf_common.hpp"

namespace wf {

constexpr int LOADER_MAX_RECORDS = 16;   // records per launch (72 bytes each in the arguments)
constexpr int LOADER_GRID_CAP = 2048;    // workgroups per launch, all planes together
constexpr int LOADER_VEC_DATA = 1, LOADER_VEC_SEG = 2;  // record flags: 4-element loads

struct LoaderRec {
  const float* data;
  const void* seg;
  int64_t plane;         // D * H * W
  int H, W;
  int dz0, nz, sz;       // outputs [dz0, dz0 + nz) of the axis read input o + sz; the rest is zero
  int dy0, ny, sy;
  int dx0, nx, sx;
  int flags;
};

struct LoaderArgs {
  LoaderRec rec[LOADER_MAX_RECORDS];
  int C, S;
  int pz, py, px;
  int out_vec_data, out_vec_seg;  // 16-byte stores: px % 4 == 0 and the output 16-byte aligned
};

// 4 consecutive x outputs x0 .. x0 + 3 of a source row as fp32.  vec: the group is wholly inside
// or wholly outside [dx0, dx0 + nx) and its source is aligned to 4 elements: one load.
template <typename T>
__device__ __forceinline__ f32x4 load_group(const T* __restrict__ row, int x0, const LoaderRec& r,
                                            bool vec) {
  typedef T tx4 __attribute__((ext_vector_type(4)));
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if ((unsigned)(x0 - r.dx0) < (unsigned)r.nx) {
      const tx4 t = *reinterpret_cast<const tx4*>(row + (x0 + r.sx));
      v = f32x4{(float)t.x, (float)t.y, (float)t.z, (float)t.w};
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((unsigned)(x0 + k - r.dx0) < (unsigned)r.nx) v[k] = (float)row[x0 + k + r.sx];
  }
  return v;
}

template <typename T>  // the segmentation's element type
__global__ __launch_bounds__(256) void crop_pad_batch_kernel(const LoaderArgs a,
                                                             float* __restrict__ out_data,
                                                             float* __restrict__ out_seg) {
  const int CS = a.C + a.S;
  const int b = (int)blockIdx.y / CS, ch = (int)blockIdx.y % CS;  // uniform over the workgroup
  const LoaderRec& r = a.rec[b];
  const bool is_seg = ch >= a.C;
  const int64_t P = (int64_t)a.pz * a.py * a.px;
  float* dst_plane = is_seg ? out_seg + ((int64_t)b * a.S + (ch - a.C)) * P
                            : out_data + ((int64_t)b * a.C + ch) * P;
  const float* src_data = r.data + (int64_t)(is_seg ? 0 : ch) * r.plane;
  const T* src_seg = static_cast<const T*>(r.seg) + (int64_t)(is_seg ? ch - a.C : 0) * r.plane;
  const bool vec = (r.flags & (is_seg ? LOADER_VEC_SEG : LOADER_VEC_DATA)) != 0;
  const bool out_vec = (is_seg ? a.out_vec_seg : a.out_vec_data) != 0;
  const unsigned px4 = (unsigned)(a.px + 3) >> 2;
  const unsigned items = (unsigned)a.pz * (unsigned)a.py * px4;  // below 2^31: checked on the host
  for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
    const unsigned row = it / px4;
    const int x0 = (int)(it - row * px4) * 4;
    const int z = (int)(row / (unsigned)a.py), y = (int)(row - (unsigned)z * (unsigned)a.py);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    // a row whose source z or y is outside the case is zeros and reads nothing
    if ((unsigned)(z - r.dz0) < (unsigned)r.nz && (unsigned)(y - r.dy0) < (unsigned)r.ny) {
      const int64_t srow = ((int64_t)(z + r.sz) * r.H + (y + r.sy)) * r.W;
      v = is_seg ? load_group<T>(src_seg + srow, x0, r, vec)
                 : load_group<float>(src_data + srow, x0, r, vec);
    }
    float* dst = dst_plane + (int64_t)row * a.px + x0;
    if (out_vec) {
      *reinterpret_cast<f32x4*>(dst) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x0 + k < a.px) dst[k] = v[k];
    }
  }
}

static bool loader_aligned(const void* p, size_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

static size_t seg_elem_bytes(int kind) {
  return kind == WF_SEG_INT8 ? 1 : (kind == WF_SEG_INT16 ? 2 : 4);
}

}  // namespace wf

using namespace wf;

extern "C" int wf_crop_pad_axis_plan(int64_t lb, int64_t patch, int64_t extent, int64_t* plan) {
  const int64_t lim = (int64_t)1 << 31;
  WF_REQUIRE(patch >= 1 && patch < lim && extent >= 1 && extent < lim,
             "need 1 <= patch, extent < 2^31");
  WF_REQUIRE_PTR(plan);
  const CropPadAxis s = crop_pad_axis(lb, patch, extent);
  plan[0] = s.dst0;
  plan[1] = s.src0;
  plan[2] = s.n;
  return WF_OK;
}

extern "C" int wf_crop_pad_batch(const int64_t* records, int64_t B, int64_t C, int64_t S,
                                 int seg_kind, int64_t pz, int64_t py, int64_t px,
                                 float* out_data, float* out_seg, void* stream) {
  const int64_t lim = (int64_t)1 << 31;
  WF_REQUIRE(B >= 1 && B < lim, "need 1 <= B < 2^31 samples");
  WF_REQUIRE(C >= 1 && S >= 1 && C + S <= 4095, "need C >= 1, S >= 1 and C + S <= 4095 channels");
  WF_REQUIRE(seg_kind == WF_SEG_INT8 || seg_kind == WF_SEG_INT16 || seg_kind == WF_SEG_FP32,
             "seg_kind must be WF_SEG_INT8 (0), WF_SEG_INT16 (1) or WF_SEG_FP32 (2)");
  WF_REQUIRE(pz >= 1 && py >= 1 && px >= 1, "the patch must be at least 1 voxel on every axis");
  WF_REQUIRE(pz < lim && py < lim && px < lim && pz * py < lim && pz * py * px < lim,
             "the patch must be below 2^31 voxels (the outputs' index type)");
  WF_REQUIRE_PTR(records);
  WF_REQUIRE_PTR(out_data);
  WF_REQUIRE_PTR(out_seg);
  for (int64_t b = 0; b < B; ++b) {
    const int64_t* q = records + b * 8;
    if (q[0] == 0 || q[1] == 0)
      return fail(WF_E_NULLPTR, std::string(__func__) + ": record " + std::to_string(b) +
                                    " has a NULL data or seg pointer");
    const int64_t D = q[2], H = q[3], W = q[4];
    if (!(D >= 1 && H >= 1 && W >= 1))
      return fail(WF_E_SHAPE, std::string(__func__) + ": record " + std::to_string(b) +
                                  " has an extent below 1");
    if (!(D < lim && H < lim && W < lim && D * H < lim && D * H * W < lim))
      return fail(WF_E_SHAPE, std::string(__func__) + ": record " + std::to_string(b) +
                                  ": D*H*W must be below 2^31 voxels");
  }

  const int64_t P = pz * py * px;
  const size_t seg_bytes = seg_elem_bytes(seg_kind);
  const int64_t items = pz * py * ((px + 3) / 4);
  for (int64_t b0 = 0; b0 < B; b0 += LOADER_MAX_RECORDS) {
    const int nb = (int)std::min<int64_t>(LOADER_MAX_RECORDS, B - b0);
    LoaderArgs a = {};
    a.C = (int)C; a.S = (int)S;
    a.pz = (int)pz; a.py = (int)py; a.px = (int)px;
    float* od = out_data + b0 * C * P;
    float* os = out_seg + b0 * S * P;
    a.out_vec_data = px % 4 == 0 && loader_aligned(od, 16);
    a.out_vec_seg = px % 4 == 0 && loader_aligned(os, 16);
    for (int j = 0; j < nb; ++j) {
      const int64_t* q = records + (b0 + j) * 8;
      const int64_t D = q[2], H = q[3], W = q[4];
      const CropPadAxis z = crop_pad_axis(q[5], pz, D), y = crop_pad_axis(q[6], py, H),
                        x = crop_pad_axis(q[7], px, W);
      LoaderRec& r = a.rec[j];
      r.data = reinterpret_cast<const float*>(static_cast<uintptr_t>(q[0]));
      r.seg = reinterpret_cast<const void*>(static_cast<uintptr_t>(q[1]));
      r.plane = D * H * W;
      r.H = (int)H; r.W = (int)W;
      r.dz0 = (int)z.dst0; r.nz = (int)z.n; r.sz = (int)(z.src0 - z.dst0);
      r.dy0 = (int)y.dst0; r.ny = (int)y.n; r.sy = (int)(y.src0 - y.dst0);
      r.dx0 = (int)x.dst0; r.nx = (int)x.n; r.sx = (int)(x.src0 - x.dst0);
      // 4-element loads: every group of 4 outputs is wholly inside or outside the case, and its
      // source starts on a 4-element boundary in every row of every channel
      const bool mult4 = x.dst0 % 4 == 0 && x.src0 % 4 == 0 && W % 4 == 0 && px % 4 == 0 &&
                         r.plane % 4 == 0;
      r.flags = (mult4 && loader_aligned(r.data, 16) ? LOADER_VEC_DATA : 0) |
                (mult4 && loader_aligned(r.seg, 4 * seg_bytes) ? LOADER_VEC_SEG : 0);
    }
    const int64_t planes = (int64_t)nb * (C + S);
    const int64_t per_plane = std::max<int64_t>(1, LOADER_GRID_CAP / planes);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min(cdiv(items, 256), per_plane)),
                    (unsigned)planes);
    hipStream_t s = (hipStream_t)stream;
    if (seg_kind == WF_SEG_INT8)
      hipLaunchKernelGGL(crop_pad_batch_kernel<int8_t>, grid, dim3(256), 0, s, a, od, os);
    else if (seg_kind == WF_SEG_INT16)
      hipLaunchKernelGGL(crop_pad_batch_kernel<int16_t>, grid, dim3(256), 0, s, a, od, os);
    else
      hipLaunchKernelGGL(crop_pad_batch_kernel<float>, grid, dim3(256), 0, s, a, od, os);
    if (int rc = check_launch("wf_crop_pad_batch")) return rc;
  }
  return WF_OK;
}
