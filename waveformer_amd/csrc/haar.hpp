// haar.hpp -- the 3D Haar arithmetic shared by the forward / inverse kernels (dwt.hip) and
// their adjoints (train.hip).  A 2x2x2 cube and its 8 bands are related by three butterfly
// stages without scaling and one multiply by (1/sqrt 2)^3; the matrix is orthogonal and
// symmetric, so analysis, synthesis and both adjoints are the same butterfly.
#pragma once
#include "wf_common.hpp"

namespace wf {

constexpr float kHaar3 = 0.35355339059327373f;  // (1/sqrt 2)^3

// Unscaled butterflies along x (slot bit 0), y (bit 1), z (bit 2).  Slot n = (i << 2) | (j << 1)
// | l holds voxel (i, j, l) of the cube on one side and band n ('a' = 0, 'd' = 1 per axis, ptwt
// key order) on the other.  T: float or f32x4.  (dwt3d_haar_fwd_kernel states the same loops
// over its f32x4[V] slots itself: through this function its LL-only instantiations schedule
// their adds in another order, and one of them measured slower)
template <typename T>
__device__ __forceinline__ void haar_butterfly(T (&v)[8]) {
#pragma unroll
  for (int bit = 1; bit < 8; bit <<= 1) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      if (!(n & bit)) {
        const T s0 = v[n], s1 = v[n | bit];
        v[n] = s0 + s1;
        v[n | bit] = s0 - s1;
      }
    }
  }
}

// Multi-level synthesis, coarse part: the level-(L-1) LL value at (z1, y1, x1) of the finest
// detail grid, from the coarsest LL `ll` at its ancestor.  Level l (0 = coarsest) turns the LL
// at the ancestor (z1, y1, x1) >> (L-1-l) into the LL of the child one level finer: the
// child's sub-position picks the sign of each of the 7 details coef(l, k, z, y, x), k = 0..6.
template <typename T, typename Coef>
__device__ __forceinline__ T haar_ll_walk(T ll, int L, int z1, int y1, int x1, Coef coef) {
  for (int l = 0; l < L - 1; ++l) {
    const int sh = L - 1 - l;
    const int zl = z1 >> sh, yl = y1 >> sh, xl = x1 >> sh;
    const int sz = (z1 >> (sh - 1)) & 1, sy = (y1 >> (sh - 1)) & 1, sx = (x1 >> (sh - 1)) & 1;
    T cv[7];
#pragma unroll
    for (int k = 1; k < 8; ++k) cv[k - 1] = coef(l, k - 1, zl, yl, xl);
    T acc = ll;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const int neg = (((k >> 2) & 1) & sz) ^ (((k >> 1) & 1) & sy) ^ ((k & 1) & sx);
      acc = neg ? acc - cv[k - 1] : acc + cv[k - 1];
    }
    ll = acc * kHaar3;
  }
  return ll;
}

}  // namespace wf
