// preprocess.hip -- the per-case array transform of 2_preprocessing_mri.py on the device
// (MultiModalityPreprocessor.run_case_npy): the nonzero mask over the modalities, scipy's
// binary_fill_holes, the bounding box of the filled mask, the crop of data and segmentation, the
// z-score of every modality over the cropped volume, and "the k-th set voxel of a label mask in
// C order" for the foreground samples.
//
// The hole fill marks the background that is 6-connected to the array border ("outside").  It is
// a sequence of line-sweep launches: a launch walks every line of one axis forward and backward
// carrying the outside state, and a line belongs to exactly one wave, so no workgroup ever reads
// what another wrote in the same launch -- a launch reads only what earlier launches (or its own
// lanes) wrote.  Every device loop runs over a line length or a tile count; nothing waits for
// another workgroup.  Each launch ORs one word when it marks a voxel, the host enqueues a batch
// of rounds and reads the words once.
//
// Moments are fp64 sums per workgroup, added up by a second kernel in a fixed order: bitwise
// repeatable, and the only atomics in this file are integer ones.
#include <algorithm>
#include <math.h>

#include "wf_common.hpp"

namespace wf {

constexpr int PP_MAX_C = 64;          // modalities of one case
constexpr int PP_MAX_W = 1 << 20;     // a row's ballot words are walked serially
constexpr int PP_FILL_BATCH = 8;      // fill rounds enqueued between two looks at the words
constexpr int PP_SEL_TILE = 1024;     // voxels per counted tile of the ranked selection
constexpr int PP_MOM_BLOCKS = 512;    // upper bound of moment partials per channel
constexpr uint8_t ST_BG = 0, ST_FG = 1, ST_OUT = 2;

typedef unsigned long long u64;

struct Box {
  int z0, y0, x0, d, h, w;
};

// ---------------------------------------------------------------------------------------
// nonzero mask: OR over channels of data[c] != 0 as numpy compares it: -0.0 is zero, a denormal
// and a NaN are not.  Tested on the bits, so that flush-to-zero cannot drop a denormal.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nonzero_mask_kernel(const uint32_t* __restrict__ bits,
                                                           int C, int64_t S,
                                                           uint8_t* __restrict__ mask, int vec) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (vec) {  // S % 4 == 0 and both pointers 16-byte aligned: every channel plane is too
    const int64_t n4 = S >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
      u32x4 acc = {0u, 0u, 0u, 0u};
      for (int c = 0; c < C; ++c)
        acc |= reinterpret_cast<const u32x4*>(bits + (int64_t)c * S)[i] & 0x7fffffffu;
      const uint32_t m = (acc.x ? 1u : 0u) | (acc.y ? 1u << 8 : 0u) | (acc.z ? 1u << 16 : 0u) |
                         (acc.w ? 1u << 24 : 0u);
      reinterpret_cast<uint32_t*>(mask)[i] = m;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += stride) {
      uint32_t acc = 0;
      for (int c = 0; c < C; ++c) acc |= bits[(int64_t)c * S + i] & 0x7fffffffu;
      mask[i] = acc ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------
// hole fill
// ---------------------------------------------------------------------------------------
// state of a voxel: foreground, background, or background known to be outside.  The seeds are
// the background voxels on the six array faces (binary_fill_holes dilates from a border of ones).
__global__ __launch_bounds__(256) void fill_init_kernel(const uint8_t* mask, uint8_t* st, int D,
                                                        int H, int W, int64_t S) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((int64_t)W * H));
    const bool face = x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1;
    st[i] = mask[i] ? ST_FG : (face ? ST_OUT : ST_BG);
  }
}

// One workgroup's report that it marked a voxel.  Thousands of workgroups do in the first
// rounds, and read-modify-writes of one word are served one after another, so a workgroup first
// looks at the word with an agent-scope atomic load (every access to it inside a launch is an
// atomic) and ORs only while it reads zero; a stale zero costs one redundant OR.
__device__ __forceinline__ void fill_report(bool ch, unsigned* changed) {
  if (__syncthreads_or(ch) && threadIdx.x == 0 &&
      __hip_atomic_load(changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
    atomicOr(changed, 1u);
}

// One pass over a line, upwards or downwards.  The line is this thread's alone, so it may read
// eight voxels ahead of its own stores: eight independent loads in flight instead of one.
template <bool UP>
__device__ __forceinline__ bool sweep_line(uint8_t* p, int64_t step, int L) {
  bool carry = false, ch = false;
  for (int b = 0; b < L; b += 8) {
    uint8_t s[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = b + k;
      s[k] = i < L ? p[(UP ? i : L - 1 - i) * step] : ST_FG;  // past the end: a wall
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (s[k] == ST_OUT) carry = true;
      else if (s[k] == ST_FG) carry = false;
      else if (carry) {
        const int i = b + k;
        p[(UP ? i : L - 1 - i) * step] = ST_OUT;
        ch = true;
      }
    }
  }
  return ch;
}

// One thread per line of the y or the z axis (neighbouring threads hold neighbouring x, so a
// wave's accesses are contiguous): forward, then backward, carrying "the previous voxel is
// outside".  `prev` is the word of the round before, written by earlier launches: a round after
// one that changed nothing has nothing to do.
__global__ __launch_bounds__(256) void fill_sweep_lines_kernel(uint8_t* st, int64_t lines,
                                                               int64_t inner, int64_t outer_stride,
                                                               int64_t step, int L,
                                                               const unsigned* prev,
                                                               unsigned* changed) {
  if (prev && *prev == 0) return;
  const int64_t line = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ch = false;
  if (line < lines) {
    uint8_t* p = st + (line / inner) * outer_stride + (line % inner);
    ch = sweep_line<true>(p, step, L);
    ch |= sweep_line<false>(p, step, L);
  }
  fill_report(ch, changed);
}

// outside bits spread through the open (non-foreground) bits of a 64-voxel word towards higher
// (UP) or lower x: the Kogge-Stone occluded fill, six steps
template <bool UP>
__device__ __forceinline__ u64 spread(u64 gen, u64 open) {
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    gen |= open & (UP ? gen << sh : gen >> sh);
    open &= UP ? open << sh : open >> sh;
  }
  return gen;
}

// The x axis: one wave per row, 64 voxels per step as ballot words; the carry between words is
// wave-uniform.  A lane re-reads in the backward pass only bytes it wrote or left itself.
__global__ __launch_bounds__(256) void fill_sweep_rows_kernel(uint8_t* st, int64_t rows, int W,
                                                              const unsigned* prev,
                                                              unsigned* changed) {
  if (prev && *prev == 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  bool ch = false;
  if (row < rows) {  // wave-uniform
    uint8_t* p = st + row * W;
    const int nw = (W + 63) >> 6;
    u64 carry = 0;
    for (int c = 0; c < nw; ++c) {
      const int x = c * 64 + lane;
      const uint8_t s = x < W ? p[x] : ST_FG;
      const u64 om = __ballot(s == ST_OUT), open = om | __ballot(s == ST_BG);
      const u64 f = spread<true>(om | (carry & open), open);
      carry = f >> 63;
      if (((f >> lane) & 1) && s == ST_BG) { p[x] = ST_OUT; ch = true; }
    }
    carry = 0;
    for (int c = nw - 1; c >= 0; --c) {
      const int x = c * 64 + lane;
      const uint8_t s = x < W ? p[x] : ST_FG;
      const u64 om = __ballot(s == ST_OUT), open = om | __ballot(s == ST_BG);
      const u64 f = spread<false>(om | ((carry << 63) & open), open);
      carry = f & 1;
      if (((f >> lane) & 1) && s == ST_BG) { p[x] = ST_OUT; ch = true; }
    }
  }
  fill_report(ch, changed);  // every thread of the block arrives
}

// state -> filled mask (everything that is not outside), its voxel count and the extremes of its
// coordinates.  raw[0..5] = max of {D - z, z + 1, H - y, y + 1, W - x, x + 1} (zeroed before),
// the count is the 64-bit word at raw + 6: integer atomics, one per block and value.
__global__ __launch_bounds__(256) void fill_finish_kernel(uint8_t* st, int D, int H, int W,
                                                          int64_t S, unsigned* raw) {
  __shared__ unsigned red[6];
  __shared__ unsigned cnt_s;
  if (threadIdx.x < 6) red[threadIdx.x] = 0;
  if (threadIdx.x == 6) cnt_s = 0;
  __syncthreads();
  unsigned m[6] = {0, 0, 0, 0, 0, 0};
  unsigned cnt = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < S; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    bool set = false;
    if (i < S) {
      set = st[i] != ST_OUT;
      st[i] = set ? 1 : 0;
      if (set) {
        const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((int64_t)W * H));
        m[0] = max(m[0], (unsigned)(D - z)); m[1] = max(m[1], (unsigned)(z + 1));
        m[2] = max(m[2], (unsigned)(H - y)); m[3] = max(m[3], (unsigned)(y + 1));
        m[4] = max(m[4], (unsigned)(W - x)); m[5] = max(m[5], (unsigned)(x + 1));
      }
    }
    cnt += (unsigned)__popcll(__ballot(set));  // the loop bound is uniform over the block
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (m[k]) atomicMax(&red[k], m[k]);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&cnt_s, cnt);
  __syncthreads();
  if (threadIdx.x < 6 && red[threadIdx.x]) atomicMax(raw + threadIdx.x, red[threadIdx.x]);
  if (threadIdx.x == 6 && cnt_s) atomicAdd(reinterpret_cast<u64*>(raw + 6), (u64)cnt_s);
}

// bbox: {z0, z1, y0, y1, x0, x1, count, 0}, half-open; all zero for an empty mask
__global__ void fill_bbox_kernel(const unsigned* raw, int D, int H, int W, long long* bbox) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u64 count = *reinterpret_cast<const u64*>(raw + 6);
  const bool any = count != 0;
  bbox[0] = any ? D - (long long)raw[0] : 0;
  bbox[1] = any ? (long long)raw[1] : 0;
  bbox[2] = any ? H - (long long)raw[2] : 0;
  bbox[3] = any ? (long long)raw[3] : 0;
  bbox[4] = any ? W - (long long)raw[4] : 0;
  bbox[5] = any ? (long long)raw[5] : 0;
  bbox[6] = (long long)count;
  bbox[7] = 0;
}

// ---------------------------------------------------------------------------------------
// moments of a box, crop, z-score
// ---------------------------------------------------------------------------------------
// item -> source offset inside a channel; G = 4 walks the rows in 16-byte groups (w % 4 == 0)
template <int G>
__device__ __forceinline__ int64_t box_src(int64_t item, const Box& b, int H, int W) {
  const int wg = b.w / G;
  const int64_t r = item / wg;
  const int q = (int)(item % wg);
  const int z = (int)(r / b.h), y = (int)(r % b.h);
  return ((int64_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0 + q * G;
}

// fp64 sum and sum of squares of (x - K), K the box's first voxel (a shift that keeps the sum of
// squares from cancelling), per workgroup: partials[c][block] = {sum, sumsq}
template <int G>
__global__ __launch_bounds__(256) void box_moments_kernel(const float* __restrict__ data,
                                                          int64_t S, int H, int W, Box b,
                                                          double* __restrict__ partials) {
  __shared__ double red[4][2];
  const int c = blockIdx.y;
  const float* src = data + (int64_t)c * S;
  const double K = (double)src[((int64_t)b.z0 * H + b.y0) * W + b.x0];
  const int64_t items = (int64_t)b.d * b.h * (b.w / G);
  double s = 0.0, ss = 0.0;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * 256) {
    const int64_t o = box_src<G>(it, b, H, W);
    if (G == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + o);
      const double d0 = (double)v.x - K, d1 = (double)v.y - K, d2 = (double)v.z - K,
                   d3 = (double)v.w - K;
      s += (d0 + d1) + (d2 + d3);
      ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    } else {
      const double d0 = (double)src[o] - K;
      s += d0;
      ss += d0 * d0;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = s;
    red[threadIdx.x >> 6][1] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = partials + ((int64_t)c * gridDim.x + blockIdx.x) * 2;
    out[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    out[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}

// one wave per channel adds the partials in a fixed order: stats[c] = {mean, population std}
__global__ __launch_bounds__(64) void box_moments_finish_kernel(const float* __restrict__ data,
                                                                int64_t S, int H, int W, Box b,
                                                                const double* __restrict__ partials,
                                                                int nblk, double* stats) {
  const int c = blockIdx.x;
  const double K = (double)data[(int64_t)c * S + ((int64_t)b.z0 * H + b.y0) * W + b.x0];
  double s = 0.0, ss = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 64) {
    s += partials[((int64_t)c * nblk + j) * 2];
    ss += partials[((int64_t)c * nblk + j) * 2 + 1];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  if (threadIdx.x == 0) {
    const double n = (double)b.d * (double)b.h * (double)b.w;
    const double m = s / n;
    const double var = ss / n - m * m;
    stats[c * 2] = K + m;
    stats[c * 2 + 1] = var > 0.0 ? sqrt(var) : (var == var ? 0.0 : var);
  }
}

// out[c] = data[c][box], z-scored when stats are given: (x - mean) / max(std, 1e-8) in fp32, as
// ZScoreNormalization does on a float32 image
template <int G>
__global__ __launch_bounds__(256) void crop_normalize_kernel(const float* data, int64_t S, int H,
                                                             int W, Box b, const double* stats,
                                                             float* out) {
  const int c = blockIdx.y;
  const float* src = data + (int64_t)c * S;
  const int64_t items = (int64_t)b.d * b.h * (b.w / G);
  float* dst = out + (int64_t)c * items * G;
  float mean = 0.f, sd = 1.f;
  if (stats) {
    mean = (float)stats[c * 2];
    sd = fmaxf((float)stats[c * 2 + 1], 1e-8f);
    if (!(sd == sd)) sd = __builtin_nanf("");  // fmaxf drops a NaN; numpy's max(std, 1e-8) too,
                                               // but the mean is NaN then and so is the result
  }
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items;
       it += (int64_t)gridDim.x * 256) {
    const int64_t o = box_src<G>(it, b, H, W);
    if (G == 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(src + o);
      if (stats) {
        v.x = (v.x - mean) / sd; v.y = (v.y - mean) / sd;
        v.z = (v.z - mean) / sd; v.w = (v.w - mean) / sd;
      }
      *reinterpret_cast<f32x4*>(dst + it * 4) = v;
    } else {
      const float v = src[o];
      dst[it] = stats ? (v - mean) / sd : v;
    }
  }
}

// cropped segmentation (crop_to_nonzero): with a seg, label where seg == 0 outside the filled
// mask; without one, 0 inside the mask and label outside.  maxv: the largest value written.
__global__ __launch_bounds__(256) void crop_seg_kernel(const int16_t* __restrict__ seg,
                                                       const uint8_t* __restrict__ filled, int H,
                                                       int W, Box b, int label,
                                                       int16_t* __restrict__ out, int* maxv) {
  // one wave per row of the box: the row's offset is computed once, the lanes walk x
  const int lane = threadIdx.x & 63;
  const int64_t rows = (int64_t)b.d * b.h, nwaves = (int64_t)gridDim.x * 4;
  int mx = INT_MIN;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
    const int z = (int)(r / b.h), y = (int)(r % b.h);
    const int64_t o = ((int64_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
    for (int x = lane; x < b.w; x += 64) {
      const int s = seg ? (int)seg[o + x] : 0;
      const int v = (s == 0 && !filled[o + x]) ? label : s;
      out[r * b.w + x] = (int16_t)v;
      mx = max(mx, v);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  __shared__ int red[4];
  if (lane == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {  // one atomic per block: they are served one after another
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    if (mx != INT_MIN) atomicMax(maxv, mx);
  }
}

// ---------------------------------------------------------------------------------------
// ranked selection: the k-th voxel, in C order, whose label satisfies a predicate
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool sel_pred(int v, int mode, int value) {
  return mode == WF_SELECT_GT ? v > value : v == value;
}

__global__ __launch_bounds__(256) void select_count_kernel(const int16_t* __restrict__ lab,
                                                           int64_t S, int mode, int value,
                                                           uint32_t* __restrict__ counts) {
  __shared__ unsigned red[4];
  const int64_t base = (int64_t)blockIdx.x * PP_SEL_TILE;
  unsigned cnt = 0;
#pragma unroll
  for (int j = 0; j < PP_SEL_TILE / 256; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    cnt += (unsigned)__popcll(__ballot(i < S && sel_pred(lab[i], mode, value)));
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// exclusive scan of the tile counts by one block: offsets[t] = voxels selected before tile t,
// offsets[nt] = the total (also written to *total)
__global__ __launch_bounds__(256) void select_scan_kernel(const uint32_t* __restrict__ counts,
                                                          int64_t nt, long long* offsets,
                                                          long long* total) {
  __shared__ long long part[256];
  const int64_t chunk = (nt + 255) / 256;
  const int64_t lo = std::min<int64_t>(nt, threadIdx.x * chunk), hi = std::min<int64_t>(nt, lo + chunk);
  long long s = 0;
  for (int64_t t = lo; t < hi; ++t) s += counts[t];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int k = 0; k < 256; ++k) {
      const long long v = part[k];
      part[k] = run;
      run += v;
    }
    offsets[nt] = run;
    *total = run;
  }
  __syncthreads();
  long long run = part[threadIdx.x];
  for (int64_t t = lo; t < hi; ++t) {
    offsets[t] = run;
    run += counts[t];
  }
}

// one wave per asked rank: binary search for the tile, then at most 16 ballots inside it.
// coords rows are (0, z, y, x) as np.argwhere gives them on a (1, D, H, W) seg; vals = image[i].
// A rank outside [0, total) gives a row of -1 / a NaN.
__global__ __launch_bounds__(256) void select_pick_kernel(const int16_t* __restrict__ lab,
                                                          int64_t S, int mode, int value,
                                                          const long long* __restrict__ offsets,
                                                          int64_t nt,
                                                          const long long* __restrict__ ranks,
                                                          int64_t nq, int H, int W,
                                                          long long* coords,
                                                          const float* __restrict__ image,
                                                          float* vals) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;  // wave-uniform
  const long long r = ranks[q];
  int64_t found = -1;
  if (r >= 0 && r < offsets[nt]) {
    int64_t lo = 0, hi = nt - 1;  // the last tile with offsets[t] <= r
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (offsets[mid] <= r) lo = mid; else hi = mid - 1;
    }
    long long rem = r - offsets[lo];
    for (int j = 0; j < PP_SEL_TILE / 64; ++j) {
      const int64_t i = lo * PP_SEL_TILE + j * 64 + lane;
      const bool p = i < S && sel_pred(lab[i], mode, value);
      const u64 bal = __ballot(p);
      const int cnt = __popcll(bal);
      if (rem < cnt) {
        const bool mine = p && __popcll(bal & (((u64)1 << lane) - 1)) == (int)rem;
        const u64 who = __ballot(mine);
        found = lo * PP_SEL_TILE + j * 64 + (__ffsll((long long)who) - 1);
        break;
      }
      rem -= cnt;
    }
  }
  if (lane == 0) {
    if (coords) {
      long long* o = coords + q * 4;
      if (found >= 0) {
        o[0] = 0;
        o[1] = found / ((int64_t)H * W);
        o[2] = (found / W) % H;
        o[3] = found % W;
      } else {
        o[0] = o[1] = o[2] = o[3] = -1;
      }
    }
    if (vals) vals[q] = found >= 0 ? image[found] : __builtin_nanf("");
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static int pp_check_volume(const char* who, int64_t D, int64_t H, int64_t W) {
  if (!(D >= 1 && H >= 1 && W >= 1)) return fail(WF_E_SHAPE, std::string(who) + ": empty volume");
  const int64_t lim = (int64_t)1 << 31;
  if (!(D < lim && H < lim && W < lim && D * H < lim && D * H * W < lim))
    return fail(WF_E_SHAPE, std::string(who) + ": D*H*W must be below 2^31 voxels");
  if (!(W <= PP_MAX_W)) return fail(WF_E_SHAPE, std::string(who) + ": supports W <= 2^20");
  return WF_OK;
}

static int pp_check_box(const char* who, const int64_t* box, int64_t D, int64_t H, int64_t W,
                        Box* out) {
  if (box == nullptr) return fail(WF_E_NULLPTR, std::string(who) + ": box is NULL");
  const int64_t dims[3] = {D, H, W};
  for (int a = 0; a < 3; ++a)
    if (!(box[2 * a] >= 0 && box[2 * a] < box[2 * a + 1] && box[2 * a + 1] <= dims[a]))
      return fail(WF_E_SHAPE, std::string(who) + ": box must be a non-empty half-open "
                                                 "[[z0, z1], [y0, y1], [x0, x1]] inside the volume");
  *out = Box{(int)box[0], (int)box[2], (int)box[4], (int)(box[1] - box[0]),
             (int)(box[3] - box[2]), (int)(box[5] - box[4])};
  return WF_OK;
}

static unsigned pp_grid(int64_t n, int64_t per_block, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min(cdiv(n, per_block), cap));
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 16-byte accesses need the box's rows to start and end on a 4-float boundary in every channel
static bool box_vec(const float* data, int64_t S, int64_t W, const Box& b) {
  return aligned16(data) && S % 4 == 0 && W % 4 == 0 && b.x0 % 4 == 0 && b.w % 4 == 0;
}

static int moments_blocks(const Box& b) {
  return (int)pp_grid((int64_t)b.d * b.h * b.w, 256 * 16, PP_MOM_BLOCKS);
}

}  // namespace wf

using namespace wf;

extern "C" int wf_nonzero_mask(const float* data, int64_t C, int64_t D, int64_t H, int64_t W,
                               uint8_t* mask, void* stream) {
  WF_REQUIRE(C >= 1 && C <= PP_MAX_C, "need 1 <= C <= 64 channels");
  if (int rc = pp_check_volume(__func__, D, H, W)) return rc;
  WF_REQUIRE(C * D * H * W < ((int64_t)1 << 40), "C*D*H*W must be below 2^40");
  WF_REQUIRE_PTR(data);
  WF_REQUIRE_PTR(mask);
  const int64_t S = D * H * W;
  const int vec = S % 4 == 0 && aligned16(data) && aligned16(mask);
  hipLaunchKernelGGL(nonzero_mask_kernel, dim3(pp_grid(vec ? S / 4 : S, 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const uint32_t*>(data), (int)C, S, mask,
                     vec);
  return check_launch("wf_nonzero_mask");
}

extern "C" int64_t wf_fill_holes_workspace_bytes(int64_t D, int64_t H, int64_t W) {
  if (pp_check_volume(__func__, D, H, W)) return -1;
  return 256;  // the batch's "changed" words at 0, the bounding-box atomics at 64
}

extern "C" int wf_fill_holes(const uint8_t* mask, int64_t D, int64_t H, int64_t W,
                             uint8_t* filled, int64_t* bbox, void* workspace,
                             int64_t workspace_bytes, int64_t* rounds, void* stream) {
  if (int rc = pp_check_volume(__func__, D, H, W)) return rc;
  WF_REQUIRE_PTR(mask);
  WF_REQUIRE_PTR(filled);
  WF_REQUIRE_PTR(bbox);
  WF_REQUIRE_PTR(workspace);
  WF_REQUIRE(workspace_bytes >= wf_fill_holes_workspace_bytes(D, H, W),
             "workspace smaller than wf_fill_holes_workspace_bytes");
  WF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
  const int64_t S = D * H * W, HW = H * W;
  hipStream_t s = (hipStream_t)stream;
  unsigned* words = static_cast<unsigned*>(workspace);
  unsigned* raw = words + 16;
  hipLaunchKernelGGL(fill_init_kernel, dim3(pp_grid(S, 256, 4096)), dim3(256), 0, s, mask, filled,
                     (int)D, (int)H, (int)W, S);
  if (int rc = check_launch("wf_fill_holes (init)")) return rc;
  // A round that changes something marks at least one background voxel, so there are at most
  // S marking rounds (S bounds the background count) and one that confirms.
  int64_t done_rounds = 0;
  bool converged = false;
  while (!converged && done_rounds <= S) {
    if (hipMemsetAsync(words, 0, 64, s) != hipSuccess) return check_launch("wf_fill_holes (memset)");
    for (int r = 0; r < PP_FILL_BATCH; ++r) {
      const unsigned* prev = r ? words + r - 1 : nullptr;
      if (W > 1)
        hipLaunchKernelGGL(fill_sweep_rows_kernel, dim3((unsigned)cdiv(D * H, 4)), dim3(256), 0, s,
                           filled, D * H, (int)W, prev, words + r);
      if (H > 1)
        hipLaunchKernelGGL(fill_sweep_lines_kernel, dim3((unsigned)cdiv(D * W, 256)), dim3(256), 0,
                           s, filled, D * W, W, HW, W, (int)H, prev, words + r);
      if (D > 1)
        hipLaunchKernelGGL(fill_sweep_lines_kernel, dim3((unsigned)cdiv(HW, 256)), dim3(256), 0, s,
                           filled, HW, HW, (int64_t)0, HW, (int)D, prev, words + r);
    }
    if (int rc = check_launch("wf_fill_holes (sweep)")) return rc;
    unsigned host[PP_FILL_BATCH];
    if (hipMemcpyAsync(host, words, sizeof(host), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return check_launch("wf_fill_holes (read back)");
    for (int r = 0; r < PP_FILL_BATCH && !converged; ++r) {
      if (host[r] == 0) converged = true;
      else ++done_rounds;
    }
  }
  if (!converged) return fail(WF_E_LAUNCH, "wf_fill_holes: no convergence within D*H*W rounds");
  if (rounds) *rounds = done_rounds;
  if (hipMemsetAsync(raw, 0, 32, s) != hipSuccess) return check_launch("wf_fill_holes (memset)");
  hipLaunchKernelGGL(fill_finish_kernel, dim3(pp_grid(S, 256 * 8, 1024)), dim3(256), 0, s, filled,
                     (int)D, (int)H, (int)W, S, raw);
  hipLaunchKernelGGL(fill_bbox_kernel, dim3(1), dim3(64), 0, s, raw, (int)D, (int)H, (int)W,
                     reinterpret_cast<long long*>(bbox));
  return check_launch("wf_fill_holes");
}

extern "C" int64_t wf_box_moments_workspace_bytes(int64_t C, int64_t d, int64_t h, int64_t w) {
  if (!(C >= 1 && C <= PP_MAX_C)) {
    fail(WF_E_SHAPE, "wf_box_moments_workspace_bytes: need 1 <= C <= 64 channels");
    return -1;
  }
  if (pp_check_volume(__func__, d, h, w)) return -1;
  const Box b{0, 0, 0, (int)d, (int)h, (int)w};
  return align256(C * moments_blocks(b) * 2 * (int64_t)sizeof(double));
}

extern "C" int wf_box_moments(const float* data, int64_t C, int64_t D, int64_t H, int64_t W,
                              const int64_t* box, double* stats, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  WF_REQUIRE(C >= 1 && C <= PP_MAX_C, "need 1 <= C <= 64 channels");
  if (int rc = pp_check_volume(__func__, D, H, W)) return rc;
  Box b;
  if (int rc = pp_check_box(__func__, box, D, H, W, &b)) return rc;
  WF_REQUIRE_PTR(data);
  WF_REQUIRE_PTR(stats);
  WF_REQUIRE_PTR(workspace);
  WF_REQUIRE(workspace_bytes >= wf_box_moments_workspace_bytes(C, b.d, b.h, b.w),
             "workspace smaller than wf_box_moments_workspace_bytes");
  WF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
  const int64_t S = D * H * W;
  const int nblk = moments_blocks(b);
  double* partials = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nblk, (unsigned)C);
  if (box_vec(data, S, W, b))
    hipLaunchKernelGGL(box_moments_kernel<4>, grid, dim3(256), 0, s, data, S, (int)H, (int)W, b,
                       partials);
  else
    hipLaunchKernelGGL(box_moments_kernel<1>, grid, dim3(256), 0, s, data, S, (int)H, (int)W, b,
                       partials);
  hipLaunchKernelGGL(box_moments_finish_kernel, dim3((unsigned)C), dim3(64), 0, s, data, S, (int)H,
                     (int)W, b, partials, nblk, stats);
  return check_launch("wf_box_moments");
}

extern "C" int wf_crop_normalize(const float* data, int64_t C, int64_t D, int64_t H, int64_t W,
                                 const int64_t* box, const double* stats, float* out,
                                 void* stream) {
  WF_REQUIRE(C >= 1 && C <= PP_MAX_C, "need 1 <= C <= 64 channels");
  if (int rc = pp_check_volume(__func__, D, H, W)) return rc;
  Box b;
  if (int rc = pp_check_box(__func__, box, D, H, W, &b)) return rc;
  WF_REQUIRE_PTR(data);
  WF_REQUIRE_PTR(out);
  const int64_t S = D * H * W, n = (int64_t)b.d * b.h * b.w;
  const bool whole = n == S;
  WF_REQUIRE(data != out || whole, "in place only when the box is the whole volume");
  hipStream_t s = (hipStream_t)stream;
  if (box_vec(data, S, W, b) && aligned16(out))
    hipLaunchKernelGGL(crop_normalize_kernel<4>, dim3(pp_grid(n / 4, 256 * 4, 4096), (unsigned)C),
                       dim3(256), 0, s, data, S, (int)H, (int)W, b, stats, out);
  else
    hipLaunchKernelGGL(crop_normalize_kernel<1>, dim3(pp_grid(n, 256 * 4, 4096), (unsigned)C),
                       dim3(256), 0, s, data, S, (int)H, (int)W, b, stats, out);
  return check_launch("wf_crop_normalize");
}

extern "C" int wf_crop_seg(const int16_t* seg, const uint8_t* filled, int64_t D, int64_t H,
                           int64_t W, const int64_t* box, int label, int16_t* out, int* maxv,
                           void* stream) {
  if (int rc = pp_check_volume(__func__, D, H, W)) return rc;
  Box b;
  if (int rc = pp_check_box(__func__, box, D, H, W, &b)) return rc;
  WF_REQUIRE(label >= -32768 && label <= 32767, "the label must fit int16");
  WF_REQUIRE_PTR(filled);
  WF_REQUIRE_PTR(out);
  WF_REQUIRE_PTR(maxv);
  const int64_t rows = (int64_t)b.d * b.h;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(maxv, 0x80, sizeof(int), s) != hipSuccess)  // 0x80808080: below any int16
    return check_launch("wf_crop_seg (memset)");
  hipLaunchKernelGGL(crop_seg_kernel, dim3(pp_grid(rows, 4 * 8, 1024)), dim3(256), 0, s, seg, filled,
                     (int)H, (int)W, b, label, out, maxv);
  return check_launch("wf_crop_seg");
}

static int64_t select_tiles(int64_t S) { return cdiv(S, PP_SEL_TILE); }

extern "C" int64_t wf_select_workspace_bytes(int64_t S) {
  if (!(S >= 1 && S < ((int64_t)1 << 31))) {
    fail(WF_E_SHAPE, "wf_select_workspace_bytes: need 1 <= S < 2^31 voxels");
    return -1;
  }
  const int64_t nt = select_tiles(S);
  return align256((nt + 1) * (int64_t)sizeof(int64_t)) + align256(nt * (int64_t)sizeof(uint32_t));
}

extern "C" int wf_select_scan(const int16_t* labels, int64_t S, int mode, int value,
                              void* workspace, int64_t workspace_bytes, int64_t* total,
                              void* stream) {
  WF_REQUIRE(S >= 1 && S < ((int64_t)1 << 31), "need 1 <= S < 2^31 voxels");
  WF_REQUIRE(mode == WF_SELECT_EQ || mode == WF_SELECT_GT, "mode must be 0 (==) or 1 (>)");
  WF_REQUIRE_PTR(labels);
  WF_REQUIRE_PTR(workspace);
  WF_REQUIRE_PTR(total);
  WF_REQUIRE(workspace_bytes >= wf_select_workspace_bytes(S),
             "workspace smaller than wf_select_workspace_bytes");
  WF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
  const int64_t nt = select_tiles(S);
  long long* offsets = static_cast<long long*>(workspace);
  uint32_t* counts = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) +
                                                 align256((nt + 1) * (int64_t)sizeof(int64_t)));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)nt), dim3(256), 0, s, labels, S, mode,
                     value, counts);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, counts, nt, offsets,
                     reinterpret_cast<long long*>(total));
  return check_launch("wf_select_scan");
}

extern "C" int wf_select_pick(const int16_t* labels, int64_t D, int64_t H, int64_t W, int mode,
                              int value, const void* workspace, int64_t workspace_bytes,
                              const int64_t* ranks, int64_t nq, int64_t* coords,
                              const float* image, float* vals, void* stream) {
  if (int rc = pp_check_volume(__func__, D, H, W)) return rc;
  WF_REQUIRE(mode == WF_SELECT_EQ || mode == WF_SELECT_GT, "mode must be 0 (==) or 1 (>)");
  WF_REQUIRE(nq >= 1 && nq < ((int64_t)1 << 31), "need 1 <= nq < 2^31 ranks");
  WF_REQUIRE_PTR(labels);
  WF_REQUIRE_PTR(workspace);
  WF_REQUIRE_PTR(ranks);
  WF_REQUIRE(coords != nullptr || vals != nullptr, "coords and vals are both NULL");
  if (vals) WF_REQUIRE_PTR(image);
  const int64_t S = D * H * W;
  WF_REQUIRE(workspace_bytes >= wf_select_workspace_bytes(S),
             "workspace smaller than wf_select_workspace_bytes");
  const int64_t nt = select_tiles(S);
  hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0,
                     (hipStream_t)stream, labels, S, mode, value,
                     static_cast<const long long*>(workspace), nt,
                     reinterpret_cast<const long long*>(ranks), nq, (int)H, (int)W,
                     reinterpret_cast<long long*>(coords), image, vals);
  return check_launch("wf_select_pick");
}
