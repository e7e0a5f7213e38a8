// metrics.hip -- evaluation: region masks, overlap counts, the exact squared Euclidean distance
// to a mask's border, surface-distance histograms and their order statistics (region Dice and
// HD95 of 5_compute_metrics.py / medpy.metric.binary).  Everything on the device is integer:
// with unit spacing a surface distance is the square root of an integer, so the squared
// distances, the histogram over them and the ranks taken from it are exact, and integer
// atomics make every output bitwise repeatable.  The square root is the host's.
#include <algorithm>

#include "wf_common.hpp"

namespace wf {

// "no border voxel on this line / plane" between the passes: a real squared distance is below
// 2^31 (validated), so EDT_INF + (i - j)^2 stays below 2^32 and never wraps
constexpr uint32_t EDT_INF = 0x80000000u;
constexpr int MET_MAX_REGIONS = 4;
constexpr int MET_MAX_CLASSES = 8;
constexpr int EDT_MAX_W = 4096;   // 64 ballot words per row
constexpr int EDT_MAX_LINE = 512; // (512 * 64 + 64) * 4 B = 128.25 KB of LDS
constexpr int HIST_LOW = 4096;    // bins a block counts in LDS before it touches global memory

// per-wave totals (every lane of a wave holds the same value) -> one atomic per block and value
template <int N>
__device__ __forceinline__ void block_flush(const unsigned (&cnt)[N], int n,
                                            unsigned long long* dst) {
  __shared__ unsigned red[4][N];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
    for (int k = 0; k < N; ++k) red[wave][k] = cnt[k];
  __syncthreads();
  if ((int)threadIdx.x < n) {
    const unsigned long long s = (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] +
                                 red[2][threadIdx.x] + red[3][threadIdx.x];
    if (s) atomicAdd(dst + threadIdx.x, s);
  }
}

struct RegionArgs {
  const void* src;
  uint8_t* masks;
  uint8_t* labels;
  unsigned long long* counts;
  int64_t S;
  int C, R;
  unsigned bits[MET_MAX_REGIONS];
};

template <typename T>
__device__ __forceinline__ unsigned argmax_label(const T* s, int64_t i, int64_t S, int C) {
  // torch.argmax: the first maximal index, a NaN being the maximum
  float best = (float)s[i];
  unsigned bi = 0;
  for (int c = 1; c < C; ++c) {
    const float v = (float)s[(int64_t)c * S + i];
    if (v > best || (v != v && best == best)) {
      best = v;
      bi = (unsigned)c;
    }
  }
  return bi;
}

template <int KIND>
__global__ __launch_bounds__(256) void region_masks_kernel(RegionArgs a) {
  unsigned cnt[MET_MAX_REGIONS] = {0, 0, 0, 0};
  // the loop bound is uniform over the block: every lane reaches the ballots
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.S; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < a.S;
    unsigned lab = 255;
    if (in) {
      if (KIND == WF_SRC_LABELS_U8) lab = ((const uint8_t*)a.src)[i];
      else if (KIND == WF_SRC_SCORES_F16) lab = argmax_label((const _Float16*)a.src, i, a.S, a.C);
      else lab = argmax_label((const float*)a.src, i, a.S, a.C);
      if (a.labels) a.labels[i] = (uint8_t)lab;
    }
    const unsigned bit = lab < MET_MAX_CLASSES ? 1u << lab : 0u;
#pragma unroll
    for (int r = 0; r < MET_MAX_REGIONS; ++r) {
      if (r < a.R) {
        const bool m = (bit & a.bits[r]) != 0;
        if (in) a.masks[(int64_t)r * a.S + i] = m ? 1 : 0;
        cnt[r] += (unsigned)__popcll(__ballot(m));
      }
    }
  }
  block_flush(cnt, a.R, a.counts);
}

__global__ __launch_bounds__(256) void overlap_counts_kernel(const uint8_t* __restrict__ a,
                                                             const uint8_t* __restrict__ b,
                                                             int64_t S,
                                                             unsigned long long* counts) {
  const int64_t off = (int64_t)blockIdx.y * S;
  unsigned cnt[3] = {0, 0, 0};
  for (int64_t base = (int64_t)blockIdx.x * 256; base < S; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool va = i < S && a[off + i] != 0;
    const bool vb = i < S && b[off + i] != 0;
    cnt[0] += (unsigned)__popcll(__ballot(va && vb));
    cnt[1] += (unsigned)__popcll(__ballot(va));
    cnt[2] += (unsigned)__popcll(__ballot(vb));
  }
  block_flush(cnt, 3, counts + (int64_t)blockIdx.y * 3);
}

// Pass x, fused with the border: one wave per row.  The row's border flags are kept as ballot
// words, and the nearest border voxel to the left and to the right of x comes from clz / ffs on
// them, so a row without any costs nothing more than a row full of them.
__global__ __launch_bounds__(256) void edt_x_kernel(const uint8_t* __restrict__ masks,
                                                    uint8_t* __restrict__ border,
                                                    uint32_t* __restrict__ f, int D, int H, int W,
                                                    int64_t rows) {
  __shared__ unsigned long long words[4][EDT_MAX_W / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nw = (W + 63) >> 6;
  const int64_t HW = (int64_t)H * W;
  for (int64_t rbase = (int64_t)blockIdx.x * 4; rbase < rows; rbase += (int64_t)gridDim.x * 4) {
    const int64_t row = rbase + wave;  // (m, z, y) flattened
    const bool valid = row < rows;
    const int y = (int)(row % H), z = (int)((row / H) % D);
    const bool yz_inner = y > 0 && y < H - 1 && z > 0 && z < D - 1;
    const uint8_t* p = masks + row * W;
    for (int c = 0; c < nw; ++c) {
      const int x = c * 64 + lane;
      bool bd = false;
      if (valid && x < W) {
        const uint8_t* q = p + x;
        if (q[0]) {
          bool inner = yz_inner && x > 0 && x < W - 1;
          if (inner) inner = q[-1] && q[1] && q[-W] && q[W] && q[-HW] && q[HW];
          bd = !inner;
        }
        border[row * W + x] = bd ? 1 : 0;
      }
      const unsigned long long bal = __ballot(bd);
      if (lane == 0) words[wave][c] = bal;
    }
    __syncthreads();
    for (int c = 0; c < nw; ++c) {
      const int x = c * 64 + lane;
      if (valid && x < W) {
        uint32_t best = EDT_INF;
        for (int wi = c; wi >= 0; --wi) {  // nearest border voxel at or left of x
          unsigned long long bits = words[wave][wi];
          if (wi == c) bits &= ~0ull >> (63 - lane);
          if (bits) {
            const uint32_t d = (uint32_t)(x - (wi * 64 + 63 - __clzll((long long)bits)));
            best = d * d;
            break;
          }
        }
        for (int wi = c; wi < nw; ++wi) {  // at or right of x
          unsigned long long bits = words[wave][wi];
          if (wi == c) bits &= ~0ull << lane;
          if (bits) {
            const uint32_t d = (uint32_t)(wi * 64 + __ffsll((long long)bits) - 1 - x);
            best = min(best, d * d);
            break;
          }
        }
        f[row * W + x] = best;
      }
    }
    __syncthreads();
  }
}

// Passes y and z: dst[i] = min_j src[j] + (i - j)^2 along a line of L voxels line_stride apart.
// A block stages the lines of 64 consecutive x (lanes along x: contiguous global accesses, no
// LDS bank conflicts) and takes the minimum by brute force outwards from i, which may stop once
// (i - j)^2 reaches the best value so far: every j beyond can only give more.  Exact.  The
// search is latency bound (each step waits for LDS and decides whether to go on), so a step
// covers EDT_STEP distances with independent reads, and 16 waves share a tile.  A read past an
// end of the line is clamped to the end: f[end] + d^2 with d beyond the end's own distance is
// above that voxel's true candidate, so it can never pull the minimum below the exact one.  A
// column with no finite entry (most of a volume with one tumour in it) is copied through.
constexpr int EDT_LINE_THREADS = 1024;
constexpr int EDT_STEP = 4;
__global__ __launch_bounds__(EDT_LINE_THREADS) void edt_line_kernel(
    const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int L, int64_t line_stride,
    int64_t outer_stride, int64_t S, int W, int last) {
  extern __shared__ uint32_t edt_tile[];  // [L][64], then the 64 column minima
  constexpr int NW = EDT_LINE_THREADS / 64;
  uint32_t* colmin = edt_tile + (size_t)L * 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = blockIdx.x * 64 + lane;
  const int64_t base = (int64_t)blockIdx.z * S + (int64_t)blockIdx.y * outer_stride + x;
  if (threadIdx.x < 64) colmin[threadIdx.x] = EDT_INF;
  __syncthreads();
  uint32_t mn = EDT_INF;
  for (int j = wave; j < L; j += NW) {
    const uint32_t v = x < W ? src[base + (int64_t)j * line_stride] : EDT_INF;
    edt_tile[j * 64 + lane] = v;
    mn = min(mn, v);
  }
  atomicMin(&colmin[lane], mn);
  __syncthreads();
  if (x >= W) return;
  const bool none = colmin[lane] >= EDT_INF;
  const uint32_t none_value = last ? WF_EDT_NONE : EDT_INF;
  for (int i = wave; i < L; i += NW) {
    uint32_t best = edt_tile[i * 64 + lane];
    if (!none) {
      const int reach = max(i, L - 1 - i);  // the farthest voxel of the line
      for (int d = 1; d <= reach && (uint32_t)d * (uint32_t)d < best; d += EDT_STEP) {
        uint32_t cand[EDT_STEP];
#pragma unroll
        for (int u = 0; u < EDT_STEP; ++u) {
          const int e = d + u;
          const uint32_t lo = edt_tile[max(i - e, 0) * 64 + lane];
          const uint32_t hi = edt_tile[min(i + e, L - 1) * 64 + lane];
          cand[u] = min(lo, hi) + (uint32_t)e * (uint32_t)e;
        }
#pragma unroll
        for (int u = 0; u < EDT_STEP; ++u) best = min(best, cand[u]);
      }
    }
    dst[base + (int64_t)i * line_stride] = best >= EDT_INF ? none_value : best;
  }
}

// hist[p][dir][d2] += 1 for every border voxel of one mask, d2 its squared distance to the
// other mask's border.  The small distances, where most of a good prediction's voxels fall,
// are counted in LDS and reach global memory as one atomic per block and non-empty bin.
__global__ __launch_bounds__(256) void surface_hist_kernel(const uint8_t* __restrict__ border_a,
                                                           const uint32_t* __restrict__ d2_b,
                                                           const uint8_t* __restrict__ border_b,
                                                           const uint32_t* __restrict__ d2_a,
                                                           int64_t S, uint32_t nbins,
                                                           uint32_t* hist) {
  __shared__ unsigned low[HIST_LOW];
  const int dir = blockIdx.z;
  const int64_t off = (int64_t)blockIdx.y * S;
  const uint8_t* bd = (dir ? border_b : border_a) + off;
  const uint32_t* d2 = (dir ? d2_a : d2_b) + off;
  uint32_t* h = hist + ((int64_t)blockIdx.y * 2 + dir) * nbins;
  for (int k = threadIdx.x; k < HIST_LOW; k += 256) low[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256) {
    if (bd[i]) {
      const uint32_t v = d2[i];
      if (v < nbins) {  // WF_EDT_NONE (the other mask is empty) is not a distance
        if (v < HIST_LOW) atomicAdd(&low[v], 1u);
        else atomicAdd(&h[v], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < HIST_LOW && k < nbins; k += 256) {
    const unsigned c = low[k];
    if (c) atomicAdd(&h[k], c);
  }
}

struct OrderArgs {
  const uint32_t* hist;
  long long* out;
  int64_t nbins;
  long long q_num, q_den;
  long long off[4];
  int group, nranks;
};

// One workgroup per histogram group: thread t sums the bins of chunk t, thread 0 turns the 256
// chunk sums into prefix sums and the requested ranks, and the thread whose chunk holds a rank
// walks it to the bin.
__global__ __launch_bounds__(256) void hist_order_stats_kernel(OrderArgs a) {
  __shared__ unsigned long long pre[257];
  __shared__ long long top[256];
  __shared__ long long rank[4];
  const int t = threadIdx.x;
  const uint32_t* h = a.hist + (int64_t)blockIdx.x * a.group * a.nbins;
  long long* out = a.out + (int64_t)blockIdx.x * WF_ORDER_STATS_STRIDE;
  const int64_t chunk = (a.nbins + 255) / 256;
  const int64_t b0 = min((int64_t)t * chunk, a.nbins), b1 = min(b0 + chunk, a.nbins);
  unsigned long long sum = 0;
  long long mx = -1;
  for (int64_t b = b0; b < b1; ++b) {
    unsigned long long c = 0;
    for (int k = 0; k < a.group; ++k) c += h[(int64_t)k * a.nbins + b];
    if (c) {
      sum += c;
      mx = b;
    }
  }
  pre[t + 1] = sum;
  top[t] = mx;
  __syncthreads();
  if (t == 0) {
    pre[0] = 0;
    long long m = -1;
    for (int i = 0; i < 256; ++i) {
      pre[i + 1] += pre[i];
      m = max(m, top[i]);
    }
    const long long n = (long long)pre[256];
    const long long base = n > 0 ? a.q_num * (n - 1) / a.q_den : 0;
    out[0] = n;
    out[1] = m;
    out[2] = base;
    for (int i = 0; i < 4; ++i) {
      rank[i] = i < a.nranks && n > 0 ? min(max(base + a.off[i], 0ll), n - 1) : -1;
      out[3 + i] = -1;
    }
    out[7] = 0;
  }
  __syncthreads();
  for (int i = 0; i < a.nranks; ++i) {
    const long long r = rank[i];
    if (r < 0 || (unsigned long long)r < pre[t] || (unsigned long long)r >= pre[t + 1]) continue;
    unsigned long long acc = pre[t];
    for (int64_t b = b0; b < b1; ++b) {
      for (int k = 0; k < a.group; ++k) acc += h[(int64_t)k * a.nbins + b];
      if ((unsigned long long)r < acc) {
        out[3 + i] = b;
        break;
      }
    }
  }
}

// the limits every evaluation entry shares: 32-bit voxel indices and squared distances
static int check_volume(const char* who, int64_t D, int64_t H, int64_t W) {
  if (!(D >= 1 && H >= 1 && W >= 1)) return fail(WF_E_SHAPE, std::string(who) + ": empty volume");
  const int64_t lim = (int64_t)1 << 31;
  if (!(D < lim && H < lim && W < lim && D * H < lim && D * H * W < lim))
    return fail(WF_E_SHAPE, std::string(who) + ": D*H*W must be below 2^31 voxels");
  if (!(D * D + H * H + W * W < lim))
    return fail(WF_E_SHAPE, std::string(who) + ": D^2 + H^2 + W^2 must be below 2^31");
  return WF_OK;
}

static unsigned grid_for(int64_t n, int64_t per_block, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min(cdiv(n, per_block), cap));
}

}  // namespace wf

using namespace wf;

extern "C" int wf_region_masks(const void* src, int src_kind, int64_t C, const int* region_bits,
                               int64_t R, uint8_t* masks, uint8_t* labels, int64_t* counts,
                               int64_t D, int64_t H, int64_t W, void* stream) {
  WF_REQUIRE(src_kind == WF_SRC_LABELS_U8 || src_kind == WF_SRC_SCORES_F16 ||
                 src_kind == WF_SRC_SCORES_F32,
             "src_kind must be 0 (uint8 labels), 1 (fp16 scores) or 2 (fp32 scores)");
  if (src_kind != WF_SRC_LABELS_U8)
    WF_REQUIRE(C >= 1 && C <= MET_MAX_CLASSES, "scores need 1 <= C <= 8 classes");
  WF_REQUIRE(R >= 1 && R <= MET_MAX_REGIONS, "need 1 <= R <= 4 regions");
  if (int rc = check_volume(__func__, D, H, W)) return rc;
  WF_REQUIRE_PTR(src);
  WF_REQUIRE_PTR(region_bits);
  WF_REQUIRE_PTR(masks);
  WF_REQUIRE_PTR(counts);
  if (src_kind != WF_SRC_LABELS_U8) WF_REQUIRE_PTR(labels);
  RegionArgs a{};
  a.src = src;
  a.masks = masks;
  a.labels = labels;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.S = D * H * W;
  a.C = (int)C;
  a.R = (int)R;
  for (int r = 0; r < (int)R; ++r) {
    WF_REQUIRE(region_bits[r] >= 0 && region_bits[r] < (1 << MET_MAX_CLASSES),
               "a region's class bitmask must be in [0, 255]");
    a.bits[r] = (unsigned)region_bits[r];
  }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)R * sizeof(int64_t), s) != hipSuccess)
    return check_launch("wf_region_masks (memset)");
  const dim3 grid(grid_for(a.S, 256, 2048));
  if (src_kind == WF_SRC_LABELS_U8)
    hipLaunchKernelGGL(region_masks_kernel<WF_SRC_LABELS_U8>, grid, dim3(256), 0, s, a);
  else if (src_kind == WF_SRC_SCORES_F16)
    hipLaunchKernelGGL(region_masks_kernel<WF_SRC_SCORES_F16>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(region_masks_kernel<WF_SRC_SCORES_F32>, grid, dim3(256), 0, s, a);
  return check_launch("wf_region_masks");
}

extern "C" int wf_overlap_counts(const uint8_t* a, const uint8_t* b, int64_t R, int64_t D,
                                 int64_t H, int64_t W, int64_t* counts, void* stream) {
  WF_REQUIRE(R >= 1 && R <= MET_MAX_REGIONS, "need 1 <= R <= 4 regions");
  if (int rc = check_volume(__func__, D, H, W)) return rc;
  WF_REQUIRE_PTR(a);
  WF_REQUIRE_PTR(b);
  WF_REQUIRE_PTR(counts);
  const int64_t S = D * H * W;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)R * 3 * sizeof(int64_t), s) != hipSuccess)
    return check_launch("wf_overlap_counts (memset)");
  hipLaunchKernelGGL(overlap_counts_kernel, dim3(grid_for(S, 256, 1024), (unsigned)R), dim3(256),
                     0, s, a, b, S, reinterpret_cast<unsigned long long*>(counts));
  return check_launch("wf_overlap_counts");
}

static int check_edt(const char* who, int64_t M, int64_t D, int64_t H, int64_t W) {
  if (!(M >= 1 && M <= 1024)) return fail(WF_E_SHAPE, std::string(who) + ": need 1 <= M <= 1024 masks");
  if (int rc = check_volume(who, D, H, W)) return rc;
  if (!(W <= EDT_MAX_W && H <= EDT_MAX_LINE && D <= EDT_MAX_LINE))
    return fail(WF_E_SHAPE, std::string(who) + ": supports W <= 4096 and D, H <= 512");
  return WF_OK;
}

extern "C" int64_t wf_surface_edt_workspace_bytes(int64_t M, int64_t D, int64_t H, int64_t W) {
  if (check_edt(__func__, M, D, H, W)) return -1;
  return align256(M * D * H * W * (int64_t)sizeof(uint32_t));  // the pass between x and z
}

extern "C" int wf_surface_edt_sq(const uint8_t* masks, int64_t M, int64_t D, int64_t H,
                                 int64_t W, uint8_t* border, uint32_t* d2, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  if (int rc = check_edt(__func__, M, D, H, W)) return rc;
  WF_REQUIRE_PTR(masks);
  WF_REQUIRE_PTR(border);
  WF_REQUIRE_PTR(d2);
  WF_REQUIRE_PTR(workspace);
  WF_REQUIRE(workspace_bytes >= wf_surface_edt_workspace_bytes(M, D, H, W),
             "workspace smaller than wf_surface_edt_workspace_bytes");
  const int64_t S = D * H * W, rows = M * D * H;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* mid = static_cast<uint32_t*>(workspace);
  hipLaunchKernelGGL(edt_x_kernel, dim3(grid_for(rows, 4, 16384)), dim3(256), 0, s, masks, border,
                     d2, (int)D, (int)H, (int)W, rows);
  const void* kern = reinterpret_cast<const void*>(edt_line_kernel);
  const unsigned gx = (unsigned)cdiv(W, 64);
  {  // along H: one block per (x tile, z, mask)
    const size_t lds = ((size_t)H * 64 + 64) * sizeof(uint32_t);
    if (lds > 64 * 1024) set_max_lds(kern, (int)lds);
    hipLaunchKernelGGL(edt_line_kernel, dim3(gx, (unsigned)D, (unsigned)M),
                       dim3(EDT_LINE_THREADS), lds, s, d2,
                       mid, (int)H, W, H * W, S, (int)W, 0);
  }
  {  // along D: one block per (x tile, y, mask)
    const size_t lds = ((size_t)D * 64 + 64) * sizeof(uint32_t);
    if (lds > 64 * 1024) set_max_lds(kern, (int)lds);
    hipLaunchKernelGGL(edt_line_kernel, dim3(gx, (unsigned)H, (unsigned)M),
                       dim3(EDT_LINE_THREADS), lds, s, mid,
                       d2, (int)D, H * W, W, S, (int)W, 1);
  }
  return check_launch("wf_surface_edt_sq");
}

extern "C" int wf_surface_hist(const uint8_t* border_a, const uint32_t* d2_b,
                               const uint8_t* border_b, const uint32_t* d2_a, int64_t P,
                               int64_t D, int64_t H, int64_t W, uint32_t* hist, void* stream) {
  WF_REQUIRE(P >= 1 && P <= 1024, "need 1 <= P <= 1024 pairs");
  if (int rc = check_volume(__func__, D, H, W)) return rc;
  WF_REQUIRE_PTR(border_a);
  WF_REQUIRE_PTR(d2_b);
  WF_REQUIRE_PTR(border_b);
  WF_REQUIRE_PTR(d2_a);
  WF_REQUIRE_PTR(hist);
  const int64_t S = D * H * W, nbins = D * D + H * H + W * W + 1;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)(P * 2 * nbins) * sizeof(uint32_t), s) != hipSuccess)
    return check_launch("wf_surface_hist (memset)");
  hipLaunchKernelGGL(surface_hist_kernel, dim3(grid_for(S, 256 * 16, 256), (unsigned)P, 2),
                     dim3(256), 0, s, border_a, d2_b, border_b, d2_a, S, (uint32_t)nbins, hist);
  return check_launch("wf_surface_hist");
}

extern "C" int wf_hist_order_stats(const uint32_t* hist, int64_t G, int64_t group,
                                   int64_t nbins, int64_t q_num, int64_t q_den,
                                   const int64_t* offsets, int64_t nranks, int64_t* out,
                                   void* stream) {
  WF_REQUIRE(G >= 1 && G <= 65535, "need 1 <= G <= 65535 histogram groups");
  WF_REQUIRE(group >= 1 && group <= 8, "need 1 <= group <= 8 histograms per group");
  WF_REQUIRE(nbins >= 1 && nbins <= ((int64_t)1 << 31), "need 1 <= nbins <= 2^31");
  WF_REQUIRE(nranks >= 0 && nranks <= 4, "at most 4 ranks");
  WF_REQUIRE(q_den >= 1 && q_num >= 0 && q_num <= q_den && q_den <= 1000000,
             "need 0 <= q_num <= q_den <= 10^6");
  WF_REQUIRE_PTR(hist);
  WF_REQUIRE_PTR(out);
  if (nranks > 0) WF_REQUIRE_PTR(offsets);
  OrderArgs a{};
  a.hist = hist;
  a.out = reinterpret_cast<long long*>(out);
  a.nbins = nbins;
  a.q_num = q_num;
  a.q_den = q_den;
  a.group = (int)group;
  a.nranks = (int)nranks;
  for (int i = 0; i < (int)nranks; ++i) a.off[i] = offsets[i];
  hipLaunchKernelGGL(hist_order_stats_kernel, dim3((unsigned)G), dim3(256), 0,
                     (hipStream_t)stream, a);
  return check_launch("wf_hist_order_stats");
}
