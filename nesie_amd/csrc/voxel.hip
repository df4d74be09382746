// Voxel ops for gfx950: dynamic / hard voxelization and dynamic_scatter (reference
// mmdet3d/ops/voxel/src/{voxelization_cpu.cpp, voxelization_cuda.cu, scatter_points_cuda.cu};
// include/nesie_ops.h states the pinned semantics).
//
// One primitive serves the three sorted ops: a STABLE least-significant-digit radix sort of
// (cell key, point index) pairs, 8 bits a pass, the pass count fixed on the host by the bit length
// of `cells` (an out-of-range point carries the key `cells` and so sorts last).  A pass is
//   vx_hist_kernel     one workgroup per tile of VX_SORT_TILE keys: 256 LDS counters, integer LDS
//                      atomics (a count does not depend on their order), written digit-major
//                      hist[digit][tile]
//   vx_scan            exclusive scan of the 256 x tiles counters (below)
//   vx_scatter_kernel  the same tile again.  A wave owns 256 consecutive keys and takes them 64 at
//                      a time; a lane finds the lanes of its round with the same digit from eight
//                      ballots, its rank among them is a popcount, and the wave's running count
//                      per digit sits in LDS private to the wave (read by all, advanced by the
//                      highest lane of each group; no atomics assign a slot).  After one barrier a
//                      thread per digit stacks the four waves on the scanned tile base.  Order
//                      inside a digit is wave, round, lane = input order: the pass is stable.
// vx_scan: a two-level exclusive scan of ints for any length -- vx_scan_tiles (VX_SCAN_TILE
// elements per workgroup, tile totals out), vx_scan_sums (one workgroup walks the totals in chunks
// of 256 with a carry, so their number is unbounded) and vx_scan_add.
//
// After the sort a cell's points are contiguous in ascending point index and the cells are in key
// (= lexicographic) order.
//   hard voxelization  vx_first_kernel marks the first point of every cell in POINT order; the
//                      exclusive scan of the marks is the first-appearance ordinal;
//                      vx_hard_fill_kernel: a thread per sorted position looks back at most
//                      max_points keys for its rank, copies its row when rank < max_points and
//                      ordinal < max_voxels; the last kept point of a cell writes the count and the
//                      zero padding, the first the coordinates.
//   scatter forward    vx_head_kernel + scan (the voxel row of a sorted position), vx_seg_kernel
//                      (coors_map, voxel_coors, voxel_start), vx_reduce_kernel: one wave per voxel
//                      walks its segment in order, lanes over channels (rap_pool_kernel's shape).
//   scatter backward   sum / mean: a gather per element through coors_map; max: one wave per voxel
//                      walks the segment again, the first point equal to the maximum takes the
//                      gradient, every other row element is written 0; the invalid rows (the tail
//                      of `order`) are zeroed by the same launch.
// No float atomics, no allocation, every launch on the caller's stream.
#include <math.h>

#include "common.h"
#include "voxel_sort.h"

namespace nesie {

constexpr int VX_BLOCK = 256;
constexpr int VX_SCAN_TILE = 1024;  // ints per scan workgroup: 256 threads x 4
constexpr int VX_CT = 256;          // channels one reduce pass holds (4 per lane)

struct VxGrid {
  float lo[3], vs[3];
  int g[3];
};

// (c_x, c_y, c_z) of a point, false when out of range (NaN and +-inf quotients fail the compares)
__device__ __forceinline__ bool vx_cell(const VxGrid &g, const float *p, int *cell) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float f = floorf(__fdiv_rn(__fsub_rn(p[j], g.lo[j]), g.vs[j]));
    if (!(f >= 0.f && f < 2147483648.f)) return false;
    const int ci = (int)f;
    if (ci >= g.g[j]) return false;
    cell[j] = ci;
  }
  return true;
}

__global__ __launch_bounds__(VX_BLOCK) void vx_dynamic_kernel(long long n, int c, VxGrid g,
                                                              const float *__restrict__ points,
                                                              int *__restrict__ coors) {
  const long long i = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (i >= n) return;
  int cell[3];
  const bool ok = vx_cell(g, points + i * c, cell);
  coors[i * 3 + 0] = ok ? cell[2] : -1;
  coors[i * 3 + 1] = ok ? cell[1] : -1;
  coors[i * 3 + 2] = ok ? cell[0] : -1;
}

__global__ __launch_bounds__(VX_BLOCK) void vx_point_keys_kernel(long long n, int c, VxGrid g,
                                                                 unsigned cells,
                                                                 const float *__restrict__ points,
                                                                 unsigned *__restrict__ keys,
                                                                 int *__restrict__ idx) {
  const long long i = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (i >= n) return;
  int cell[3];
  const bool ok = vx_cell(g, points + i * c, cell);
  keys[i] = ok ? (unsigned)((cell[2] * g.g[1] + cell[1]) * g.g[0] + cell[0]) : cells;
  idx[i] = (int)i;
}

__global__ __launch_bounds__(VX_BLOCK) void vx_coor_keys_kernel(long long n, int d0, int d1, int d2,
                                                                unsigned cells,
                                                                const int *__restrict__ coors,
                                                                unsigned *__restrict__ keys,
                                                                int *__restrict__ idx) {
  const long long i = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int a = coors[i * 3], b = coors[i * 3 + 1], e = coors[i * 3 + 2];
  const bool ok = a >= 0 && a < d0 && b >= 0 && b < d1 && e >= 0 && e < d2;
  keys[i] = ok ? (unsigned)((a * d1 + b) * d2 + e) : cells;
  idx[i] = (int)i;
}

// ---- radix sort pass
__global__ __launch_bounds__(VX_BLOCK) void vx_hist_kernel(long long n, int shift, long long nb,
                                                           const unsigned *__restrict__ keys,
                                                           int *__restrict__ hist) {
  __shared__ int h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * VX_SORT_TILE;
#pragma unroll
  for (int k = 0; k < VX_SORT_TILE / VX_BLOCK; ++k) {
    const long long i = base + k * VX_BLOCK + tid;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[(long long)tid * nb + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__(VX_BLOCK) void vx_scatter_kernel(
    long long n, int shift, long long nb, const unsigned *__restrict__ kin,
    const int *__restrict__ iin, unsigned *__restrict__ kout, int *__restrict__ iout,
    const int *__restrict__ hist) {
  constexpr int W = VX_BLOCK / 64, R = VX_SORT_TILE / VX_BLOCK;
  __shared__ int wcnt[W][256];
  __shared__ int off[W][256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < W * 256; i += VX_BLOCK) (&wcnt[0][0])[i] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * VX_SORT_TILE + w * (R * 64);
  volatile int *mine = wcnt[w];
  unsigned key[R];
  int id[R], rank[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = base + r * 64 + lane;
    const bool valid = i < n;
    key[r] = valid ? kin[i] : 0u;
    id[r] = valid ? iin[i] : 0;
    const unsigned d = (key[r] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    // the wave's count of digit d before this round: every lane of the group reads it, then the
    // group's highest lane advances it (LDS serves one wave's accesses in program order)
    const int before = mine[d];
    rank[r] = before + __popcll(peers & ((1ull << lane) - 1ull));
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers >> lane) == 1ull) mine[d] = before + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    int run = hist[(long long)tid * nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      off[k][tid] = run;
      run += wcnt[k][tid];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = base + r * 64 + lane;
    if (i < n) {
      const int dst = off[w][(key[r] >> shift) & 255u] + rank[r];
      kout[dst] = key[r];
      iout[dst] = id[r];
    }
  }
}

// ---- exclusive scan of ints
// exclusive prefix of t over the workgroup's 256 threads; total in every thread.  lds: 4 ints.
__device__ __forceinline__ int vx_block_excl(int t, int *lds, int &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int wbase = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < VX_BLOCK / 64; ++k) {
    const int s = lds[k];
    if (k < w) wbase += s;
    total += s;
  }
  __syncthreads();
  return wbase + inc - t;
}

__global__ __launch_bounds__(VX_BLOCK) void vx_scan_tiles_kernel(long long n,
                                                                 const int *in, int *out,
                                                                 int *__restrict__ sums) {
  __shared__ int lds[VX_BLOCK / 64];
  const long long i0 = (long long)blockIdx.x * VX_SCAN_TILE + threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
  int total;
  int run = vx_block_excl(v[0] + v[1] + v[2] + v[3], lds, total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the tile totals become their exclusive prefix; the grand total goes to *total
// and, when given, min(total, cap) to *capped
__global__ __launch_bounds__(VX_BLOCK) void vx_scan_sums_kernel(long long nt, int *__restrict__ sums,
                                                                int *__restrict__ total_out,
                                                                int *__restrict__ capped, int cap) {
  __shared__ int lds[VX_BLOCK / 64];
  int carry = 0;
  for (long long b = 0; b < nt; b += VX_BLOCK) {
    const long long i = b + threadIdx.x;
    const int v = i < nt ? sums[i] : 0;
    int total;
    const int ex = vx_block_excl(v, lds, total);
    if (i < nt) sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (total_out) *total_out = carry;
    if (capped) *capped = carry < cap ? carry : cap;
  }
}

__global__ __launch_bounds__(VX_BLOCK) void vx_scan_add_kernel(long long n, int *__restrict__ out,
                                                               const int *__restrict__ sums) {
  const long long i0 = (long long)blockIdx.x * VX_SCAN_TILE + threadIdx.x * 4;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < n) out[i0 + k] += add;
}

// ---- hard voxelization
// first[i] = 1 iff point i is the first of its cell (the head of a sorted segment: the sort is stable)
__global__ __launch_bounds__(VX_BLOCK) void vx_first_kernel(long long n, unsigned cells,
                                                            const unsigned *__restrict__ keys,
                                                            const int *__restrict__ idx,
                                                            int *__restrict__ first) {
  const long long j = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (j >= n) return;
  const unsigned k = keys[j];
  first[idx[j]] = k != cells && (j == 0 || keys[j - 1] != k);
}

__global__ __launch_bounds__(VX_BLOCK) void vx_hard_fill_kernel(
    long long n, int c, unsigned cells, int gx, int gy, int max_points, int max_voxels,
    const unsigned *__restrict__ keys, const int *__restrict__ idx, const int *__restrict__ ordinal,
    const float *__restrict__ points, float *__restrict__ voxels, int *__restrict__ coors,
    int *__restrict__ num) {
  const long long j = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (j >= n) return;
  const unsigned k = keys[j];
  if (k == cells) return;
  int r = 0;
  while (r < max_points && j - r - 1 >= 0 && keys[j - r - 1] == k) ++r;
  if (r >= max_points) return;  // the cell is full
  const long long v = ordinal[idx[j - r]];
  if (v >= max_voxels) return;  // the cell came after the cap
  const float *src = points + (long long)idx[j] * c;
  float *row = voxels + (v * max_points + r) * c;
  for (int ch = 0; ch < c; ++ch) row[ch] = src[ch];
  if (r == 0) {
    const int cx = (int)(k % (unsigned)gx), cy = (int)((k / (unsigned)gx) % (unsigned)gy);
    const int cz = (int)(k / ((unsigned)gx * (unsigned)gy));
    coors[v * 3 + 0] = cz;
    coors[v * 3 + 1] = cy;
    coors[v * 3 + 2] = cx;
  }
  const bool last = j == n - 1 || keys[j + 1] != k;
  if (last) {
    num[v] = r + 1;
    const long long pad = (long long)(max_points - 1 - r) * c;
    for (long long e = 0; e < pad; ++e) row[c + e] = 0.f;
  } else if (r == max_points - 1) {
    num[v] = max_points;
  }
}

// ---- dynamic_scatter
__global__ __launch_bounds__(VX_BLOCK) void vx_head_kernel(long long n, unsigned cells,
                                                           const unsigned *__restrict__ keys,
                                                           int *__restrict__ head) {
  const long long j = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (j >= n) return;
  const unsigned k = keys[j];
  head[j] = k != cells && (j == 0 || keys[j - 1] != k);
}

// heads_before[j] = heads among sorted positions < j.  *nvalid = the valid (sorted-first) points.
__global__ __launch_bounds__(VX_BLOCK) void vx_seg_kernel(
    long long n, unsigned cells, const unsigned *__restrict__ keys, const int *__restrict__ order,
    const int *__restrict__ heads_before, const int *__restrict__ coors,
    int *__restrict__ coors_map, int *__restrict__ voxel_coors, int *__restrict__ voxel_start,
    int *__restrict__ nvalid) {
  const long long j = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (j >= n) return;
  const unsigned k = keys[j];
  const long long i = order[j];
  if (k == cells) {
    coors_map[i] = -1;
    if (j == 0 || keys[j - 1] != cells) *nvalid = (int)j;
    return;
  }
  if (j == n - 1) *nvalid = (int)n;
  const bool head = j == 0 || keys[j - 1] != k;
  const long long v = heads_before[j] + (head ? 0 : -1);
  coors_map[i] = (int)v;
  if (head) {
    voxel_start[v] = (int)j;
    voxel_coors[v * 3 + 0] = coors[i * 3 + 0];
    voxel_coors[v * 3 + 1] = coors[i * 3 + 1];
    voxel_coors[v * 3 + 2] = coors[i * 3 + 2];
  }
}

// MODE 0 sum, 1 mean, 2 max.  One wave per voxel, lanes over channels, the segment in order.
template <int MODE>
__global__ __launch_bounds__(VX_BLOCK) void vx_reduce_kernel(
    int c, const float *__restrict__ feats, const int *__restrict__ order,
    const int *__restrict__ voxel_start, const int *__restrict__ num_voxels,
    const int *__restrict__ nvalid, float *__restrict__ voxel_feats,
    int *__restrict__ reduce_count) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (VX_BLOCK / 64) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (VX_BLOCK / 64);
  const long long m = *num_voxels;
  for (long long v = wave; v < m; v += stride) {
    const int s = voxel_start[v];
    const int e = v + 1 < m ? voxel_start[v + 1] : *nvalid;
    const int count = e - s;
    if (lane == 0) reduce_count[v] = count;
    for (int c0 = 0; c0 < c; c0 += VX_CT) {
      float acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = MODE == 2 ? -INFINITY : 0.f;
      for (int s0 = s; s0 < e; s0 += 64) {
        const int mine = s0 + lane < e ? order[s0 + lane] : 0;
        const int ns = e - s0 < 64 ? e - s0 : 64;
        for (int t = 0; t < ns; ++t) {
          const int pi = __shfl(mine, t, 64);
          const float *f = feats + (long long)pi * c + c0 + lane;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (c0 + lane + 64 * k < c) {
              const float val = f[64 * k];
              if (MODE == 2) acc[k] = val > acc[k] ? val : acc[k];
              else acc[k] = __fadd_rn(acc[k], val);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int cc = c0 + lane + 64 * k;
        if (cc < c)
          voxel_feats[v * c + cc] = MODE == 1 ? __fdiv_rn(acc[k], (float)count) : acc[k];
      }
    }
  }
}

template <int MODE>  // 0 sum, 1 mean
__global__ __launch_bounds__(VX_BLOCK) void vx_backward_add_kernel(
    long long total, int c, const float *__restrict__ grad_voxel, const int *__restrict__ coors_map,
    const int *__restrict__ reduce_count, float *__restrict__ grad_feats) {
  const long long e = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (e >= total) return;
  const long long i = e / c;
  const int ch = (int)(e - i * c);
  const long long v = coors_map[i];
  float g = 0.f;
  if (v >= 0) {
    g = grad_voxel[v * c + ch];
    if (MODE == 1) g = __fdiv_rn(g, (float)reduce_count[v]);
  }
  grad_feats[e] = g;
}

__global__ __launch_bounds__(VX_BLOCK) void vx_backward_max_kernel(
    long long n, int c, const float *__restrict__ grad_voxel, const float *__restrict__ feats,
    const float *__restrict__ voxel_feats, const int *__restrict__ order,
    const int *__restrict__ voxel_start, const int *__restrict__ reduce_count,
    const int *__restrict__ num_voxels, float *__restrict__ grad_feats) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (VX_BLOCK / 64) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (VX_BLOCK / 64);
  const long long m = *num_voxels;
  for (long long v = wave; v < m; v += stride) {
    const int s = voxel_start[v];
    const int e = s + reduce_count[v];
    for (int c0 = 0; c0 < c; c0 += VX_CT) {
      float top[4], g[4];
      bool open[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int cc = c0 + lane + 64 * k;
        open[k] = cc < c;
        top[k] = open[k] ? voxel_feats[v * c + cc] : 0.f;
        g[k] = open[k] ? grad_voxel[v * c + cc] : 0.f;
      }
      for (int s0 = s; s0 < e; s0 += 64) {
        const int mine = s0 + lane < e ? order[s0 + lane] : 0;
        const int ns = e - s0 < 64 ? e - s0 : 64;
        for (int t = 0; t < ns; ++t) {
          const int pi = __shfl(mine, t, 64);
          const long long o = (long long)pi * c + c0 + lane;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (c0 + lane + 64 * k < c) {
              const bool take = open[k] && feats[o + 64 * k] == top[k];
              grad_feats[o + 64 * k] = take ? g[k] : 0.f;
              if (take) open[k] = false;
            }
          }
        }
      }
    }
  }
  // the invalid rows: the tail of the sorted order
  const long long nv = m > 0 ? (long long)voxel_start[m - 1] + reduce_count[m - 1] : 0;
  for (long long j = nv + wave; j < n; j += stride) {
    float *row = grad_feats + (long long)order[j] * c;
    for (int ch = lane; ch < c; ch += 64) row[ch] = 0.f;
  }
}

// ---- host side
static long long vx_cdiv(long long a, long long b) { return (a + b - 1) / b; }

VxWorkspace vx_carve(void *ws, long long n) {
  VxWorkspace w;
  w.nb = vx_cdiv(n, VX_SORT_TILE);
  const long long hist = 256 * w.nb;
  const long long sums = vx_cdiv(hist > n ? hist : n, VX_SCAN_TILE) + 1;
  int *p = (int *)ws;
  w.ka = (unsigned *)p; p += n;
  w.kb = (unsigned *)p; p += n;
  w.ia = p; p += n;
  w.ib = p; p += n;
  w.flag = p; p += n;
  w.hist = p; p += hist;
  w.sums = p; p += sums;
  w.meta = p; p += 4;
  w.ints = 5 * n + hist + sums + 4;
  return w;
}

int vx_check_n_cells(const char *W, long long n, long long cells) {
  NESIE_REQUIRE(n >= 0, W);
  if (cells < 1 || cells >= 2147483648LL) {
    set_error("%s: %lld cells outside 1 .. 2^31 - 1", W, cells);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (n > VX_MAX_N) {
    set_error("%s: %lld points, at most %lld", W, n, VX_MAX_N);
    return NESIE_ERR_UNSUPPORTED;
  }
  return NESIE_OK;
}

// grid[j] = roundf((hi - lo) / vs) in fp32; every grid[j] >= 1 and the product below 2^31
static int vx_grid(const char *W, const float *voxel_size, const float *coors_range, VxGrid &g,
                   long long &cells) {
  NESIE_REQUIRE(voxel_size && coors_range, W);
  cells = 1;
  for (int j = 0; j < 3; ++j) {
    const float extent = coors_range[3 + j] - coors_range[j];
    const float q = extent / voxel_size[j];
    const float r = roundf(q);
    if (!(r >= 1.f && r < 2147483648.f)) {
      set_error("%s: grid size %g along axis %d outside 1 .. 2^31 - 1", W, (double)r, j);
      return NESIE_ERR_UNSUPPORTED;
    }
    g.lo[j] = coors_range[j];
    g.vs[j] = voxel_size[j];
    g.g[j] = (int)r;
    cells *= g.g[j];
    if (cells >= 2147483648LL) {
      set_error("%s: the grid has 2^31 cells or more", W);
      return NESIE_ERR_UNSUPPORTED;
    }
  }
  return NESIE_OK;
}

#define VX_LAUNCHED(W)                      \
  do {                                      \
    const int e_ = check_launch(W);         \
    if (e_ != NESIE_OK) return e_;          \
  } while (0)

// out may alias in.  total_out / capped: see vx_scan_sums_kernel
int vx_scan(const char *W, long long n, const int *in, int *out, int *sums, int *total_out,
            int *capped, int cap, hipStream_t s) {
  const long long nt = vx_cdiv(n, VX_SCAN_TILE);
  hipLaunchKernelGGL(vx_scan_tiles_kernel, dim3((unsigned)nt), dim3(VX_BLOCK), 0, s, n, in, out,
                     sums);
  VX_LAUNCHED(W);
  hipLaunchKernelGGL(vx_scan_sums_kernel, dim3(1), dim3(VX_BLOCK), 0, s, nt, sums, total_out,
                     capped, cap);
  VX_LAUNCHED(W);
  if (nt > 1) {
    hipLaunchKernelGGL(vx_scan_add_kernel, dim3((unsigned)nt), dim3(VX_BLOCK), 0, s, n, out, sums);
    VX_LAUNCHED(W);
  }
  return NESIE_OK;
}

static int vx_passes(long long cells) {  // keys lie in 0 .. cells
  int bits = 0;
  while ((cells >> bits) != 0) ++bits;
  return (bits + 7) / 8;
}

// sorts (w.ka, w.ia) by key; the sorted keys end in *keys, the indices in *idx (`last_idx` when
// given receives the indices of the last pass directly)
int vx_sort(const char *W, long long n, long long cells, const VxWorkspace &w, int *last_idx,
            const unsigned **keys, const int **idx, hipStream_t s) {
  const int passes = vx_passes(cells);
  unsigned *const kbuf[2] = {w.ka, w.kb};
  int *const ibuf[2] = {w.ia, w.ib};
  int *iout = w.ia;
  for (int p = 0; p < passes; ++p) {
    const int src = p & 1, dst = src ^ 1;
    const int *iin = iout;
    iout = (p == passes - 1 && last_idx) ? last_idx : ibuf[dst];
    hipLaunchKernelGGL(vx_hist_kernel, dim3((unsigned)w.nb), dim3(VX_BLOCK), 0, s, n, 8 * p, w.nb,
                       kbuf[src], w.hist);
    VX_LAUNCHED(W);
    const int e = vx_scan(W, 256 * w.nb, w.hist, w.hist, w.sums, nullptr, nullptr, 0, s);
    if (e != NESIE_OK) return e;
    hipLaunchKernelGGL(vx_scatter_kernel, dim3((unsigned)w.nb), dim3(VX_BLOCK), 0, s, n, 8 * p,
                       w.nb, kbuf[src], iin, kbuf[dst], iout, w.hist);
    VX_LAUNCHED(W);
  }
  *keys = kbuf[passes & 1];
  *idx = iout;
  return NESIE_OK;
}

static int vx_zero_int(const char *W, int *p, hipStream_t s) {
  if (p && hipMemsetAsync(p, 0, sizeof(int), s) != hipSuccess) return check_launch(W);
  return NESIE_OK;
}

static unsigned vx_wave_grid(long long n) {
  const long long want = vx_cdiv(n, VX_BLOCK / 64);
  return (unsigned)(want < 16384 ? want : 16384);
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_voxel_grid_size(const float *voxel_size, const float *coors_range, int *grid,
                                     long long *cells) {
  const char *W = "voxel_grid_size";
  NESIE_REQUIRE(grid && cells, W);
  VxGrid g;
  const int st = vx_grid(W, voxel_size, coors_range, g, *cells);
  if (st != NESIE_OK) return st;
  for (int j = 0; j < 3; ++j) grid[j] = g.g[j];
  return NESIE_OK;
}

extern "C" int nesie_voxel_workspace_bytes(long long n, long long cells, long long *out) {
  const char *W = "voxel_workspace_bytes";
  const int st = vx_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(out, W);
  *out = vx_carve(nullptr, n).ints * (long long)sizeof(int);
  return NESIE_OK;
}

extern "C" int nesie_dynamic_voxelize(long long n, int c, const float *points,
                                      const float *voxel_size, const float *coors_range,
                                      int *coors, void *stream) {
  const char *W = "dynamic_voxelize";
  NESIE_REQUIRE(n >= 0 && c >= 0, W);
  VxGrid g;
  long long cells;
  int st = vx_grid(W, voxel_size, coors_range, g, cells);
  if (st == NESIE_OK) st = vx_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  if (n == 0) return NESIE_OK;
  NESIE_REQUIRE(c >= 3, W);
  NESIE_REQUIRE(points && coors, W);
  hipLaunchKernelGGL(vx_dynamic_kernel, dim3((unsigned)vx_cdiv(n, VX_BLOCK)), dim3(VX_BLOCK), 0,
                     (hipStream_t)stream, n, c, g, points, coors);
  return check_launch(W);
}

extern "C" int nesie_hard_voxelize(long long n, int c, const float *points, const float *voxel_size,
                                   const float *coors_range, int max_points, int max_voxels,
                                   float *voxels, int *coors, int *num_points_per_voxel,
                                   int *voxel_num, void *workspace, void *stream) {
  const char *W = "hard_voxelize";
  NESIE_REQUIRE(n >= 0 && c >= 0 && max_points >= 1 && max_voxels >= 1, W);
  VxGrid g;
  long long cells;
  int st = vx_grid(W, voxel_size, coors_range, g, cells);
  if (st == NESIE_OK) st = vx_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(voxel_num, W);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || c == 0) return vx_zero_int(W, voxel_num, s);
  NESIE_REQUIRE(c >= 3, W);
  NESIE_REQUIRE(points && voxels && coors && num_points_per_voxel && workspace, W);
  const VxWorkspace w = vx_carve(workspace, n);
  const unsigned pts_grid = (unsigned)vx_cdiv(n, VX_BLOCK);
  hipLaunchKernelGGL(vx_point_keys_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, c, g,
                     (unsigned)cells, points, w.ka, w.ia);
  VX_LAUNCHED(W);
  const unsigned *keys;
  const int *idx;
  st = vx_sort(W, n, cells, w, nullptr, &keys, &idx, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_first_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, (unsigned)cells,
                     keys, idx, w.flag);
  VX_LAUNCHED(W);
  st = vx_scan(W, n, w.flag, w.flag, w.sums, nullptr, voxel_num, max_voxels, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_hard_fill_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, c,
                     (unsigned)cells, g.g[0], g.g[1], max_points, max_voxels, keys, idx, w.flag,
                     points, voxels, coors, num_points_per_voxel);
  return check_launch(W);
}

extern "C" int nesie_dynamic_scatter_forward(long long n, int c, const float *feats,
                                             const int *coors, const int *dims, int reduce_type,
                                             float *voxel_feats, int *voxel_coors, int *coors_map,
                                             int *reduce_count, int *num_voxels, int *order,
                                             int *voxel_start, void *workspace, void *stream) {
  const char *W = "dynamic_scatter_forward";
  NESIE_REQUIRE(n >= 0 && c >= 0 && reduce_type >= 0 && reduce_type <= 2, W);
  NESIE_REQUIRE(dims, W);
  long long cells = 1;
  for (int j = 0; j < 3; ++j) {
    if (dims[j] < 1 || (cells *= dims[j]) >= 2147483648LL) {
      set_error("%s: dims (%d, %d, %d): each must be >= 1 and the product below 2^31", W, dims[0],
                dims[1], dims[2]);
      return NESIE_ERR_UNSUPPORTED;
    }
  }
  int st = vx_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(num_voxels, W);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || c == 0) return vx_zero_int(W, num_voxels, s);
  NESIE_REQUIRE(feats && coors && voxel_feats && voxel_coors && coors_map && reduce_count &&
                    order && voxel_start && workspace, W);
  const VxWorkspace w = vx_carve(workspace, n);
  const unsigned pts_grid = (unsigned)vx_cdiv(n, VX_BLOCK);
  hipLaunchKernelGGL(vx_coor_keys_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, dims[0],
                     dims[1], dims[2], (unsigned)cells, coors, w.ka, w.ia);
  VX_LAUNCHED(W);
  const unsigned *keys;
  const int *idx;
  st = vx_sort(W, n, cells, w, order, &keys, &idx, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_head_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, (unsigned)cells,
                     keys, w.flag);
  VX_LAUNCHED(W);
  st = vx_scan(W, n, w.flag, w.flag, w.sums, num_voxels, nullptr, 0, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_seg_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, (unsigned)cells, keys,
                     order, w.flag, coors, coors_map, voxel_coors, voxel_start, w.meta);
  VX_LAUNCHED(W);
  const dim3 grid(vx_wave_grid(n)), block(VX_BLOCK);
  if (reduce_type == 0)
    hipLaunchKernelGGL(vx_reduce_kernel<0>, grid, block, 0, s, c, feats, order, voxel_start,
                       num_voxels, w.meta, voxel_feats, reduce_count);
  else if (reduce_type == 1)
    hipLaunchKernelGGL(vx_reduce_kernel<1>, grid, block, 0, s, c, feats, order, voxel_start,
                       num_voxels, w.meta, voxel_feats, reduce_count);
  else
    hipLaunchKernelGGL(vx_reduce_kernel<2>, grid, block, 0, s, c, feats, order, voxel_start,
                       num_voxels, w.meta, voxel_feats, reduce_count);
  return check_launch(W);
}

extern "C" int nesie_dynamic_scatter_backward(long long n, int c, const float *grad_voxel,
                                              const float *feats, const float *voxel_feats,
                                              const int *coors_map, const int *reduce_count,
                                              const int *order, const int *voxel_start,
                                              const int *num_voxels, int reduce_type,
                                              float *grad_feats, void *stream) {
  const char *W = "dynamic_scatter_backward";
  NESIE_REQUIRE(n >= 0 && c >= 0 && reduce_type >= 0 && reduce_type <= 2, W);
  if (n > VX_MAX_N) {
    set_error("%s: %lld points, at most %lld", W, n, VX_MAX_N);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (n == 0 || c == 0) return NESIE_OK;
  NESIE_REQUIRE(grad_voxel && coors_map && reduce_count && grad_feats, W);
  hipStream_t s = (hipStream_t)stream;
  const long long total = n * c;
  const dim3 block(VX_BLOCK);
  if (reduce_type == 2) {
    NESIE_REQUIRE(feats && voxel_feats && order && voxel_start && num_voxels, W);
    hipLaunchKernelGGL(vx_backward_max_kernel, dim3(vx_wave_grid(n)), block, 0, s, n, c,
                       grad_voxel, feats, voxel_feats, order, voxel_start, reduce_count,
                       num_voxels, grad_feats);
    return check_launch(W);
  }
  const long long blocks = vx_cdiv(total, VX_BLOCK);
  if (blocks > 2147483647LL) {
    set_error("%s: %lld x %d elements are more than one launch covers", W, n, c);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (reduce_type == 0)
    hipLaunchKernelGGL(vx_backward_add_kernel<0>, dim3((unsigned)blocks), block, 0, s, total, c,
                       grad_voxel, coors_map, reduce_count, grad_feats);
  else
    hipLaunchKernelGGL(vx_backward_add_kernel<1>, dim3((unsigned)blocks), block, 0, s, total, c,
                       grad_voxel, coors_map, reduce_count, grad_feats);
  return check_launch(W);
}
