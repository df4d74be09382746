// Voxel ops for gfx950: dynamic / hard voxelization and dynamic_scatter (reference
// mmdet3d/ops/voxel/src/{voxelization_cpu.cpp, voxelization_cuda.cu, scatter_points_cuda.cu};
// include/nesie_ops.h states the pinned semantics).
//
// One primitive serves the three sorted ops: the stable radix sort of index_sort.hip (ix_sort) on
// (cell key, point index) pairs; an out-of-range point carries the key `cells` and so sorts last.
// The scans are ix_scan, the any-length exclusive scan of the same unit.
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
#include "index_sort.h"

namespace nesie {

constexpr int VX_BLOCK = 256;
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

static int vx_zero_int(const char *W, int *p, hipStream_t s) {
  if (p && hipMemsetAsync(p, 0, sizeof(int), s) != hipSuccess) return check_launch(W);
  return NESIE_OK;
}

static unsigned vx_wave_grid(long long n) {
  const long long want = cdiv_ll(n, VX_BLOCK / 64);
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
  const int st = ix_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(out, W);
  *out = ix_carve(nullptr, n).ints * (long long)sizeof(int);
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
  if (st == NESIE_OK) st = ix_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  if (n == 0) return NESIE_OK;
  NESIE_REQUIRE(c >= 3, W);
  NESIE_REQUIRE(points && coors, W);
  hipLaunchKernelGGL(vx_dynamic_kernel, dim3((unsigned)cdiv_ll(n, VX_BLOCK)), dim3(VX_BLOCK), 0,
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
  if (st == NESIE_OK) st = ix_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(voxel_num, W);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || c == 0) return vx_zero_int(W, voxel_num, s);
  NESIE_REQUIRE(c >= 3, W);
  NESIE_REQUIRE(points && voxels && coors && num_points_per_voxel && workspace, W);
  const IxWorkspace w = ix_carve(workspace, n);
  const unsigned pts_grid = (unsigned)cdiv_ll(n, VX_BLOCK);
  hipLaunchKernelGGL(vx_point_keys_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, c, g,
                     (unsigned)cells, points, w.ka, w.ia);
  NESIE_LAUNCHED(W);
  const unsigned *keys;
  const int *idx;
  st = ix_sort(W, n, cells, w, nullptr, &keys, &idx, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_first_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, (unsigned)cells,
                     keys, idx, w.flag);
  NESIE_LAUNCHED(W);
  st = ix_scan(W, n, w.flag, w.flag, w.sums, nullptr, voxel_num, max_voxels, s);
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
  int st = ix_check_n_cells(W, n, cells);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(num_voxels, W);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0 || c == 0) return vx_zero_int(W, num_voxels, s);
  NESIE_REQUIRE(feats && coors && voxel_feats && voxel_coors && coors_map && reduce_count &&
                    order && voxel_start && workspace, W);
  const IxWorkspace w = ix_carve(workspace, n);
  const unsigned pts_grid = (unsigned)cdiv_ll(n, VX_BLOCK);
  hipLaunchKernelGGL(vx_coor_keys_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, dims[0],
                     dims[1], dims[2], (unsigned)cells, coors, w.ka, w.ia);
  NESIE_LAUNCHED(W);
  const unsigned *keys;
  const int *idx;
  st = ix_sort(W, n, cells, w, order, &keys, &idx, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_head_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, (unsigned)cells,
                     keys, w.flag);
  NESIE_LAUNCHED(W);
  st = ix_scan(W, n, w.flag, w.flag, w.sums, num_voxels, nullptr, 0, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(vx_seg_kernel, dim3(pts_grid), dim3(VX_BLOCK), 0, s, n, (unsigned)cells, keys,
                     order, w.flag, coors, coors_map, voxel_coors, voxel_start, w.meta);
  NESIE_LAUNCHED(W);
  const dim3 grid(vx_wave_grid(n)), block(VX_BLOCK);
  const bool built = with_int<0, 1, 2>(reduce_type, [&](auto RT) {
    hipLaunchKernelGGL(vx_reduce_kernel<RT()>, grid, block, 0, s, c, feats, order, voxel_start, num_voxels, w.meta,
                       voxel_feats, reduce_count);
  });
  NESIE_REQUIRE(built, W);
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
  if (n > IX_MAX_N) {
    set_error("%s: %lld points, at most %lld", W, n, IX_MAX_N);
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
  const long long blocks = cdiv_ll(total, VX_BLOCK);
  if (blocks > 2147483647LL) {
    set_error("%s: %lld x %d elements are more than one launch covers", W, n, c);
    return NESIE_ERR_UNSUPPORTED;
  }
  const bool built = with_int<0, 1>(reduce_type, [&](auto RT) {   // (2 has left above)
    hipLaunchKernelGGL(vx_backward_add_kernel<RT()>, dim3((unsigned)blocks), block, 0, s, total, c, grad_voxel,
                       coors_map, reduce_count, grad_feats);
  });
  NESIE_REQUIRE(built, W);
  return check_launch(W);
}
