// RoI-aware 3-D pooling for gfx950 (reference mmdet3d/ops/roiaware_pool3d/src/
// roiaware_pool3d_kernel.cu; include/nesie_ops.h states the pinned semantics).
//
// forward, two launches on the caller's stream, no allocation:
//   rap_collect_kernel  one workgroup per box walks the points in tiles of 256, in ascending
//                       order.  A lane tests its point (pib_test.h) and computes its voxel
//                       (:65-78).  A tile that holds an inside point ranks it among the tile's
//                       points of the same voxel (the tile's voxels and one ballot per wave sit
//                       in LDS; a lane visits the inside lanes only) on top of the voxel's
//                       running count, so slot order is ascending point index, the order of the
//                       reference's serial walk (:93-127).  One barrier per tile without an
//                       inside point, two with.  The counters live in LDS when the grid has at
//                       most RAP_LDS_VOX voxels, else in slot 0 itself.  The box's whole
//                       pts_idx_of_voxels block is cleared first by the same workgroup, and
//                       the membership row pts_voxel[box, :] (the voxel a point is KEPT in, else
//                       -1: the reference's pts_mask, :45-91, after the capacity rule) is written
//                       in full.  The box is blockIdx.x: no 65 535 limit.
//   rap_pool_kernel     one wave per voxel; lanes own channels (4 per lane, so C <= 256 reads the
//                       slot list once), the slot list is loaded 64 entries at a time into the
//                       lanes and broadcast, pts_feature rows are read coalesced along C.
// backward, one launch: a GATHER.  A wave owns 16 consecutive points and walks the boxes in
// ascending order reading pts_voxel rows, four boxes per load; for every membership found
// (ballot) the lanes turn to channels and add the voxel's grad_out row into the point's
// accumulator row (LDS, every cell private to one lane).  A point lies in at most one voxel per
// box, so ascending box IS ascending (box, voxel).  No float atomics; grad_in is written in full.
#include "pib_test.h"

namespace nesie {

constexpr int RAP_BLOCK = 256;
constexpr int RAP_LDS_VOX = 4096;   // voxels per box whose counters fit in LDS (16 KB)
constexpr int RAP_CT = 256;         // channels one pooling pass holds (4 per lane)
constexpr int RAP_BWD_PT = 16;      // points per backward wave
constexpr int RAP_BWD_CT = 128;     // channels per backward workgroup (16 x 128 fp32 = 8 KB LDS)

__device__ __forceinline__ int rap_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(RAP_BLOCK) void rap_collect_kernel(
    int pts_num, int ox, int oy, int oz, int m, const float *__restrict__ rois,
    const float *__restrict__ pts, int *__restrict__ idx, int *__restrict__ pts_voxel) {
  __shared__ PibBox sq;
  __shared__ int sv[2][RAP_BLOCK];
  __shared__ unsigned long long smask[2][RAP_BLOCK / 64];
  __shared__ int scnt[RAP_LDS_VOX];
  const int tid = threadIdx.x;
  const long long n = blockIdx.x;
  const int V = ox * oy * oz;  // <= 2^24
  int *vox = idx + n * V * m;
  int *row = pts_voxel ? pts_voxel + n * pts_num : nullptr;
  const float *r = rois + n * 7;
  const long long cells = (long long)V * m;
  for (long long i = tid; i < cells; i += RAP_BLOCK) vox[i] = 0;
  const bool lds = V <= RAP_LDS_VOX;
  if (lds)
    for (int i = tid; i < V; i += RAP_BLOCK) scnt[i] = 0;
  if (tid == 0) sq = pib_expand(r);
  __syncthreads();
  const PibBox q = sq;
  const float w = r[3], l = r[4], h = r[5], zb = r[2];
  const float x_res = __fdiv_rn(l, (float)ox), y_res = __fdiv_rn(w, (float)oy),
              z_res = __fdiv_rn(h, (float)oz);
  const float half_l = __fdiv_rn(l, 2.f), half_w = __fdiv_rn(w, 2.f);
  const int kept_max = m - 1;  // slot 0 is the counter

  const int lane = tid & 63, wave = tid >> 6;
  for (int p0 = 0, it = 0; p0 < pts_num; p0 += RAP_BLOCK, ++it) {
    const int p = p0 + tid;
    int v = -1;
    if (p < pts_num) {
      const float *pt = pts + (long long)p * 3;
      const float x = pt[0], y = pt[1], z = pt[2];
      float lx, ly;
      if (pib_inside(q, x, y, z, lx, ly)) {
        const int xi = rap_clamp((int)__fdiv_rn(__fadd_rn(lx, half_l), x_res), ox - 1);
        const int yi = rap_clamp((int)__fdiv_rn(__fadd_rn(ly, half_w), y_res), oy - 1);
        const int zi = rap_clamp((int)__fdiv_rn(__fsub_rn(z, zb), z_res), oz - 1);
        v = (xi * oy + yi) * oz + zi;
      }
    }
    // The tile's voxels and, per wave, which lanes are inside; two buffers by tile parity, so the
    // one barrier of the next tile also separates this tile's reads from the refill after it.
    int *tv = sv[it & 1];
    unsigned long long *tm = smask[it & 1];
    const unsigned long long bal = __ballot(v >= 0);
    tv[tid] = v;
    if (lane == 0) tm[wave] = bal;
    __syncthreads();  // (also orders the previous tile's counter updates before the reads below)
    if ((tm[0] | tm[1] | tm[2] | tm[3]) == 0) {
      if (row && p < pts_num) row[p] = -1;
      continue;
    }
    int slot = 0;
    bool last = true;
    if (v >= 0) {
      slot = lds ? scnt[v] : vox[(long long)v * m];
      for (int w = 0; w < RAP_BLOCK / 64; ++w) {
        unsigned long long mask = tm[w];
        while (mask) {
          const int j = w * 64 + __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          if (tv[j] == v) {
            slot += j < tid;
            last &= j <= tid;
          }
        }
      }
    }
    __syncthreads();  // every running count is read before any is advanced
    const bool kept = v >= 0 && slot < kept_max;
    if (kept) vox[(long long)v * m + 1 + slot] = p;
    if (v >= 0 && last) {
      if (lds) scnt[v] = slot + 1; else vox[(long long)v * m] = slot + 1;
    }
    if (row && p < pts_num) row[p] = kept ? v : -1;
  }
  __syncthreads();
  for (int i = tid; i < V; i += RAP_BLOCK) {
    const int c = lds ? scnt[i] : vox[(long long)i * m];
    vox[(long long)i * m] = c < kept_max ? c : kept_max;
  }
}

// MODE 0: max with strict > from -inf in slot order (:129-187), MODE 1: fp32 running sum in slot
// order divided by the count (:189-226).  argmax is written in both modes (0 in MODE 1, the state
// the reference's new_zeros leaves it in).
template <int MODE>
__global__ __launch_bounds__(RAP_BLOCK) void rap_pool_kernel(
    long long nvox, int c, int m, const float *__restrict__ feat, const int *__restrict__ idx,
    float *__restrict__ pooled, int *__restrict__ argmax) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (RAP_BLOCK / 64) + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * (RAP_BLOCK / 64);
  for (long long vx = wave; vx < nvox; vx += stride) {
    const int *sl = idx + vx * m;
    const int count = sl[0];
    for (int c0 = 0; c0 < c; c0 += RAP_CT) {
      float acc[4];
      int arg[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { acc[k] = MODE == 0 ? -INFINITY : 0.f; arg[k] = -1; }
      for (int s0 = 0; s0 < count; s0 += 64) {
        const int mine = s0 + lane < count ? sl[1 + s0 + lane] : 0;
        const int ns = count - s0 < 64 ? count - s0 : 64;
        for (int s = 0; s < ns; ++s) {
          const int pi = __shfl(mine, s, 64);
          const float *f = feat + (long long)pi * c + c0 + lane;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (c0 + lane + 64 * k < c) {
              const float val = f[64 * k];
              if (MODE == 0) {
                if (val > acc[k]) { acc[k] = val; arg[k] = pi; }
              } else {
                acc[k] = __fadd_rn(acc[k], val);
              }
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int cc = c0 + lane + 64 * k;
        if (cc < c) {
          const long long o = vx * c + cc;
          if (MODE == 0) {
            pooled[o] = arg[k] == -1 ? 0.f : acc[k];
            argmax[o] = arg[k];
          } else {
            pooled[o] = count > 0 ? __fdiv_rn(acc[k], (float)count) : 0.f;
            argmax[o] = 0;
          }
        }
      }
    }
  }
}

// grid (ceil(P / RAP_BWD_PT), ceil(C / RAP_BWD_CT)), one wave per workgroup; dynamic LDS
// RAP_BWD_PT * ct floats, ct = the channels of this tile rounded up to 64.  One load reads the
// table for RAP_BWD_PT points of 64 / RAP_BWD_PT consecutive boxes (lane = box * PT + point), so a
// ballot's bits are already in ascending box order.
template <int MODE>
__global__ __launch_bounds__(64) void rap_backward_kernel(
    int boxes_num, int pts_num, int V, int c, int m, int ct, const int *__restrict__ idx,
    const int *__restrict__ argmax, const int *__restrict__ pts_voxel,
    const float *__restrict__ grad_out, float *__restrict__ grad_in) {
  extern __shared__ float acc[];  // [PT points][ct], cell (b, k*64 + lane) touched by `lane` only
  constexpr int PT = RAP_BWD_PT, RPL = 64 / PT, U = 8;
  const int lane = threadIdx.x;
  const int p0 = blockIdx.x * PT;
  const int p = p0 + lane % PT, rl = lane / PT;
  const int c0 = blockIdx.y * RAP_BWD_CT;
  const int nk = ct / 64;
  for (int i = lane; i < PT * ct; i += 64) acc[i] = 0.f;
  for (int n0 = 0; n0 < boxes_num; n0 += U * RPL) {
    int v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = n0 + u * RPL + rl;
      v[u] = (n < boxes_num && p < pts_num) ? pts_voxel[(long long)n * pts_num + p] : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unsigned long long mask = __ballot(v[u] >= 0);
      while (mask) {
        const int i = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int vb = __shfl(v[u], i, 64);
        const int b = i % PT;
        const long long cell = (long long)(n0 + u * RPL + i / PT) * V + vb;
        float scale = 1.f;
        if (MODE == 1) {
          const int cnt = idx[cell * m];
          scale = __fdiv_rn(1.f, fmaxf((float)cnt, 1.f));
        }
        for (int k = 0; k < nk; ++k) {
          const int cc = c0 + k * 64 + lane;
          if (cc < c) {
            const long long o = cell * c + cc;
            float *a = acc + b * ct + k * 64 + lane;
            if (MODE == 0) {
              if (argmax[o] == p0 + b) *a = __fadd_rn(*a, grad_out[o]);
            } else {
              *a = __fadd_rn(*a, __fmul_rn(grad_out[o], scale));
            }
          }
        }
      }
    }
  }
  const int np = pts_num - p0 < PT ? pts_num - p0 : PT;
  for (int b = 0; b < np; ++b)
    for (int k = 0; k < nk; ++k) {
      const int cc = c0 + k * 64 + lane;
      if (cc < c) grad_in[(long long)(p0 + b) * c + cc] = acc[b * ct + k * 64 + lane];
    }
}

static int rap_check_sizes(const char *W, int boxes_num, int pts_num, int channels, int out_x,
                           int out_y, int out_z, int m) {
  NESIE_REQUIRE(boxes_num >= 0 && pts_num >= 0 && channels >= 0 && m >= 1, W);
  if (out_x < 1 || out_x > 256 || out_y < 1 || out_y > 256 || out_z < 1 || out_z > 256) {
    set_error("%s: out_size (%d, %d, %d) outside 1 .. 256", W, out_x, out_y, out_z);
    return NESIE_ERR_UNSUPPORTED;
  }
  return NESIE_OK;
}

static int rap_fill(const char *W, void *p, int byte, long long elems, hipStream_t s) {
  if (!p || elems <= 0) return NESIE_OK;
  if (hipMemsetAsync(p, byte, (size_t)elems * 4, s) != hipSuccess) return check_launch(W);
  return NESIE_OK;
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_roiaware_pool3d_sizes(int boxes_num, int pts_num, int channels, int out_x,
                                           int out_y, int out_z, int max_pts_each_voxel,
                                           long long *out) {
  const char *W = "roiaware_pool3d_sizes";
  const int st = rap_check_sizes(W, boxes_num, pts_num, channels, out_x, out_y, out_z,
                                 max_pts_each_voxel);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(out, W);
  const long long nvox = (long long)boxes_num * out_x * out_y * out_z;
  out[0] = nvox * max_pts_each_voxel;
  out[1] = nvox * channels;
  out[2] = (long long)boxes_num * pts_num;
  return NESIE_OK;
}

extern "C" int nesie_roiaware_pool3d_forward(int boxes_num, int pts_num, int channels,
                                             int max_pts_each_voxel, int out_x, int out_y,
                                             int out_z, const float *rois, const float *pts,
                                             const float *pts_feature, int *argmax,
                                             int *pts_idx_of_voxels, float *pooled_features,
                                             int *pts_voxel, int pool_method, void *stream) {
  const char *W = "roiaware_pool3d_forward";
  const int m = max_pts_each_voxel;
  const int st = rap_check_sizes(W, boxes_num, pts_num, channels, out_x, out_y, out_z, m);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(pool_method == 0 || pool_method == 1, W);
  hipStream_t s = (hipStream_t)stream;
  const long long nvox = (long long)boxes_num * out_x * out_y * out_z;
  if (boxes_num == 0 || pts_num == 0 || channels == 0) {  // no launch; what is not empty is cleared
    int e = rap_fill(W, pts_idx_of_voxels, 0, nvox * m, s);
    if (e == NESIE_OK) e = rap_fill(W, pooled_features, 0, nvox * channels, s);
    if (e == NESIE_OK) e = rap_fill(W, argmax, 0, nvox * channels, s);
    if (e == NESIE_OK) e = rap_fill(W, pts_voxel, 0xff, (long long)boxes_num * pts_num, s);
    return e;
  }
  NESIE_REQUIRE(rois && pts && pts_feature && argmax && pts_idx_of_voxels && pooled_features, W);
  hipLaunchKernelGGL(rap_collect_kernel, dim3(boxes_num), dim3(RAP_BLOCK), 0, s, pts_num, out_x,
                     out_y, out_z, m, rois, pts, pts_idx_of_voxels, pts_voxel);
  int e = check_launch(W);
  if (e != NESIE_OK) return e;
  const long long want = (nvox + RAP_BLOCK / 64 - 1) / (RAP_BLOCK / 64);
  const int grid = (int)(want < 16384 ? want : 16384);
  const bool built = with_int<0, 1>(pool_method, [&](auto MODE) {
    hipLaunchKernelGGL(rap_pool_kernel<MODE()>, dim3(grid), dim3(RAP_BLOCK), 0, s, nvox, channels, m, pts_feature,
                       pts_idx_of_voxels, pooled_features, argmax);
  });
  NESIE_REQUIRE(built, W);
  return check_launch(W);
}

extern "C" int nesie_roiaware_pool3d_backward(int boxes_num, int pts_num, int out_x, int out_y,
                                              int out_z, int channels, int max_pts_each_voxel,
                                              const int *pts_idx_of_voxels, const int *argmax,
                                              const int *pts_voxel, const float *grad_out,
                                              float *grad_in, int pool_method, void *stream) {
  const char *W = "roiaware_pool3d_backward";
  const int m = max_pts_each_voxel;
  const int st = rap_check_sizes(W, boxes_num, pts_num, channels, out_x, out_y, out_z, m);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(pool_method == 0 || pool_method == 1, W);
  hipStream_t s = (hipStream_t)stream;
  if (pts_num == 0 || channels == 0) return NESIE_OK;
  if (boxes_num == 0) return rap_fill(W, grad_in, 0, (long long)pts_num * channels, s);
  NESIE_REQUIRE(pts_idx_of_voxels && argmax && pts_voxel && grad_out && grad_in, W);
  const int tiles = cdiv(channels, RAP_BWD_CT);
  NESIE_REQUIRE(tiles <= 65535, W);
  const int ct = channels <= 64 ? 64 : RAP_BWD_CT;
  const dim3 grid(cdiv(pts_num, RAP_BWD_PT), tiles);
  const size_t lds = (size_t)RAP_BWD_PT * ct * sizeof(float);
  const int V = out_x * out_y * out_z;
  const bool built = with_int<0, 1>(pool_method, [&](auto MODE) {
    hipLaunchKernelGGL(rap_backward_kernel<MODE()>, grid, dim3(64), lds, s, boxes_num, pts_num, V, channels, m, ct,
                       pts_idx_of_voxels, argmax, pts_voxel, grad_out, grad_in);
  });
  NESIE_REQUIRE(built, W);
  return check_launch(W);
}
