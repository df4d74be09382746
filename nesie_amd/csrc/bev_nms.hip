// BEV non-maximum suppression of iou3d_cuda.nms_gpu / nms_normal_gpu (ops/iou3d/src/
// iou3d_kernel.cu:244-345, host walk iou3d.cpp:95-200) over S independent segments at once
// (one segment per class in merge_aug_bboxes_3d).  Three launches, no host round trip:
//   1. rank:  one workgroup per (segment, 64-row block); the rank of a box is the number of
//             boxes of its segment that come before it (descending score, equal scores by
//             ascending index, NaN after every number, boxes with valid == 0 after those), and
//             the boxes are scattered to their sorted positions
//   2. mask:  one wave per (segment, 64-row block, 64-column block) of the upper triangle:
//             bit j of word (row, cb) <=> iou(row, 64 cb + j) > thr, as nms_kernel /
//             nms_normal_kernel build it
//   3. walk:  one wave per segment runs the greedy `remv` pass of iou3d.cpp on the device
// The rotated IoU takes its overlap from bev_overlap.h, the function behind
// nesie_boxes_overlap_bev.
#include "bev_overlap.h"
#include "common.h"

namespace nesie {

constexpr int BNMS_MAX_SEG = 8192;              // boxes per segment
constexpr int BNMS_RANK_BLOCK = 256;            // 4 waves share the columns of 64 rows
constexpr int BNMS_WALK_ROWS = 16;              // kept rows whose mask words load together

__device__ __forceinline__ void seg_bounds(const int *offsets, int s, int n, int &beg, int &len) {
  int b = offsets[s], e = offsets[s + 1];
  b = b < 0 ? 0 : (b > n ? n : b);
  e = e < b ? b : (e > n ? n : e);
  beg = b;
  len = e - b;
}

// ascending key: (class, descending score bits); class 0 = a number, 1 = NaN, 2 = not valid
__device__ __forceinline__ unsigned long long order_key(float s, bool ok) {
  if (!ok) return 2ull << 32;
  if (s != s) return 1ull << 32;
  if (s == 0.f) s = 0.f;                        // -0 ties with +0, as in a float compare
  const unsigned u = __float_as_uint(s);
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (unsigned long long)(~asc);
}

__global__ __launch_bounds__(BNMS_RANK_BLOCK) void bev_nms_rank_kernel(
    int n, int max_seg, const float *__restrict__ boxes, const float *__restrict__ scores,
    const uint8_t *__restrict__ valid, const int *__restrict__ offsets,
    float *__restrict__ sboxes, int *__restrict__ order) {
  __shared__ unsigned long long tile_key[BNMS_RANK_BLOCK];
  __shared__ int part_rank[BNMS_RANK_BLOCK];
  int beg, len;
  seg_bounds(offsets, blockIdx.y, n, beg, len);
  const int r0 = blockIdx.x * 64;
  if (len > max_seg || r0 >= len) return;       // uniform across the workgroup
  const int tid = threadIdx.x, row = tid & 63, part = tid >> 6;
  const bool live = r0 + row < len;
  const int i = beg + (live ? r0 + row : 0);
  const unsigned long long ki = order_key(scores[i], valid ? valid[i] != 0 : true);
  int rank = 0;
  for (int c0 = 0; c0 < len; c0 += BNMS_RANK_BLOCK) {
    __syncthreads();
    const int c = c0 + tid;
    if (c < len) {
      const int j = beg + c;
      tile_key[tid] = order_key(scores[j], valid ? valid[j] != 0 : true);
    }
    __syncthreads();
    const int cn = len - c0 < BNMS_RANK_BLOCK ? len - c0 : BNMS_RANK_BLOCK;
    const int jb = part * 64, je = jb + 64 < cn ? jb + 64 : cn;
    for (int jj = jb; jj < je; ++jj) {
      const unsigned long long kj = tile_key[jj];
      rank += (kj < ki) || (kj == ki && beg + c0 + jj < i);
    }
  }
  part_rank[tid] = rank;
  __syncthreads();
  if (part == 0 && live) {
    const int r = beg + part_rank[row] + part_rank[row + 64] + part_rank[row + 128] +
                  part_rank[row + 192];
    order[r] = i;
#pragma unroll
    for (int q = 0; q < 5; ++q) sboxes[(size_t)r * 5 + q] = boxes[(size_t)i * 5 + q];
  }
}

struct AaBox { float x1, y1, x2, y2; };

// iou_bev (iou3d_kernel.cu:244-250) on prepared rectangles
__device__ __forceinline__ float iou_rotated(const Rect &a, float sa, const Rect &b, float sb) {
  const float ov = bev_overlap(a, b);
  return __fdiv_rn(ov, fmaxf(__fsub_rn(__fadd_rn(sa, sb), ov), 1e-8f));
}

// iou_normal (iou3d_kernel.cu:335-343): axis-aligned, ry ignored
__device__ __forceinline__ float iou_aligned(const AaBox &a, float sa, const AaBox &b, float sb) {
  const float left = fmaxf(a.x1, b.x1), right = fminf(a.x2, b.x2);
  const float top = fmaxf(a.y1, b.y1), bottom = fminf(a.y2, b.y2);
  const float width = fmaxf(__fsub_rn(right, left), 0.f);
  const float height = fmaxf(__fsub_rn(bottom, top), 0.f);
  const float inter = __fmul_rn(width, height);
  return __fdiv_rn(inter, fmaxf(__fsub_rn(__fadd_rn(sa, sb), inter), 1e-8f));
}

__device__ __forceinline__ float box_area(const float *b) {
  return __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1]));
}

template <bool ROTATED>
__global__ __launch_bounds__(64) void bev_nms_mask_kernel(
    int n, int max_seg, int words, const float *__restrict__ sboxes,
    const int *__restrict__ order, const uint8_t *__restrict__ valid,
    const int *__restrict__ offsets, float thr, unsigned long long *__restrict__ mask) {
  __shared__ Rect col_rect[ROTATED ? 64 : 1];
  __shared__ AaBox col_box[64];
  __shared__ float col_area[64];
  __shared__ unsigned char col_ok[64];
  const int cb = blockIdx.x, rb = blockIdx.y;
  if (cb < rb) return;
  int beg, len;
  seg_bounds(offsets, blockIdx.z, n, beg, len);
  const int r0 = rb * 64, c0 = cb * 64;
  if (len > max_seg || c0 >= len) return;
  // sorted order puts the boxes with valid == 0 last: a block whose first row is one of them
  // holds no row the walk can keep
  if (valid && !valid[order[beg + r0]]) return;
  const int t = threadIdx.x;
  const int cn = len - c0 < 64 ? len - c0 : 64;
  if (t < cn) {
    const float *b = sboxes + (size_t)(beg + c0 + t) * 5;
    col_box[t] = AaBox{b[0], b[1], b[2], b[3]};
    col_area[t] = box_area(b);
    col_ok[t] = valid ? (valid[order[beg + c0 + t]] != 0) : 1;
    if (ROTATED) load_rect(b, col_rect[t]);
  }
  __syncthreads();
  const int row = r0 + t;
  if (row >= len) return;
  if (valid && !valid[order[beg + row]]) return;
  const float *b = sboxes + (size_t)(beg + row) * 5;
  const float sa = box_area(b);
  unsigned long long bits = 0ull;
  const int start = rb == cb ? t + 1 : 0;
  if (ROTATED) {
    Rect a;
    load_rect(b, a);
    for (int j = start; j < cn; ++j)
      if (col_ok[j] && iou_rotated(a, sa, col_rect[j], col_area[j]) > thr) bits |= 1ull << j;
  } else {
    const AaBox a{b[0], b[1], b[2], b[3]};
    for (int j = start; j < cn; ++j)
      if (col_ok[j] && iou_aligned(a, sa, col_box[j], col_area[j]) > thr) bits |= 1ull << j;
  }
  mask[(size_t)(beg + row) * words + cb] = bits;
}

// The greedy pass of iou3d.cpp:134-150 for one segment.  Lane l holds words l and l + 64 of
// `remv`.  Per block of 64 sorted boxes: the diagonal words resolve the picks inside the block
// (one shuffle per box), then the kept rows' later words are OR-ed in, BNMS_WALK_ROWS rows
// per round so that their loads overlap (the walk is latency-bound: one wave per segment).
__global__ __launch_bounds__(64) void bev_nms_walk_kernel(
    int n, int max_seg, int words, const int *__restrict__ order,
    const uint8_t *__restrict__ valid, const int *__restrict__ offsets,
    const unsigned long long *__restrict__ mask, int *__restrict__ keep, int *__restrict__ count) {
  const int s = blockIdx.x, lane = threadIdx.x;
  int beg, len;
  seg_bounds(offsets, s, n, beg, len);
  if (len > max_seg) {
    if (lane == 0) count[s] = -1;
    return;
  }
  int nvalid = len;
  if (valid) {
    nvalid = 0;
    for (int c = 0; c < len; c += 64) {
      const bool ok = c + lane < len && valid[beg + c + lane] != 0;
      nvalid += __popcll(__ballot(ok));
    }
  }
  const int nw = (nvalid + 63) >> 6;
  unsigned long long rem0 = 0ull, rem1 = 0ull;
  int np = 0;
  for (int blk = 0; blk < nw; ++blk) {
    const int t0 = blk * 64;
    const int row = t0 + lane;
    const unsigned long long diag =
        row < nvalid ? mask[(size_t)(beg + row) * words + blk] : 0ull;
    unsigned long long cur = __shfl(blk < 64 ? rem0 : rem1, blk & 63, 64);
    if (nvalid - t0 < 64) cur |= ~0ull << (nvalid - t0);   // past the valid boxes
    unsigned long long picked = 0ull;
    for (int j = 0; j < 64; ++j) {
      const unsigned long long dj = __shfl(diag, j, 64);
      if (!((cur >> j) & 1ull)) {
        picked |= 1ull << j;
        cur |= dj;
      }
    }
    if ((picked >> lane) & 1ull)
      keep[beg + np + __popcll(picked & ((1ull << lane) - 1ull))] = order[beg + row];
    np += __popcll(picked);
    const bool own0 = lane > blk && lane < nw;
    const bool own1 = lane + 64 > blk && lane + 64 < nw;
    while (picked) {
      int r[BNMS_WALK_ROWS];
#pragma unroll
      for (int q = 0; q < BNMS_WALK_ROWS; ++q) {
        r[q] = picked ? t0 + __builtin_ctzll(picked) : -1;
        picked &= picked - 1ull;
      }
      unsigned long long w0[BNMS_WALK_ROWS], w1[BNMS_WALK_ROWS];
#pragma unroll
      for (int q = 0; q < BNMS_WALK_ROWS; ++q) {
        const size_t base = (size_t)(beg + (r[q] < 0 ? 0 : r[q])) * words;
        w0[q] = (r[q] >= 0 && own0) ? mask[base + lane] : 0ull;
        w1[q] = (r[q] >= 0 && own1) ? mask[base + lane + 64] : 0ull;
      }
#pragma unroll
      for (int q = 0; q < BNMS_WALK_ROWS; ++q) { rem0 |= w0[q]; rem1 |= w1[q]; }
    }
  }
  if (lane == 0) count[s] = np;
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_bev_nms(int n, int s, int max_seg, const float *boxes, const float *scores,
                             const uint8_t *valid, const int *offsets, float thr, int rotated,
                             int *keep, int *count, void *workspace, size_t workspace_bytes,
                             void *stream) {
  const char *W = "bev_nms";
  NESIE_REQUIRE(n >= 0 && s >= 0 && max_seg >= 0, W);
  if (max_seg > BNMS_MAX_SEG) {
    set_error("%s: max_seg = %d boxes per segment, built for <= %d", W, max_seg, BNMS_MAX_SEG);
    return NESIE_ERR_INVALID_ARG;
  }
  NESIE_REQUIRE(s <= 65535, W);
  if (s == 0) return NESIE_OK;
  NESIE_REQUIRE(count, W);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 || max_seg == 0) {
    zero_i32(count, s, st);
    return check_launch(W);
  }
  NESIE_REQUIRE(boxes && scores && offsets && keep && workspace, W);
  const int words = cdiv(max_seg, 64);
  const size_t need = (size_t)n * (8 * (size_t)words + 24);
  NESIE_REQUIRE(workspace_bytes >= need, W);
  // workspace: mask (n, words) u64 | sorted boxes (n, 5) f32 | order (n) i32
  unsigned long long *mask = (unsigned long long *)workspace;
  float *sboxes = (float *)(mask + (size_t)n * words);
  int *order = (int *)(sboxes + (size_t)n * 5);
  hipLaunchKernelGGL(bev_nms_rank_kernel, dim3(words, s), dim3(BNMS_RANK_BLOCK), 0, st, n,
                     max_seg, boxes, scores, valid, offsets, sboxes, order);
  with_bool(rotated, [&](auto ROT) {
    hipLaunchKernelGGL(bev_nms_mask_kernel<ROT()>, dim3(words, words, s), dim3(64), 0, st, n, max_seg, words,
                       sboxes, order, valid, offsets, thr, mask);
  });
  hipLaunchKernelGGL(bev_nms_walk_kernel, dim3(s), dim3(64), 0, st, n, max_seg, words, order,
                     valid, offsets, mask, keep, count);
  return check_launch(W);
}
