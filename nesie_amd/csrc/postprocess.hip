// Inference post-processing and evaluation geometry for gfx950:
//   * aligned_3d_nms        -- core/post_processing/box3d_nms.py:129-176, batched over scenes
//   * points_in_boxes_count -- the `box_indices.T.sum(1) > 5` of NesieHead.multiclass_nms_single
//                              (dense_heads/nesie_head.py:740-750) without the (M, T) table
//   * boxes_overlap_bev     -- ops/iou3d/src/iou3d_kernel.cu:127-264 (rotated BEV overlap of
//                              BaseInstance3DBoxes.overlaps, base_box3d.py:387-438)
// The reference runs the NMS as a python loop of ~10 torch launches per pick and per scene;
// here one workgroup per scene sorts, builds the K x K suppression bit matrix in LDS and
// walks it once.
#include "bev_overlap.h"
#include "pib_test.h"

namespace nesie {

// ---- aligned_3d_nms -----------------------------------------------------------------
// Candidate order: ascending (score, index), read from the end -- a stable
// torch.argsort(scores) (the reference's own sort leaves equal scores unordered).
// Box u leaves the list when a picked box t before it has NOT (iou(t,u) * same <= thr), in
// fp32 with the reference's operation order; NaN (0/0 of two degenerate boxes) fails `<=`
// and therefore removes u, as in the reference.
constexpr int NMS_MAX_K = 512;
constexpr int NMS_BLOCK = 256;

struct NmsBox { float x1, y1, z1, x2, y2, z2, area; int cls; };

__global__ __launch_bounds__(NMS_BLOCK) void aligned_nms_kernel(
    int k, const float *__restrict__ boxes, const float *__restrict__ scores,
    const int *__restrict__ classes, const uint8_t *__restrict__ valid, float thr,
    int *__restrict__ picks, int *__restrict__ count) {
  __shared__ NmsBox sb[NMS_MAX_K];            // candidates, best first
  __shared__ int src[NMS_MAX_K];              // their positions in the input
  __shared__ float sc[NMS_MAX_K];
  __shared__ unsigned char ok[NMS_MAX_K];
  __shared__ unsigned long long sup[NMS_MAX_K * (NMS_MAX_K / 64)];
  __shared__ int n_live;
  const int bi = blockIdx.x, tid = threadIdx.x;
  boxes += (size_t)bi * k * 6;
  scores += (size_t)bi * k;
  classes += (size_t)bi * k;
  if (valid) valid += (size_t)bi * k;
  picks += (size_t)bi * k;
  if (tid == 0) n_live = 0;
  for (int i = tid; i < k; i += NMS_BLOCK) {
    const float s0 = scores[i];
    sc[i] = s0 != s0 ? INFINITY : s0;   // NaN sorts last, as in torch.argsort
    ok[i] = valid ? (valid[i] != 0) : 1;
    picks[i] = -1;
  }
  __syncthreads();
  // rank = number of live candidates that come before me (greater (score, index))
  for (int i = tid; i < k; i += NMS_BLOCK) {
    if (!ok[i]) continue;
    const float s = sc[i];
    int r = 0;
    for (int j = 0; j < k; ++j) r += ok[j] && (sc[j] > s || (sc[j] == s && j > i));
    const float *bx = boxes + (size_t)i * 6;
    NmsBox q;
    q.x1 = bx[0]; q.y1 = bx[1]; q.z1 = bx[2]; q.x2 = bx[3]; q.y2 = bx[4]; q.z2 = bx[5];
    q.area = __fmul_rn(__fmul_rn(__fsub_rn(q.x2, q.x1), __fsub_rn(q.y2, q.y1)),
                       __fsub_rn(q.z2, q.z1));
    q.cls = classes[i];
    sb[r] = q;
    src[r] = i;
    atomicAdd(&n_live, 1);
  }
  __syncthreads();
  const int n = n_live;
  const int words = (n + 63) >> 6;
  // suppression matrix: bit u of row t <=> t removes u (u after t)
  for (int w = tid; w < n * words; w += NMS_BLOCK) {
    const int t = w / words, u0 = (w % words) << 6;
    const NmsBox a = sb[t];
    unsigned long long bits = 0ull;
    const int uend = n - u0 < 64 ? n - u0 : 64;
    for (int j = 0; j < uend; ++j) {
      const int u = u0 + j;
      if (u <= t) continue;
      const NmsBox q = sb[u];
      const float l = fmaxf(0.f, __fsub_rn(fminf(a.x2, q.x2), fmaxf(a.x1, q.x1)));
      const float wd = fmaxf(0.f, __fsub_rn(fminf(a.y2, q.y2), fmaxf(a.y1, q.y1)));
      const float h = fmaxf(0.f, __fsub_rn(fminf(a.z2, q.z2), fmaxf(a.z1, q.z1)));
      const float inter = __fmul_rn(__fmul_rn(l, wd), h);
      float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(a.area, q.area), inter));
      iou = __fmul_rn(iou, a.cls == q.cls ? 1.f : 0.f);
      if (!(iou <= thr)) bits |= 1ull << j;
    }
    sup[w] = bits;
  }
  __syncthreads();
  // greedy walk by the first wave: lane w owns word w of the removed set
  if (tid < 64) {
    unsigned long long removed = 0ull;
    int np = 0;
    for (int t = 0; t < n; ++t) {
      const unsigned long long word = __shfl(removed, t >> 6, 64);
      if ((word >> (t & 63)) & 1ull) continue;   // uniform across the wave
      if (tid == 0) picks[np] = src[t];
      ++np;
      if (tid < words) removed |= sup[t * words + tid];
    }
    if (tid == 0) count[bi] = np;
  }
}

// ---- points_in_boxes_count ------------------------------------------------------------
// The inside-test of points_in_boxes.hip (pib_test.h; points_in_boxes_cuda.cu:24-49), LiDAR-frame
// boxes; counts[b, t] = number of the scene's points inside box t.
constexpr int PIC_BLOCK = 256;
constexpr int PIC_TILE = 256;

__global__ __launch_bounds__(PIC_BLOCK) void points_in_boxes_count_kernel(
    int boxes_num, int pts_num, const float *__restrict__ boxes,
    const float *__restrict__ pts, int *__restrict__ counts) {
  __shared__ PibBox sb[PIC_TILE];
  __shared__ int cnt[PIC_TILE];
  const int bi = blockIdx.y;
  const int p = blockIdx.x * PIC_BLOCK + threadIdx.x;
  const bool live = p < pts_num;
  boxes += (size_t)bi * boxes_num * 7;
  const float *pt = pts + ((size_t)bi * pts_num + (live ? p : pts_num - 1)) * 3;
  const float x = pt[0], y = pt[1], z = pt[2];
  for (int t0 = 0; t0 < boxes_num; t0 += PIC_TILE) {
    const int tn = boxes_num - t0 < PIC_TILE ? boxes_num - t0 : PIC_TILE;
    __syncthreads();
    for (int k = threadIdx.x; k < tn; k += PIC_BLOCK) {
      sb[k] = pib_expand(boxes + (size_t)(t0 + k) * 7);
      cnt[k] = 0;
    }
    __syncthreads();
    for (int k = 0; k < tn; ++k) {
      const bool in = live && pib_inside(sb[k], x, y, z);
      const unsigned long long m = __ballot(in);
      if (m && (threadIdx.x & 63) == 0) atomicAdd(&cnt[k], __popcll(m));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < tn; k += PIC_BLOCK)
      if (cnt[k]) atomicAdd(&counts[(size_t)bi * boxes_num + t0 + k], cnt[k]);
  }
}

// ---- rotated BEV overlap (bev_overlap.h) ---------------------------------------------------
__global__ __launch_bounds__(64) void boxes_overlap_bev_kernel(
    int num_a, const float *__restrict__ boxes_a, int num_b, const float *__restrict__ boxes_b,
    float *__restrict__ out) {
  const long long pair = (long long)blockIdx.x * 64 + threadIdx.x;
  if (pair >= (long long)num_a * num_b) return;
  const int ia = (int)(pair / num_b), ib = (int)(pair % num_b);
  Rect A, B;
  load_rect(boxes_a + (size_t)ia * 5, A);
  load_rect(boxes_b + (size_t)ib * 5, B);
  out[pair] = bev_overlap(A, B);
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_aligned_3d_nms(int b, int k, const float *boxes, const float *scores,
                                    const int *classes, const uint8_t *valid, float thr,
                                    int *picks, int *count, void *stream) {
  const char *W = "aligned_3d_nms";
  NESIE_REQUIRE(b >= 0 && k >= 0, W);
  if (b == 0) return NESIE_OK;
  NESIE_REQUIRE(count, W);
  if (k > NMS_MAX_K) {
    set_error("%s: k = %d boxes per scene, built for <= %d", W, k, NMS_MAX_K);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (k == 0) {
    zero_i32(count, b, (hipStream_t)stream);
    return check_launch(W);
  }
  NESIE_REQUIRE(boxes && scores && classes && picks, W);
  hipLaunchKernelGGL(aligned_nms_kernel, dim3(b), dim3(NMS_BLOCK), 0, (hipStream_t)stream, k,
                     boxes, scores, classes, valid, thr, picks, count);
  return check_launch(W);
}

extern "C" int nesie_points_in_boxes_count(int b, int boxes_num, int pts_num,
                                           const float *boxes, const float *pts, int *counts,
                                           void *stream) {
  const char *W = "points_in_boxes_count";
  NESIE_REQUIRE(b >= 0 && boxes_num >= 0 && pts_num >= 0, W);
  if (b == 0 || boxes_num == 0) return NESIE_OK;
  NESIE_REQUIRE(counts, W);
  zero_i32(counts, b * boxes_num, (hipStream_t)stream);   // (the count kernel adds into it)
  if (pts_num == 0) return NESIE_OK;
  NESIE_REQUIRE(boxes && pts && b <= 65535, W);
  hipLaunchKernelGGL(points_in_boxes_count_kernel, dim3(cdiv(pts_num, PIC_BLOCK), b),
                     dim3(PIC_BLOCK), 0, (hipStream_t)stream, boxes_num, pts_num, boxes, pts,
                     counts);
  return check_launch(W);
}

extern "C" int nesie_boxes_overlap_bev(int num_a, const float *boxes_a, int num_b,
                                       const float *boxes_b, float *ans_overlap, void *stream) {
  const char *W = "boxes_overlap_bev";
  NESIE_REQUIRE(num_a >= 0 && num_b >= 0, W);
  if (num_a == 0 || num_b == 0) return NESIE_OK;
  NESIE_REQUIRE(boxes_a && boxes_b && ans_overlap, W);
  const long long pairs = (long long)num_a * num_b;
  NESIE_REQUIRE(pairs / 64 + 1 < (1ll << 31), W);
  hipLaunchKernelGGL(boxes_overlap_bev_kernel, dim3((unsigned)cdiv(pairs, 64)), dim3(64), 0,
                     (hipStream_t)stream, num_a, boxes_a, num_b, boxes_b, ans_overlap);
  return check_launch(W);
}
