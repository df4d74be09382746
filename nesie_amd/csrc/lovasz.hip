// Lovasz-Softmax loss for gfx950 (semantics and formulas: include/nesie_ops.h).
//
// The reference (lovasz_loss.py:38-126) runs, per class, a descending torch.sort of the errors, a
// cumsum of the sorted labels, the difference jaccard[i] - jaccard[i - 1] and a dot product.  Here
// all segments (one per class, or per image and class) are served by one chain of launches on the
// primitives of index_sort.hip:
//   lv_key_kernel    entry j = segment * L + point: the error e = |fg - p| in fp32, its
//                    order-reversing integer key (larger error = smaller key; +inf / NaN = 0, a void
//                    point = the largest key) and the index j with the foreground flag in bit 31
//   ix_sort          stable, over all B * C * S entries by the 31-bit key (4 passes)
//   lv_segkey_kernel + ix_sort   one more stable 8-bit-a-pass sort by the segment number: every
//                    segment's entries are contiguous again, by error descending, ties by
//                    ascending point index (both sorts are stable and the entries start in it)
//   lv_count_kernel  foreground count of every tile of LV_TILE sorted entries
//   lv_carry_kernel  per segment: the tiles' counts -> their exclusive prefix, and G
//   lv_grad_kernel   block_excl inside the tile + the carry = cf_i; the Lovasz gradient g_i from
//                    the integer counts in double (no difference of two numbers near 1), the
//                    gradient scattered through the sorted index (one owner per element, no
//                    atomics) and the tile's sum of e_i * g_i in double
//   lv_finish_kernel the tiles' sums in a fixed order, the class mean and the image mean
// Nothing allocates, reads back or uses an atomic; the loss and the gradient have the same bits in
// every run.
#include "index_sort.h"

namespace nesie {

constexpr int LV_BLOCK = 256;
constexpr int LV_TILE = 1024;                    // sorted entries per workgroup: 256 threads x 4
constexpr unsigned LV_KEY_ZERO = 0x7F800000u;    // the key of e = 0; finite e > 0 lie below
constexpr unsigned LV_KEY_VOID = 0x7F800001u;    // a void point: after every valid one
constexpr unsigned LV_FG = 0x80000000u;          // bit 31 of the sorted index: foreground
enum { LV_ALL = 0, LV_PRESENT = 1, LV_MASK = 2 };

struct lv_problem {
  int images, classes, points;   // B, C, S
  int per_image;
  int nseg, seg_len, tiles;      // segments, entries per segment (L), tiles per segment
  const float *probas;
  long long sb, sc, ss;
  const long long *labels;
  int has_ignore;
  long long ignore;
  int class_mode;
  const int *class_mask;
};

// entry i of segment seg -> the element (b, c, s) it stands for
__device__ __forceinline__ void lv_where(const lv_problem &q, int seg, int i, int &b, int &c, int &s) {
  if (q.per_image) {
    b = seg / q.classes; c = seg - b * q.classes; s = i;
  } else {
    c = seg; b = i / q.points; s = i - b * q.points;
  }
}

__device__ __forceinline__ long long lv_offset(const lv_problem &q, int b, int c, int s) {
  return b * q.sb + c * q.sc + s * q.ss;
}

// how many times class c of a segment with G foreground points enters the class mean
__device__ __forceinline__ int lv_weight(const lv_problem &q, int c, int G) {
  if (q.class_mode == LV_ALL) return 1;
  if (q.class_mode == LV_PRESENT) return G > 0 ? 1 : 0;
  const int m = q.class_mask[c];
  return m > 0 ? m : 0;
}

__global__ __launch_bounds__(LV_BLOCK) void lv_key_kernel(lv_problem q, long long n,
                                                          unsigned *__restrict__ keys,
                                                          int *__restrict__ idx) {
  const long long j = (long long)blockIdx.x * LV_BLOCK + threadIdx.x;
  if (j >= n) return;
  const int seg = (int)((unsigned)j / (unsigned)q.seg_len), i = (int)(j - (long long)seg * q.seg_len);
  int b, c, s;
  lv_where(q, seg, i, b, c, s);
  const long long label = q.labels[(long long)b * q.points + s];
  const bool is_void = q.has_ignore && label == q.ignore;
  const bool fg = !is_void && label == (long long)c;
  const float p = q.probas[lv_offset(q, b, c, s)];
  const float e = fabsf((fg ? 1.f : 0.f) - p);
  const unsigned bits = __float_as_uint(e) & 0x7FFFFFFFu;
  unsigned key = bits < LV_KEY_ZERO ? LV_KEY_ZERO - bits : 0u;   // +inf and NaN: first
  if (is_void) key = LV_KEY_VOID;
  keys[j] = key;
  idx[j] = (int)((unsigned)j | (fg ? LV_FG : 0u));
}

__global__ __launch_bounds__(LV_BLOCK) void lv_segkey_kernel(long long n, int seg_len,
                                                             const int *idx_in, unsigned *keys,
                                                             int *idx_out) {
  const long long j = (long long)blockIdx.x * LV_BLOCK + threadIdx.x;
  if (j >= n) return;
  const int v = idx_in[j];
  keys[j] = ((unsigned)v & ~LV_FG) / (unsigned)seg_len;
  idx_out[j] = v;
}

__global__ __launch_bounds__(LV_BLOCK) void lv_count_kernel(int seg_len, int tiles,
                                                            const int *__restrict__ idx,
                                                            int *__restrict__ tile_count) {
  __shared__ int lds[LV_BLOCK / 64];
  const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
  const int pos0 = tile * LV_TILE + threadIdx.x * 4;
  const int *row = idx + (long long)seg * seg_len;
  int t = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (pos0 + k < seg_len) t += (unsigned)row[pos0 + k] >> 31;
  int total;
  block_excl<LV_BLOCK>(t, lds, total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// one workgroup per segment: tile_count becomes its exclusive prefix inside the segment
__global__ __launch_bounds__(LV_BLOCK) void lv_carry_kernel(int tiles, int *__restrict__ tile_count,
                                                            int *__restrict__ seg_fg) {
  __shared__ int lds[LV_BLOCK / 64];
  int *row = tile_count + (long long)blockIdx.x * tiles;
  int carry = 0;
  for (int t0 = 0; t0 < tiles; t0 += LV_BLOCK) {
    const int t = t0 + threadIdx.x;
    const int v = t < tiles ? row[t] : 0;
    int total;
    const int ex = block_excl<LV_BLOCK>(v, lds, total);
    if (t < tiles) row[t] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) seg_fg[blockIdx.x] = carry;
}

// the Lovasz gradient of the sorted entry with cf foreground entries up to and including it, `at`
// entries up to and including it, in a segment of G foreground entries
__device__ __forceinline__ double lv_g(bool fg, int G, int cf, int at) {
  const int U = G + (at - cf), I = G - cf;
  if (fg) return 1.0 / (double)U;
  if (U <= 1) return 1.0;                                  // G = 0 and the first entry
  return (double)I / ((double)U * (double)(U - 1));
}

__global__ __launch_bounds__(LV_BLOCK) void lv_grad_kernel(lv_problem q, const int *__restrict__ idx,
                                                           const int *__restrict__ tile_base,
                                                           const int *__restrict__ seg_fg,
                                                           float *__restrict__ grad,
                                                           double *__restrict__ tile_loss) {
  __shared__ int lds[LV_BLOCK / 64];
  __shared__ double sh[LV_BLOCK / 64];
  const int seg = blockIdx.x / q.tiles, tile = blockIdx.x - seg * q.tiles;
  const int image = q.per_image ? seg / q.classes : 0;
  const int cls = q.per_image ? seg - image * q.classes : seg;
  const int G = seg_fg[seg];
  // the divisor of this segment's mean: the averaged classes of its image (times the images)
  long long n = 0;
  for (int c = 0; c < q.classes; ++c) n += lv_weight(q, c, seg_fg[image * q.classes + c]);
  const int wgt = lv_weight(q, cls, G);
  const double scale =
      n > 0 ? (double)wgt / ((double)n * (double)(q.per_image ? q.images : 1)) : 0.0;

  const int pos0 = tile * LV_TILE + threadIdx.x * 4;
  const long long seg0 = (long long)seg * q.seg_len;
  int v[4], t = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = pos0 + k < q.seg_len ? idx[seg0 + pos0 + k] : 0;
    t += (unsigned)v[k] >> 31;
  }
  int total;
  int cf = tile_base[blockIdx.x] + block_excl<LV_BLOCK>(t, lds, total);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (pos0 + k >= q.seg_len) break;
    const bool fg = ((unsigned)v[k] >> 31) != 0;
    const long long i = (long long)((unsigned)v[k] & ~LV_FG) - seg0;
    if (i < 0 || i >= q.seg_len) continue;                 // never: the sorts keep a segment's entries
    int b, c, s;
    lv_where(q, seg, (int)i, b, c, s);
    const long long off = lv_offset(q, b, c, s);
    const bool is_void = q.has_ignore && q.labels[(long long)b * q.points + s] == q.ignore;
    if (is_void) {                                         // behind every valid entry: no prefix sees it
      grad[off] = 0.f;
      continue;
    }
    cf += fg ? 1 : 0;
    const double g = lv_g(fg, G, cf, pos0 + k + 1);
    const float e = fabsf((fg ? 1.f : 0.f) - q.probas[off]);
    acc += (double)e * g;
    grad[off] = (float)((fg ? -g : g) * scale);
  }
  const double sum = block_sum<LV_BLOCK>(acc, sh);
  if (threadIdx.x == 0) tile_loss[blockIdx.x] = sum;
}

// one workgroup: every segment's tiles in a fixed order, then the means, sequentially
__global__ __launch_bounds__(LV_BLOCK) void lv_finish_kernel(lv_problem q,
                                                             const int *__restrict__ seg_fg,
                                                             const double *__restrict__ tile_loss,
                                                             float *__restrict__ loss) {
  __shared__ double sh[LV_BLOCK / 64];
  double total = 0.0, image_sum = 0.0;
  long long image_n = 0;
  for (int seg = 0; seg < q.nseg; ++seg) {
    const double *row = tile_loss + (long long)seg * q.tiles;
    double acc = 0.0;
    for (int t = threadIdx.x; t < q.tiles; t += LV_BLOCK) acc += row[t];
    const double seg_loss = block_sum<LV_BLOCK>(acc, sh);
    const int cls = q.per_image ? seg % q.classes : seg;
    const int wgt = lv_weight(q, cls, seg_fg[seg]);
    if (wgt > 0) {                                         // a class left out: not even its NaN counts
      image_sum += (double)wgt * seg_loss;
      image_n += wgt;
    }
    if (cls == q.classes - 1) {                            // the last class of an image (or of all)
      if (image_n > 0) total += image_sum / (double)image_n;
      image_sum = 0.0;
      image_n = 0;
    }
  }
  if (threadIdx.x == 0) loss[0] = (float)(total / (double)(q.per_image ? q.images : 1));
}

struct lv_layout {
  long long n, sort_ints, count_ints, ints;   // ints: everything in front of the doubles, even
  size_t bytes;
};

// NESIE_OK with q and l filled; `go` = whether there is anything to launch
static int lv_check(const char *W, int images, int classes, long long points, int per_image,
                    int class_mode, lv_problem *q, lv_layout *l, bool *go) {
  NESIE_REQUIRE(images >= 0 && classes >= 0 && points >= 0, W);
  NESIE_REQUIRE(class_mode >= LV_ALL && class_mode <= LV_MASK, W);
  const long long segs = (long long)images * classes;          // < 2^62
  long long n = 0;
  bool too_many = false;
  if (segs > 0 && points > 0) {
    too_many = segs > IX_MAX_N || points > IX_MAX_N / segs;
    n = too_many ? 0 : segs * points;
  }
  if (too_many) {
    set_error("%s: %d x %d x %lld entries, at most %lld", W, images, classes, points, IX_MAX_N);
    return NESIE_ERR_UNSUPPORTED;
  }
  *go = n > 0;
  if (!*go) return NESIE_OK;
  q->images = images; q->classes = classes; q->points = (int)points;
  q->per_image = per_image ? 1 : 0;
  q->nseg = per_image ? (int)segs : classes;
  q->seg_len = (int)(n / q->nseg);
  q->tiles = cdiv(q->seg_len, LV_TILE);
  q->class_mode = class_mode;
  l->n = n;
  l->sort_ints = ix_carve(nullptr, n).ints;
  l->count_ints = (long long)q->nseg * q->tiles;
  l->ints = (l->sort_ints + l->count_ints + q->nseg + 1) & ~1LL;
  l->bytes = (size_t)l->ints * sizeof(int) + (size_t)l->count_ints * sizeof(double);
  return NESIE_OK;
}

}  // namespace nesie

using namespace nesie;

extern "C" size_t nesie_lovasz_softmax_workspace_bytes(int images, int classes, long long points) {
  lv_problem q;
  lv_layout l;
  bool go;
  // the per-image segmentation needs the most: B * C segments, and B * ceil(S / tile) tiles a class
  // where the other has ceil(B * S / tile)
  if (lv_check("lovasz_softmax_workspace_bytes", images, classes, points, 1, LV_ALL, &q, &l, &go) ||
      !go)
    return 0;
  return l.bytes;
}

extern "C" int nesie_lovasz_softmax(int images, int classes, long long points, const float *probas,
                                    long long stride_b, long long stride_c, long long stride_s,
                                    const long long *labels, int has_ignore, long long ignore,
                                    int per_image, int class_mode, const int *class_mask,
                                    float *loss, float *grad, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  const char *W = "lovasz_softmax";
  lv_problem q;
  lv_layout l;
  bool go;
  const int st = lv_check(W, images, classes, points, per_image, class_mode, &q, &l, &go);
  if (st || !go) return st;
  NESIE_REQUIRE(probas && labels && loss && grad, W);
  NESIE_REQUIRE(class_mode != LV_MASK || class_mask, W);
  NESIE_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, W);
  NESIE_REQUIRE(workspace_bytes >= nesie_lovasz_softmax_workspace_bytes(images, classes, points), W);
  q.probas = probas; q.sb = stride_b; q.sc = stride_c; q.ss = stride_s;
  q.labels = labels; q.has_ignore = has_ignore ? 1 : 0; q.ignore = ignore;
  q.class_mask = class_mask;
  hipStream_t s = (hipStream_t)stream;
  const IxWorkspace w = ix_carve(workspace, l.n);
  int *tile_count = (int *)workspace + l.sort_ints;
  int *seg_fg = tile_count + l.count_ints;
  double *tile_loss = (double *)((int *)workspace + l.ints);

  const unsigned flat = (unsigned)cdiv_ll(l.n, LV_BLOCK);
  hipLaunchKernelGGL(lv_key_kernel, dim3(flat), dim3(LV_BLOCK), 0, s, q, l.n, w.ka, w.ia);
  NESIE_LAUNCHED(W);
  const unsigned *keys;
  const int *idx;
  int e = ix_sort(W, l.n, LV_KEY_VOID, w, nullptr, &keys, &idx, s);
  if (e != NESIE_OK) return e;
  if (q.nseg > 1) {
    hipLaunchKernelGGL(lv_segkey_kernel, dim3(flat), dim3(LV_BLOCK), 0, s, l.n, q.seg_len, idx,
                       w.ka, w.ia);
    NESIE_LAUNCHED(W);
    e = ix_sort(W, l.n, q.nseg - 1, w, nullptr, &keys, &idx, s);
    if (e != NESIE_OK) return e;
  }
  const unsigned grid = (unsigned)l.count_ints;
  hipLaunchKernelGGL(lv_count_kernel, dim3(grid), dim3(LV_BLOCK), 0, s, q.seg_len, q.tiles, idx,
                     tile_count);
  NESIE_LAUNCHED(W);
  hipLaunchKernelGGL(lv_carry_kernel, dim3((unsigned)q.nseg), dim3(LV_BLOCK), 0, s, q.tiles,
                     tile_count, seg_fg);
  NESIE_LAUNCHED(W);
  hipLaunchKernelGGL(lv_grad_kernel, dim3(grid), dim3(LV_BLOCK), 0, s, q, idx,
                     (const int *)tile_count, (const int *)seg_fg, grad, tile_loss);
  NESIE_LAUNCHED(W);
  hipLaunchKernelGGL(lv_finish_kernel, dim3(1), dim3(LV_BLOCK), 0, s, q, (const int *)seg_fg,
                     (const double *)tile_loss, loss);
  return check_launch(W);
}
