// Sigmoid focal loss for gfx950 (semantics and formulas: include/nesie_ops.h).
//
// mmcv's sigmoid_focal_loss_{forward,backward}_cuda_kernel run one thread per element, form
// 1 - sigmoid(x) by subtraction, clamp the logarithm's argument at FLT_MIN and index the class
// weight with the label whatever it is.  Here both directions are built on
//   softplus(v) = max(v, 0) + log1p(exp(-|v|))
// so nothing is subtracted, no power of a difference is taken and nothing is clamped: every finite
// logit gives a finite loss and gradient, accurate to a few ulp relative in both tails.
//
// One kernel body serves the three modes.  The flat index over (N, C) is cut into chunks of
// FL_CHUNK = 4096 elements, one workgroup each; a thread owns FL_ITEMS runs of four consecutive
// elements (one 16-byte load of the logits, one 16-byte store), FL_BLOCK * 4 elements apart.  C is
// rarely a multiple of four, so the row of a run's first element comes from one 32-bit division
// and the column then walks with a wrap.  Which thread owns which element depends on the flat
// index alone; the scalar lanes (VEC = false: a base that is not 16-byte aligned) keep the same
// assignment and differ only in the width of the accesses.
//
//   FL_NONE   loss[i]   = term * class weight * sample weight * scale
//   FL_SUM    a thread adds its 16 terms in ascending index, the 64 lanes of a wave and then the
//             four waves fold in a fixed butterfly; chunk p's sum goes to partial[p], and a second
//             launch of one workgroup adds the partials (thread t: p = t, t + 256, ... ascending,
//             then the same butterfly) and multiplies by the scale.  A single chunk writes the
//             scaled scalar itself: one launch.  The order is a function of N * C only.
//   FL_GRAD   grad_x[i] = d term/dx * class weight * sample weight * upstream
//             with upstream = grad_out[i] * scale or the scalar *grad_scalar * scale.
#include <math.h>

#include "common.h"

namespace nesie {

constexpr int FL_BLOCK = 256;
constexpr int FL_ITEMS = 4;                        // 16-byte runs per thread
constexpr int FL_CHUNK = FL_BLOCK * FL_ITEMS * 4;  // elements per workgroup

enum { FL_NONE = 0, FL_SUM = 1, FL_GRAD = 2 };

struct fl_problem {
  unsigned total;   // n * c < 2^31
  int n, c;
  const float *x;
  const long long *target;
  const float *class_weight;    // (C,) or null
  const float *sample_weight;   // (N,), (N, C) or null
  int sw_mode;                  // 0 none, 1 per row, 2 per element
  float gamma, alpha;
};

// The loss (GRAD = false) or d loss/dx (GRAD = true) of one element, without the weights.
template <bool GRAD>
__device__ __forceinline__ float fl_term(float x, bool pos, float gamma, float alpha) {
  const float z = pos ? x : -x;
  const float a = pos ? alpha : 1.f - alpha;
  const float e = expf(-fabsf(z));
  const float l = log1pf(e);
  const float sp_pos = fmaxf(z, 0.f) + l;    // softplus(z)  = -log(1 - p_t)
  const float sp_neg = fmaxf(-z, 0.f) + l;   // softplus(-z) = -log p_t
  const float w = a * expf(-(gamma * sp_pos));
  if (!GRAD) return w * sp_neg;
  const float r = 1.f / (1.f + e);
  const float s_pos = z >= 0.f ? r : e * r;  // sigmoid(z)
  const float s_neg = z >= 0.f ? e * r : r;  // sigmoid(-z)
  const float dz = w * (gamma * s_pos * sp_neg + s_neg);   // -d loss/dz, both terms >= 0
  return pos ? -dz : dz;
}

// sum over the workgroup, the same bits in every run; valid in thread 0
__device__ __forceinline__ float fl_block_sum(float v) {
  __shared__ float sh[FL_BLOCK / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

template <bool VEC>
__device__ __forceinline__ void fl_load4(const float *p, unsigned i0, unsigned total, float (&v)[4]) {
  if (VEC && i0 + 4 <= total) {
    const float4 t = *(const float4 *)(p + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i0 + j < total ? p[i0 + j] : 0.f;
  }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(FL_BLOCK) void focal_kernel(
    fl_problem q, const float *__restrict__ upstream, const float *__restrict__ grad_scalar,
    float scale, const float *__restrict__ scale_dev, float *__restrict__ out,
    float *__restrict__ partial) {
  float s = scale;
  if (scale_dev) s *= *scale_dev;
  if (MODE == FL_GRAD && grad_scalar) s *= *grad_scalar;
  float acc = 0.f;
  const unsigned base = blockIdx.x * (unsigned)FL_CHUNK + threadIdx.x * 4u;
#pragma unroll
  for (int it = 0; it < FL_ITEMS; ++it) {
    const unsigned i0 = base + it * (FL_BLOCK * 4u);
    if (i0 >= q.total) break;
    float x[4], sw[4], up[4], res[4];
    fl_load4<VEC>(q.x, i0, q.total, x);
    if (q.sw_mode == 2) fl_load4<VEC>(q.sample_weight, i0, q.total, sw);
    if (MODE == FL_GRAD && upstream) fl_load4<VEC>(upstream, i0, q.total, up);
    unsigned row = i0 / (unsigned)q.c;
    int col = (int)(i0 - row * (unsigned)q.c);
    long long label = 0;
    float row_w = 1.f;
    bool fresh = true;   // row < n here: i0 < total
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      res[j] = 0.f;
      if (i0 + j >= q.total) break;
      if (fresh) {
        label = q.target[row];
        // a label outside [0, C) is never an index: the row is all negative and its class weight 1
        row_w = (q.class_weight && label >= 0 && label < q.c) ? q.class_weight[label] : 1.f;
        if (q.sw_mode == 1) row_w *= q.sample_weight[row];
        fresh = false;
      }
      float v = fl_term<MODE == FL_GRAD>(x[j], label == (long long)col, q.gamma, q.alpha) * row_w;
      if (q.sw_mode == 2) v *= sw[j];
      if (MODE == FL_GRAD && upstream) v *= up[j];
      if (MODE == FL_SUM) acc += v;
      else res[j] = v * s;
      if (++col == q.c) { col = 0; ++row; fresh = true; }
    }
    if (MODE != FL_SUM) {
      if (VEC && i0 + 4 <= q.total) {
        *(float4 *)(out + i0) = make_float4(res[0], res[1], res[2], res[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i0 + j < q.total) out[i0 + j] = res[j];
      }
    }
  }
  if (MODE == FL_SUM) {
    const float total = fl_block_sum(acc);
    if (threadIdx.x == 0) {
      if (gridDim.x == 1) out[0] = total * s;
      else partial[blockIdx.x] = total;
    }
  }
}

__global__ __launch_bounds__(FL_BLOCK) void focal_finish_kernel(
    int parts, const float *__restrict__ partial, float scale, const float *__restrict__ scale_dev,
    float *__restrict__ out) {
  float acc = 0.f;
  for (int p = threadIdx.x; p < parts; p += FL_BLOCK) acc += partial[p];
  const float total = fl_block_sum(acc);
  if (threadIdx.x == 0) {
    float s = scale;
    if (scale_dev) s *= *scale_dev;
    out[0] = total * s;
  }
}


// NESIE_OK with `go` = whether there is anything to launch
static int fl_check(const char *W, int n, int c, const float *x, const long long *target,
                    const float *class_weight, const float *sample_weight, int sw_mode, float gamma,
                    fl_problem *q, bool *go) {
  NESIE_REQUIRE(n >= 0 && c >= 0, W);
  NESIE_REQUIRE(sw_mode >= 0 && sw_mode <= 2, W);
  NESIE_REQUIRE(gamma >= 0.f, W);   // a NaN fails too
  const long long total = (long long)n * c;
  if (total >= (1ll << 31)) {
    set_error("%s: 2^31 elements or more (n %d, c %d)", W, n, c);
    return NESIE_ERR_UNSUPPORTED;
  }
  *go = total > 0;
  if (!*go) return NESIE_OK;
  NESIE_REQUIRE(x && target, W);
  NESIE_REQUIRE((sw_mode != 0) == (sample_weight != nullptr), W);
  q->total = (unsigned)total; q->n = n; q->c = c;
  q->x = x; q->target = target; q->class_weight = class_weight;
  q->sample_weight = sample_weight; q->sw_mode = sw_mode;
  q->gamma = gamma;
  return NESIE_OK;
}

static inline bool fl_vec(const fl_problem &q, const void *a, const void *b) {
  return aligned16(q.x) && aligned16(a) && aligned16(b) &&
         (q.sw_mode != 2 || aligned16(q.sample_weight));
}

// one launch of focal_kernel<MODE, vec> over `grid` workgroups
template <int MODE, typename... Args>
static void fl_launch(bool vec, int grid, void *stream, Args... args) {
  with_bool(vec, [&](auto VEC) {
    hipLaunchKernelGGL((focal_kernel<MODE, VEC()>), dim3((unsigned)grid), dim3(FL_BLOCK), 0, (hipStream_t)stream,
                       args...);
  });
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_sigmoid_focal_loss_forward(int n, int c, const float *x, const long long *target,
                                                const float *class_weight, const float *sample_weight,
                                                int sample_weight_mode, float gamma, float alpha,
                                                float scale, float *loss, void *stream) {
  const char *W = "sigmoid_focal_loss_forward";
  fl_problem q;
  bool go;
  const int st = fl_check(W, n, c, x, target, class_weight, sample_weight, sample_weight_mode, gamma,
                          &q, &go);
  if (st || !go) return st;
  NESIE_REQUIRE(loss, W);
  q.alpha = alpha;
  const float *none = nullptr;
  float *no_partial = nullptr;
  fl_launch<FL_NONE>(fl_vec(q, loss, nullptr), cdiv(q.total, FL_CHUNK), stream, q, none, none, scale, none, loss,
                     no_partial);
  return check_launch(W);
}

extern "C" size_t nesie_sigmoid_focal_loss_workspace_bytes(int n, int c) {
  const long long total = (long long)n * c;
  if (n < 0 || c < 0 || total >= (1ll << 31)) return 0;
  const size_t parts = (size_t)cdiv(total, FL_CHUNK);
  return parts > 1 ? (parts * sizeof(float) + 15) & ~(size_t)15 : 0;
}

extern "C" int nesie_sigmoid_focal_loss_forward_sum(int n, int c, const float *x,
                                                    const long long *target,
                                                    const float *class_weight,
                                                    const float *sample_weight,
                                                    int sample_weight_mode, float gamma, float alpha,
                                                    float scale, const float *scale_dev, float *out,
                                                    void *workspace, size_t workspace_bytes,
                                                    void *stream) {
  const char *W = "sigmoid_focal_loss_forward_sum";
  fl_problem q;
  bool go;
  const int st = fl_check(W, n, c, x, target, class_weight, sample_weight, sample_weight_mode, gamma,
                          &q, &go);
  if (st || !go) return st;
  NESIE_REQUIRE(out, W);
  q.alpha = alpha;
  const int parts = cdiv(q.total, FL_CHUNK);
  if (parts > 1) {
    NESIE_REQUIRE(workspace && ((uintptr_t)workspace & 3) == 0, W);
    NESIE_REQUIRE(workspace_bytes >= nesie_sigmoid_focal_loss_workspace_bytes(n, c), W);
  }
  const float *none = nullptr;
  float *partial = (float *)workspace;
  fl_launch<FL_SUM>(fl_vec(q, nullptr, nullptr), parts, stream, q, none, none, scale, scale_dev, out, partial);
  int st2 = check_launch(W);
  if (st2 || parts == 1) return st2;
  hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(FL_BLOCK), 0, (hipStream_t)stream, parts,
                     (const float *)partial, scale, scale_dev, out);
  return check_launch(W);
}

extern "C" int nesie_sigmoid_focal_loss_backward(int n, int c, const float *x, const long long *target,
                                                 const float *class_weight,
                                                 const float *sample_weight, int sample_weight_mode,
                                                 float gamma, float alpha, const float *grad_out,
                                                 const float *grad_scalar, float scale,
                                                 const float *scale_dev, float *grad_x,
                                                 void *stream) {
  const char *W = "sigmoid_focal_loss_backward";
  fl_problem q;
  bool go;
  const int st = fl_check(W, n, c, x, target, class_weight, sample_weight, sample_weight_mode, gamma,
                          &q, &go);
  if (st || !go) return st;
  NESIE_REQUIRE(grad_x, W);
  NESIE_REQUIRE((grad_out != nullptr) != (grad_scalar != nullptr), W);
  q.alpha = alpha;
  float *no_partial = nullptr;
  fl_launch<FL_GRAD>(fl_vec(q, grad_x, grad_out), cdiv(q.total, FL_CHUNK), stream, q, grad_out, grad_scalar, scale,
                     scale_dev, grad_x, no_partial);
  return check_launch(W);
}
