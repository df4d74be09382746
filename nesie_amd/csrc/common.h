// Shared helpers for the gfx950 kernels of libnesie_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/nesie_ops.h"
#include "dispatch.h"

namespace nesie {

void set_error(const char *fmt, ...);
int distance_form();   // 0 (default), 1, 2: see sqdist_form
int cu_count();        // CUs the persistent grids are sized for (nesie_set_cu_count; 256)
// 1: a persistent launch over an operand of this size walks its tiles last-to-first (nesie_lib.hip)
int walk_dir(long long operand_bytes);

inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return NESIE_ERR_LAUNCH;
  }
  return NESIE_OK;
}

#define NESIE_REQUIRE(cond, what)                                   \
  do {                                                              \
    if (!(cond)) {                                                  \
      nesie::set_error("%s: requirement failed: %s", what, #cond);  \
      return NESIE_ERR_INVALID_ARG;                                 \
    }                                                               \
  } while (0)

// after a launch: return its error from the enclosing launcher, go on when there is none
#define NESIE_LAUNCHED(what)                        \
  do {                                              \
    const int e_ = nesie::check_launch(what);       \
    if (e_ != NESIE_OK) return e_;                  \
  } while (0)

// p[0 .. n) = 0 as a launch (nesie_lib.hip says why not hipMemsetAsync): for a buffer that the next
// kernel adds into
void zero_i32(int *p, int n, hipStream_t s);

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline long long cdiv_ll(long long a, long long b) { return (a + b - 1) / b; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// true when a tensor of this size should be streamed with non-temporal accesses (bn.hip): the norm
// and pooling passes ask; the blend stores (same-box A/B: neutral) and the norm statistics do not
bool stream_nt(long long bytes);

// Squared distance in the canonical, contraction-free form
// ((dx*dx) + (dy*dy)) + (dz*dz)   (SURVEY.md appendix A.0).
__device__ __forceinline__ float sqdist_nofma(float dx, float dy, float dz) {
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)),
                   __fmul_rn(dz, dz));
}

// The same distance in a selectable form (nesie_set_distance_form): nvcc's default -fmad=true MAY
// contract the reference's `(x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)`
// (furthest_point_sample_cuda.cu:65-66, ball_query_cuda.cu:41-42, three_nn_cuda.cu:41); whether and how
// cannot be known without a run of the reference's own CUDA build.
//   FORM 0  ((dx*dx) + (dy*dy)) + (dz*dz)        no contraction: the product's form
//   FORM 1  fma(dz, dz, fma(dx, dx, dy*dy))       LLVM's contraction of the expression as written
//   FORM 2  fma(dz, dz, fma(dy, dy, dx*dx))       the other choice for the inner sum
// FORM != 0 is served by the plain (un-pruned, un-indexed) kernels only: a checking aid for the day
// a CUDA-produced fixture exists, not a fast path.  oracle/nesie_oracle.c carries the same switch.
template <int FORM>
__device__ __forceinline__ float sqdist_form(float dx, float dy, float dz) {
  if (FORM == 1) return __fmaf_rn(dz, dz, __fmaf_rn(dx, dx, __fmul_rn(dy, dy)));
  if (FORM == 2) return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
  return sqdist_nofma(dx, dy, dz);
}

// with_int over FORM = distance_form() (dispatch.h): a launcher writes its kernel<FORM()> once,
// inside a generic lambda.
template <typename F>
inline void with_distance_form(F &&f) {
  const int form = distance_form();
  with_int<0, 1, 2>(form == 1 || form == 2 ? form : 0, f);
}

// Launches Kern with `lds` bytes of dynamic LDS.  One rule for every kernel that may need more
// than the 64 KB a kernel gets by default: the limit requested so far is kept per kernel
// instantiation (the static belongs to this template's instantiation; 64 KB at first) and is
// raised whenever max(lds, CEIL) exceeds it.  CEIL is for a site that knows its kernel's maximum:
// the first launch then asks for it, whatever its own size, and no later one asks again.
template <auto Kern, size_t CEIL = 0, typename... Args>
inline void launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static size_t limit = 65536;
  const size_t want = lds > CEIL ? lds : CEIL;
  if (want > limit) {
    (void)hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
    limit = want;
  }
  hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
}

// 64-bit max across the 64 lanes of a wave (result valid in every lane).
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// Sum across the 64 lanes of a wave (float, double, int), result in every lane: the xor butterfly,
// offsets 32 down to 1 -- a fixed order, so a float sum is reproducible.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// v of the lane that DPP control CTRL names (full row and bank masks): inside a row of 16 lanes, no
// LDS, full rate
template <int CTRL>
__device__ __forceinline__ unsigned dppm(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}

// Sum across each run of LANES (32 or 64) consecutive lanes, result in every lane of the run, in
// another fixed order: lane ^ 1, lane ^ 2, the mirror within 8 and the mirror within 16 by DPP,
// then xor 16 (and xor 32).  Four LDS-free steps, but not wave_sum's order, so a float sum differs
// from wave_sum's bitwise: the outputs pinned on one must not move to the other.
template <int LANES>
__device__ __forceinline__ float wave_sum_dpp(float v) {
  static_assert(LANES == 32 || LANES == 64, "a half or a whole wave");
  v += __uint_as_float(dppm<0xB1>(__float_as_uint(v)));   // quad_perm [1,0,3,2]
  v += __uint_as_float(dppm<0x4E>(__float_as_uint(v)));   // quad_perm [2,3,0,1]
  v += __uint_as_float(dppm<0x141>(__float_as_uint(v)));  // row_half_mirror
  v += __uint_as_float(dppm<0x140>(__float_as_uint(v)));  // row_mirror
  v += __shfl_xor(v, 16, 64);
  if (LANES == 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// Sum over a workgroup of BLOCK threads, result in every thread: wave_sum, then the waves' sums
// in ascending wave order.  sh: BLOCK / 64 values (float or double) of LDS; the barrier in front
// lets a caller hand in the same sh for one sum after another.
template <int BLOCK, typename T>
__device__ __forceinline__ T block_sum(T v, T *sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  T t = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; ++w) t += sh[w];
  return t;
}

// ---- arg-max inside a row of <= 16 lanes, through dppm
// (value, index) max with smallest-index tie-break, exchanged with the lane given by CTRL
template <int CTRL>
__device__ __forceinline__ void argmax_step(float &v, int &i) {
  const float ov = __uint_as_float(dppm<CTRL>(__float_as_uint(v)));
  const int oi = (int)dppm<CTRL>((unsigned)i);
  const bool take = ov > v || (ov == v && oi < i);
  v = take ? ov : v;
  i = take ? oi : i;
}

// arg-max over the 4 elements a lane holds, then over the LPR lanes of its row (LPR <= 16):
// smallest index on ties, result in every lane of the row
template <int LPR>
__device__ __forceinline__ void row_argmax4(const float4 q, int part, float &v, int &i) {
  v = q.x; i = part * 4;
  if (q.y > v) { v = q.y; i = part * 4 + 1; }
  if (q.z > v) { v = q.z; i = part * 4 + 2; }
  if (q.w > v) { v = q.w; i = part * 4 + 3; }
  if (LPR >= 2) argmax_step<0xB1>(v, i);    // lane ^ 1
  if (LPR >= 4) argmax_step<0x4E>(v, i);    // lane ^ 2
  if (LPR >= 8) argmax_step<0x141>(v, i);   // row_half_mirror: 7 - lane (within 8)
  if (LPR >= 16) argmax_step<0x140>(v, i);  // row_mirror: 15 - lane (within 16)
}


// Streaming accesses.  NT = non-temporal: a tensor larger than the 256 MB Infinity Cache that is
// not read again soon should not displace what is (tools/clk/stream.hip: 6.65 vs 6.0 TB/s for a
// read + write pass over 268 MB).  The launchers choose NT by tensor size (stream_nt).
typedef float f4v __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float *p) {
  if (NT) {
    const f4v t = __builtin_nontemporal_load((const f4v *)p);
    return make_float4(t.x, t.y, t.z, t.w);
  }
  return *(const float4 *)p;
}
template <bool NT>
__device__ __forceinline__ void st4(float *p, const float4 v) {
  if (NT) {
    const f4v t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, (f4v *)p);
  } else {
    *(float4 *)p = v;
  }
}
}  // namespace nesie
