// three_nn / three_interpolate (+grad) for gfx950.
//
// Replaces three_nn_kernel (reference mmdet3d/ops/interpolate/src/three_nn_cuda.cu:11-65),
// three_interpolate_kernel and three_interpolate_grad_kernel
// (reference .../three_interpolate_cuda.cu:11-35, :61-84).
//
// three_nn: the known set (m <= a few thousand points) is staged through LDS in
// tiles of (x, y, z, -) float4s, so the inner scan reads one LDS broadcast per point instead of
// global memory; each thread owns one query and keeps its three best
// (distance, index) pairs in registers.  The reference keeps the bests in
// double but compares them with a float candidate, which orders exactly like
// float compares with a +inf start (1e40 rounds to +inf on output), so floats
// are used here.  Ties keep the earlier index in the better slot (strict <).
#include "common.h"
#include "index_sort.h"
#include "wave_sort.h"
#include <math.h>

namespace nesie {

constexpr int NN_BLOCK = 256;
constexpr int NN_TILE = 1024;  // known points per LDS tile (12 KB)

// The three nearest of the m points of `known` to (ux, uy, uz): squared distances b1 <= b2 <= b3
// and their indices (+inf and 0 where m < 3).
struct ThreeNN {
  float b1, b2, b3;
  int i1, i2, i3;
};

// `known` streams through the workgroup's tile `kk` with two barriers per tile, so EVERY thread of
// the workgroup must call this, a thread without a query of its own with any valid point.  A
// candidate displaces a best only when strictly nearer, so of two equally distant points the
// earlier index keeps the better slot: the tie rule the reference has, written this once.
// (The bests are locals returned by value: through reference parameters they stay in scratch.)
template <int FORM>
__device__ __forceinline__ ThreeNN three_nn_scan(float ux, float uy, float uz,
                                                 const float *__restrict__ known, int m, float4 *kk) {
  float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
  int i1 = 0, i2 = 0, i3 = 0;
  for (int t0 = 0; t0 < m; t0 += NN_TILE) {
    const int tn = m - t0 < NN_TILE ? m - t0 : NN_TILE;
    __syncthreads();
    for (int i = threadIdx.x; i < tn; i += NN_BLOCK)
      kk[i] = make_float4(known[(t0 + i) * 3 + 0], known[(t0 + i) * 3 + 1],
                          known[(t0 + i) * 3 + 2], 0.f);
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < tn; ++i) {
      const float4 kp = kk[i];
      const float d = sqdist_form<FORM>(ux - kp.x, uy - kp.y, uz - kp.z);
      if (d < b3) {  // rare once the three bests have settled: one compare on the common path
        const int k = t0 + i;
        if (d < b1) {
          b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = d; i1 = k;
        } else if (d < b2) {
          b3 = b2; i3 = i2; b2 = d; i2 = k;
        } else {
          b3 = d; i3 = k;
        }
      }
    }
  }
  return {b1, b2, b3, i1, i2, i3};
}

template <int FORM>
__global__ __launch_bounds__(NN_BLOCK) void three_nn_kernel(
    int n, int m, const float *__restrict__ unknown, const float *__restrict__ known,
    float *__restrict__ dist2, int *__restrict__ idx) {
  __shared__ float4 kk[NN_TILE];  // (x, y, z, -): one ds_read_b128 broadcast per known point
  const int bi = blockIdx.y;
  const int q = blockIdx.x * NN_BLOCK + threadIdx.x;
  const bool live = q < n;
  unknown += (size_t)bi * n * 3;
  known += (size_t)bi * m * 3;
  const int qq = live ? q : n - 1;
  const float ux = unknown[qq * 3 + 0], uy = unknown[qq * 3 + 1], uz = unknown[qq * 3 + 2];
  const ThreeNN nn = three_nn_scan<FORM>(ux, uy, uz, known, m, kk);
  if (live) {
    float *od = dist2 + ((size_t)bi * n + q) * 3;
    int *oi = idx + ((size_t)bi * n + q) * 3;
    od[0] = nn.b1; od[1] = nn.b2; od[2] = nn.b3;
    oi[0] = nn.i1; oi[1] = nn.i2; oi[2] = nn.i3;
  }
}

// ---- grid points of the quality head + their 3-NN taps, in one kernel -------------------------
// Per proposal k and grid point g (gp points per proposal, box-frame multipliers mult[g] in
// [-1, 1]^3 and plane[g] = the +-10 % plane offsets of the SAQE variant, else 0):
//   f     = mult * size / 2;  local = f + f * plane                (generate_grid / planes)
//   world = R(heading) . local + centre                            (_to_scene)
//   3-NN of `world` among the seeds (three_nn, same compare order), then
//   weight_t = (1 / (sqrt(d2_t) + 1e-8)) / sum_t(...),  rel = world - centre
// Stands in for side_pooling_module.py:87-157 (grids) and :204-225 (taps): ~55 ATen launches.
template <int FORM>
__global__ __launch_bounds__(NN_BLOCK) void grid_taps_kernel(
    int kprop, int gp, int m, const float *__restrict__ centre, const float *__restrict__ size,
    const float *__restrict__ heading, const float *__restrict__ mult,
    const float *__restrict__ plane, const float *__restrict__ known, int *__restrict__ idx,
    float *__restrict__ weight, float *__restrict__ rel) {
  __shared__ float4 kk[NN_TILE];
  const int bi = blockIdx.y;
  const int n = kprop * gp;
  const int q = blockIdx.x * NN_BLOCK + threadIdx.x;
  const bool live = q < n;
  const int qq = live ? q : n - 1;
  const int k = qq / gp, g = qq - k * gp;
  const float *c3 = centre + ((size_t)bi * kprop + k) * 3;
  const float *s3 = size + ((size_t)bi * kprop + k) * 3;
  const float cx = c3[0], cy = c3[1], cz = c3[2];
  float l[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float f = __fmul_rn(mult[g * 3 + d], s3[d]) / 2.f;
    l[d] = __fadd_rn(f, __fmul_rn(f, plane[g * 3 + d]));
  }
  const float h = heading[(size_t)bi * kprop + k];
  const float ch = cosf(h), sh = sinf(h);
  const float ux = __fadd_rn(__fadd_rn(__fmul_rn(l[0], ch), __fmul_rn(l[1], sh)), cx);
  const float uy = __fadd_rn(__fadd_rn(__fmul_rn(l[0], -sh), __fmul_rn(l[1], ch)), cy);
  const float uz = __fadd_rn(l[2], cz);
  known += (size_t)bi * m * 3;
  const ThreeNN nn = three_nn_scan<FORM>(ux, uy, uz, known, m, kk);
  if (live) {
    const size_t o = ((size_t)bi * n + q) * 3;
    const float w1 = 1.f / __fadd_rn(sqrtf(nn.b1), 1e-8f), w2 = 1.f / __fadd_rn(sqrtf(nn.b2), 1e-8f),
                w3 = 1.f / __fadd_rn(sqrtf(nn.b3), 1e-8f);
    const float ws = __fadd_rn(__fadd_rn(w1, w2), w3);
    idx[o] = nn.i1; idx[o + 1] = nn.i2; idx[o + 2] = nn.i3;
    weight[o] = w1 / ws; weight[o + 1] = w2 / ws; weight[o + 2] = w3 / ws;
    rel[o] = ux - cx; rel[o + 1] = uy - cy; rel[o + 2] = uz - cz;
  }
}

constexpr int TI_BLOCK = 256;
constexpr int TI_CH = 8;

// points (B,C,M), idx/weight (B,N,3) -> out (B,C,N)
__global__ __launch_bounds__(TI_BLOCK) void three_interpolate_kernel(
    int c, int m, int n, const float *__restrict__ points, const int *__restrict__ idx,
    const float *__restrict__ weight, float *__restrict__ out) {
  const int p = blockIdx.x * TI_BLOCK + threadIdx.x;
  const int c0 = blockIdx.y * TI_CH;
  const int bi = blockIdx.z;
  if (p >= n) return;
  const int *ix = idx + ((size_t)bi * n + p) * 3;
  const float *w = weight + ((size_t)bi * n + p) * 3;
  int j0 = ix[0], j1 = ix[1], j2 = ix[2];
  j0 = j0 < 0 ? 0 : (j0 >= m ? m - 1 : j0);
  j1 = j1 < 0 ? 0 : (j1 >= m ? m - 1 : j1);
  j2 = j2 < 0 ? 0 : (j2 >= m ? m - 1 : j2);
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const int cend = c - c0 < TI_CH ? c - c0 : TI_CH;
#pragma unroll
  for (int i = 0; i < TI_CH; ++i) {
    if (i < cend) {
      const float *src = points + ((size_t)bi * c + c0 + i) * m;
      // products rounded one by one, summed left to right (.cu:33-34)
      float r = __fadd_rn(__fadd_rn(__fmul_rn(w0, src[j0]), __fmul_rn(w1, src[j1])),
                          __fmul_rn(w2, src[j2]));
      out[((size_t)bi * c + c0 + i) * n + p] = r;
    }
  }
}

// ---- the quality head's grid features, blended straight into their consumer's layout ----
// Query p = (k, s, g) of n = K * segs * seg_len (proposal, face, grid point) goes to
// out[b, s, c_offset + ch, k * seg_len + g] of out (B, segs, c_total, K * seg_len): one
// (c_total, K, seg_len) block per scene and face -- what the reference reaches with
// interpolate -> view -> cat -> split -> contiguous (side_pooling_module.py:226-243, 304-313).
//
//   out = w0 * T[j0] + w1 * T[j1] + w2 * T[j2]  (+ wx . rel)
//
// T is a POINT-major table (B, M, pitch): the three taps of a query are dense rows of up to
// 1 KB (a lane owns c / 64 consecutive channels); a (channels x 64 queries) tile turns through
// LDS and leaves as dense rows along the query axis (lane = query).  With T = the seed
// features this is three_interpolate in the segmented layout.  With T = F . W_f^T (the seed features already multiplied by the
// feature columns of a MiniPointNet's first 1x1 conv, one column block per face: seg_off) and
// wx = that conv's three xyz columns, it IS the first conv's output,
//   W . cat[rel_xyz, blend(F)] = W_xyz . rel_xyz + blend(W_f . F)      (the conv is linear),
// at ~1/250 of the multiply-adds and without ever storing the 259-channel feature tensor.
constexpr int TS_Q = 64;  // queries per workgroup (one tile side; per_seg % 64 == 0)
constexpr int BF_LD = TS_Q + 1;   // tile row pitch in floats: odd, so both tile phases meet no bank conflict
typedef float bf_f2 __attribute__((ext_vector_type(2)));
constexpr int BF_NQ = 8;          // queries whose taps are in flight before the first is consumed

// CPT = channels per lane: a workgroup covers CW = 64 * CPT channels (c > 256 runs as chunks of 256
// along blockIdx.y, a remainder as a launch of its own starting at channel `cb`).
//  * A wave keeps its 16 consecutive queries for all CW channels.  Lane l & 15 reads query l's
//    three (clamped seed, weight, rel) once; v_readlane makes them wave-uniform, so a tap is a
//    scalar row base plus one per-lane offset and moves as ONE load of 4 * CPT bytes per lane (a
//    1 KB row per instruction at CPT = 4), and the weights and rel multiply from scalar registers.
//  * The 3 * BF_NQ loads of BF_NQ queries are issued back to back before the first is consumed;
//    `wx` and the statistics are template parameters, so nothing branches inside the loop.
//  * Channel lane * CPT + e sits in tile row e * 64 + lane: the 64 lanes of a tile write land in 64
//    different banks, and so do the 4 rows x 16 lanes of a row read of the store phase.
// The arithmetic is the tile kernel's of rounds 1-6, rounding by rounding:
//   v = (w0 a0 + w1 a1) + w2 a2   [+ x0 r0, + x1 r1, + x2 r2, added left to right], every product
//   rounded on its own; per (channel, tile) the sums of v and of v * v run over a wave's 16 queries
//   in ascending order from 0, and the four waves' sums combine as (0 + 1) + (2 + 3).
template <int CPT, bool WX, bool STAT>
__global__ __launch_bounds__(256) void blend_fwd_kernel(
    int c, int cb, int m, int n, int segs, int seg_len, int c_total, int c_offset, int pitch,
    int seg_off, const float *__restrict__ table, const int *__restrict__ idx,
    const float *__restrict__ weight, const float *__restrict__ rel,
    const float *__restrict__ wx, float *__restrict__ out, float *__restrict__ stat_partial,
    int nb) {
#pragma clang fp contract(off)
  constexpr int CW = CPT * 64;
  extern __shared__ float bf_lds[];
  float *tile = bf_lds;                      // [CW][BF_LD]
  float *red = bf_lds + CW * BF_LD;          // [4][CW][2]  (STAT only)
  // 1-D grid with the scene fastest: workgroup i runs on XCD i % 8, so with B = 8 every scene's
  // table rows are gathered through ONE XCD's L2 instead of all eight
  const int bi = blockIdx.x % nb;
  const int q0 = (blockIdx.x / nb) * TS_Q;  // output order: s * per_seg + k * seg_len + g
  const int c0 = cb + blockIdx.y * CW;
  const int per_seg = n / segs;
  const int sg = q0 / per_seg, r0 = q0 - sg * per_seg;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // the taps of this wave's 16 queries: lane l (and l + 16, l + 32, l + 48) holds query wv * 16 + l
  int pj[3];
  float pw[3], pr[3];
  {
    const int r = r0 + wv * 16 + (lane & 15);
    const int k = r / seg_len, g = r - k * seg_len;
    const size_t p = (size_t)bi * n + (size_t)(k * segs + sg) * seg_len + g;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int j = idx[p * 3 + t];
      pj[t] = j < 0 ? 0 : (j >= m ? m - 1 : j);
      pw[t] = weight[p * 3 + t];
      pr[t] = WX ? rel[p * 3 + t] : 0.f;
    }
  }
  const float *feat = table + (size_t)bi * m * pitch + (size_t)sg * seg_off + c0;   // uniform
  const unsigned voff = (unsigned)(lane * CPT * 4);
  float x[CPT][3] = {};
  if (WX) {
    __builtin_memcpy(&x[0][0], wx + ((size_t)sg * c + c0 + lane * CPT) * 3, sizeof(x));
  }
  // Two channels per instruction where CPT allows: v_pk_mul_f32 / v_pk_add_f32 round each half like
  // the scalar forms, and contraction is off, so no product is fused into its add.
  constexpr int CP2 = CPT / 2;
  bf_f2 s2[CP2 ? CP2 : 1], q2[CP2 ? CP2 : 1];
  float s1 = 0.f, q1 = 0.f;                          // the odd channel (CPT = 1, 3)
#pragma unroll
  for (int e = 0; e < CP2; ++e) s2[e] = q2[e] = bf_f2{0.f, 0.f};
#pragma unroll
  for (int i0 = 0; i0 < 16; i0 += BF_NQ) {
    float a[BF_NQ][3][CPT];
#pragma unroll
    for (int i = 0; i < BF_NQ; ++i)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int j = __builtin_amdgcn_readlane(pj[t], i0 + i);
        const float *row = feat + (size_t)j * pitch;                                // uniform
        __builtin_memcpy(a[i][t], (const char *)row + voff, CPT * 4);
      }
    // (without this the scheduler sinks every load to its use to save registers that the LDS-bound
    // residency cannot use: three loads in flight and a full wait per query)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < BF_NQ; ++i) {
      const int qi = wv * 16 + i0 + i;
      float sw[3], sr[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        sw[t] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pw[t]), i0 + i));
        sr[t] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pr[t]), i0 + i));
      }
      // products rounded one by one, summed left to right (three_interpolate_cuda.cu:33-34)
      auto blend = [&](auto a0, auto a1, auto a2, auto x0, auto x1, auto x2) {
        auto v = (a0 * sw[0] + a1 * sw[1]) + a2 * sw[2];
        if (WX) v = ((v + x0 * sr[0]) + x1 * sr[1]) + x2 * sr[2];
        return v;
      };
#pragma unroll
      for (int h = 0; h < CP2; ++h) {
        const int e = 2 * h;
        const bf_f2 v = blend(bf_f2{a[i][0][e], a[i][0][e + 1]}, bf_f2{a[i][1][e], a[i][1][e + 1]},
                              bf_f2{a[i][2][e], a[i][2][e + 1]}, bf_f2{x[e][0], x[e + 1][0]},
                              bf_f2{x[e][1], x[e + 1][1]}, bf_f2{x[e][2], x[e + 1][2]});
        tile[(e * 64 + lane) * BF_LD + qi] = v.x;
        tile[((e + 1) * 64 + lane) * BF_LD + qi] = v.y;
        if (STAT) {
          s2[h] = s2[h] + v;
          q2[h] = q2[h] + v * v;
        }
      }
      if (CPT & 1) {
        constexpr int e = CPT - 1;
        const float v = blend(a[i][0][e], a[i][1][e], a[i][2][e], x[e][0], x[e][1], x[e][2]);
        tile[(e * 64 + lane) * BF_LD + qi] = v;
        if (STAT) {
          s1 = s1 + v;
          q1 = q1 + v * v;
        }
      }
    }
  }
  if (STAT) {
#pragma unroll
    for (int e = 0; e < CPT; ++e) {
      const bool odd = (CPT & 1) && e == CPT - 1;
      red[((wv * CW) + e * 64 + lane) * 2] = odd ? s1 : s2[e / 2][e & 1];
      red[((wv * CW) + e * 64 + lane) * 2 + 1] = odd ? q1 : q2[e / 2][e & 1];
    }
  }
  __syncthreads();
  // wave wv stores tile rows wv * 16 CPT .. + 16 CPT - 1: four 256-byte rows per instruction (16
  // lanes x 16 bytes each) instead of one -- a quarter of the store instructions for the same bytes.
  // NON-TEMPORAL: the output is written once and is far larger than L2; plain stores allocate there
  // and push out the table rows the gather lives on (measured at the step's shapes with
  // tools/blend_bench.py fwd-side / fwd-box: 154 / 92 us plain, 103 / 67 us non-temporal)
  float *dst = out + (((size_t)bi * segs + sg) * c_total + c_offset + c0) * per_seg + r0;
#pragma unroll
  for (int i = 0; i < 4 * CPT; ++i) {
    const int row = wv * (16 * CPT) + i * 4 + (lane >> 4), q4 = (lane & 15) * 4;
    const int ch = (row & 63) * CPT + (row >> 6);
    const float *tr = tile + row * BF_LD + q4;
    st4<true>(dst + (size_t)ch * per_seg + q4, make_float4(tr[0], tr[1], tr[2], tr[3]));
  }
  if (STAT && threadIdx.x < CW) {
    // (sum, sum of squares) of this tile per stacked channel, for the norm layer that follows:
    // partial[(chan * nslice + slice) * 2], nslice = B * per_seg / 64 (bn.hip's layout)
    const int row = threadIdx.x, ch = (row & 63) * CPT + (row >> 6);
    const float *rd = red + row * 2;
    const float ss = (rd[0] + rd[CW * 2]) + (rd[2 * CW * 2] + rd[3 * CW * 2]);
    const float qq = (rd[1] + rd[CW * 2 + 1]) + (rd[2 * CW * 2 + 1] + rd[3 * CW * 2 + 1]);
    const int nslice = nb * (per_seg / TS_Q);
    const int slice = bi * (per_seg / TS_Q) + r0 / TS_Q;
    float *pd = stat_partial + ((size_t)(sg * c + c0 + ch) * nslice + slice) * 2;
    pd[0] = ss; pd[1] = qq;
  }
}

// Any shape (c % 64 != 0 or per_seg % 64 != 0): one thread per output-order query.
__global__ __launch_bounds__(TI_BLOCK) void blend_fwd_generic_kernel(
    int c, int m, int n, int segs, int seg_len, int c_total, int c_offset, int pitch,
    int seg_off, const float *__restrict__ table, const int *__restrict__ idx,
    const float *__restrict__ weight, const float *__restrict__ rel,
    const float *__restrict__ wx, float *__restrict__ out) {
  const int q = blockIdx.x * TI_BLOCK + threadIdx.x;
  const int c0 = blockIdx.y * TI_CH;
  const int bi = blockIdx.z;
  if (q >= n) return;
  const int per_seg = n / segs;
  const int sg = q / per_seg, r = q - sg * per_seg;
  const int k = r / seg_len, g = r - k * seg_len;
  const size_t p = (size_t)bi * n + (size_t)(k * segs + sg) * seg_len + g;
  int j0 = idx[p * 3], j1 = idx[p * 3 + 1], j2 = idx[p * 3 + 2];
  j0 = j0 < 0 ? 0 : (j0 >= m ? m - 1 : j0);
  j1 = j1 < 0 ? 0 : (j1 >= m ? m - 1 : j1);
  j2 = j2 < 0 ? 0 : (j2 >= m ? m - 1 : j2);
  const float w0 = weight[p * 3], w1 = weight[p * 3 + 1], w2 = weight[p * 3 + 2];
  const float rx = rel ? rel[p * 3] : 0.f, ry = rel ? rel[p * 3 + 1] : 0.f,
              rz = rel ? rel[p * 3 + 2] : 0.f;
  const int cend = c - c0 < TI_CH ? c - c0 : TI_CH;
  const float *feat = table + (size_t)bi * m * pitch + (size_t)sg * seg_off + c0;
  float *dst = out + (((size_t)bi * segs + sg) * c_total + c_offset + c0) * per_seg + r;
#pragma unroll
  for (int i = 0; i < TI_CH; ++i) {
    if (i < cend) {
      float v = __fadd_rn(
          __fadd_rn(__fmul_rn(w0, feat[(size_t)j0 * pitch + i]), __fmul_rn(w1, feat[(size_t)j1 * pitch + i])),
          __fmul_rn(w2, feat[(size_t)j2 * pitch + i]));
      if (wx) {
        const float *wr = wx + ((size_t)sg * c + c0 + i) * 3;
        v = __fadd_rn(__fadd_rn(__fadd_rn(v, __fmul_rn(wr[0], rx)), __fmul_rn(wr[1], ry)),
                      __fmul_rn(wr[2], rz));
      }
      dst[(size_t)i * per_seg] = v;
    }
  }
}

// Backward of the blended first conv: d_table[b, j, s*seg_off + ch] += sum over the queries
// of face s whose tap t lands on seed j of w_t * dy, and d_wx[s, ch, :] += sum_q dy * rel.
// It replaces the reference's atomicAdd scatter (three_interpolate_cuda.cu:61-84) together
// with the first conv's weight-gradient GEMM.
// Measured here (tools/clk/lds_atomic.hip): ds_add_f32 sustains 0.32 lanes/clk/CU and
// ds_add_u32/u64 0.93, i.e. 0.2-0.57 T adds/s chip-wide, and global float atomics ~1.3 TB/s of
// added bytes; this scatter has 0.5 G adds.  So the number of adds must shrink: lane = channel
// (the mirror image of blend_fwd_kernel: dy tiles turn through LDS) and a wave owns 16
// consecutive queries = 48 taps (one face of one proposal when seg_len = 16).  The taps of such
// a group land on ~19 distinct seeds (tools/blend_locality.py), so the wave sorts its 48
// (seed, tap) keys -- a 64-lane bitonic network in registers -- walks them in seed order with
// ONE running sum per lane, and emits one 256-byte global_atomic_add_f32 row per channel
// block only when the seed changes: ~2.5x fewer adds, no slot bookkeeping, and all control
// flow wave-uniform.  d_table must be zero on entry; d_wx leaves as one partial per workgroup
// (plain stores: thousands of workgroups adding into the same few KB serialise at the memory
// side), summed by the caller.
constexpr int BL_RUN = 512;  // consecutive queries per workgroup (long runs: the per-workgroup
                             // set-up and the d_wx partial are paid once per run)

// CPT = c / 64 channels per lane: a wave covers ALL c channels of its 16 queries.
// BNB: `dy` is the gradient dA of relu(bn(Z)) with Z = this blend's own output (`bnz`, same layout):
// the BatchNorm + ReLU backward's apply pass runs on the tile load,
//     dZ = a g + (e0 - (z - mean) d1),  g = dA [fma(z, scale, shift) > 0],
// with bnb[sg * C + ch] = (scale, shift, a, mean, d1, e0, -, -) (pw_bnb_coef_kernel, pwconv_wgrad.hip),
// so the separate pass that read (dA, Z) and wrote dZ for this kernel to read disappears.
// STAGED (round 4): the row a wave has summed for one seed is not ADDED into d_table with float
// atomics (whose arrival order differs from run to run, so the gradient of every MiniPointNet's
// first convolution did) but STORED to a staging slot of its own: slot (16-query group, rank of
// the seed inside the group's 48 sorted taps), 48 slots per group, `slot_seed` naming each slot's
// seed (-1: unused).  A second kernel (blend_bwd_gather_kernel) owns one (scene, face, seed) per
// wave and adds that seed's slots in ascending slot order, through the inverted index of slot_seed:
// every d_table row is written once, in an order fixed by the taps alone.
constexpr int BL_SLOTS = 48;   // staging slots per 16-query group (= its taps: the worst case)

template <int CPT, bool BNB, bool STAGED>
__global__ __launch_bounds__(256, 2) void blend_bwd_rows_kernel(
    int m, int n, int segs, int seg_len, int pitch, int seg_off,
    const float *__restrict__ dy /* (B, segs, C, per_seg) */, const int *__restrict__ idx,
    const float *__restrict__ weight, const float *__restrict__ rel,
    float *__restrict__ d_table, float *__restrict__ d_wx_part, int nb, int nruns,
    const float *__restrict__ bnz, const float *__restrict__ bnb,
    float *__restrict__ stage, int *__restrict__ slot_seed) {
  constexpr int C = CPT * 64;
  __shared__ float tile[C * (TS_Q + 1)];
  __shared__ int sj[TS_Q][3];
  __shared__ float sw[TS_Q][3];
  __shared__ float sr[TS_Q][3];
  // 1-D grid, scene fastest (workgroup i -> XCD i % 8): a scene's d_table rows take the atomic
  // adds of one XCD's L2
  const int bi = blockIdx.x % nb, run_i = (blockIdx.x / nb) % nruns, sg = blockIdx.x / (nb * nruns);
  const int per_seg = n / segs;
  const int run0 = run_i * BL_RUN;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float *src = dy + ((size_t)bi * segs + sg) * C * per_seg;
  const float *zsrc = BNB ? bnz + ((size_t)bi * segs + sg) * C * per_seg : nullptr;
  const int wvu = __builtin_amdgcn_readfirstlane(wv);     // (wave-uniform row index: scalar loads of the coefficients)
  float *dt = d_table + (size_t)bi * m * pitch + (size_t)sg * seg_off + lane;
  float dx[CPT][3];
#pragma unroll
  for (int e = 0; e < CPT; ++e) dx[e][0] = dx[e][1] = dx[e][2] = 0.f;
  const int run_end = run0 + BL_RUN < per_seg ? run0 + BL_RUN : per_seg;
  // Round 5: the loads of tile t + 1 (C rows of dA [and of Z], the 64 queries' taps) are issued into
  // REGISTERS at the top of tile t's compute phase and land while it runs; the top of the next
  // iteration applies the norm backward and moves them into LDS.  (Round 4 loaded a tile in four
  // batches of 16 rows BETWEEN two barriers: per tile four memory latencies with every wave of the
  // workgroup waiting, then the compute phase with nothing in flight -- the ablation added up to the
  // whole kernel: loads 186 us + taps 64 + row stores 78 + skeleton 125 of the side grid's 520.)
  // The barriers wait for LDS only (`s_waitcnt lgkmcnt(0)`): __syncthreads() would also drain the
  // prefetch.  2 workgroups per CU (66 KB of LDS each) = 2 waves per SIMD: 256 VGPRs per wave.
  constexpr int NR = C / 4;                                  // rows per thread (row = 4 i + wave)
  float traw[NR], zraw[BNB ? NR : 1];
  int pj[3];
  float pw[3], pr[3];
  auto prefetch = [&](int r0) {
    if (threadIdx.x < TS_Q) {
      const int r = r0 + threadIdx.x;
      const int k = r / seg_len, g = r - k * seg_len;
      const size_t p = (size_t)bi * n + (size_t)(k * segs + sg) * seg_len + g;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        pj[t] = idx[p * 3 + t];
        pw[t] = weight[p * 3 + t];
        pr[t] = rel ? rel[p * 3 + t] : 0.f;
      }
    }
    // wave-uniform base (scalar registers) + ONE per-lane byte offset: no per-row address registers
    const unsigned voff = (unsigned)(((size_t)wv * per_seg + lane) * 4);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const float *sb_ = src + (size_t)(i * 4) * per_seg + r0;          // uniform
      traw[i] = *(const float *)((const char *)sb_ + voff);
    }
  };
  auto load_z = [&](int r0) {
    const unsigned voff = (unsigned)(((size_t)wv * per_seg + lane) * 4);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const float *zb_ = zsrc + (size_t)(i * 4) * per_seg + r0;       // uniform
      zraw[i] = *(const float *)((const char *)zb_ + voff);
    }
  };
  auto lds_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  if (run0 < run_end) prefetch(run0);
  for (int r0 = run0; r0 < run_end; r0 += TS_Q) {
    // (Z is loaded here, one exposed latency per tile: with its 64 registers in flight beside dA's
    // through the tap loop the kernel spills -- 60 registers, 523 us against 415 for the side grid)
    if (BNB) load_z(r0);
    lds_barrier();                                           // every wave is done with the previous tile
    if (threadIdx.x < TS_Q) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int j = pj[t];
        sj[threadIdx.x][t] = j < 0 ? 0 : (j >= m ? m - 1 : j);
        sw[threadIdx.x][t] = pw[t];
        sr[threadIdx.x][t] = pr[t];
      }
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      float v = traw[i];
      if (BNB) {
        const float *cf = bnb + ((size_t)sg * C + i * 4 + wvu) * 8;      // uniform
        const float zz = zraw[i];
        const float gg = __builtin_fmaf(zz, cf[0], cf[1]) > 0.f ? v : 0.f;
        v = __builtin_fmaf(cf[2], gg, __builtin_fmaf(cf[3] - zz, cf[4], cf[5]));
      }
      tile[(i * 4 + wv) * (TS_Q + 1) + lane] = v;
    }
    lds_barrier();
    // (unconditional: past the run's last tile the last tile is read again -- a conditional prefetch
    // keeps the old and the new register set alive across the join)
    const int rn = r0 + TS_Q < run_end ? r0 + TS_Q : r0;
    prefetch(rn);                                            // lands during the compute phase below
    const int q0 = wv * 16;
    // d_wx: sum_q dy * rel over this wave's 16 queries (lane = channel)
    if (d_wx_part) {
#pragma unroll 4
      for (int u = 0; u < 16; ++u) {
        const float r0x = sr[q0 + u][0], r1x = sr[q0 + u][1], r2x = sr[q0 + u][2];
#pragma unroll
        for (int e = 0; e < CPT; ++e) {
          const float v = tile[(e * 64 + lane) * (TS_Q + 1) + q0 + u];
          dx[e][0] += v * r0x; dx[e][1] += v * r1x; dx[e][2] += v * r2x;
        }
      }
    }
    // the 48 taps of these 16 queries in seed order: key = seed << 6 | tap
    unsigned key = 0xFFFFFFFFu;
    if (lane < 48) key = ((unsigned)sj[q0 + lane / 3][lane % 3] << 6) | (unsigned)lane;
    key = wave_sort64(key, lane);
    int cur = -1;
    float acc[CPT];
#pragma unroll
    for (int e = 0; e < CPT; ++e) acc[e] = 0.f;
    // STAGED: first slot of this wave's 16-query group, and the seeds emitted so far
    const size_t gslot = STAGED ? ((size_t)((size_t)bi * segs + sg) * (per_seg / 16) + (r0 + q0) / 16) * BL_SLOTS : 0;
    int rank = 0;
    if (STAGED) {
      // the group's distinct seeds in ascending order name its staging slots: lane i of the sorted
      // keys opens a slot when its seed differs from lane i - 1's; ONE store instruction per group
      const int sd = lane < 48 ? (int)(key >> 6) : -1;
      const int sp = __shfl_up(sd, 1, 64);
      const bool first = lane < 48 && (lane == 0 || sd != sp);
      const unsigned long long fm = __ballot(first);
      const int nvalid = __popcll(fm);
      if (first) slot_seed[gslot + __popcll(fm & ((1ull << lane) - 1ull))] = sd;
      if (lane >= nvalid && lane < BL_SLOTS) slot_seed[gslot + lane] = -1;     // the unused slots
    }
    auto emit = [&]() {
      if (STAGED) {
        float *row = stage + (gslot + rank) * C + lane;
#pragma unroll
        for (int e = 0; e < CPT; ++e) row[e * 64] = acc[e];
        ++rank;
      } else {
#pragma unroll
        for (int e = 0; e < CPT; ++e) atomicAdd(dt + (size_t)cur * pitch + e * 64, acc[e]);
      }
    };
#pragma unroll 1
    for (int i0 = 0; i0 < 48; i0 += 8) {
      // phase A: eight taps' products, all loads independent (they overlap in the LDS queue)
      int seeds[8];
      float x[8][CPT];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned u = (unsigned)__builtin_amdgcn_readlane((int)key, i0 + i);
        const int tap = (int)(u & 63u);
        const int q = q0 + tap / 3, t = tap % 3;
        seeds[i] = (int)(u >> 6);
        const float w = sw[q][t];
#pragma unroll
        for (int e = 0; e < CPT; ++e) x[i][e] = tile[(e * 64 + lane) * (TS_Q + 1) + q] * w;
      }
      // phase B: the running sum; a row of adds leaves only when the seed changes
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (seeds[i] != cur) {
          if (cur >= 0) emit();
          cur = seeds[i];
#pragma unroll
          for (int e = 0; e < CPT; ++e) acc[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < CPT; ++e) acc[e] += x[i][e];
      }
    }
    emit();
  }
  if (d_wx_part) {
    // partial[b][run][s][c][3]: the four waves hold different queries of the same channels
    __syncthreads();
    float *red = tile;  // [4][C][3]
#pragma unroll
    for (int e = 0; e < CPT; ++e)
#pragma unroll
      for (int d = 0; d < 3; ++d) red[(wv * C + e * 64 + lane) * 3 + d] = dx[e][d];
    __syncthreads();
    float *dst = d_wx_part + ((((size_t)bi * nruns + run_i) * segs + sg) * C) * 3;
    for (int i = threadIdx.x; i < C * 3; i += 256)
      dst[i] = (red[i] + red[C * 3 + i]) + (red[2 * C * 3 + i] + red[3 * C * 3 + i]);
  }
}

// Second half of the STAGED blend backward (round 5 form).  The staging slots of one (scene, face)
// are indexed by SEED in two steps that never leave the chip-wide grid idle:
//   blend_slot_index_kernel: one 1024-thread workgroup per CHUNK of SI_GROUPS 16-query groups
//     (6 144 slots; 4 chunks per side face, 16 per box grid: 192 / 128 workgroups where the
//     round-4 index ran one workgroup per face) counting-sorts its chunk's valid slots by seed --
//     per-wave histogram rows in LDS (a group's valid seeds are pairwise distinct, so a group is
//     counted and later placed by one LDS add per lane), block scan, placement in group order: the
//     STABLE order, every seed's run ascending in slot number -- and leaves `order` (the chunk's
//     slots seed-major) and `offs` (m + 1 run starts per chunk);
//   blend_bwd_gather_kernel: one wave per (scene, face, seed) walks the chunks in order, reads its
//     run bounds from `offs` (no bisection: the round-4 kernel spent 2 x 15 dependent L2 loads per
//     wave finding them), adds the rows in ascending slot order and WRITES the d_table row (zeros
//     for a seed no tap landed on): d_table needs no zero fill and meets no atomic, and the sum
//     order is fixed by the taps alone.
constexpr int SI_GROUPS = 128;                         // 16-query groups per index workgroup
constexpr int SI_BLOCK = 1024, SI_WAVES = SI_BLOCK / 64;
constexpr int SI_MAX_BINS = 2048;                      // seeds + 1 (LDS: 16 histogram rows)

__global__ __launch_bounds__(SI_BLOCK) void blend_slot_index_kernel(
    int m, int groups_per_face, int nchunk, const int *__restrict__ slot_seed,
    int *__restrict__ order, int *__restrict__ offs) {
  extern __shared__ int si_lds[];                      // cnt[SI_WAVES][m], then scan scratch [SI_WAVES]
  int *cnt = si_lds, *scratch = si_lds + SI_WAVES * m;
  const int face = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g0 = chunk * SI_GROUPS;
  const int g1 = g0 + SI_GROUPS < groups_per_face ? g0 + SI_GROUPS : groups_per_face;
  const int *ss = slot_seed + (size_t)face * groups_per_face * BL_SLOTS;
  for (int j = tid; j < SI_WAVES * m; j += SI_BLOCK) cnt[j] = 0;
  __syncthreads();
  constexpr int GPW = SI_GROUPS / SI_WAVES;            // groups per wave, consecutive
  int *mine = cnt + wave * m;
  int sv[GPW];
#pragma unroll
  for (int u = 0; u < GPW; ++u) {
    const int g = g0 + wave * GPW + u;
    int v = -1;
    if (g < g1 && lane < BL_SLOTS) v = ss[(size_t)g * BL_SLOTS + lane];
    sv[u] = (v >= 0 && v < m) ? v : -1;
  }
#pragma unroll
  for (int u = 0; u < GPW; ++u)
    if (sv[u] >= 0) atomicAdd(&mine[sv[u]], 1);        // (distinct bins inside a group)
  __syncthreads();
  counting_sort_starts<SI_BLOCK>(cnt, m, scratch, offs + ((size_t)face * nchunk + chunk) * (m + 1));
  int *ord = order + ((size_t)face * nchunk + chunk) * (SI_GROUPS * BL_SLOTS);
#pragma unroll
  for (int u = 0; u < GPW; ++u) {                      // groups in order: the stable placement
    if (sv[u] >= 0) {
      const int pos = atomicAdd(&mine[sv[u]], 1);      // (one lane per cursor inside a group)
      ord[pos] = (g0 + wave * GPW + u) * BL_SLOTS + lane;
    }
  }
}

// lane = CPT consecutive channels (one 4 * CPT-byte load per row and lane: 1 KB rows move as ONE
// 16-byte-per-lane instruction at C = 256)
template <int CPT>
__global__ __launch_bounds__(256) void blend_bwd_gather_kernel(
    int m, int segs, int pitch, int seg_off, int slots_per_face, int nchunk,
    const float *__restrict__ stage, const int *__restrict__ order, const int *__restrict__ offs,
    float *__restrict__ d_table, int nb) {
  constexpr int C = CPT * 64;
  // CPT floats per lane as one load (CPT = 3 is padded to 16 bytes as a vector type: three scalars)
  struct Row {
    float v[CPT];
    __device__ __forceinline__ void load(const float *p) {
      if constexpr (CPT == 4) { const float4 t = *(const float4 *)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
      else if constexpr (CPT == 2) { const float2 t = *(const float2 *)p; v[0] = t.x; v[1] = t.y; }
      else {
#pragma unroll
        for (int e = 0; e < CPT; ++e) v[e] = p[e];
      }
    }
    __device__ __forceinline__ void store(float *p) const {
      if constexpr (CPT == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
      else if constexpr (CPT == 2) *(float2 *)p = make_float2(v[0], v[1]);
      else {
#pragma unroll
        for (int e = 0; e < CPT; ++e) p[e] = v[e];
      }
    }
  };
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long long)nb * segs * m) return;
  // seed fastest: the four waves of a workgroup write neighbouring d_table rows
  const int seed = (int)(w % m), face = (int)(w / m);                      // face = bi * segs + sg
  const int bi = face / segs, sg = face % segs;
  // run bounds of this seed in every chunk: lane c holds chunk c's (lo, hi)
  int lo = 0, hi = 0;
  if (lane < nchunk) {
    const int *of = offs + ((size_t)face * nchunk + lane) * (m + 1) + seed;
    lo = of[0]; hi = of[1];
  }
  const float *base = stage + (size_t)face * slots_per_face * C + lane * CPT;
  Row acc;
#pragma unroll
  for (int e = 0; e < CPT; ++e) acc.v[e] = 0.f;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int l = __builtin_amdgcn_readlane(lo, ch), h = __builtin_amdgcn_readlane(hi, ch);
    const int *ob = order + ((size_t)face * nchunk + ch) * (SI_GROUPS * BL_SLOTS);
    for (int j0 = l; j0 < h; j0 += 64) {               // (a seed rarely has more than 64 slots per chunk)
      const int cntj = h - j0 < 64 ? h - j0 : 64;
      const int myslot = lane < cntj ? ob[j0 + lane] : 0;
      int u = 0;
      for (; u + 3 < cntj; u += 4) {                   // four rows in flight, added in order
        Row v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k].load(base + (size_t)__builtin_amdgcn_readlane(myslot, u + k) * C);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int e = 0; e < CPT; ++e) acc.v[e] += v[k].v[e];
      }
      for (; u < cntj; ++u) {
        Row v;
        v.load(base + (size_t)__builtin_amdgcn_readlane(myslot, u) * C);
#pragma unroll
        for (int e = 0; e < CPT; ++e) acc.v[e] += v.v[e];
      }
    }
  }
  acc.store(d_table + ((size_t)bi * m + seed) * pitch + (size_t)sg * seg_off + lane * CPT);
}

// grad_out (B,C,N) -> grad_points (B,C,M) += w * g   (3 float atomics, .cu:81-83)
__global__ __launch_bounds__(TI_BLOCK) void three_interpolate_grad_kernel(
    int c, int n, int m, const float *__restrict__ grad_out, const int *__restrict__ idx,
    const float *__restrict__ weight, float *__restrict__ grad_points) {
  const int p = blockIdx.x * TI_BLOCK + threadIdx.x;
  const int c0 = blockIdx.y * TI_CH;
  const int bi = blockIdx.z;
  if (p >= n) return;
  const int *ix = idx + ((size_t)bi * n + p) * 3;
  const float *w = weight + ((size_t)bi * n + p) * 3;
  int j0 = ix[0], j1 = ix[1], j2 = ix[2];
  j0 = j0 < 0 ? 0 : (j0 >= m ? m - 1 : j0);
  j1 = j1 < 0 ? 0 : (j1 >= m ? m - 1 : j1);
  j2 = j2 < 0 ? 0 : (j2 >= m ? m - 1 : j2);
  const float w0 = w[0], w1 = w[1], w2 = w[2];
  const int cend = c - c0 < TI_CH ? c - c0 : TI_CH;
#pragma unroll
  for (int i = 0; i < TI_CH; ++i) {
    if (i < cend) {
      const float g = grad_out[((size_t)bi * c + c0 + i) * n + p];
      float *dst = grad_points + ((size_t)bi * c + c0 + i) * m;
      atomicAdd(dst + j0, __fmul_rn(g, w0));
      atomicAdd(dst + j1, __fmul_rn(g, w1));
      atomicAdd(dst + j2, __fmul_rn(g, w2));
    }
  }
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_three_nn_wrapper(int b, int n, int m, const float *unknown,
                                      const float *known, float *dist2, int *idx,
                                      void *stream) {
  const char *W = "three_nn_wrapper";
  NESIE_REQUIRE(b >= 0 && n >= 0 && m >= 0, W);
  if (b == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(unknown && dist2 && idx && (m == 0 || known), W);
  NESIE_REQUIRE(b <= 65535 && (long long)n * 3 < (1ll << 31) && (long long)m * 3 < (1ll << 31), W);
  with_distance_form([&](auto form) {
    hipLaunchKernelGGL(three_nn_kernel<decltype(form)::value>, dim3(cdiv(n, NN_BLOCK), b), dim3(NN_BLOCK), 0,
                       (hipStream_t)stream, n, m, unknown, known, dist2, idx);
  });
  return check_launch(W);
}

extern "C" int nesie_grid_taps(int b, int kprop, int gp, int m, const float *centre,
                               const float *size, const float *heading, const float *mult,
                               const float *plane, const float *known, int *idx, float *weight,
                               float *rel, void *stream) {
  const char *W = "grid_taps";
  NESIE_REQUIRE(b >= 0 && kprop >= 0 && gp >= 0 && m >= 0, W);
  if (b == 0 || kprop == 0 || gp == 0) return NESIE_OK;
  NESIE_REQUIRE(m >= 3 && centre && size && heading && mult && plane && known, W);
  NESIE_REQUIRE(idx && weight && rel && b <= 65535 && (long long)kprop * gp * 3 < (1ll << 31), W);
  with_distance_form([&](auto form) {   // (mmcv.ops.three_nn is an nvcc build as well)
    hipLaunchKernelGGL(grid_taps_kernel<decltype(form)::value>, dim3(cdiv((long long)kprop * gp, NN_BLOCK), b),
                       dim3(NN_BLOCK), 0, (hipStream_t)stream, kprop, gp, m, centre, size, heading, mult,
                       plane, known, idx, weight, rel);
  });
  return check_launch(W);
}

extern "C" int nesie_three_interpolate_wrapper(int b, int c, int m, int n,
                                               const float *points, const int *idx,
                                               const float *weight, float *out,
                                               void *stream) {
  const char *W = "three_interpolate_wrapper";
  NESIE_REQUIRE(b >= 0 && c >= 0 && m >= 0 && n >= 0, W);
  if (b == 0 || c == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(m >= 1 && points && idx && weight && out, W);
  NESIE_REQUIRE(b <= 65535 && cdiv(c, TI_CH) <= 65535, W);
  hipLaunchKernelGGL(three_interpolate_kernel, dim3(cdiv(n, TI_BLOCK), cdiv(c, TI_CH), b),
                     dim3(TI_BLOCK), 0, (hipStream_t)stream, c, m, n, points, idx, weight,
                     out);
  return check_launch(W);
}

static int blend_check(const char *W, int b, int c, int m, int n, int segs, int seg_len,
                       int pitch, int seg_off) {
  NESIE_REQUIRE(b >= 0 && c >= 0 && m >= 0 && n >= 0 && segs >= 1 && seg_len >= 1, W);
  NESIE_REQUIRE(n % (segs * seg_len) == 0 && seg_off >= 0, W);
  NESIE_REQUIRE(pitch >= (long long)(segs - 1) * seg_off + c, W);
  NESIE_REQUIRE(b <= 65535 && cdiv(c, TI_CH) <= 65535, W);
  return NESIE_OK;
}

// `chunks` workgroup columns of 64 * CPT channels each, the first at channel cb.  The tile and the
// statistics scratch are dynamic LDS (73 KB at CPT = 4: two workgroups per CU).
template <int CPT>
static void blend_fwd_launch(int chunks, int cb, int b, int c, int m, int n, int segs, int seg_len,
                             int c_total, int c_offset, int pitch, int seg_off, const float *table,
                             const int *idx, const float *weight, const float *rel, const float *wx,
                             float *out, float *stat_partial, hipStream_t s) {
  if (chunks <= 0) return;
  constexpr int CW = CPT * 64;
  const size_t lds = (size_t)CW * (BF_LD + 4 * 2) * sizeof(float);
  const dim3 grid((unsigned)((n / TS_Q) * b), (unsigned)chunks);
  with_bool(wx != nullptr, [&](auto WXF) {
    with_bool(stat_partial != nullptr, [&](auto STF) {
      launch_lds<blend_fwd_kernel<CPT, WXF(), STF()>>(grid, dim3(256), lds, s, c, cb, m, n, segs, seg_len, c_total,
                                                      c_offset, pitch, seg_off, table, idx, weight, rel, wx, out,
                                                      stat_partial, b);
    });
  });
}

extern "C" int nesie_blend_conv_forward(int b, int c, int m, int n, const float *table,
                                        int pitch, int seg_off, const int *idx,
                                        const float *weight, const float *rel, const float *wx,
                                        float *out, int segs, int seg_len, int c_total,
                                        int c_offset, float *stat_partial, void *stream) {
  const char *W = "blend_conv_forward";
  int st = blend_check(W, b, c, m, n, segs, seg_len, pitch, seg_off);
  if (st) return st;
  NESIE_REQUIRE(c_offset >= 0 && c_offset + c <= c_total && (wx == nullptr) == (rel == nullptr), W);
  if (b == 0 || c == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(m >= 1 && table && idx && weight && out, W);
  if (stat_partial && !(c % 64 == 0 && (n / segs) % TS_Q == 0)) {
    set_error("%s: stat_partial needs c %% 64 == 0 and %d-multiple faces", W, TS_Q);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (c % 64 == 0 && (n / segs) % TS_Q == 0) {
    NESIE_REQUIRE((long long)(n / TS_Q) * b < (1ll << 31) && ((uintptr_t)out & 15) == 0, W);   // (float4 row stores)
    // whole chunks of 256 channels along grid y, then the 64 / 128 / 192 that remain
    blend_fwd_launch<4>(c / 256, 0, b, c, m, n, segs, seg_len, c_total, c_offset, pitch, seg_off, table,
                        idx, weight, rel, wx, out, stat_partial, (hipStream_t)stream);
    const int cb = c / 256 * 256, left = (c - cb) / 64;
    with_int<1, 2, 3>(left, [&](auto CPT) {   // (0: nothing remains)
      blend_fwd_launch<CPT()>(1, cb, b, c, m, n, segs, seg_len, c_total, c_offset, pitch, seg_off, table, idx,
                              weight, rel, wx, out, stat_partial, (hipStream_t)stream);
    });
  } else
    hipLaunchKernelGGL(blend_fwd_generic_kernel, dim3(cdiv(n, TI_BLOCK), cdiv(c, TI_CH), b),
                       dim3(TI_BLOCK), 0, (hipStream_t)stream, c, m, n, segs, seg_len, c_total,
                       c_offset, pitch, seg_off, table, idx, weight, rel, wx, out);
  return check_launch(W);
}

extern "C" int nesie_blend_conv_runs(int n, int segs) {
  return segs >= 1 && n >= 0 ? cdiv(n / segs, BL_RUN) : 0;
}

// staging workspace of the STAGED backward: rows [b * segs * groups * 48][c] floats, then
// slot_seed and order (one int per slot each; order chunk-major, SI_GROUPS * 48 per chunk) and the
// run starts offs [faces * chunks][SI_MAX_BINS]
static size_t blend_stage_slots(int b, int n, int segs) { return (size_t)b * (n / 16) * BL_SLOTS; }   // n / 16 groups in all
static int blend_index_chunks(int n, int segs) { return cdiv(n / segs / 16, SI_GROUPS); }

extern "C" size_t nesie_blend_conv_backward_workspace_bytes(int b, int c, int n, int segs) {
  if (b <= 0 || c <= 0 || n <= 0 || segs <= 0) return 0;
  const size_t slots = blend_stage_slots(b, n, segs);
  const size_t order_ints = (size_t)b * segs * blend_index_chunks(n, segs) * SI_GROUPS * BL_SLOTS;
  const size_t offs_ints = (size_t)b * segs * blend_index_chunks(n, segs) * SI_MAX_BINS;
  return slots * c * sizeof(float) + (slots + order_ints + offs_ints) * sizeof(int);
}

static int blend_conv_backward_impl(const char *W, int b, int c, int m, int n, const float *dy,
                                    int pitch, int seg_off, const int *idx, const float *weight,
                                    const float *rel, float *d_table, float *d_wx, int segs,
                                    int seg_len, const float *bnz, const float *bnb, void *stream,
                                    void *workspace = nullptr, size_t workspace_bytes = 0) {
  int st = blend_check(W, b, c, m, n, segs, seg_len, pitch, seg_off);
  if (st) return st;
  if (b == 0 || c == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(m >= 1 && dy && idx && weight && d_table && segs <= 65535, W);
  NESIE_REQUIRE((d_wx == nullptr) || rel, W);
  const int per_seg = n / segs;
  if (c % 64 != 0 || c > 256 || per_seg % TS_Q != 0) {
    set_error("%s: c %d (needs 64, 128, 192 or 256) / %d queries per face (needs a multiple "
              "of %d)", W, c, per_seg, TS_Q);
    return NESIE_ERR_UNSUPPORTED;
  }
  const int nruns = cdiv(per_seg, BL_RUN);
  NESIE_REQUIRE((long long)nruns * b * segs < (1ll << 31), W);
  const dim3 grid((unsigned)(nruns * b * segs));
  hipStream_t s = (hipStream_t)stream;
  // STAGED (workspace): no float atomics, d_table written (not accumulated), reproducible
  float *stage = nullptr;
  int *slot_seed = nullptr, *order = nullptr, *offs = nullptr;
  const int groups_per_face = per_seg / 16, slots_per_face = groups_per_face * BL_SLOTS;
  const int nchunk = blend_index_chunks(n, segs);
  if (workspace) {
    const size_t slots = blend_stage_slots(b, n, segs);
    NESIE_REQUIRE(workspace_bytes >= nesie_blend_conv_backward_workspace_bytes(b, c, n, segs), W);
    NESIE_REQUIRE(((uintptr_t)workspace & 15) == 0 && m + 1 <= SI_MAX_BINS, W);     // (the index: <= 2048 bins)
    NESIE_REQUIRE(pitch % 4 == 0 && seg_off % 4 == 0 && ((uintptr_t)d_table & 15) == 0, W);   // (vector row stores)
    NESIE_REQUIRE(nchunk <= 64 && (long long)b * segs * nchunk < (1ll << 31) &&
                  (long long)b * segs * m < (1ll << 33), W);
    stage = (float *)workspace;
    slot_seed = (int *)(stage + slots * c);
    order = slot_seed + slots;
    offs = order + (size_t)b * segs * nchunk * SI_GROUPS * BL_SLOTS;
  }
  const bool built = with_int<1, 2, 3, 4>(c / 64, [&](auto CPT) {
    with_bool(bnb != nullptr, [&](auto BNB) {
      with_bool(workspace != nullptr, [&](auto STAGED) {
        hipLaunchKernelGGL((blend_bwd_rows_kernel<CPT(), BNB(), STAGED()>), grid, dim3(256), 0, s, m, n, segs,
                           seg_len, pitch, seg_off, dy, idx, weight, rel, d_table, d_wx, b, nruns, bnz, bnb, stage,
                           slot_seed);
      });
    });
    if (!workspace) return;
    launch_lds<blend_slot_index_kernel, ((size_t)SI_WAVES * SI_MAX_BINS + SI_WAVES) * sizeof(int)>(
        dim3((unsigned)(b * segs * nchunk)), dim3(SI_BLOCK), ((size_t)SI_WAVES * m + SI_WAVES) * sizeof(int), s, m,
        groups_per_face, nchunk, slot_seed, order, offs);
    const long long waves = (long long)b * segs * m;
    hipLaunchKernelGGL((blend_bwd_gather_kernel<CPT()>), dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, m, segs,
                       pitch, seg_off, slots_per_face, nchunk, stage, order, offs, d_table, b);
  });
  NESIE_REQUIRE(built, W);
  return check_launch(W);
}

// The same two entry points with the staging workspace: reproducible (no float atomics), d_table is
// WRITTEN in full (no zero fill needed).  workspace = nesie_blend_conv_backward_workspace_bytes.
extern "C" int nesie_blend_conv_backward_staged(int b, int c, int m, int n, const float *dy, const float *z,
                                                const float *bnb, int pitch, int seg_off, const int *idx,
                                                const float *weight, const float *rel, float *d_table,
                                                float *d_wx, int segs, int seg_len, void *workspace,
                                                size_t workspace_bytes, void *stream) {
  const char *W = "blend_conv_backward_staged";
  NESIE_REQUIRE(workspace && (z == nullptr) == (bnb == nullptr), W);
  return blend_conv_backward_impl(W, b, c, m, n, dy, pitch, seg_off, idx, weight, rel, d_table, d_wx, segs,
                                  seg_len, z, bnb, stream, workspace, workspace_bytes);
}

extern "C" int nesie_blend_conv_backward(int b, int c, int m, int n, const float *dy,
                                         int pitch, int seg_off, const int *idx,
                                         const float *weight, const float *rel,
                                         float *d_table, float *d_wx, int segs, int seg_len,
                                         void *stream) {
  return blend_conv_backward_impl("blend_conv_backward", b, c, m, n, dy, pitch, seg_off, idx, weight, rel,
                                  d_table, d_wx, segs, seg_len, nullptr, nullptr, stream);
}

extern "C" int nesie_blend_conv_backward_bn(int b, int c, int m, int n, const float *da, const float *z,
                                            const float *bnb, int pitch, int seg_off, const int *idx,
                                            const float *weight, const float *rel, float *d_table,
                                            float *d_wx, int segs, int seg_len, void *stream) {
  const char *W = "blend_conv_backward_bn";
  NESIE_REQUIRE(b == 0 || c == 0 || n == 0 || (z && bnb), W);
  return blend_conv_backward_impl(W, b, c, m, n, da, pitch, seg_off, idx, weight, rel, d_table, d_wx, segs,
                                  seg_len, z, bnb, stream);
}

extern "C" int nesie_three_interpolate_grad_wrapper(int b, int c, int n, int m,
                                                    const float *grad_out,
                                                    const int *idx, const float *weight,
                                                    float *grad_points, void *stream) {
  const char *W = "three_interpolate_grad_wrapper";
  NESIE_REQUIRE(b >= 0 && c >= 0 && m >= 0 && n >= 0, W);
  if (b == 0 || c == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(m >= 1 && grad_out && idx && weight && grad_points, W);
  NESIE_REQUIRE(b <= 65535 && cdiv(c, TI_CH) <= 65535, W);
  hipLaunchKernelGGL(three_interpolate_grad_kernel,
                     dim3(cdiv(n, TI_BLOCK), cdiv(c, TI_CH), b), dim3(TI_BLOCK), 0,
                     (hipStream_t)stream, c, n, m, grad_out, idx, weight, grad_points);
  return check_launch(W);
}
