// PAConv's assign_score_withk for gfx950 (semantics: include/nesie_ops.h).
//
// Replaces assign_score_withk_{forward,backward_points,backward_scores}_kernel (reference
// mmdet3d/ops/paconv/src/assign_score_withk_cuda.cu:38-141): one thread per (b, o, n, k, m) product
// with an atomicAdd into the output, and two kernels of atomicAdd scatters for the backward.  Here
// every output element has ONE owner that adds its terms in a fixed order; nothing is atomic.
//
//   forward       a workgroup owns one centre n and up to 256 output channels.  The centre row
//                 C[cn, m-tile, o-chunk] is staged in LDS once and shared by the centre's pairs;
//                 a thread owns up to eight (pair, 4 channels) items, streams the gathered rows
//                 P[kn, m, o..o+3] with 16-byte loads and keeps one accumulator chain per output
//                 element (m ascending).  The (B, O, N1, K) output is k-fastest while the reads are
//                 o-fastest: the tile goes through LDS (rows permuted so that the four channels of
//                 a lane land a whole pitch apart) and leaves as runs of K contiguous floats.
//   grad_scores   a workgroup owns one centre; each wave takes four pairs at a time and stages
//                 (P[kn] - C[cn])[16 m][32 o] per pair in LDS (pitch 33), lane (pair, m) then walks
//                 its row with o ascending against the pair's gradient row.
//   grad_points / grad_centers
//                 grad_out is first transposed to (B, N1*K, O), so a pair's gradient is one
//                 contiguous row.  knn_idx is narrowed to int32 with invalid entries sent to the
//                 sentinel source N0, nesie_inverted_index sorts the pairs by source point (and the
//                 centres by cn), a workgroup finds its source row's run by bisection and walks it
//                 in ascending n*K + k.  The sentinel's run is never visited.
//
// Scalar lanes (V = 1) serve O % 4 != 0 or a base that is not 16-byte aligned.
#include "common.h"

namespace nesie {

constexpr int PA_BLOCK = 256;
constexpr int PA_KT = 32;      // pairs per forward output tile
constexpr int PA_MT = 16;      // bank kernels per staged tile
constexpr int PA_UNITS = 64;   // V-wide channel units per forward chunk
constexpr int PA_R = PA_KT * PA_UNITS / PA_BLOCK;   // items per thread in the forward (8)
constexpr int PA_SR = 4;       // items per thread in the scatter
constexpr int PA_GO = 32;      // channels per grad_scores slab
constexpr int PA_GP = PA_GO + 1;

template <int V>
__device__ __forceinline__ void pa_load(const float *p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *(const float4 *)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void pa_store(float *p, const float (&v)[V]) {
  if constexpr (V == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

template <int V>
__global__ __launch_bounds__(PA_BLOCK) void paconv_fwd_kernel(
    int n0, int n1, int K, int M, int O, int ochunks, const float *__restrict__ points,
    const float *__restrict__ centers, const float *__restrict__ scores,
    const long long *__restrict__ knn, float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ctile[PA_MT * PA_UNITS * V];
  __shared__ float otile[PA_UNITS * V * (PA_KT + 1)];
  __shared__ int kn_s[PA_KT];
  const int tid = threadIdx.x;
  const int oc = blockIdx.x % ochunks;
  const int bn = blockIdx.x / ochunks;   // b * n1 + n
  const int b = bn / n1, n = bn - b * n1;
  const int o0 = oc * PA_UNITS * V;
  const int ow = O - o0 < PA_UNITS * V ? O - o0 : PA_UNITS * V;
  const int units = (ow + V - 1) / V;    // V == 4 only with O % 4 == 0: exact
  const long long *kr = knn + (size_t)bn * K;
  const long long cn = kr[0];
  const bool cvalid = cn >= 0 && cn < n0;
  const float *crow = centers + ((size_t)b * n0 + (cvalid ? cn : 0)) * M * O + o0;
  const float *pbase = points + (size_t)b * n0 * M * O + o0;
  const float *srow = scores + (size_t)bn * K * M;

  for (int k0 = 0; k0 < K; k0 += PA_KT) {
    const int kw = K - k0 < PA_KT ? K - k0 : PA_KT;
    const int items = kw * units;
    __syncthreads();   // the previous tile has left otile; kn_s is free
    if (tid < PA_KT) {
      const long long v = tid < kw ? kr[k0 + tid] : -1;
      kn_s[tid] = (v >= 0 && v < n0) ? (int)v : -1;
    }
    float acc[PA_R][V];
#pragma unroll
    for (int r = 0; r < PA_R; ++r)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[r][j] = 0.f;

    for (int m0 = 0; m0 < M; m0 += PA_MT) {
      const int mw = M - m0 < PA_MT ? M - m0 : PA_MT;
      __syncthreads();   // kn_s written; the previous centre tile is consumed
      for (int i = tid; i < mw * units; i += PA_BLOCK) {
        const int mm = i / units, u = i - mm * units;
        float c[V];
        if (cvalid) {
          pa_load<V>(crow + (size_t)(m0 + mm) * O + u * V, c);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) c[j] = 0.f;   // an out-of-range centre index: a zero row
        }
        pa_store<V>(ctile + (mm * PA_UNITS + u) * V, c);
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < PA_R; ++r) {
        const int it = tid + r * PA_BLOCK;
        if (it >= items) continue;
        const int kk = it / units, u = it - kk * units;
        const int kn = kn_s[kk];
        if (kn < 0) continue;   // an invalid pair stays exactly 0
        const float *pr = pbase + ((size_t)kn * M + m0) * O + u * V;
        const float *sr = srow + (size_t)(k0 + kk) * M + m0;
        for (int mm = 0; mm < mw; ++mm) {
          float p[V], c[V];
          pa_load<V>(pr + (size_t)mm * O, p);
          pa_load<V>(ctile + (mm * PA_UNITS + u) * V, c);
          const float s = sr[mm];
#pragma unroll
          for (int j = 0; j < V; ++j) acc[r][j] = __fmaf_rn(s, __fsub_rn(p[j], c[j]), acc[r][j]);
        }
      }
    }
    // tile row j * units + u holds channel o0 + u * V + j: a lane's V channels lie `units` rows
    // apart, consecutive lanes one row (PA_KT + 1 words) apart
#pragma unroll
    for (int r = 0; r < PA_R; ++r) {
      const int it = tid + r * PA_BLOCK;
      if (it >= items) continue;
      const int kk = it / units, u = it - kk * units;
#pragma unroll
      for (int j = 0; j < V; ++j) otile[(j * units + u) * (PA_KT + 1) + kk] = acc[r][j];
    }
    __syncthreads();
    const int rows = units * V;   // == ow
    for (int i = tid; i < rows * kw; i += PA_BLOCK) {
      const int row = i / kw, kk = i - row * kw;
      const int j = row / units, u = row - j * units;
      const int o = o0 + u * V + j;
      out[(((size_t)b * O + o) * n1 + n) * K + k0 + kk] = otile[row * (PA_KT + 1) + kk];
    }
  }
}

// idx32[b, n, k] = knn_idx narrowed, an invalid entry -> the sentinel source n0; cn32[b, n] likewise
__global__ __launch_bounds__(PA_BLOCK) void paconv_prep_kernel(
    long long pairs, int K, int n0, const long long *__restrict__ knn, int *__restrict__ idx32,
    int *__restrict__ cn32) {
  const long long i = (long long)blockIdx.x * PA_BLOCK + threadIdx.x;
  if (i >= pairs) return;
  const long long v = knn[i];
  const int s = (v >= 0 && v < n0) ? (int)v : n0;
  idx32[i] = s;
  if (i % K == 0) cn32[i / K] = s;
}

// g (B, O, E) -> gT (B, E, O)
__global__ __launch_bounds__(PA_BLOCK) void paconv_transpose_kernel(
    int O, int E, int tiles_o, int tiles_e, const float *__restrict__ g, float *__restrict__ gT) {
  __shared__ float t[32][33];
  const int te = blockIdx.x % tiles_e;
  const int to = (blockIdx.x / tiles_e) % tiles_o;
  const int b = blockIdx.x / (tiles_e * tiles_o);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int o = to * 32 + ty + j * 8, e = te * 32 + tx;
    if (o < O && e < E) t[ty + j * 8][tx] = g[((size_t)b * O + o) * E + e];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = te * 32 + ty + j * 8, o = to * 32 + tx;
    if (o < O && e < E) gT[((size_t)b * E + e) * O + o] = t[tx][ty + j * 8];
  }
}

// grad_scores[b, n, k, m] = sum_o (P[kn, m, o] - C[cn, m, o]) * gT[b, n*K + k, o], o ascending
__global__ __launch_bounds__(PA_BLOCK) void paconv_grad_scores_kernel(
    int n0, int n1, int K, int M, int O, int vec, const float *__restrict__ points,
    const float *__restrict__ centers, const float *__restrict__ gT,
    const long long *__restrict__ knn, float *__restrict__ gs) {
  __shared__ float D_all[4][64 * PA_GP];
  __shared__ float G_all[4][4 * PA_GO];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *D = D_all[wave], *G = G_all[wave];
  const int bn = blockIdx.x;
  const int b = bn / n1;
  const long long *kr = knn + (size_t)bn * K;
  const long long cn = kr[0];
  const bool cvalid = cn >= 0 && cn < n0;
  const float *crow = centers + ((size_t)b * n0 + (cvalid ? cn : 0)) * M * O;
  const float *pbase = points + (size_t)b * n0 * M * O;
  const int my_kk = lane >> 4, my_mm = lane & 15;

  for (int kg = 0; kg < K; kg += 16) {
    const int kbase = kg + wave * 4;   // this wave's four pairs
    long long my_kn = kbase + my_kk < K ? kr[kbase + my_kk] : -1;
    const bool my_valid = my_kn >= 0 && my_kn < n0;
    for (int m0 = 0; m0 < M; m0 += PA_MT) {
      float acc = 0.f;
      for (int o0 = 0; o0 < O; o0 += PA_GO) {
        const int ow = O - o0 < PA_GO ? O - o0 : PA_GO;
        __syncthreads();   // the previous slab is consumed
        // slab row r = (pair r >> 4, kernel r & 15), 32 channels: 8 lanes x 4 channels per row
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int r = it * 8 + (lane >> 3), c4 = (lane & 7) * 4;
          const int k = kbase + (r >> 4), m = m0 + (r & 15);
          float d[4] = {0.f, 0.f, 0.f, 0.f};
          if (k < K && m < M && c4 < ow) {
            const long long kn = kr[k];
            if (kn >= 0 && kn < n0) {
              const float *pp = pbase + ((size_t)kn * M + m) * O + o0 + c4;
              const float *cp = crow + (size_t)m * O + o0 + c4;
              if (vec) {   // O % 4 == 0: c4 < ow means c4 + 3 < ow
                const float4 p = *(const float4 *)pp;
                float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                if (cvalid) c = *(const float4 *)cp;
                d[0] = __fsub_rn(p.x, c.x); d[1] = __fsub_rn(p.y, c.y);
                d[2] = __fsub_rn(p.z, c.z); d[3] = __fsub_rn(p.w, c.w);
              } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  if (c4 + j < ow) d[j] = __fsub_rn(pp[j], cvalid ? cp[j] : 0.f);
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) D[r * PA_GP + c4 + j] = d[j];
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const int i = it * 64 + lane, kk = i >> 5, oo = i & 31;
          const int k = kbase + kk;
          G[i] = (k < K && oo < ow) ? gT[((size_t)bn * K + k) * O + o0 + oo] : 0.f;
        }
        __syncthreads();
        const float *dr = D + lane * PA_GP, *gr = G + my_kk * PA_GO;
        for (int oo = 0; oo < ow; ++oo) acc = __fmaf_rn(dr[oo], gr[oo], acc);
      }
      const int k = kbase + my_kk, m = m0 + my_mm;
      if (k < K && m < M) gs[((size_t)bn * K + k) * M + m] = my_valid ? acc : 0.f;
    }
  }
}

// One workgroup per (source row, chunk of PA_BLOCK * PA_SR items); an item is V consecutive
// channels of one bank kernel, so item i covers the floats [i * V, i * V + V) of the row.
//   CENTER = false: the index is over the pairs; entry e = n*K + k contributes  s[e, m] * gT[e, o]
//   CENTER = true:  the index is over the centres; entry n contributes its valid pairs k = 0 .. K-1
//                   in turn, and the row is negated at the end
template <int V, bool CENTER>
__global__ __launch_bounds__(PA_BLOCK) void paconv_scatter_kernel(
    int n0, int K, int M, int O, int entries, int pairs, int chunks,
    const float *__restrict__ scores, const float *__restrict__ gT, const int *__restrict__ idx32,
    const int *__restrict__ order, const int *__restrict__ sources, float *__restrict__ grad) {
  const int chunk = blockIdx.x % chunks;
  const int row = blockIdx.x / chunks;   // b * n0 + j
  const int b = row / n0, j = row - b * n0;
  const int total = M * O / V;           // V == 4 only with O % 4 == 0
  int item[PA_SR], mi[PA_SR], off[PA_SR];
  float acc[PA_SR][V];
#pragma unroll
  for (int r = 0; r < PA_SR; ++r) {
    item[r] = chunk * (PA_BLOCK * PA_SR) + r * PA_BLOCK + threadIdx.x;
    const int it = item[r] < total ? item[r] : 0;
    mi[r] = it * V / O;
    off[r] = it * V - mi[r] * O;
#pragma unroll
    for (int q = 0; q < V; ++q) acc[r][q] = 0.f;
  }
  const int *sb = sources + (size_t)b * entries, *ob = order + (size_t)b * entries;
  const int *vb = idx32 + (size_t)b * pairs;
  const float *sc = scores + (size_t)b * pairs * M;
  const float *gb = gT + (size_t)b * pairs * O;
  int lo = 0, hi = entries;   // first sorted entry with source >= j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb[mid] < j) lo = mid + 1; else hi = mid;
  }
  auto add = [&](int e) {
#pragma unroll
    for (int r = 0; r < PA_SR; ++r) {
      if (item[r] >= total) continue;
      float g[V];
      pa_load<V>(gb + (size_t)e * O + off[r], g);
      const float s = sc[(size_t)e * M + mi[r]];
#pragma unroll
      for (int q = 0; q < V; ++q) acc[r][q] = __fmaf_rn(s, g[q], acc[r][q]);
    }
  };
  for (int i = lo; i < entries && sb[i] == j; ++i) {
    const int e0 = ob[i];
    if (CENTER) {
      for (int k = 0; k < K; ++k)
        if (vb[(size_t)e0 * K + k] < n0) add(e0 * K + k);
    } else {
      add(e0);
    }
  }
  float *orow = grad + (size_t)row * M * O;
#pragma unroll
  for (int r = 0; r < PA_SR; ++r) {
    if (item[r] >= total) continue;
    if (CENTER) {
#pragma unroll
      for (int q = 0; q < V; ++q) acc[r][q] = -acc[r][q];
    }
    pa_store<V>(orow + (size_t)item[r] * V, acc[r]);
  }
}

struct pa_sizes {
  long long pts, sc, out, pairs;
};

// NESIE_OK with `go` = whether there is anything to launch
static int pa_check(const char *W, int b, int n0, int n1, int k, int m, int o, pa_sizes *z, bool *go) {
  NESIE_REQUIRE(b >= 0 && n0 >= 0 && n1 >= 0 && k > 0 && m > 0 && o > 0, W);
  const long long lim = 1ll << 31;
  // the factors are below 2^31 each; stop before a product can leave 64 bits
  const long long mo = (long long)m * o, km = (long long)k * m, ko = (long long)k * o;
  const long long bn0 = (long long)b * n0, bn1 = (long long)b * n1;
  const bool fits = mo < lim && km < lim && ko < lim && bn0 < lim && bn1 < lim &&
                    bn0 * mo < lim && bn1 * km < lim && bn1 * ko < lim;
  if (!fits) {
    set_error("%s: a tensor of 2^31 elements or more (b %d, n0 %d, n1 %d, k %d, m %d, o %d)", W, b, n0,
              n1, k, m, o);
    return NESIE_ERR_UNSUPPORTED;
  }
  z->pts = bn0 * mo; z->sc = bn1 * km; z->out = bn1 * ko; z->pairs = bn1 * k;
  *go = b > 0 && n0 > 0 && n1 > 0;
  return NESIE_OK;
}

static inline size_t pa_round16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_assign_score_withk_forward(int b, int n0, int n1, int k, int m, int o,
                                                const float *points, const float *centers,
                                                const float *scores, const long long *knn_idx,
                                                float *output, void *stream) {
  const char *W = "assign_score_withk_forward";
  pa_sizes z;
  bool go;
  const int st = pa_check(W, b, n0, n1, k, m, o, &z, &go);
  if (st || !go) return st;
  NESIE_REQUIRE(points && centers && scores && knn_idx && output, W);
  const bool vec = o % 4 == 0 && aligned16(points) && aligned16(centers);
  const int per = PA_UNITS * (vec ? 4 : 1);
  const int ochunks = cdiv(o, per);
  const long long grid = (long long)b * n1 * ochunks;   // <= elements of the output
  NESIE_REQUIRE(grid < (1ll << 31), W);
  with_int<4, 1>(vec ? 4 : 1, [&](auto V) {
    hipLaunchKernelGGL(paconv_fwd_kernel<V()>, dim3((unsigned)grid), dim3(PA_BLOCK), 0, (hipStream_t)stream, n0,
                       n1, k, m, o, ochunks, points, centers, scores, knn_idx, output);
  });
  return check_launch(W);
}

extern "C" size_t nesie_assign_score_withk_backward_workspace_bytes(int b, int n0, int n1, int k,
                                                                    int m, int o) {
  pa_sizes z;
  bool go;
  if (pa_check("assign_score_withk_backward_workspace_bytes", b, n0, n1, k, m, o, &z, &go) || !go)
    return 0;
  // gT | idx32, order, sources, scratch over the pairs | cn32, order, sources, scratch over the centres
  return pa_round16((size_t)z.out * sizeof(float)) + 4 * pa_round16((size_t)z.pairs * sizeof(int)) +
         4 * pa_round16((size_t)b * n1 * sizeof(int));
}

extern "C" int nesie_assign_score_withk_backward(int b, int n0, int n1, int k, int m, int o,
                                                 const float *grad_out, const float *points,
                                                 const float *centers, const float *scores,
                                                 const long long *knn_idx, float *grad_points,
                                                 float *grad_centers, float *grad_scores,
                                                 void *workspace, size_t workspace_bytes,
                                                 void *stream) {
  const char *W = "assign_score_withk_backward";
  pa_sizes z;
  bool go;
  int st = pa_check(W, b, n0, n1, k, m, o, &z, &go);
  if (st || !go) return st;
  if (!grad_points && !grad_centers && !grad_scores) return NESIE_OK;
  NESIE_REQUIRE(grad_out && knn_idx && workspace && aligned16(workspace), W);
  NESIE_REQUIRE(workspace_bytes >= nesie_assign_score_withk_backward_workspace_bytes(b, n0, n1, k, m, o), W);
  NESIE_REQUIRE(!grad_scores || (points && centers), W);
  NESIE_REQUIRE(!(grad_points || grad_centers) || scores, W);
  hipStream_t s = (hipStream_t)stream;
  const int pairs = n1 * k;   // per scene; b * n1 * k < 2^31
  char *w = (char *)workspace;
  float *gT = (float *)w;              w += pa_round16((size_t)z.out * sizeof(float));
  const size_t pstep = pa_round16((size_t)z.pairs * sizeof(int));
  int *idx32 = (int *)w, *p_order = (int *)(w + pstep), *p_src = (int *)(w + 2 * pstep),
      *p_tmp = (int *)(w + 3 * pstep);
  w += 4 * pstep;
  const size_t cstep = pa_round16((size_t)b * n1 * sizeof(int));
  int *cn32 = (int *)w, *c_order = (int *)(w + cstep), *c_src = (int *)(w + 2 * cstep),
      *c_tmp = (int *)(w + 3 * cstep);

  const int tiles_o = cdiv(o, 32), tiles_e = cdiv(pairs, 32);
  const long long tgrid = (long long)b * tiles_o * tiles_e;
  NESIE_REQUIRE(tgrid < (1ll << 31), W);
  hipLaunchKernelGGL(paconv_transpose_kernel, dim3((unsigned)tgrid), dim3(PA_BLOCK), 0, s, o, pairs,
                     tiles_o, tiles_e, grad_out, gT);
  NESIE_LAUNCHED(W);

  if (grad_scores) {
    const int vec = o % 4 == 0 && aligned16(points) && aligned16(centers);
    hipLaunchKernelGGL(paconv_grad_scores_kernel, dim3((unsigned)(b * n1)), dim3(PA_BLOCK), 0, s, n0, n1,
                       k, m, o, vec, points, centers, gT, knn_idx, grad_scores);
    NESIE_LAUNCHED(W);
  }
  if (!grad_points && !grad_centers) return NESIE_OK;

  hipLaunchKernelGGL(paconv_prep_kernel, dim3((unsigned)cdiv(z.pairs, PA_BLOCK)), dim3(PA_BLOCK), 0, s,
                     z.pairs, k, n0, knn_idx, idx32, cn32);
  NESIE_LAUNCHED(W);
  const bool vec = o % 4 == 0 && (!grad_points || aligned16(grad_points)) &&
                   (!grad_centers || aligned16(grad_centers));
  const int total = (int)((long long)m * o / (vec ? 4 : 1));
  const int chunks = cdiv(total, PA_BLOCK * PA_SR);
  const long long sgrid = (long long)b * n0 * chunks;   // <= elements of grad_points
  NESIE_REQUIRE(sgrid < (1ll << 31) && n0 < (1ll << 31) - 1, W);
  // grad[i] of a point (a centre: CENTER) from the `entries` pairs a scene has, through their inverted index
  auto scatter = [&](auto CENTER, int entries, const int *order, const int *src, float *grad) {
    with_int<4, 1>(vec ? 4 : 1, [&](auto V) {
      hipLaunchKernelGGL((paconv_scatter_kernel<V(), CENTER()>), dim3((unsigned)sgrid), dim3(PA_BLOCK), 0, s, n0, k,
                         m, o, entries, pairs, chunks, scores, gT, idx32, order, src, grad);
    });
  };
  if (grad_points) {
    if ((st = nesie_inverted_index(b, n0 + 1, pairs, idx32, p_order, p_src, p_tmp, stream))) return st;
    scatter(std::false_type(), pairs, p_order, p_src, grad_points);
    NESIE_LAUNCHED(W);
  }
  if (grad_centers) {
    if ((st = nesie_inverted_index(b, n0 + 1, n1, cn32, c_order, c_src, c_tmp, stream))) return st;
    scatter(std::true_type(), n1, c_order, c_src, grad_centers);
    NESIE_LAUNCHED(W);
  }
  return NESIE_OK;
}
