// Sparse 3-D convolution for gfx950 (the role of mmdet3d/ops/spconv; include/nesie_ops.h states the
// pinned semantics).  No dense grid, no float atomics, no slot handed out by an atomic.
//
// Rulebook = two gather tables built from sorted keys.
//   phase 1, nesie_spconv_out_sites
//     sc_in_keys_kernel   key of every input row, `cells` for a row outside the grid (the range
//                         test comes before the key is formed)
//     ix_sort             the stable radix sort (index_sort.hip) -> sorted_keys, sorted_rows
//     sc_mark_kernel      copies the sorted keys out, flags and counts the offending rows
//                         (outside the grid; every row of an equal-key run after its first)
//     regular conv        sc_cand_kernel forms the n * K candidate output keys (an impossible
//                         candidate carries the key `cells` of the output grid and sorts last),
//                         ix_sort on (key, i * K + k), sc_head_kernel + ix_scan: the scan value
//                         is the output row; sc_fill_kernel writes it to nbr_t and the head of
//                         every run writes its out_indices row
//     submanifold         M = n; sc_subm_nbrt_kernel binary-searches sorted_keys
//   phase 2, nesie_spconv_gather_table (the host knows M by now)
//     sc_table_kernel     a thread per (o, k) binary-searches sorted_keys for the site
//                         o * stride - padding + k and writes nbr[M, K] in full; the valid entries
//                         of every column are counted in LDS, then one integer atomic per column
//                         and workgroup (a count does not depend on the order of its increments)
//
// Feature products: sc_gather_gemm_kernel.  A workgroup owns 128 output rows x TN = 32 / 64 / 128
// destination channels for ALL taps; a wave owns 32 rows and TN / 32 accumulators of
// v_mfma_f32_32x32x2_f32 (issue interval = dependent latency, so one chain per accumulator runs at
// rate) which stay in registers across the taps and are stored once.  Per tap: the tile's table
// column goes to LDS, a workgroup vote skips a tap that nobody uses (and a wave vote the MFMAs of
// a wave whose 32 rows do not), the gathered source rows (zero rows for -1) and the c_src x TN
// slice of W[k] are staged 32 source channels at a time, 16-byte lanes when c_src % 4 == 0 and the
// base is aligned.  Channel tails are zero padding inside LDS only.  The weight is staged
// [k][n] (pitch = 32 mod 64: the two half-waves of a B read hit disjoint banks) or, read
// transposed, [n][k] with pitch 33, so the global read is coalesced either way.  The A tile is
// [row][k] with pitch 36 for the 16-byte stores; an A read meets a 2-way bank conflict (rows r and
// r + 16 share a bank): a known cost, unmeasured.  One output element = one accumulator chain:
// taps ascending, channels ascending inside a tap.
//
// Weight gradient: sc_wgrad_kernel, one workgroup per (row chunk, tap, 64 x 64 tile of dW[k]),
// the product G^T . dOut over the chunk's rows 32 at a time with the same MFMA (K = rows), partial
// products into scratch; sc_wgrad_sum_kernel adds the partials in ascending chunk order.
#include "common.h"
#include "index_sort.h"

namespace nesie {

constexpr int SC_BLOCK = 256;
constexpr int SC_MAX_KVOL = 512;  // taps: the LDS counters of sc_table_kernel

struct ScGeom {
  int batch, kvol;
  int in[3], out[3], k[3], s[3], p[3];
  unsigned cells_in, cells_out;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- rulebook
__global__ __launch_bounds__(SC_BLOCK) void sc_in_keys_kernel(long long n, ScGeom g,
                                                              const int *__restrict__ indices,
                                                              unsigned *__restrict__ keys,
                                                              int *__restrict__ idx) {
  const long long i = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int b = indices[i * 4], z = indices[i * 4 + 1], y = indices[i * 4 + 2],
            x = indices[i * 4 + 3];
  const bool ok = b >= 0 && b < g.batch && z >= 0 && z < g.in[0] && y >= 0 && y < g.in[1] &&
                  x >= 0 && x < g.in[2];
  keys[i] = ok ? (((unsigned)b * g.in[0] + z) * g.in[1] + y) * g.in[2] + x : g.cells_in;
  idx[i] = (int)i;
}

// m_subm >= 0: counts[0] = m_subm (a submanifold conv's M is n)
__global__ __launch_bounds__(SC_BLOCK) void sc_mark_kernel(long long n, unsigned cells,
                                                           const unsigned *__restrict__ keys,
                                                           const int *__restrict__ rows,
                                                           int *__restrict__ sorted_keys,
                                                           int *__restrict__ bad,
                                                           int *__restrict__ counts, int m_subm) {
  const long long j = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (j >= n) return;
  const unsigned k = keys[j];
  sorted_keys[j] = (int)k;
  const bool isbad = k == cells || (j > 0 && keys[j - 1] == k);
  bad[rows[j]] = isbad;
  if (isbad) atomicAdd(&counts[1], 1);
  if (j == 0 && m_subm >= 0) counts[0] = m_subm;
}

// the row of sorted_rows whose key is `key`, or -1.  Reads sorted_keys[0 .. n - 1] only.
__device__ __forceinline__ int sc_find(long long n, const int *__restrict__ sorted_keys,
                                       const int *__restrict__ sorted_rows, int key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (sorted_keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && sorted_keys[lo] == key) ? sorted_rows[lo] : -1;
}

__device__ __forceinline__ void sc_tap(const ScGeom &g, int k, int *t) {
  t[2] = k % g.k[2];
  t[1] = (k / g.k[2]) % g.k[1];
  t[0] = k / (g.k[2] * g.k[1]);
}

__global__ __launch_bounds__(SC_BLOCK) void sc_cand_kernel(long long nk, ScGeom g,
                                                           const int *__restrict__ indices,
                                                           const int *__restrict__ bad,
                                                           unsigned *__restrict__ keys,
                                                           int *__restrict__ payload) {
  const long long e = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (e >= nk) return;
  const long long i = e / g.kvol;
  const int k = (int)(e - i * g.kvol);
  unsigned key = g.cells_out;
  if (!bad[i]) {
    int t[3], o[3];
    sc_tap(g, k, t);
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long v = (long long)indices[i * 4 + 1 + a] + g.p[a] - t[a];  // = o * stride
      ok = ok && v >= 0 && v % g.s[a] == 0 && v / g.s[a] < g.out[a];
      o[a] = (int)(v / g.s[a]);
    }
    if (ok)
      key = (((unsigned)indices[i * 4] * g.out[0] + o[0]) * g.out[1] + o[1]) * g.out[2] + o[2];
  }
  keys[e] = key;
  payload[e] = (int)e;
}

__global__ __launch_bounds__(SC_BLOCK) void sc_head_kernel(long long nk, unsigned cells,
                                                           const unsigned *__restrict__ keys,
                                                           int *__restrict__ head) {
  const long long j = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (j >= nk) return;
  const unsigned k = keys[j];
  head[j] = k != cells && (j == 0 || keys[j - 1] != k);
}

__global__ __launch_bounds__(SC_BLOCK) void sc_fill_kernel(long long nk, ScGeom g,
                                                           const unsigned *__restrict__ keys,
                                                           const int *__restrict__ payload,
                                                           const int *__restrict__ heads_before,
                                                           int *__restrict__ nbr_t,
                                                           int *__restrict__ out_indices) {
  const long long j = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (j >= nk) return;
  const unsigned k = keys[j];
  if (k == g.cells_out) {
    nbr_t[payload[j]] = -1;
    return;
  }
  const bool head = j == 0 || keys[j - 1] != k;
  const long long row = heads_before[j] - (head ? 0 : 1);
  nbr_t[payload[j]] = (int)row;
  if (head) {
    unsigned r = k;
    out_indices[row * 4 + 3] = (int)(r % (unsigned)g.out[2]); r /= (unsigned)g.out[2];
    out_indices[row * 4 + 2] = (int)(r % (unsigned)g.out[1]); r /= (unsigned)g.out[1];
    out_indices[row * 4 + 1] = (int)(r % (unsigned)g.out[0]); r /= (unsigned)g.out[0];
    out_indices[row * 4 + 0] = (int)r;
  }
}

// submanifold: input row i feeds the output row at site i + padding - k
__global__ __launch_bounds__(SC_BLOCK) void sc_subm_nbrt_kernel(
    long long nk, long long n, ScGeom g, const int *__restrict__ indices,
    const int *__restrict__ bad, const int *__restrict__ sorted_keys,
    const int *__restrict__ sorted_rows, int *__restrict__ nbr_t) {
  const long long e = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (e >= nk) return;
  const long long i = e / g.kvol;
  const int k = (int)(e - i * g.kvol);
  int found = -1;
  if (!bad[i]) {
    int t[3], o[3];
    sc_tap(g, k, t);
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long v = (long long)indices[i * 4 + 1 + a] + g.p[a] - t[a];
      ok = ok && v >= 0 && v < g.in[a];
      o[a] = (int)v;
    }
    if (ok) {
      const unsigned key =
          (((unsigned)indices[i * 4] * g.in[0] + o[0]) * g.in[1] + o[1]) * g.in[2] + o[2];
      found = sc_find(n, sorted_keys, sorted_rows, (int)key);
    }
  }
  nbr_t[e] = found;
}

__global__ __launch_bounds__(SC_BLOCK) void sc_table_kernel(
    long long total, long long n, ScGeom g, int subm, const int *__restrict__ out_indices,
    const int *__restrict__ sorted_keys, const int *__restrict__ sorted_rows,
    int *__restrict__ nbr, int *__restrict__ pair_num) {
  __shared__ int cnt[SC_MAX_KVOL];
  for (int i = threadIdx.x; i < g.kvol; i += SC_BLOCK) cnt[i] = 0;
  __syncthreads();
  const long long e = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (e < total) {
    const long long o = e / g.kvol;
    const int k = (int)(e - o * g.kvol);
    const int b = out_indices[o * 4];
    int t[3], c[3], site[3];
    sc_tap(g, k, t);
    bool ok = b >= 0 && b < g.batch;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = out_indices[o * 4 + 1 + a];
      ok = ok && c[a] >= 0 && c[a] < g.out[a];
    }
    if (ok) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        // o * stride can pass 2^31 for a row that is no output site: form the site in 64 bits
        const long long v = (long long)c[a] * g.s[a] - g.p[a] + t[a];
        ok = ok && v >= 0 && v < g.in[a];
        site[a] = (int)v;
      }
    }
    // a submanifold output row is an input row: an offending one (not the first of its key) reads
    // nothing
    if (ok && subm) {
      const unsigned own = (((unsigned)b * g.in[0] + c[0]) * g.in[1] + c[1]) * g.in[2] + c[2];
      ok = sc_find(n, sorted_keys, sorted_rows, (int)own) == (int)o;
    }
    int found = -1;
    if (ok) {
      const unsigned key =
          (((unsigned)b * g.in[0] + site[0]) * g.in[1] + site[1]) * g.in[2] + site[2];
      found = sc_find(n, sorted_keys, sorted_rows, (int)key);
    }
    nbr[e] = found;
    if (found >= 0) atomicAdd(&cnt[k], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < g.kvol; i += SC_BLOCK)
    if (cnt[i]) atomicAdd(&pair_num[i], cnt[i]);
}

// ---- gather-GEMM
constexpr int SG_TM = 128;          // output rows per workgroup: 4 waves x 32
constexpr int SG_KC = 32;           // source channels per staging step
constexpr int SG_PA = SG_KC + 4;    // A tile pitch (16-byte stores)
constexpr int SG_PT = SG_KC + 1;    // transposed weight tile pitch

template <int NB, bool TRANS, bool VEC>
__global__ __launch_bounds__(SC_BLOCK) void sc_gather_gemm_kernel(
    long long rows, long long src_rows, int kvol, int c_src, int c_dst,
    const float *__restrict__ src, const float *__restrict__ weight,
    const int *__restrict__ table, float *__restrict__ dst) {
  constexpr int TN = 32 * NB;
  constexpr int PB = TN % 64 == 0 ? TN + 32 : TN;
  constexpr int WS = TRANS ? TN * SG_PT : SG_KC * PB;
  __shared__ __attribute__((aligned(16))) float As[SG_TM * SG_PA];
  __shared__ float Ws[WS];
  __shared__ int srow[SG_TM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const long long row0 = (long long)blockIdx.x * SG_TM;
  const int n0 = blockIdx.y * TN;
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

  for (int k = 0; k < kvol; ++k) {
    int mine = -1;
    if (tid < SG_TM) {
      const long long r = row0 + tid;
      if (r < rows) {
        const int e = table[r * kvol + k];
        mine = (e >= 0 && e < src_rows) ? e : -1;
      }
      srow[tid] = mine;
    }
    if (!__syncthreads_or(mine >= 0)) continue;  // nobody in the tile uses this tap
    const bool wave_any = __ballot(srow[w * 32 + l31] >= 0) != 0ull;
    const float *wk = weight + (long long)k * c_src * c_dst;
    for (int k0 = 0; k0 < c_src; k0 += SG_KC) {
      if (VEC) {
#pragma unroll
        for (int p = 0; p < SG_TM / 32; ++p) {
          const int r = p * 32 + (tid >> 3), q = tid & 7, c = k0 + 4 * q;
          const int sr = srow[r];
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (sr >= 0 && c < c_src) v = *(const float4 *)(src + (long long)sr * c_src + c);
          *(float4 *)&As[r * SG_PA + 4 * q] = v;
        }
      } else {
#pragma unroll
        for (int p = 0; p < SG_TM / 8; ++p) {
          const int r = p * 8 + (tid >> 5), c = k0 + (tid & 31);
          const int sr = srow[r];
          As[r * SG_PA + (tid & 31)] = (sr >= 0 && c < c_src) ? src[(long long)sr * c_src + c] : 0.f;
        }
      }
      if (!TRANS) {
        for (int idx = tid; idx < SG_KC * TN; idx += SC_BLOCK) {
          const int kk = idx / TN, n = idx % TN, c = k0 + kk, ch = n0 + n;
          Ws[kk * PB + n] = (c < c_src && ch < c_dst) ? wk[(long long)c * c_dst + ch] : 0.f;
        }
      } else {
        for (int idx = tid; idx < SG_KC * TN; idx += SC_BLOCK) {
          const int n = idx / SG_KC, kk = idx % SG_KC, c = k0 + kk, ch = n0 + n;
          Ws[n * SG_PT + kk] = (c < c_src && ch < c_dst) ? wk[(long long)ch * c_src + c] : 0.f;
        }
      }
      __syncthreads();
      if (wave_any) {
        const int left = c_src - k0;
        const int steps = ((left < SG_KC ? left : SG_KC) + 1) >> 1;
        const float *ap = As + (w * 32 + l31) * SG_PA + h;
        for (int s = 0; s < steps; ++s) {
          const float a = ap[2 * s];
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const float b = TRANS ? Ws[(nb * 32 + l31) * SG_PT + 2 * s + h]
                                  : Ws[(2 * s + h) * PB + nb * 32 + l31];
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[nb], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int ch = n0 + nb * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = row0 + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row < rows && ch < c_dst) dst[row * c_dst + ch] = acc[nb][r];
    }
  }
}

// ---- weight gradient
constexpr int SW_RB = 32;   // rows per step (the MFMA's K dimension, 16 steps of 2)
constexpr int SW_T = 64;    // tile of dW[k]: 64 x 64, a wave per 32 x 32
constexpr int SW_P = 96;    // pitch = 32 mod 64: the half-waves of an operand read hit disjoint banks
constexpr int SW_MAX_CHUNKS = 16;
constexpr int SW_CHUNK_ROWS = 512;

static int sw_chunks(long long rows) {
  const long long c = (rows + SW_CHUNK_ROWS - 1) / SW_CHUNK_ROWS;
  return (int)(c < 1 ? 1 : (c > SW_MAX_CHUNKS ? SW_MAX_CHUNKS : c));
}

template <bool VEC>
__device__ __forceinline__ void sw_stage(float *tile, const float *__restrict__ base, int c,
                                         int c0, const int *srow, long long row_base,
                                         const int *use, int tid) {
  // tile[r][0 .. 63] = base[row(r)][c0 .. c0 + 63], zero outside; row(r) = use ? use[r] : row_base + r
  if (VEC) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int r = p * 16 + (tid >> 4), q = tid & 15, ch = c0 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (srow[r] >= 0 && ch < c) {
        const long long row = use ? (long long)use[r] : row_base + r;
        v = *(const float4 *)(base + row * c + ch);
      }
      *(float4 *)&tile[r * SW_P + 4 * q] = v;
    }
  } else {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int r = p * 4 + (tid >> 6), q = tid & 63, ch = c0 + q;
      float v = 0.f;
      if (srow[r] >= 0 && ch < c) {
        const long long row = use ? (long long)use[r] : row_base + r;
        v = base[row * c + ch];
      }
      tile[r * SW_P + q] = v;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(SC_BLOCK) void sc_wgrad_kernel(
    long long rows, long long src_rows, int kvol, int c_in, int c_out, long long chunk_rows,
    int nchunks, const float *__restrict__ src, const float *__restrict__ dout,
    const int *__restrict__ table, float *__restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float G[SW_RB * SW_P];
  __shared__ __attribute__((aligned(16))) float D[SW_RB * SW_P];
  __shared__ int srow[SW_RB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int chunk = blockIdx.x, k = blockIdx.y;
  const int tiles_j = (c_out + SW_T - 1) / SW_T;
  const int i0 = (blockIdx.z / tiles_j) * SW_T, j0 = (blockIdx.z % tiles_j) * SW_T;
  const int ib = w & 1, jb = w >> 1;
  const bool wave_live = i0 + ib * 32 < c_in && j0 + jb * 32 < c_out;
  const long long r_begin = (long long)chunk * chunk_rows;
  const long long r_end = r_begin + chunk_rows < rows ? r_begin + chunk_rows : rows;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (long long rb = r_begin; rb < r_end; rb += SW_RB) {
    int mine = -1;
    if (tid < SW_RB) {
      const long long r = rb + tid;
      if (r < r_end) {
        const int e = table[r * kvol + k];
        mine = (e >= 0 && e < src_rows) ? e : -1;
      }
      srow[tid] = mine;
    }
    if (!__syncthreads_or(mine >= 0)) continue;
    sw_stage<VEC>(G, src, c_in, i0, srow, 0, srow, tid);
    sw_stage<VEC>(D, dout, c_out, j0, srow, rb, nullptr, tid);
    __syncthreads();
    if (wave_live) {
      const float *gp = G + h * SW_P + ib * 32 + l31, *dp = D + h * SW_P + jb * 32 + l31;
#pragma unroll
      for (int s = 0; s < SW_RB / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gp[2 * s * SW_P], dp[2 * s * SW_P], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  float *out = partial + ((long long)k * nchunks + chunk) * c_in * c_out;
  const int j = j0 + jb * 32 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (i < c_in && j < c_out) out[(long long)i * c_out + j] = acc[r];
  }
}

__global__ __launch_bounds__(SC_BLOCK) void sc_wgrad_sum_kernel(long long total, long long cc,
                                                                int nchunks,
                                                                const float *__restrict__ partial,
                                                                float *__restrict__ dw) {
  const long long e = (long long)blockIdx.x * SC_BLOCK + threadIdx.x;
  if (e >= total) return;
  const long long k = e / cc, r = e - k * cc;
  const float *p = partial + k * nchunks * cc + r;
  float s = p[0];
  for (int c = 1; c < nchunks; ++c) s = __fadd_rn(s, p[c * cc]);
  dw[e] = s;
}

// ---- host side

static int sc_geom(const char *W, int batch, const int *shape, const int *ksize, const int *stride,
                   const int *padding, int subm, ScGeom &g) {
  NESIE_REQUIRE(shape && ksize && stride && padding, W);
  NESIE_REQUIRE(batch >= 1, W);
  g.batch = batch;
  long long cells_in = batch, cells_out = batch, kvol = 1;
  for (int a = 0; a < 3; ++a) {
    NESIE_REQUIRE(shape[a] >= 1 && ksize[a] >= 1 && stride[a] >= 1 && padding[a] >= 0, W);
    g.in[a] = shape[a];
    g.k[a] = ksize[a];
    g.s[a] = subm ? 1 : stride[a];
    g.p[a] = subm ? ksize[a] / 2 : padding[a];
    const long long o =
        subm ? shape[a] : ((long long)shape[a] + 2LL * g.p[a] - ksize[a]) / g.s[a] + 1;
    if ((long long)shape[a] + 2LL * g.p[a] < ksize[a] || o < 1 || o >= 2147483648LL) {
      set_error("%s: axis %d: size %d, kernel %d, stride %d, padding %d leave no output", W, a,
                shape[a], ksize[a], g.s[a], g.p[a]);
      return NESIE_ERR_UNSUPPORTED;
    }
    g.out[a] = (int)o;
    cells_in *= shape[a];
    cells_out *= o;
    kvol *= ksize[a];
    if (cells_in >= 2147483648LL || cells_out >= 2147483648LL) {
      set_error("%s: batch_size * D * H * W must stay below 2^31 for the input and the output grid",
                W);
      return NESIE_ERR_UNSUPPORTED;
    }
    if (kvol > SC_MAX_KVOL) {
      set_error("%s: more than %d taps", W, SC_MAX_KVOL);
      return NESIE_ERR_UNSUPPORTED;
    }
  }
  g.kvol = (int)kvol;
  g.cells_in = (unsigned)cells_in;
  g.cells_out = (unsigned)cells_out;
  return NESIE_OK;
}

static int sc_check_nk(const char *W, long long n, long long kvol) {
  NESIE_REQUIRE(n >= 0, W);
  NESIE_REQUIRE(kvol >= 1, W);
  if (kvol > SC_MAX_KVOL || n > IX_MAX_N / kvol) {
    set_error("%s: %lld sites x %lld taps, at most %lld candidates and %d taps", W, n, kvol,
              IX_MAX_N, SC_MAX_KVOL);
    return NESIE_ERR_UNSUPPORTED;
  }
  return NESIE_OK;
}

// scratch: bad[n], then the sort's carve for max(n, n * K) elements (n for a submanifold conv)
static long long sc_rules_ints(long long n, long long kvol, int subm) {
  return n + ix_carve(nullptr, subm ? n : n * kvol).ints;
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_spconv_rules_workspace_bytes(long long n, int kvol, int subm, long long *out) {
  const char *W = "spconv_rules_workspace_bytes";
  const int st = sc_check_nk(W, n, kvol);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(out, W);
  *out = sc_rules_ints(n, kvol, subm) * (long long)sizeof(int);
  return NESIE_OK;
}

extern "C" int nesie_spconv_out_shape(const int *spatial_shape, const int *ksize, const int *stride,
                                      const int *padding, int subm, int batch_size, int *out_shape,
                                      long long *out_cells) {
  const char *W = "spconv_out_shape";
  ScGeom g;
  const int st = sc_geom(W, batch_size, spatial_shape, ksize, stride, padding, subm, g);
  if (st != NESIE_OK) return st;
  NESIE_REQUIRE(out_shape && out_cells, W);
  for (int a = 0; a < 3; ++a) out_shape[a] = g.out[a];
  *out_cells = g.cells_out;
  return NESIE_OK;
}

extern "C" int nesie_spconv_out_sites(long long n, const int *indices, int batch_size,
                                      const int *spatial_shape, const int *ksize,
                                      const int *stride, const int *padding, int subm,
                                      int *sorted_keys, int *sorted_rows, int *nbr_t,
                                      int *out_indices, int *counts, void *workspace,
                                      void *stream) {
  const char *W = "spconv_out_sites";
  NESIE_REQUIRE(n >= 0, W);
  ScGeom g;
  int st = sc_geom(W, batch_size, spatial_shape, ksize, stride, padding, subm, g);
  if (st == NESIE_OK) st = sc_check_nk(W, n, g.kvol);
  if (st != NESIE_OK) return st;
  if (n == 0) return NESIE_OK;
  NESIE_REQUIRE(indices && sorted_keys && sorted_rows && nbr_t && counts && workspace, W);
  NESIE_REQUIRE(subm || out_indices, W);
  hipStream_t s = (hipStream_t)stream;
  int *bad = (int *)workspace;
  void *sort_ws = bad + n;
  const long long nk = n * g.kvol;
  const unsigned n_grid = (unsigned)cdiv_ll(n, SC_BLOCK), nk_grid = (unsigned)cdiv_ll(nk, SC_BLOCK);
  zero_i32(counts, 2, s);   // (sc_mark_kernel adds into it)
  NESIE_LAUNCHED(W);

  const IxWorkspace w = ix_carve(sort_ws, n);
  hipLaunchKernelGGL(sc_in_keys_kernel, dim3(n_grid), dim3(SC_BLOCK), 0, s, n, g, indices, w.ka,
                     w.ia);
  NESIE_LAUNCHED(W);
  const unsigned *keys;
  const int *idx;
  st = ix_sort(W, n, g.cells_in, w, sorted_rows, &keys, &idx, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(sc_mark_kernel, dim3(n_grid), dim3(SC_BLOCK), 0, s, n, g.cells_in, keys, idx,
                     sorted_keys, bad, counts, subm ? (int)n : -1);
  NESIE_LAUNCHED(W);
  if (subm) {
    hipLaunchKernelGGL(sc_subm_nbrt_kernel, dim3(nk_grid), dim3(SC_BLOCK), 0, s, nk, n, g, indices,
                       bad, sorted_keys, sorted_rows, nbr_t);
    return check_launch(W);
  }
  // the first sort's scratch is dead: its results sit in sorted_keys, sorted_rows and bad
  const IxWorkspace w2 = ix_carve(sort_ws, nk);
  hipLaunchKernelGGL(sc_cand_kernel, dim3(nk_grid), dim3(SC_BLOCK), 0, s, nk, g, indices, bad,
                     w2.ka, w2.ia);
  NESIE_LAUNCHED(W);
  st = ix_sort(W, nk, g.cells_out, w2, nullptr, &keys, &idx, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(sc_head_kernel, dim3(nk_grid), dim3(SC_BLOCK), 0, s, nk, g.cells_out, keys,
                     w2.flag);
  NESIE_LAUNCHED(W);
  st = ix_scan(W, nk, w2.flag, w2.flag, w2.sums, counts, nullptr, 0, s);
  if (st != NESIE_OK) return st;
  hipLaunchKernelGGL(sc_fill_kernel, dim3(nk_grid), dim3(SC_BLOCK), 0, s, nk, g, keys, idx,
                     w2.flag, nbr_t, out_indices);
  return check_launch(W);
}

extern "C" int nesie_spconv_gather_table(long long m, const int *out_indices, long long n,
                                         const int *sorted_keys, const int *sorted_rows,
                                         int batch_size, const int *spatial_shape,
                                         const int *ksize, const int *stride, const int *padding,
                                         int subm, int *nbr, int *pair_num, void *stream) {
  const char *W = "spconv_gather_table";
  NESIE_REQUIRE(m >= 0 && n >= 0, W);
  ScGeom g;
  int st = sc_geom(W, batch_size, spatial_shape, ksize, stride, padding, subm, g);
  if (st == NESIE_OK) st = sc_check_nk(W, m, g.kvol);
  if (st != NESIE_OK) return st;
  if (m == 0) return NESIE_OK;
  NESIE_REQUIRE(out_indices && nbr && pair_num, W);
  NESIE_REQUIRE(n == 0 || (sorted_keys && sorted_rows), W);
  hipStream_t s = (hipStream_t)stream;
  zero_i32(pair_num, g.kvol, s);   // (sc_table_kernel adds into it)
  const long long total = m * g.kvol;
  hipLaunchKernelGGL(sc_table_kernel, dim3((unsigned)cdiv_ll(total, SC_BLOCK)), dim3(SC_BLOCK), 0,
                     s, total, n, g, subm, out_indices, sorted_keys, sorted_rows, nbr, pair_num);
  return check_launch(W);
}

namespace {
template <int NB>
void sg_launch(bool trans, bool vec, dim3 grid, hipStream_t s, long long rows, long long src_rows,
               int kvol, int c_src, int c_dst, const float *src, const float *weight,
               const int *table, float *dst) {
  const dim3 block(SC_BLOCK);
  if (trans && vec)
    hipLaunchKernelGGL((sc_gather_gemm_kernel<NB, true, true>), grid, block, 0, s, rows, src_rows,
                       kvol, c_src, c_dst, src, weight, table, dst);
  else if (trans)
    hipLaunchKernelGGL((sc_gather_gemm_kernel<NB, true, false>), grid, block, 0, s, rows, src_rows,
                       kvol, c_src, c_dst, src, weight, table, dst);
  else if (vec)
    hipLaunchKernelGGL((sc_gather_gemm_kernel<NB, false, true>), grid, block, 0, s, rows, src_rows,
                       kvol, c_src, c_dst, src, weight, table, dst);
  else
    hipLaunchKernelGGL((sc_gather_gemm_kernel<NB, false, false>), grid, block, 0, s, rows,
                       src_rows, kvol, c_src, c_dst, src, weight, table, dst);
}
}  // namespace

extern "C" int nesie_spconv_gather_gemm(long long rows, long long src_rows, int kvol, int c_src,
                                        int c_dst, const float *src, const float *weight,
                                        int weight_transposed, const int *table, float *dst,
                                        void *stream) {
  const char *W = "spconv_gather_gemm";
  NESIE_REQUIRE(rows >= 0 && src_rows >= 0 && kvol >= 1 && c_src >= 1 && c_dst >= 1, W);
  if (rows == 0) return NESIE_OK;
  NESIE_REQUIRE(weight && table && dst, W);
  NESIE_REQUIRE(src_rows == 0 || src, W);
  const long long row_tiles = cdiv_ll(rows, SG_TM);
  if (row_tiles > 2147483647LL || src_rows > 2147483647LL) {
    set_error("%s: %lld rows from %lld are more than one launch covers", W, rows, src_rows);
    return NESIE_ERR_UNSUPPORTED;
  }
  const int nb = c_dst <= 32 ? 1 : (c_dst <= 64 ? 2 : 4);
  const long long col_tiles = cdiv_ll(c_dst, 32 * nb);
  if (col_tiles > 65535) {
    set_error("%s: %d destination channels are more than one launch covers", W, c_dst);
    return NESIE_ERR_UNSUPPORTED;
  }
  const bool vec = c_src % 4 == 0 && ((uintptr_t)src & 15) == 0;
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles);
  hipStream_t s = (hipStream_t)stream;
  const bool trans = weight_transposed != 0;
  if (nb == 1)
    sg_launch<1>(trans, vec, grid, s, rows, src_rows, kvol, c_src, c_dst, src, weight, table, dst);
  else if (nb == 2)
    sg_launch<2>(trans, vec, grid, s, rows, src_rows, kvol, c_src, c_dst, src, weight, table, dst);
  else
    sg_launch<4>(trans, vec, grid, s, rows, src_rows, kvol, c_src, c_dst, src, weight, table, dst);
  return check_launch(W);
}

extern "C" int nesie_spconv_wgrad_workspace_bytes(long long rows, int kvol, int c_in, int c_out,
                                                  long long *out) {
  const char *W = "spconv_wgrad_workspace_bytes";
  NESIE_REQUIRE(rows >= 0 && kvol >= 1 && c_in >= 1 && c_out >= 1, W);
  NESIE_REQUIRE(out, W);
  *out = (long long)kvol * sw_chunks(rows) * c_in * c_out * (long long)sizeof(float);
  return NESIE_OK;
}

extern "C" int nesie_spconv_wgrad(long long rows, long long src_rows, int kvol, int c_in, int c_out,
                                  const float *src, const float *dout, const int *table, float *dw,
                                  void *workspace, void *stream) {
  const char *W = "spconv_wgrad";
  NESIE_REQUIRE(rows >= 0 && src_rows >= 0 && kvol >= 1 && c_in >= 1 && c_out >= 1, W);
  if (rows == 0 || src_rows == 0) return NESIE_OK;
  NESIE_REQUIRE(src && dout && table && dw && workspace, W);
  const long long tiles = cdiv_ll(c_in, SW_T) * cdiv_ll(c_out, SW_T);
  if (kvol > 65535 || tiles > 65535 || src_rows > 2147483647LL) {
    set_error("%s: %d taps x %lld tiles are more than one launch covers", W, kvol, tiles);
    return NESIE_ERR_UNSUPPORTED;
  }
  const int nchunks = sw_chunks(rows);
  const long long chunk_rows = cdiv_ll(cdiv_ll(rows, nchunks), SW_RB) * SW_RB;
  const bool vec = c_in % 4 == 0 && c_out % 4 == 0 && ((uintptr_t)src & 15) == 0 &&
                   ((uintptr_t)dout & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nchunks, (unsigned)kvol, (unsigned)tiles), block(SC_BLOCK);
  float *partial = (float *)workspace;
  if (vec)
    hipLaunchKernelGGL(sc_wgrad_kernel<true>, grid, block, 0, s, rows, src_rows, kvol, c_in, c_out,
                       chunk_rows, nchunks, src, dout, table, partial);
  else
    hipLaunchKernelGGL(sc_wgrad_kernel<false>, grid, block, 0, s, rows, src_rows, kvol, c_in,
                       c_out, chunk_rows, nchunks, src, dout, table, partial);
  NESIE_LAUNCHED(W);
  const long long cc = (long long)c_in * c_out, total = cc * kvol;
  hipLaunchKernelGGL(sc_wgrad_sum_kernel, dim3((unsigned)cdiv_ll(total, SC_BLOCK)), block, 0, s,
                     total, cc, nchunks, partial, dw);
  return check_launch(W);
}
