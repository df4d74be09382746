// The blend backward for ANY shape, without float atomics (nesie_blend_conv_backward_any): what the
// 64 x 64-tile kernels of interpolate.hip refuse -- channel counts that are no whole 64-block or
// exceed 256, faces that are no whole 64-query tiles, 2048 seeds and more, free pitch -- and the
// same function for the shapes they serve.  Three steps, every one with a fixed order:
//   blend_any_rows_kernel    dy (B, segs, c, per_seg) -> dZ^T (B, segs, per_seg, c) query-major rows
//                            through a 64 x 64 LDS tile (tails masked, the norm backward on the
//                            load), and the partial sums of dy x rel per (scene, run, face);
//   launch_inverted_index    the 3n taps of a scene sorted by seed, ascending tap position 3p + t
//                            inside a seed's run; blend_any_offs_kernel lists the m + 1 run starts;
//   blend_any_gather_kernel  one wave per (scene, face, seed, block of 256 channels) walks the
//                            seed's run in that order, skips the other faces' taps, adds
//                            weight * row and WRITES the d_table row (zeros for an empty run).
#include "common.h"
#include "index_sort.h"

namespace nesie {

constexpr int BA_Q = 64;            // queries per tile
constexpr int BA_C = 64;            // channels per tile
constexpr int BA_RUN = 1024;        // queries per workgroup of the rows kernel (16 tiles)
constexpr int BA_CB = 256;          // channels per gather wave (4 per lane, lane + 64 e)

// grid: scene fastest, then run, channel block, face.  256 threads; load phase lane = query
// (coalesced along per_seg), store phase lane = channel (coalesced along c).
template <bool BNB>
__global__ __launch_bounds__(256) void blend_any_rows_kernel(
    int c, int n, int segs, int seg_len, const float *__restrict__ dy,
    const float *__restrict__ rel, const float *__restrict__ bnz, const float *__restrict__ bnb,
    float *__restrict__ dzt, float *__restrict__ wx_part, int nb, int nruns, int ncblk) {
  __shared__ float tile[BA_C * (BA_Q + 1)];
  __shared__ float sr[BA_Q][3];
  const int bi = blockIdx.x % nb, run_i = (blockIdx.x / nb) % nruns;
  const int cb = (blockIdx.x / (nb * nruns)) % ncblk, sg = blockIdx.x / (nb * nruns * ncblk);
  const int per_seg = n / segs;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c0 = cb * BA_C;
  const size_t face = (size_t)bi * segs + sg;
  const float *src = dy + face * c * per_seg;
  const float *zsrc = BNB ? bnz + face * c * per_seg : nullptr;
  float *dst = dzt + face * per_seg * c;
  const int run0 = run_i * BA_RUN;
  const int run_end = run0 + BA_RUN < per_seg ? run0 + BA_RUN : per_seg;
  float dx0 = 0.f, dx1 = 0.f, dx2 = 0.f;
  for (int r0 = run0; r0 < run_end; r0 += BA_Q) {
    const int q = r0 + lane;
    if (threadIdx.x < BA_Q) {
      float a = 0.f, b_ = 0.f, d = 0.f;
      if (rel && q < per_seg) {
        const int k = q / seg_len, g = q - k * seg_len;
        const size_t p = (size_t)bi * n + (size_t)(k * segs + sg) * seg_len + g;
        a = rel[p * 3]; b_ = rel[p * 3 + 1]; d = rel[p * 3 + 2];
      }
      sr[threadIdx.x][0] = a; sr[threadIdx.x][1] = b_; sr[threadIdx.x][2] = d;
    }
#pragma unroll 4
    for (int i = 0; i < BA_C / 4; ++i) {
      const int ch = c0 + i * 4 + wv;
      float v = 0.f;
      if (ch < c && q < per_seg) {
        v = src[(size_t)ch * per_seg + q];
        if (BNB) {
          const float *cf = bnb + ((size_t)sg * c + ch) * 8;
          const float zz = zsrc[(size_t)ch * per_seg + q];
          const float gg = __builtin_fmaf(zz, cf[0], cf[1]) > 0.f ? v : 0.f;
          v = __builtin_fmaf(cf[2], gg, __builtin_fmaf(cf[3] - zz, cf[4], cf[5]));
        }
      }
      tile[(i * 4 + wv) * (BA_Q + 1) + lane] = v;
    }
    __syncthreads();
    const int ch = c0 + lane;
#pragma unroll 4
    for (int u = 0; u < 16; ++u) {
      const int ql = wv * 16 + u;
      const float v = tile[lane * (BA_Q + 1) + ql];       // (0 outside the shape)
      if (ch < c && r0 + ql < per_seg) dst[(size_t)(r0 + ql) * c + ch] = v;
      dx0 += v * sr[ql][0]; dx1 += v * sr[ql][1]; dx2 += v * sr[ql][2];
    }
    __syncthreads();
  }
  if (wx_part) {
    float *red = tile;   // [4][64][3]: the four waves hold different queries of the same channels
    red[(wv * 64 + lane) * 3 + 0] = dx0;
    red[(wv * 64 + lane) * 3 + 1] = dx1;
    red[(wv * 64 + lane) * 3 + 2] = dx2;
    __syncthreads();
    float *out = wx_part + ((((size_t)bi * nruns + run_i) * segs + sg) * c + c0) * 3;
    const int live = (c - c0 < BA_C ? c - c0 : BA_C) * 3;
    for (int i = threadIdx.x; i < live; i += 256)
      out[i] = (red[i] + red[192 + i]) + (red[384 + i] + red[576 + i]);
  }
}

// d_wx[s][ch][d] = the partials of one (face, channel, d) added in ascending (scene, run) order
__global__ __launch_bounds__(256) void blend_any_wx_kernel(int nparts, int per_part,
                                                           const float *__restrict__ part,
                                                           float *__restrict__ d_wx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= per_part) return;
  float acc = 0.f;
  for (int p = 0; p < nparts; ++p) acc += part[(size_t)p * per_part + i];
  d_wx[i] = acc;
}

// run starts of the sorted taps: offs[b][s] = first sorted position whose seed is >= s, s = 0..m
__global__ __launch_bounds__(256) void blend_any_offs_kernel(int m, int e_total,
                                                             const int *__restrict__ sources,
                                                             int *__restrict__ offs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int bi = blockIdx.y;
  if (i > e_total) return;
  const int *sb = sources + (size_t)bi * e_total;
  int *of = offs + (size_t)bi * (m + 1);
  int prev = i > 0 ? sb[i - 1] : -1;
  int cur = i < e_total ? sb[i] : m;
  prev = prev < -1 ? -1 : (prev >= m ? m - 1 : prev);
  cur = cur < 0 ? 0 : (cur > m ? m : cur);
  for (int s = prev + 1; s <= cur; ++s) of[s] = i;       // (sorted: every s is written exactly once)
}

__global__ __launch_bounds__(256) void blend_any_gather_kernel(
    int c, int m, int n, int segs, int seg_len, int pitch, int seg_off,
    const float *__restrict__ dzt, const float *__restrict__ weight, const int *__restrict__ order,
    const int *__restrict__ offs, float *__restrict__ d_table, int nb, int ncb) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long long)nb * segs * ncb * m) return;
  // seed fastest: the four waves of a workgroup write neighbouring d_table rows
  const int seed = (int)(w % m);
  const int cb = (int)((w / m) % ncb), face = (int)(w / ((long long)m * ncb));   // face = bi * segs + sg
  const int bi = face / segs, sg = face % segs;
  const int per_seg = n / segs;
  const int e_total = n * 3;
  int lo = 0, hi = 0;
  if (n > 0) {
    lo = __builtin_amdgcn_readfirstlane(offs[(size_t)bi * (m + 1) + seed]);
    hi = __builtin_amdgcn_readfirstlane(offs[(size_t)bi * (m + 1) + seed + 1]);
  }
  const int *ob = order + (size_t)bi * e_total;
  const float *wb = weight + (size_t)bi * e_total;
  const float *base = dzt + (size_t)face * per_seg * c;
  const int ch0 = cb * BA_CB + lane;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = lo; j0 < hi; j0 += 64) {
    // 64 sorted taps of this seed: lanes pick out this face's and name their dZ^T rows
    bool mine = false;
    int row = 0;
    float tw = 0.f;
    if (j0 + lane < hi) {
      int e = ob[j0 + lane];
      e = e < 0 ? 0 : (e >= e_total ? e_total - 1 : e);
      const int p = e / 3;
      const int ks = p / seg_len, g = p - ks * seg_len;
      const int k = ks / segs;
      mine = ks - k * segs == sg;
      row = k * seg_len + g;
      tw = wb[e];
    }
    unsigned long long todo = __ballot(mine);
    while (todo) {                                       // four rows in flight, added in order
      int l[4];
      int cnt = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        l[u] = 0;
        if (todo) { l[u] = __builtin_ctzll(todo); todo &= todo - 1; ++cnt; }
      }
      float v[4][4], tws[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < cnt) {
          const int lu = __builtin_amdgcn_readfirstlane(l[u]);
          const int r = __builtin_amdgcn_readlane(row, lu);
          tws[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tw), lu));
          const float *rp = base + (size_t)r * c;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][e] = ch0 + e * 64 < c ? rp[ch0 + e * 64] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < cnt) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += __fmul_rn(v[u][e], tws[u]);
        }
      }
    }
  }
  float *out = d_table + ((size_t)bi * m + seed) * pitch + (size_t)sg * seg_off;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (ch0 + e * 64 < c) out[ch0 + e * 64] = acc[e];
}

// workspace: dZ^T [b * n * c] floats, d_wx partials [b * runs * segs * c * 3] floats, then order,
// sources, scratch [b * 3n] ints each and the run starts [b * (m + 1)] ints
struct BlendAnyLayout {
  size_t dzt, part, taps, offs;
  size_t bytes() const { return (dzt + part) * sizeof(float) + (3 * taps + offs) * sizeof(int); }
};
static BlendAnyLayout blend_any_layout(int b, int c, int m, int n, int segs) {
  BlendAnyLayout l;
  l.dzt = (size_t)b * n * c;
  l.part = (size_t)b * cdiv(n / segs, BA_RUN) * segs * c * 3;
  l.taps = (size_t)b * n * 3;
  l.offs = (size_t)b * ((size_t)m + 1);
  return l;
}

}  // namespace nesie

using namespace nesie;

extern "C" size_t nesie_blend_conv_backward_any_workspace_bytes(int b, int c, int m, int n, int segs) {
  if (b <= 0 || c <= 0 || m <= 0 || n <= 0 || segs <= 0) return 0;
  return blend_any_layout(b, c, m, n, segs).bytes();
}

extern "C" int nesie_blend_conv_backward_any(int b, int c, int m, int n, const float *dy,
                                             const float *z, const float *bnb, int pitch,
                                             int seg_off, const int *idx, const float *weight,
                                             const float *rel, float *d_table, float *d_wx, int segs,
                                             int seg_len, void *workspace, size_t workspace_bytes,
                                             void *stream) {
  const char *W = "blend_conv_backward_any";
  NESIE_REQUIRE(b >= 0 && c >= 0 && m >= 0 && n >= 0 && segs >= 1 && seg_len >= 1, W);
  NESIE_REQUIRE(n % (segs * seg_len) == 0 && seg_off >= 0, W);
  NESIE_REQUIRE(pitch >= (long long)(segs - 1) * seg_off + c, W);
  NESIE_REQUIRE((z == nullptr) == (bnb == nullptr), W);
  if (b == 0 || c == 0) return NESIE_OK;
  NESIE_REQUIRE(m >= 1 && d_table && ((d_wx == nullptr) || rel || n == 0), W);
  NESIE_REQUIRE((long long)n * 3 < (1ll << 31) && b <= 65535, W);
  hipStream_t s = (hipStream_t)stream;
  const int ncb = cdiv(c, BA_CB);
  const long long waves = (long long)b * segs * ncb * m;
  NESIE_REQUIRE(cdiv(waves, 4) < (1ll << 31), W);
  if (n == 0) {   // no taps: every row is an empty run
    hipLaunchKernelGGL(blend_any_gather_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, c, m,
                       0, segs, seg_len, pitch, seg_off, (const float *)nullptr,
                       (const float *)nullptr, (const int *)nullptr, (const int *)nullptr, d_table,
                       b, ncb);
    if (d_wx)
      hipLaunchKernelGGL(blend_any_wx_kernel, dim3((unsigned)cdiv((long long)segs * c * 3, 256)),
                         dim3(256), 0, s, 0, segs * c * 3, (const float *)nullptr, d_wx);
    return check_launch(W);
  }
  NESIE_REQUIRE(dy && idx && weight && workspace, W);
  NESIE_REQUIRE(((uintptr_t)workspace & 3) == 0, W);
  const BlendAnyLayout l = blend_any_layout(b, c, m, n, segs);
  NESIE_REQUIRE(workspace_bytes >= l.bytes(), W);
  float *dzt = (float *)workspace, *part = dzt + l.dzt;
  int *order = (int *)(part + l.part), *sources = order + l.taps, *scratch = sources + l.taps,
      *offs = scratch + l.taps;
  const int per_seg = n / segs;
  const int nruns = cdiv(per_seg, BA_RUN), ncblk = cdiv(c, BA_C);
  NESIE_REQUIRE((long long)nruns * b * segs * ncblk < (1ll << 31) && (long long)segs * c * 3 < (1ll << 31), W);
  const dim3 grid((unsigned)(nruns * b * segs * ncblk));
  with_bool(bnb != nullptr, [&](auto BNB) {
    hipLaunchKernelGGL(blend_any_rows_kernel<BNB()>, grid, dim3(256), 0, s, c, n, segs, seg_len, dy, rel, z, bnb,
                       dzt, d_wx ? part : (float *)nullptr, b, nruns, ncblk);
  });
  NESIE_LAUNCHED(W);
  if (d_wx)
    hipLaunchKernelGGL(blend_any_wx_kernel, dim3((unsigned)cdiv((long long)segs * c * 3, 256)),
                       dim3(256), 0, s, b * nruns, segs * c * 3, part, d_wx);
  const int st = launch_inverted_index(b, m, (long long)n * 3, idx, order, sources, scratch, s);
  if (st) return st;
  hipLaunchKernelGGL(blend_any_offs_kernel, dim3((unsigned)cdiv((long long)n * 3 + 1, 256), b),
                     dim3(256), 0, s, m, n * 3, sources, offs);
  hipLaunchKernelGGL(blend_any_gather_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, c, m,
                     n, segs, seg_len, pitch, seg_off, dzt, weight, order, offs, d_table, b, ncb);
  return check_launch(W);
}
