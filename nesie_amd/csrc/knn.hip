// k nearest neighbours for gfx950.
//
// Replaces knn_kernel (reference mmdet3d/ops/knn/src/knn_cuda.cu:58-94), which gives every centre
// one thread with a private 100-entry binary heap: scratch memory and divergent sifting on this
// chip.  Here a WAVE owns one centre and keeps its best list SORTED ACROSS LANES as 64-bit keys
//     key = (bits(d2) << 32) | point index
// (d2 >= +0, so unsigned key order = ascending (distance, index), ties included): one key per lane
// for nsample <= 64, two per lane up to 128, as separate instantiations.  The scene streams through
// LDS in tiles shared by the workgroup's four waves; a wave evaluates 64 points per step, compares
// them against its current k-th key and, as ball_query_indexed_kernel does for its hits, parks
// the few that beat it in a per-wave pending buffer; only a full buffer (64 keys) is sorted by a
// bitonic network in registers and merged into the list.  The k-th key only ever falls, so a key
// admitted against a stale threshold is merely dropped by the merge: the result is exactly the
// nsample smallest keys in ascending order.
//
// The pending buffer is private to one wave and needs no barrier: wave_pend_push (wave_sort.h) says why.
#include <string.h>

#include "common.h"
#include "wave_sort.h"

namespace nesie {

constexpr int KNN_WAVES = 4;
constexpr int KNN_TILE = 1024;   // points per LDS tile: 12 KiB, read with stride 3 (conflict-free)
constexpr int KNN_MAX = 128;     // two keys per lane
constexpr unsigned long long KNN_EMPTY = ~0ull;   // larger than every key of a point

typedef unsigned long long knn_key;

template <int FORM, bool WIDE>
__global__ __launch_bounds__(KNN_WAVES * 64) void knn_kernel(
    int b, int n, int m, int nsample, const float *__restrict__ xyz,
    const float *__restrict__ new_xyz, int *__restrict__ idx, float *__restrict__ dist2) {
  __shared__ float tile[KNN_TILE * 3];
  __shared__ knn_key pend_all[KNN_WAVES][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int scene = blockIdx.x % b;  // one scene's workgroups on one XCD's L2 when b | 8
  const int c = (blockIdx.x / b) * KNN_WAVES + wave;
  const bool live = c < m;  // wave-uniform; a wave without a centre still loads tiles and meets the barriers
  volatile knn_key *pend = pend_all[wave];
  xyz += (size_t)scene * n * 3;
  const float *ctr = new_xyz + ((size_t)scene * m + (live ? c : m - 1)) * 3;
  const float cx = ctr[0], cy = ctr[1], cz = ctr[2];

  knn_key lo = KNN_EMPTY, hi = KNN_EMPTY;  // lane i: i-th (lo) and (64+i)-th (hi, WIDE) smallest key so far
  knn_key kth = KNN_EMPTY;                 // the nsample-th smallest key at the last merge
  int npend = 0;

  auto merge = [&](knn_key v) {
    v = wave_sort64(v, lane);
    if (WIDE) {
      wave_merge64<true>(lo, v, lane);
      wave_merge64<false>(hi, v, lane);
      kth = __shfl(hi, nsample - 65, 64);
    } else {
      wave_merge64<false>(lo, v, lane);
      kth = __shfl(lo, nsample - 1, 64);
    }
  };

  for (int base = 0; base < n; base += KNN_TILE) {
    const int cnt = n - base < KNN_TILE ? n - base : KNN_TILE;
    __syncthreads();  // every wave is done with the previous tile
    for (int i = threadIdx.x; i < cnt * 3; i += KNN_WAVES * 64) tile[i] = xyz[(size_t)base * 3 + i];
    __syncthreads();
    if (!live) continue;
    for (int s = 0; s < cnt; s += 64) {
      const int p = s + lane;  // < KNN_TILE; past cnt the tile holds stale values that are not used
      const float d2 = sqdist_form<FORM>(cx - tile[p * 3 + 0], cy - tile[p * 3 + 1], cz - tile[p * 3 + 2]);
      const knn_key key = p < cnt ? ((knn_key)__float_as_uint(d2) << 32) | (unsigned)(base + p) : KNN_EMPTY;
      wave_pend_push(pend, npend, lane, key < kth, key, merge);
    }
  }
  if (!live) return;
  wave_pend_flush(pend, npend, lane, KNN_EMPTY, merge);

  // a slot no point reached (n < nsample) keeps the state the reference's heap starts from
  // (knn_cuda.cu:74-77): index 0, distance 1e10
  const size_t row = ((size_t)scene * m + c) * nsample;
  if (lane < nsample) {
    idx[row + lane] = lo == KNN_EMPTY ? 0 : (int)(unsigned)lo;
    dist2[row + lane] = lo == KNN_EMPTY ? 1e10f : __uint_as_float((unsigned)(lo >> 32));
  }
  if (WIDE && 64 + lane < nsample) {
    idx[row + 64 + lane] = hi == KNN_EMPTY ? 0 : (int)(unsigned)hi;
    dist2[row + 64 + lane] = hi == KNN_EMPTY ? 1e10f : __uint_as_float((unsigned)(hi >> 32));
  }
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_knn_wrapper(int b, int n, int m, int nsample, const float *xyz,
                                 const float *new_xyz, int *idx, float *dist2, void *stream) {
  const char *W = "knn_wrapper";
  NESIE_REQUIRE(b >= 0 && n >= 0 && m >= 0 && nsample > 0, W);
  if (nsample > KNN_MAX) {
    set_error("%s: nsample %d is more than the %d the sorted list holds", W, nsample, KNN_MAX);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (b == 0 || m == 0) return NESIE_OK;
  NESIE_REQUIRE(idx && dist2, W);
  if (n == 0) {  // nothing to scan: every slot is padding
    const size_t slots = (size_t)b * m * nsample;
    const float pad = 1e10f;
    int pad_bits;
    memcpy(&pad_bits, &pad, sizeof pad_bits);
    hipError_t e = hipMemsetAsync(idx, 0, slots * sizeof(int), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)dist2, pad_bits, slots, (hipStream_t)stream);
    if (e != hipSuccess) {
      set_error("%s: %s", W, hipGetErrorString(e));
      return NESIE_ERR_LAUNCH;
    }
    return NESIE_OK;
  }
  NESIE_REQUIRE(xyz && new_xyz, W);
  NESIE_REQUIRE((long long)n * 3 < (1ll << 31), W);
  const long long groups = cdiv(m, KNN_WAVES);
  NESIE_REQUIRE(groups * b < (1ll << 31), W);
  const dim3 grid((unsigned)(groups * b)), block(KNN_WAVES * 64);
  with_distance_form([&](auto form) {
    constexpr int FORM = decltype(form)::value;
    if (nsample <= 64)
      hipLaunchKernelGGL((knn_kernel<FORM, false>), grid, block, 0, (hipStream_t)stream, b, n, m, nsample,
                         xyz, new_xyz, idx, dist2);
    else
      hipLaunchKernelGGL((knn_kernel<FORM, true>), grid, block, 0, (hipStream_t)stream, b, n, m, nsample,
                         xyz, new_xyz, idx, dist2);
  });
  return check_launch(W);
}
