// Sorted-index primitives shared by the ops that sort, scan or invert an index (index_sort.hip
// holds the kernels and the host side): the device-wide stable radix sort of (key, index) pairs,
// the any-length exclusive scan of ints with the scratch layout of both, the inverted index, and
// the two workgroup-level pieces they and the staged blend backward are built from.
#pragma once
#include "common.h"

namespace nesie {

constexpr int IX_SORT_TILE = 1024;  // keys per sort workgroup: 4 waves x 4 rounds x 64 lanes
constexpr long long IX_MAX_N = 2147483647LL - IX_SORT_TILE;

struct IxWorkspace {
  unsigned *ka, *kb;
  int *ia, *ib, *flag, *hist, *sums, *meta;
  long long nb, ints;
};

// the layout of `ints` ints of scratch for n elements (ws may be null for the size query)
IxWorkspace ix_carve(void *ws, long long n);

// n >= 0 (else NESIE_ERR_INVALID_ARG), 1 <= cells < 2^31 and n <= IX_MAX_N (else NESIE_ERR_UNSUPPORTED)
int ix_check_n_cells(const char *W, long long n, long long cells);

// exclusive scan of n ints; out may alias in.  sums: scratch (IxWorkspace::sums).  *total_out =
// the grand total and *capped = min(total, cap), each when given; both on the device
int ix_scan(const char *W, long long n, const int *in, int *out, int *sums, int *total_out,
            int *capped, int cap, hipStream_t s);

// sorts (w.ka, w.ia) by key, keys in 0 .. cells, stable; the sorted keys end in *keys, the indices
// in *idx (`last_idx` when given receives the indices of the last pass directly)
int ix_sort(const char *W, long long n, long long cells, const IxWorkspace &w, int *last_idx,
            const unsigned **keys, const int **idx, hipStream_t s);

// nesie_inverted_index (include/nesie_ops.h) for callers inside the library.  An entry outside
// [0, n) is clamped to the nearest point (0 or n - 1) in both kernels: it sorts, and appears in
// `sources`, as that point.  e_total = 0 is a no-op: nothing is launched or written.
int launch_inverted_index(int b, int n, long long e_total, const int *idx, int *order, int *sources,
                          int *scratch, hipStream_t s);

// exclusive prefix of t over the workgroup's BLOCK threads; total in every thread.  lds: BLOCK / 64
// ints, free again on return.
template <int BLOCK>
__device__ __forceinline__ int block_excl(int t, int *lds, int &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int wbase = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < BLOCK / 64; ++k) {
    const int s = lds[k];
    if (k < w) wbase += s;
    total += s;
  }
  __syncthreads();
  return wbase + inc - t;
}

// The middle of a stable counting sort by a workgroup of BLOCK threads whose wave w has counted
// its own contiguous share of the entries into the LDS row cnt[w * bins + s] (the caller's barrier
// stands between the counting and this call): totals per bin -> exclusive scan over the bins ->
// cnt[w * bins + s] becomes the position of wave w's first entry of bin s, bin-major and
// wave-minor, so placing every wave's entries in their order gives the stable order.  run_starts,
// when given, receives the bins + 1 run starts (global memory).  lds: BLOCK / 64 ints.  Ends with
// a barrier: the positions are ready for every wave.
template <int BLOCK>
__device__ __forceinline__ void counting_sort_starts(int *cnt, int bins, int *lds,
                                                     int *__restrict__ run_starts) {
  constexpr int WAVES = BLOCK / 64;
  const int tid = threadIdx.x;
  const int bper = (bins + BLOCK - 1) / BLOCK;       // bins per thread (contiguous)
  const int b0 = tid * bper, b1 = b0 + bper < bins ? b0 + bper : bins;
  int sum = 0;
  for (int sbin = b0; sbin < b1; ++sbin)
    for (int w = 0; w < WAVES; ++w) sum += cnt[w * bins + sbin];
  int total;
  int run = block_excl<BLOCK>(sum, lds, total);      // first position of this thread's first bin
  for (int sbin = b0; sbin < b1; ++sbin) {
    if (run_starts) run_starts[sbin] = run;
    for (int w = 0; w < WAVES; ++w) {
      const int c = cnt[w * bins + sbin];
      cnt[w * bins + sbin] = run;
      run += c;
    }
  }
  if (run_starts && tid == 0) run_starts[bins] = total;
  __syncthreads();
}

}  // namespace nesie
