// The sorted voxel ops' host helpers that other translation units reuse (defined in voxel.hip,
// where their kernels live: no __global__ symbol is defined twice): the stable radix sort of
// (key, index) pairs, the any-length exclusive scan of ints, and the scratch layout of both.
#pragma once
#include "common.h"

namespace nesie {

constexpr int VX_SORT_TILE = 1024;  // keys per sort workgroup: 4 waves x 4 rounds x 64 lanes
constexpr long long VX_MAX_N = 2147483647LL - VX_SORT_TILE;

struct VxWorkspace {
  unsigned *ka, *kb;
  int *ia, *ib, *flag, *hist, *sums, *meta;
  long long nb, ints;
};

// the layout of `ints` ints of scratch for n elements (ws may be null for the size query)
VxWorkspace vx_carve(void *ws, long long n);

// n >= 0 (else NESIE_ERR_INVALID_ARG), 1 <= cells < 2^31 and n <= VX_MAX_N (else NESIE_ERR_UNSUPPORTED)
int vx_check_n_cells(const char *W, long long n, long long cells);

// exclusive scan of n ints; out may alias in.  sums: scratch (VxWorkspace::sums).  *total_out =
// the grand total and *capped = min(total, cap), each when given; both on the device
int vx_scan(const char *W, long long n, const int *in, int *out, int *sums, int *total_out,
            int *capped, int cap, hipStream_t s);

// sorts (w.ka, w.ia) by key, keys in 0 .. cells, stable; the sorted keys end in *keys, the indices
// in *idx (`last_idx` when given receives the indices of the last pass directly)
int vx_sort(const char *W, long long n, long long cells, const VxWorkspace &w, int *last_idx,
            const unsigned **keys, const int **idx, hipStream_t s);

}  // namespace nesie
