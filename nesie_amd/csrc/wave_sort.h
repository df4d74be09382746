// Sorting inside one wavefront, shared by the neighbour searches (knn.hip, ball_query.hip) and the
// blend backward (interpolate.hip): a 64-lane bitonic sort and merge of one key per lane, the rank
// of a lane inside a ballot, and the wave-private pending list that feeds the merge.  K is the key
// type: unsigned, or unsigned long long for a (distance, index) pair.
#pragma once
#include "common.h"

namespace nesie {

// one key per lane, any order -> ascending over the lanes: the bitonic network
template <typename K>
__device__ __forceinline__ K wave_sort64(K v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      const K o = __shfl_xor(v, j, 64);
      const bool up = (lane & k) == 0;     // this block of k lanes sorts ascending
      const bool lower = (lane & j) == 0;  // this lane keeps the smaller of the pair
      v = (up == lower) ? (v < o ? v : o) : (v > o ? v : o);
    }
  }
  return v;
}

// a bitonic sequence over the lanes -> ascending
template <typename K>
__device__ __forceinline__ K wave_bitonic_finish(K v, int lane) {
#pragma unroll
  for (int j = 32; j >= 1; j >>= 1) {
    const K o = __shfl_xor(v, j, 64);
    v = ((lane & j) == 0) ? (v < o ? v : o) : (v > o ? v : o);
  }
  return v;
}

// best, add: ascending over the lanes; best <- the 64 smallest of the 128, ascending; with HIGH,
// add <- the 64 largest, ascending
template <bool HIGH, typename K>
__device__ __forceinline__ void wave_merge64(K &best, K &add, int lane) {
  const K rev = __shfl(add, 63 - lane, 64);
  const K low = best < rev ? best : rev;  // both halves of the split are bitonic
  if (HIGH) add = wave_bitonic_finish(best < rev ? rev : best, lane);
  best = wave_bitonic_finish(low, lane);
}

// the number of set bits of a ballot below this lane
__device__ __forceinline__ int wave_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

// The pending list of one wave: keys that passed a cheap test wait in pend[0 .. npend) of 128
// entries of LDS until 64 of them are worth one sort and merge.  wave_pend_push() appends the keys
// of the lanes with `cand` in lane order and, once 64 are pending, hands them to
// merge(one key per lane, unsorted) and carries the rest down; it returns how many it appended.
// wave_pend_flush() hands over a partial tail, padded with `empty`.  Every lane of the wave calls
// both, under wave-uniform control flow, with npend = 0 at the start.
//
// The list is PRIVATE TO ONE WAVE: its lanes hand keys to each other through volatile LDS without
// a barrier or fence, which rests on the LDS operations of one wave completing in program order,
// on `volatile` keeping the compiler from reordering or caching the accesses, and on the branches
// around them being wave-uniform.  Sharing it between waves, or dropping the `volatile`, needs a
// barrier.  The carry reads pend[64 + lane] and writes pend[lane], never the region just merged;
// npend <= 63 carried + 64 new = 127 fits the 128 entries.  The storage is the caller's.
template <typename K, typename M>
__device__ __forceinline__ int wave_pend_push(volatile K *pend, int &npend, int lane, bool cand, K key,
                                              M &&merge) {
  const unsigned long long hm = __builtin_amdgcn_ballot_w64(cand);
  const int got = __popcll(hm);
  if (hm) {
    if (cand) pend[npend + wave_rank(hm)] = key;
    npend += got;
    if (npend >= 64) {
      merge(pend[lane]);
      const K carry = pend[64 + lane];
      npend -= 64;
      if (lane < npend) pend[lane] = carry;
    }
  }
  return got;
}

template <typename K, typename M>
__device__ __forceinline__ void wave_pend_flush(volatile K *pend, int npend, int lane, K empty, M &&merge) {
  if (npend > 0) {
    // (not `lane < npend ? pend[lane] : empty`: with two lvalues that selects an ADDRESS, and `empty`
    // then lives in scratch to have one)
    K v = empty;
    if (lane < npend) v = pend[lane];
    merge(v);
  }
}

}  // namespace nesie
