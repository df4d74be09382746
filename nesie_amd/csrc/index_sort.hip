// Sorted-index primitives for gfx950 (index_sort.h declares them): what the voxel ops, the sparse
// convolution's rulebook, the grouping / interpolation / blend backward and PAConv sort, scan and
// invert their integer indices with.
//
// ix_sort: a STABLE least-significant-digit radix sort of (key, index) pairs, 8 bits a pass, the
// pass count fixed on the host by the bit length of `cells` (the largest key).  A pass is
//   ix_hist_kernel     one workgroup per tile of IX_SORT_TILE keys: 256 LDS counters, integer LDS
//                      atomics (a count does not depend on their order), written digit-major
//                      hist[digit][tile]
//   ix_scan            exclusive scan of the 256 x tiles counters (below)
//   ix_scatter_kernel  the same tile again.  A wave owns 256 consecutive keys and takes them 64 at
//                      a time; a lane finds the lanes of its round with the same digit from eight
//                      ballots, its rank among them is a popcount, and the wave's running count
//                      per digit sits in LDS private to the wave (read by all, advanced by the
//                      highest lane of each group; no atomics assign a slot).  After one barrier a
//                      thread per digit stacks the four waves on the scanned tile base.  Order
//                      inside a digit is wave, round, lane = input order: the pass is stable.
// ix_scan: a two-level exclusive scan of ints for any length -- ix_scan_tiles (IX_SCAN_TILE
// elements per workgroup, tile totals out), ix_scan_sums (one workgroup walks the totals in chunks
// of 256 with a carry, so their number is unbounded) and ix_scan_add.
//
// launch_inverted_index (nesie_inverted_index): the entries of an index row sorted by the source
// point they name, each point's run in ascending entry order; one 1024-thread workgroup per scene
// (and window of source points), the histogram in LDS.
// No float anywhere, no allocation, every launch on the caller's stream.
#include "index_sort.h"

namespace nesie {

constexpr int IX_BLOCK = 256;
constexpr int IX_SCAN_TILE = 1024;  // ints per scan workgroup: 256 threads x 4

// ---- radix sort pass
__global__ __launch_bounds__(IX_BLOCK) void ix_hist_kernel(long long n, int shift, long long nb,
                                                           const unsigned *__restrict__ keys,
                                                           int *__restrict__ hist) {
  __shared__ int h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * IX_SORT_TILE;
#pragma unroll
  for (int k = 0; k < IX_SORT_TILE / IX_BLOCK; ++k) {
    const long long i = base + k * IX_BLOCK + tid;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[(long long)tid * nb + blockIdx.x] = h[tid];
}

__global__ __launch_bounds__(IX_BLOCK) void ix_scatter_kernel(
    long long n, int shift, long long nb, const unsigned *__restrict__ kin,
    const int *__restrict__ iin, unsigned *__restrict__ kout, int *__restrict__ iout,
    const int *__restrict__ hist) {
  constexpr int W = IX_BLOCK / 64, R = IX_SORT_TILE / IX_BLOCK;
  __shared__ int wcnt[W][256];
  __shared__ int off[W][256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < W * 256; i += IX_BLOCK) (&wcnt[0][0])[i] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * IX_SORT_TILE + w * (R * 64);
  volatile int *mine = wcnt[w];
  unsigned key[R];
  int id[R], rank[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = base + r * 64 + lane;
    const bool valid = i < n;
    key[r] = valid ? kin[i] : 0u;
    id[r] = valid ? iin[i] : 0;
    const unsigned d = (key[r] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    // the wave's count of digit d before this round: every lane of the group reads it, then the
    // group's highest lane advances it (LDS serves one wave's accesses in program order)
    const int before = mine[d];
    rank[r] = before + __popcll(peers & ((1ull << lane) - 1ull));
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers >> lane) == 1ull) mine[d] = before + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    int run = hist[(long long)tid * nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      off[k][tid] = run;
      run += wcnt[k][tid];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = base + r * 64 + lane;
    if (i < n) {
      const int dst = off[w][(key[r] >> shift) & 255u] + rank[r];
      kout[dst] = key[r];
      iout[dst] = id[r];
    }
  }
}

// ---- exclusive scan of ints
__global__ __launch_bounds__(IX_BLOCK) void ix_scan_tiles_kernel(long long n,
                                                                 const int *in, int *out,
                                                                 int *__restrict__ sums) {
  __shared__ int lds[IX_BLOCK / 64];
  const long long i0 = (long long)blockIdx.x * IX_SCAN_TILE + threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
  int total;
  int run = block_excl<IX_BLOCK>(v[0] + v[1] + v[2] + v[3], lds, total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the tile totals become their exclusive prefix; the grand total goes to *total
// and, when given, min(total, cap) to *capped
__global__ __launch_bounds__(IX_BLOCK) void ix_scan_sums_kernel(long long nt, int *__restrict__ sums,
                                                                int *__restrict__ total_out,
                                                                int *__restrict__ capped, int cap) {
  __shared__ int lds[IX_BLOCK / 64];
  int carry = 0;
  for (long long b = 0; b < nt; b += IX_BLOCK) {
    const long long i = b + threadIdx.x;
    const int v = i < nt ? sums[i] : 0;
    int total;
    const int ex = block_excl<IX_BLOCK>(v, lds, total);
    if (i < nt) sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (total_out) *total_out = carry;
    if (capped) *capped = carry < cap ? carry : cap;
  }
}

__global__ __launch_bounds__(IX_BLOCK) void ix_scan_add_kernel(long long n, int *__restrict__ out,
                                                               const int *__restrict__ sums) {
  const long long i0 = (long long)blockIdx.x * IX_SCAN_TILE + threadIdx.x * 4;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < n) out[i0 + k] += add;
}

// ---- host side of the sort and the scan
IxWorkspace ix_carve(void *ws, long long n) {
  IxWorkspace w;
  w.nb = cdiv_ll(n, IX_SORT_TILE);
  const long long hist = 256 * w.nb;
  const long long sums = cdiv_ll(hist > n ? hist : n, IX_SCAN_TILE) + 1;
  int *p = (int *)ws;
  w.ka = (unsigned *)p; p += n;
  w.kb = (unsigned *)p; p += n;
  w.ia = p; p += n;
  w.ib = p; p += n;
  w.flag = p; p += n;
  w.hist = p; p += hist;
  w.sums = p; p += sums;
  w.meta = p; p += 4;
  w.ints = 5 * n + hist + sums + 4;
  return w;
}

int ix_check_n_cells(const char *W, long long n, long long cells) {
  NESIE_REQUIRE(n >= 0, W);
  if (cells < 1 || cells >= 2147483648LL) {
    set_error("%s: %lld cells outside 1 .. 2^31 - 1", W, cells);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (n > IX_MAX_N) {
    set_error("%s: %lld points, at most %lld", W, n, IX_MAX_N);
    return NESIE_ERR_UNSUPPORTED;
  }
  return NESIE_OK;
}

// out may alias in.  total_out / capped: see ix_scan_sums_kernel
int ix_scan(const char *W, long long n, const int *in, int *out, int *sums, int *total_out,
            int *capped, int cap, hipStream_t s) {
  const long long nt = cdiv_ll(n, IX_SCAN_TILE);
  hipLaunchKernelGGL(ix_scan_tiles_kernel, dim3((unsigned)nt), dim3(IX_BLOCK), 0, s, n, in, out,
                     sums);
  NESIE_LAUNCHED(W);
  hipLaunchKernelGGL(ix_scan_sums_kernel, dim3(1), dim3(IX_BLOCK), 0, s, nt, sums, total_out,
                     capped, cap);
  NESIE_LAUNCHED(W);
  if (nt > 1) {
    hipLaunchKernelGGL(ix_scan_add_kernel, dim3((unsigned)nt), dim3(IX_BLOCK), 0, s, n, out, sums);
    NESIE_LAUNCHED(W);
  }
  return NESIE_OK;
}

static int ix_passes(long long cells) {  // keys lie in 0 .. cells
  int bits = 0;
  while ((cells >> bits) != 0) ++bits;
  return (bits + 7) / 8;
}

// sorts (w.ka, w.ia) by key; the sorted keys end in *keys, the indices in *idx (`last_idx` when
// given receives the indices of the last pass directly)
int ix_sort(const char *W, long long n, long long cells, const IxWorkspace &w, int *last_idx,
            const unsigned **keys, const int **idx, hipStream_t s) {
  const int passes = ix_passes(cells);
  unsigned *const kbuf[2] = {w.ka, w.kb};
  int *const ibuf[2] = {w.ia, w.ib};
  int *iout = w.ia;
  for (int p = 0; p < passes; ++p) {
    const int src = p & 1, dst = src ^ 1;
    const int *iin = iout;
    iout = (p == passes - 1 && last_idx) ? last_idx : ibuf[dst];
    hipLaunchKernelGGL(ix_hist_kernel, dim3((unsigned)w.nb), dim3(IX_BLOCK), 0, s, n, 8 * p, w.nb,
                       kbuf[src], w.hist);
    NESIE_LAUNCHED(W);
    const int e = ix_scan(W, 256 * w.nb, w.hist, w.hist, w.sums, nullptr, nullptr, 0, s);
    if (e != NESIE_OK) return e;
    hipLaunchKernelGGL(ix_scatter_kernel, dim3((unsigned)w.nb), dim3(IX_BLOCK), 0, s, n, 8 * p,
                       w.nb, kbuf[src], iin, kbuf[dst], iout, w.hist);
    NESIE_LAUNCHED(W);
  }
  *keys = kbuf[passes & 1];
  *idx = iout;
  return NESIE_OK;
}

// ---- inverted index
// Inverted index of idx[b][0..e_total) over n source points, one workgroup per scene: LDS
// histogram (integer ds_add), exclusive scan, then each column takes the next free slot of its
// point's run (returning ds_add).  Built on the side stream with the ball query: 8 workgroups,
// tens of microseconds.  The slots are claimed in arrival order into `scratch`; a second pass
// ranks every entry inside its run (runs are short: M ns / N on average), so `order` lists each
// run in ascending column order and the segmented sums of the backward are reproducible.
constexpr int II_BLOCK = 1024, II_WAVES = II_BLOCK / 64;
constexpr int II_WINDOW = 8192;     // source points per workgroup (LDS histogram + cursor)

// Any n (round 5): workgroup (scene, window w) owns the source points [w * II_WINDOW, + II_WINDOW):
// it first counts the entries that belong to EARLIER windows (that many positions of order / srcs lie
// in front of its own), then sorts its own entries as before.  Every window reads the whole index
// row, so the cost grows with the window count -- 5 windows at 40 000 points; the step itself only
// ever inverts indices over <= 2 048 points (the 40 000-point level carries no feature gradient).
__global__ __launch_bounds__(II_BLOCK) void inverted_index_kernel(
    int n, int e_total, const int *__restrict__ idx, int *__restrict__ order,
    int *__restrict__ srcs, int *__restrict__ scratch_out) {
  extern __shared__ int lds[];  // cursor[bins]; scan scratch [II_BLOCK]; base counter
  const int lo_pt = blockIdx.y * II_WINDOW;
  const int bins = n - lo_pt < II_WINDOW ? n - lo_pt : II_WINDOW;
  int *cur = lds, *scratch = lds + bins, *before = scratch + II_BLOCK;
  const int bi = blockIdx.x, tid = threadIdx.x;
  const int *ix = idx + (size_t)bi * e_total;
  for (int j = tid; j < bins; j += II_BLOCK) cur[j] = 0;
  if (tid == 0) *before = 0;
  __syncthreads();
  int mine_before = 0;
  for (int e = tid; e < e_total; e += II_BLOCK) {
    int s = ix[e];
    s = s < 0 ? 0 : (s >= n ? n - 1 : s);
    if (s < lo_pt) ++mine_before;
    else if (s < lo_pt + bins) atomicAdd(&cur[s - lo_pt], 1);
  }
  if (lo_pt > 0) {
    mine_before = wave_sum(mine_before);
    if ((tid & 63) == 0 && mine_before) atomicAdd(before, mine_before);
  }
  __syncthreads();
  const int base = *before;
  // exclusive scan over the bins: each thread owns a contiguous chunk
  const int per = (bins + II_BLOCK - 1) / II_BLOCK;
  const int lo = tid * per, hi = lo + per < bins ? lo + per : bins;
  int sum = 0;
  for (int j = lo; j < hi; ++j) sum += cur[j];
  // (Hillis-Steele over one int per thread, kept here: block_excl measured 4 % slower in this kernel)
  scratch[tid] = sum;
  __syncthreads();
  for (int d = 1; d < II_BLOCK; d <<= 1) {
    const int v = tid >= d ? scratch[tid - d] : 0;
    __syncthreads();
    scratch[tid] += v;
    __syncthreads();
  }
  int run = base + scratch[tid] - sum;  // first position of this chunk
  for (int j = lo; j < hi; ++j) {
    const int cnt = cur[j];
    cur[j] = run;  // becomes the cursor of point lo_pt + j
    run += cnt;
  }
  __syncthreads();
  int *ord = order + (size_t)bi * e_total;
  int *sr = srcs + (size_t)bi * e_total;
  int *tmp = scratch_out + (size_t)bi * e_total;
  for (int e = tid; e < e_total; e += II_BLOCK) {
    int s = ix[e];
    s = s < 0 ? 0 : (s >= n ? n - 1 : s);
    if (s >= lo_pt && s < lo_pt + bins) tmp[atomicAdd(&cur[s - lo_pt], 1)] = e;
  }
  __syncthreads();   // cur[j] is now the END of run j; run j starts where run j - 1 ends (run 0: at base)
  const int total = cur[bins - 1];
  for (int i = base + tid; i < total; i += II_BLOCK) {
    const int e = tmp[i];
    int s = ix[e];
    s = (s < 0 ? 0 : (s >= n ? n - 1 : s)) - lo_pt;
    sr[i] = s + lo_pt;
    const int lo_s = s > 0 ? cur[s - 1] : base, hi_s = cur[s];
    int rank = 0;
    for (int k = lo_s; k < hi_s; ++k) rank += tmp[k] < e ? 1 : 0;
    ord[lo_s + rank] = e;
  }
}

// The same index by a STABLE counting sort (n <= II_STABLE_N bins): no ranking pass.  Wave w of the
// 16 owns a contiguous range of entries and keeps its own histogram row cnt[w][.] in LDS; after the
// scan cnt[w][s] is where wave w's first entry of bin s goes (bin-major, wave-minor), and the wave
// places its entries 64 at a time in ascending order: the lanes that hold the same bin find each
// other with a ballot per distinct bin of the round and take consecutive positions in lane order.
// The result is `order` ascending inside every run by construction -- what the ranking pass of
// inverted_index_kernel computes in time quadratic in the run length.
constexpr int II_STABLE_N = 2048;

__global__ __launch_bounds__(II_BLOCK) void inverted_index_stable_kernel(
    int n, int e_total, const int *__restrict__ idx, int *__restrict__ order,
    int *__restrict__ srcs) {
  extern __shared__ int lds[];                       // cnt[II_WAVES][n], then scan scratch [II_WAVES]
  int *cnt = lds, *scratch = lds + II_WAVES * n;
  const int bi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int *ix = idx + (size_t)bi * e_total;
  for (int j = tid; j < II_WAVES * n; j += II_BLOCK) cnt[j] = 0;
  __syncthreads();
  const int per = ((e_total + II_WAVES - 1) / II_WAVES + 63) / 64 * 64;   // entries per wave, whole rounds
  const int e0 = wave * per, e1 = e0 + per < e_total ? e0 + per : e_total;
  int *mine = cnt + wave * n;
  for (int e = e0 + lane; e < e1; e += 64) {
    int s = ix[e];
    s = s < 0 ? 0 : (s >= n ? n - 1 : s);
    atomicAdd(&mine[s], 1);
  }
  __syncthreads();
  counting_sort_starts<II_BLOCK>(cnt, n, scratch, nullptr);
  int *ord = order + (size_t)bi * e_total;
  int *sr = srcs + (size_t)bi * e_total;
  volatile int *cur = mine;                          // this wave's cursors (only this wave touches them)
  for (int base = e0; base < e1; base += 64) {
    const int e = base + lane;
    const bool live = e < e1;
    int s = live ? ix[e] : 0;
    s = s < 0 ? 0 : (s >= n ? n - 1 : s);
    unsigned long long todo = __ballot(live);
    while (todo) {                                   // one trip per distinct bin of the round
      const int leader = __builtin_ctzll(todo);
      const int s0 = __builtin_amdgcn_readlane(s, leader);
      const unsigned long long mask = __ballot(live && s == s0);
      const int start = cur[s0];
      if (live && s == s0) {
        const int pos = start + __popcll(mask & ((1ull << lane) - 1ull));
        ord[pos] = e;
        sr[pos] = s0;
      }
      if (lane == leader) cur[s0] = start + __popcll(mask);
      __builtin_amdgcn_wave_barrier();
      todo &= ~mask;
    }
  }
}

int launch_inverted_index(int b, int n, long long e_total, const int *idx, int *order, int *sources,
                          int *scratch, hipStream_t s) {
  const char *W = "inverted_index";
  NESIE_REQUIRE(b >= 0 && n >= 1 && e_total >= 0 && e_total < (1ll << 31), W);
  if (b == 0 || e_total == 0) return NESIE_OK;  // nothing to sort: no launch, null tensors allowed
  NESIE_REQUIRE(idx && order && sources && scratch, W);
  if (n <= II_STABLE_N) {               // stable counting sort: ascending runs without a ranking pass
    const size_t lds = ((size_t)II_WAVES * n + II_WAVES) * sizeof(int);
    launch_lds<inverted_index_stable_kernel, ((size_t)II_WAVES * II_STABLE_N + II_WAVES) * sizeof(int)>(
        dim3(b), dim3(II_BLOCK), lds, s, n, (int)e_total, idx, order, sources);
    return check_launch(W);
  }
  const int windows = cdiv(n, II_WINDOW);
  NESIE_REQUIRE(windows <= 65535, W);
  const size_t lds = ((size_t)(n < II_WINDOW ? n : II_WINDOW) + II_BLOCK + 1) * sizeof(int);
  hipLaunchKernelGGL(inverted_index_kernel, dim3(b, windows), dim3(II_BLOCK), lds, s, n, (int)e_total, idx, order,
                     sources, scratch);
  return check_launch(W);
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_inverted_index(int b, int n, long long e_total, const int *idx, int *order,
                                    int *sources, int *scratch, void *stream) {
  return launch_inverted_index(b, n, e_total, idx, order, sources, scratch, (hipStream_t)stream);
}
