// Axis-aligned 3-D IoU / GIoU of corner boxes (x1, y1, z1, x2, y2, z2): the reference's
// axis_aligned_bbox_overlaps_3d (core/bbox/iou_calculators/iou3d_calculator.py:201-320) in its
// order of operations, with the derivative torch autograd takes of that function.
//
//   nesie_aa_iou3d_paired_forward    is_aligned=True : one thread per pair, value + both Jacobians
//   nesie_aa_iou3d_matrix_forward    is_aligned=False: out (b, m, n), box2 tiles staged in LDS
//   nesie_aa_iou3d_matrix_backward   grad1 (b, m, 6) row sums, grad2 (b, n, 6) column sums, the
//                                    Jacobian recomputed, every sum in a fixed order (no atomics)
//
// Subgradients are autograd's: clamp(x, 0) passes the gradient where x >= 0 (x == 0 included), a
// binary max / min with equal arguments gives each side one half.  The Makefile compiles with
// -ffp-contract=off, so a product and the sum after it round separately, as the reference's
// separate tensor ops do.
#include "common.h"
#include "aa_iou3d_pair.h"

namespace nesie {
namespace {

struct AaPair {          // what one kernel needs of one launch, filled by name at the entry points
  int b, m, n;           // paired: b = m = 1
  const float *box1;     // (b, m, 6)
  const float *box2;     // (b, n, 6)
  int mode;              // 0 IoU, 1 GIoU
  float eps;
};

// 6 floats of a row: three 8-byte accesses (a row starts at a multiple of 24 bytes)
__device__ __forceinline__ void load6(const float *p, float (&v)[6]) {
  const float2 *q = (const float2 *)p;
  const float2 a = q[0], b = q[1], c = q[2];
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y;
}
__device__ __forceinline__ void store6(float *p, const float (&v)[6]) {
  float2 *q = (float2 *)p;
  q[0] = make_float2(v[0], v[1]);
  q[1] = make_float2(v[2], v[3]);
  q[2] = make_float2(v[4], v[5]);
}

// ---- paired ---------------------------------------------------------------------------------
template <bool J1, bool J2>
__global__ __launch_bounds__(256) void aa_paired_kernel(AaPair A, float *__restrict__ out,
                                                        float *__restrict__ jac1,
                                                        float *__restrict__ jac2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  float a[6], b[6], j1[6], j2[6];
  load6(A.box1 + i * 6, a);
  load6(A.box2 + i * 6, b);
  out[i] = aa_pair<J1, J2>(a, b, A.mode, A.eps, j1, j2);
  if (J1) store6(jac1 + i * 6, j1);
  if (J2) store6(jac2 + i * 6, j2);
}

// ---- matrix forward ----------------------------------------------------------------------------
// A workgroup owns MF_ROWS rows x MF_COLS columns of one batch entry.  The column tile of box2 is
// read as one contiguous run (coalesced) and laid out per coordinate in LDS; each thread keeps its
// column's box in registers and walks the rows, whose box is the same address for the whole wave.
constexpr int MF_COLS = 256;
constexpr int MF_ROWS = 32;

__global__ __launch_bounds__(MF_COLS) void aa_matrix_forward_kernel(AaPair A, int row_chunks,
                                                                    int col_tiles,
                                                                    float *__restrict__ out) {
  __shared__ float tile[6][MF_COLS];
  long long t = blockIdx.x;
  const int ct = (int)(t % col_tiles); t /= col_tiles;
  const int rc = (int)(t % row_chunks);
  const int bi = (int)(t / row_chunks);
  const int j0 = ct * MF_COLS;
  const int cols = min(MF_COLS, A.n - j0);
  const float *src = A.box2 + ((long long)bi * A.n + j0) * 6;
  for (int e = threadIdx.x; e < cols * 6; e += MF_COLS) tile[e % 6][e / 6] = src[e];
  __syncthreads();
  if ((int)threadIdx.x >= cols) return;
  float bx[6], unused1[6], unused2[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) bx[c] = tile[c][threadIdx.x];
  const int i0 = rc * MF_ROWS;
  const int i1 = min(i0 + MF_ROWS, A.m);
  for (int i = i0; i < i1; ++i) {
    const long long row = (long long)bi * A.m + i;
    float ax[6];
    load6(A.box1 + row * 6, ax);
    out[row * A.n + j0 + threadIdx.x] =
        aa_pair<false, false>(ax, bx, A.mode, A.eps, unused1, unused2);
  }
}

// ---- matrix backward ---------------------------------------------------------------------------
// grad1[b, i, :] = sum_j grad_out[b, i, j] * d out[b, i, j] / d box1[b, i]: one wave per row, lane l
// takes the columns l, l + 64, ... in ascending order, then the fixed tree of wave_sum_dpp.
constexpr int BR_WAVES = 4;

__global__ __launch_bounds__(64 * BR_WAVES) void aa_matrix_backward_rows_kernel(
    AaPair A, const float *__restrict__ grad_out, float *__restrict__ grad1) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * BR_WAVES + (threadIdx.x >> 6);
  if (row >= (long long)A.b * A.m) return;        // whole waves leave: no barrier below
  const long long bi = row / A.m;
  float ax[6], acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  load6(A.box1 + row * 6, ax);
  const float *g = grad_out + row * A.n;
  const float *b2 = A.box2 + bi * A.n * 6;
  for (int j = lane; j < A.n; j += 64) {
    float bx[6], j1[6], unused[6];
    load6(b2 + (long long)j * 6, bx);
    aa_pair<true, false>(ax, bx, A.mode, A.eps, j1, unused);
    const float gj = g[j];
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += gj * j1[c];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) acc[c] = wave_sum_dpp<64>(acc[c]);
  if (lane == 0) store6(grad1 + row * 6, acc);
}

// grad2[b, j, :] = sum_i grad_out[b, i, j] * d out[b, i, j] / d box2[b, j]: a workgroup owns 64
// columns of one batch entry; lane l of wave w takes column j0 + l and the rows w, w + BC_WAVES, ...
// in ascending order (grad_out reads are coalesced along the row), then the waves' partials are
// added through LDS in wave order.
constexpr int BC_WAVES = 4;

__global__ __launch_bounds__(64 * BC_WAVES) void aa_matrix_backward_cols_kernel(
    AaPair A, int col_tiles, const float *__restrict__ grad_out, float *__restrict__ grad2) {
  __shared__ float part[BC_WAVES][6][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long bi = blockIdx.x / col_tiles;
  const int j = (int)(blockIdx.x % col_tiles) * 64 + lane;
  const bool live = j < A.n;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    float bx[6];
    load6(A.box2 + (bi * A.n + j) * 6, bx);
    for (int i = wave; i < A.m; i += BC_WAVES) {
      const long long row = bi * A.m + i;
      float ax[6], unused[6], j2[6];
      load6(A.box1 + row * 6, ax);
      aa_pair<false, true>(ax, bx, A.mode, A.eps, unused, j2);
      const float gi = grad_out[row * A.n + j];
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += gi * j2[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) part[wave][c][lane] = acc[c];
  __syncthreads();
  if (wave == 0 && live) {
    float s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      s[c] = part[0][c][lane];
#pragma unroll
      for (int w = 1; w < BC_WAVES; ++w) s[c] += part[w][c][lane];
    }
    store6(grad2 + (bi * A.n + j) * 6, s);
  }
}

constexpr long long MAX_GRID = 2147483647LL;

// rows are read and written as three 8-byte accesses
inline bool aligned8(const void *a, const void *b = nullptr, const void *c = nullptr,
                     const void *d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 7) == 0;
}

}  // namespace
}  // namespace nesie

using namespace nesie;

extern "C" int nesie_aa_iou3d_paired_forward(int n, const float *box1, const float *box2, int mode,
                                             float eps, float *out, float *jac1, float *jac2,
                                             void *stream) {
  const char *W = "aa_iou3d_paired_forward";
  NESIE_REQUIRE(n >= 0 && (mode == 0 || mode == 1), W);
  if (n == 0) return NESIE_OK;
  NESIE_REQUIRE(box1 && box2 && out, W);
  NESIE_REQUIRE(aligned8(box1, box2, jac1, jac2), W);
  AaPair A{};
  A.b = 1; A.m = 1; A.n = n;
  A.box1 = box1; A.box2 = box2;
  A.mode = mode; A.eps = eps;
  const dim3 grid(cdiv(n, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  with_bool(jac1 != nullptr, [&](auto J1) {
    with_bool(jac2 != nullptr, [&](auto J2) {
      hipLaunchKernelGGL((aa_paired_kernel<J1(), J2()>), grid, block, 0, s, A, out, jac1, jac2);
    });
  });
  return check_launch(W);
}

extern "C" int nesie_aa_iou3d_matrix_forward(int b, int m, int n, const float *box1,
                                             const float *box2, int mode, float eps, float *out,
                                             void *stream) {
  const char *W = "aa_iou3d_matrix_forward";
  NESIE_REQUIRE(b >= 0 && m >= 0 && n >= 0 && (mode == 0 || mode == 1), W);
  if (b == 0 || m == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(box1 && box2 && out, W);
  NESIE_REQUIRE(aligned8(box1, box2), W);
  AaPair A{};
  A.b = b; A.m = m; A.n = n;
  A.box1 = box1; A.box2 = box2;
  A.mode = mode; A.eps = eps;
  const int row_chunks = cdiv(m, MF_ROWS), col_tiles = cdiv(n, MF_COLS);
  const long long groups = (long long)b * row_chunks * col_tiles;
  if (groups > MAX_GRID) {
    set_error("%s: %d x %d x %d needs %lld workgroups, more than one launch holds", W, b, m, n,
              groups);
    return NESIE_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(aa_matrix_forward_kernel, dim3((unsigned)groups), dim3(MF_COLS), 0,
                     (hipStream_t)stream, A, row_chunks, col_tiles, out);
  return check_launch(W);
}

extern "C" int nesie_aa_iou3d_matrix_backward(int b, int m, int n, const float *box1,
                                              const float *box2, int mode, float eps,
                                              const float *grad_out, float *grad1, float *grad2,
                                              void *stream) {
  const char *W = "aa_iou3d_matrix_backward";
  NESIE_REQUIRE(b >= 0 && m >= 0 && n >= 0 && (mode == 0 || mode == 1), W);
  if (b == 0 || m == 0 || n == 0) return NESIE_OK;
  NESIE_REQUIRE(box1 && box2 && grad_out, W);
  NESIE_REQUIRE(aligned8(box1, box2, grad1, grad2), W);
  AaPair A{};
  A.b = b; A.m = m; A.n = n;
  A.box1 = box1; A.box2 = box2;
  A.mode = mode; A.eps = eps;
  const int col_tiles = cdiv(n, 64);
  const long long row_groups = ((long long)b * m + BR_WAVES - 1) / BR_WAVES;
  const long long col_groups = (long long)b * col_tiles;
  if (row_groups > MAX_GRID || col_groups > MAX_GRID) {
    set_error("%s: %d x %d x %d needs more workgroups than one launch holds", W, b, m, n);
    return NESIE_ERR_UNSUPPORTED;
  }
  if (grad1) {
    hipLaunchKernelGGL(aa_matrix_backward_rows_kernel, dim3((unsigned)row_groups),
                       dim3(64 * BR_WAVES), 0, (hipStream_t)stream, A, grad_out, grad1);
    NESIE_LAUNCHED(W);
  }
  if (grad2) {
    hipLaunchKernelGGL(aa_matrix_backward_cols_kernel, dim3((unsigned)col_groups),
                       dim3(64 * BC_WAVES), 0, (hipStream_t)stream, A, col_tiles, grad_out, grad2);
    return check_launch(W);
  }
  return NESIE_OK;
}
