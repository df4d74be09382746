// Differentiable rotated 3-D IoU of box pairs in ONE kernel (value + Jacobian).
//
// Replaces, for the IoU3D loss and the IoU labels of the quality head, the ~100 small
// torch kernels per call of the reference's chain
//   cal_iou_3d -> cal_iou -> box2corners_th / oriented_box_intersection_2d
//   (mmdet3d/ops/rotated_iou/oriented_iou_loss.py:6-109, box_intersection_2d.py:13-184)
// plus its sort_vertices launch.  One thread owns one (prediction, target) pair and walks
// the same formulas in the same order: corners, 4x4 edge intersections with the
// t,u in (0,1) test and the `num + 1e-8` re-division, corner-in-box tests with 1e-6
// slack, mean-centred angular sort (vertex_order.h), shoelace area, z overlap.
// Gradients w.r.t. the 7 parameters of the FIRST box are carried forward as dual numbers
// (masks and the vertex order are piecewise constant, exactly as autograd treats them);
// the second box is a constant (targets never require grad on this path).
#include "vertex_order.h"
#include <math.h>

namespace nesie {

template <int ND>
struct Dual {
  float v;
  float d[ND > 0 ? ND : 1];
  __device__ Dual() {}
  __device__ explicit Dual(float c) : v(c) {
#pragma unroll
    for (int i = 0; i < ND; ++i) d[i] = 0.f;
  }
  __device__ static Dual var(float c, int k) {
    Dual r(c);
    if (ND > 0) r.d[k] = 1.f;
    return r;
  }
};
#define DUAL_BIN(OP, VAL, DA, DB)                                         \
  template <int ND>                                                        \
  __device__ __forceinline__ Dual<ND> OP(const Dual<ND> &a, const Dual<ND> &b) { \
    Dual<ND> r;                                                            \
    r.v = VAL;                                                             \
    _Pragma("unroll") for (int i = 0; i < ND; ++i) r.d[i] = (DA)*a.d[i] + (DB)*b.d[i]; \
    return r;                                                              \
  }
DUAL_BIN(operator+, a.v + b.v, 1.f, 1.f)
DUAL_BIN(operator-, a.v - b.v, 1.f, -1.f)
DUAL_BIN(operator*, a.v * b.v, b.v, a.v)
DUAL_BIN(operator/, a.v / b.v, 1.f / b.v, -(a.v / b.v) / b.v)
template <int ND>
__device__ __forceinline__ Dual<ND> operator*(const Dual<ND> &a, float c) {
  Dual<ND> r;
  r.v = a.v * c;
#pragma unroll
  for (int i = 0; i < ND; ++i) r.d[i] = a.d[i] * c;
  return r;
}
template <int ND>
__device__ __forceinline__ Dual<ND> operator+(const Dual<ND> &a, float c) {
  Dual<ND> r = a;
  r.v = a.v + c;
  return r;
}
template <int ND>
__device__ __forceinline__ Dual<ND> operator-(const Dual<ND> &a) { return a * -1.f; }
template <int ND>
__device__ __forceinline__ Dual<ND> dsin(const Dual<ND> &a) {
  Dual<ND> r;
  r.v = sinf(a.v);
  const float c = cosf(a.v);
#pragma unroll
  for (int i = 0; i < ND; ++i) r.d[i] = c * a.d[i];
  return r;
}
template <int ND>
__device__ __forceinline__ Dual<ND> dcos(const Dual<ND> &a) {
  Dual<ND> r;
  r.v = cosf(a.v);
  const float s = -sinf(a.v);
#pragma unroll
  for (int i = 0; i < ND; ++i) r.d[i] = s * a.d[i];
  return r;
}
template <int ND>
__device__ __forceinline__ Dual<ND> dmin(const Dual<ND> &a, const Dual<ND> &b) {
  return a.v <= b.v ? a : b;
}
template <int ND>
__device__ __forceinline__ Dual<ND> dmax(const Dual<ND> &a, const Dual<ND> &b) {
  return a.v >= b.v ? a : b;
}

// corners of (x, y, w, h, alpha): (+,+) (-,+) (-,-) (+,-) halves rotated by +alpha
template <int ND>
__device__ __forceinline__ void corners_of(const Dual<ND> &x, const Dual<ND> &y, const Dual<ND> &w,
                                           const Dual<ND> &h, const Dual<ND> &al,
                                           Dual<ND> (&cx)[4], Dual<ND> (&cy)[4]) {
  const Dual<ND> s = dsin(al), c = dcos(al);
  const Dual<ND> hw = w * 0.5f, hh = h * 0.5f;
  const float sx[4] = {1.f, -1.f, -1.f, 1.f}, sy[4] = {1.f, 1.f, -1.f, -1.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const Dual<ND> x4 = hw * sx[k], y4 = hh * sy[k];
    cx[k] = (x4 * c + y4 * (-s)) + x;   // [x4, y4] @ [[c, s], [-s, c]]
    cy[k] = (x4 * s + y4 * c) + y;
  }
}

// What one (prediction, target) pair yields: the IoU chain of cal_iou_3d(verbose=True) up to the
// 3-D IoU, with the pieces the enclosing-box losses read on top of it.
template <int ND>
struct PairGeom {
  Dual<ND> b1[7], b2[7];
  Dual<ND> c1x[4], c1y[4], c2x[4], c2y[4];   // BEV corners, box2corners_th order
  Dual<ND> zmax1, zmin1, zmax2, zmin2;
  Dual<ND> u3d, iou3d;
};

// The per-pair body shared by iou3d_kernel and giou3d_kernel.  SPLIT (with ND = 1): the thread
// carries the derivative with respect to parameter `comp` only.
template <int ND, bool SPLIT>
__device__ __forceinline__ void pair_body(const float *__restrict__ p, const float *__restrict__ q,
                                          int comp, PairGeom<ND> &g) {
  typedef Dual<ND> D;
  D (&b1)[7] = g.b1, (&b2)[7] = g.b2;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    if (SPLIT) { b1[k] = D(p[k]); if (k == comp) b1[k].d[0] = 1.f; }
    else b1[k] = D::var(p[k], k);
    b2[k] = D(q[k]);
  }

  // ---- BEV corners -----------------------------------------------------------------
  D (&c1x)[4] = g.c1x, (&c1y)[4] = g.c1y, (&c2x)[4] = g.c2x, (&c2y)[4] = g.c2y;
  corners_of(b1[0], b1[1], b1[3], b1[4], b1[6], c1x, c1y);
  corners_of(b2[0], b2[1], b2[3], b2[4], b2[6], c2x, c2y);

  // ---- candidate vertices: 4 + 4 corners, 16 edge intersections ----------------------
  D vx[SV_MAXV], vy[SV_MAXV];
  unsigned mbits = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) { vx[k] = c1x[k]; vy[k] = c1y[k]; vx[4 + k] = c2x[k]; vy[4 + k] = c2y[k]; }
#pragma unroll
  for (int e1 = 0; e1 < 4; ++e1) {
#pragma unroll
    for (int e2 = 0; e2 < 4; ++e2) {
      const D x1 = c1x[e1], y1 = c1y[e1], x2 = c1x[(e1 + 1) & 3], y2 = c1y[(e1 + 1) & 3];
      const D x3 = c2x[e2], y3 = c2y[e2], x4 = c2x[(e2 + 1) & 3], y4 = c2y[(e2 + 1) & 3];
      const D num = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4);
      const D den_t = (x1 - x3) * (y3 - y4) - (y1 - y3) * (x3 - x4);
      const D den_u = (x1 - x2) * (y1 - y3) - (y1 - y2) * (x1 - x3);
      const bool zero = num.v == 0.f;
      const float t = zero ? -1.f : den_t.v / num.v;
      const float u = zero ? -1.f : -den_u.v / num.v;
      const bool m = (t > 0.f) && (t < 1.f) && (u > 0.f) && (u < 1.f);
      const D t2 = den_t / (num + 1e-8f);
      const int slot = 8 + e1 * 4 + e2;
      if (m) {
        vx[slot] = x1 + t2 * (x2 - x1);
        vy[slot] = y1 + t2 * (y2 - y1);
        mbits |= 1u << slot;
      } else {
        vx[slot] = D(0.f); vy[slot] = D(0.f);  // masked: value 0, zero gradient
      }
    }
  }
  // corner-in-other-box tests (values only)
  {
    const float ax = c2x[0].v, ay = c2y[0].v;
    const float abx = c2x[1].v - ax, aby = c2y[1].v - ay, adx = c2x[3].v - ax, ady = c2y[3].v - ay;
    const float nab = abx * abx + aby * aby, nad = adx * adx + ady * ady;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float amx = c1x[k].v - ax, amy = c1y[k].v - ay;
      const float pab = (abx * amx + aby * amy) / nab, pad = (adx * amx + ady * amy) / nad;
      if (pab > -1e-6f && pab < 1.f + 1e-6f && pad > -1e-6f && pad < 1.f + 1e-6f) mbits |= 1u << k;
    }
  }
  {
    const float ax = c1x[0].v, ay = c1y[0].v;
    const float abx = c1x[1].v - ax, aby = c1y[1].v - ay, adx = c1x[3].v - ax, ady = c1y[3].v - ay;
    const float nab = abx * abx + aby * aby, nad = adx * adx + ady * ady;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float amx = c2x[k].v - ax, amy = c2y[k].v - ay;
      const float pab = (abx * amx + aby * amy) / nab, pad = (adx * amx + ady * amy) / nad;
      if (pab > -1e-6f && pab < 1.f + 1e-6f && pad > -1e-6f && pad < 1.f + 1e-6f) mbits |= 1u << (4 + k);
    }
  }
  // ---- order the valid vertices about their mean -------------------------------------
  const int nv = __popc(mbits);
  float sxm = 0.f, sym = 0.f;
#pragma unroll
  for (int k = 0; k < SV_MAXV; ++k) {
    const float mk = (mbits >> k) & 1u ? 1.f : 0.f;
    sxm += vx[k].v * mk; sym += vy[k].v * mk;
  }
  const float mxv = sxm / (float)nv, myv = sym / (float)nv;  // 0/0 -> NaN when nv == 0, unused
  float nx[SV_MAXV], ny[SV_MAXV];
#pragma unroll
  for (int k = 0; k < SV_MAXV; ++k) { nx[k] = vx[k].v - mxv; ny[k] = vy[k].v - myv; }
  int o[SV_NIDX];
  sv_sort_one(nx, ny, mbits, nv, SV_MAXV, o);

  // ---- shoelace over the 9 gathered (un-centred) vertices -----------------------------
  D total(0.f);
  for (int k = 0; k < SV_NIDX - 1; ++k) {
    const int a = o[k], b = o[k + 1];
    total = total + (vx[a] * vy[b] - vy[a] * vx[b]);
  }
  const D inter = (total.v >= 0.f ? total : -total) * 0.5f;

  // ---- IoU in the plane, then with the z overlap ---------------------------------------
  const D area1 = b1[3] * b1[4], area2 = b2[3] * b2[4];
  const D uni = area1 + area2 - inter;
  const D iou2d = inter / uni;
  g.zmax1 = b1[2] + b1[5] * 0.5f; g.zmin1 = b1[2] - b1[5] * 0.5f;
  g.zmax2 = b2[2] + b2[5] * 0.5f; g.zmin2 = b2[2] - b2[5] * 0.5f;
  D zov = dmin(g.zmax1, g.zmax2) - dmax(g.zmin1, g.zmin2);
  if (zov.v < 0.f) zov = D(0.f);  // clamp_min(0)
  const D inter3 = iou2d * uni * zov;
  const D v1 = b1[3] * b1[4] * b1[5], v2 = b2[3] * b2[4] * b2[5];
  g.u3d = v1 + v2 - inter3;
  g.iou3d = inter3 / g.u3d;
}

// SPLIT (with ND = 1): eight threads per pair, thread `comp` carries the derivative with respect
// to parameter `comp` only (the components of a dual number never mix, so every derivative is
// the same chain of operations as in the 7-wide form: identical bits) -- a quarter of the serial
// work per thread and eight times the threads for a kernel that is pure latency at 2 048 pairs.
template <int ND, bool SPLIT>
__global__ __launch_bounds__(64) void iou3d_kernel(int n, const float *__restrict__ box1,
                                                   const float *__restrict__ box2,
                                                   float *__restrict__ iou,
                                                   float *__restrict__ jac) {
  const int gid = blockIdx.x * 64 + threadIdx.x;
  const int i = SPLIT ? gid >> 3 : gid;
  const int comp = gid & 7;
  if (i >= n || (SPLIT && comp == 7)) return;
  PairGeom<ND> g;
  pair_body<ND, SPLIT>(box1 + (size_t)i * 7, box2 + (size_t)i * 7, comp, g);
  const Dual<ND> &out = g.iou3d;
  if (SPLIT) {
    if (comp == 0) iou[i] = out.v;
    jac[(size_t)i * 7 + comp] = out.d[0];
    return;
  }
  iou[i] = out.v;
  if (ND > 0) {
#pragma unroll
    for (int k = 0; k < ND; ++k) jac[(size_t)i * 7 + k] = out.d[k];
  }
}

// ---- enclosing boxes of the 8 BEV corners (cal_giou_3d / cal_diou_3d) ---------------------------
template <int ND>
__device__ __forceinline__ Dual<ND> dsqrt(const Dual<ND> &a) {
  Dual<ND> r;
  r.v = sqrtf(a.v);
  const float c = 0.5f / r.v;
#pragma unroll
  for (int i = 0; i < ND; ++i) r.d[i] = c * a.d[i];
  return r;
}
template <int ND>
__device__ __forceinline__ Dual<ND> dabs(const Dual<ND> &a) {   // sign(0) = 0, as torch.abs
  Dual<ND> r;
  r.v = fabsf(a.v);
  const float s = a.v > 0.f ? 1.f : (a.v < 0.f ? -1.f : 0.f);
#pragma unroll
  for (int i = 0; i < ND; ++i) r.d[i] = s * a.d[i];
  return r;
}
// torch.max / torch.min of two tensors: on a tie each side gets half the gradient
template <int ND>
__device__ __forceinline__ Dual<ND> dhalf_tie(const Dual<ND> &a, const Dual<ND> &b) {
  Dual<ND> r;
  r.v = a.v;
#pragma unroll
  for (int i = 0; i < ND; ++i) r.d[i] = 0.5f * a.d[i] + 0.5f * b.d[i];
  return r;
}
template <int ND>
__device__ __forceinline__ Dual<ND> dmax_tie(const Dual<ND> &a, const Dual<ND> &b) {
  return a.v > b.v ? a : (b.v > a.v ? b : dhalf_tie(a, b));
}
template <int ND>
__device__ __forceinline__ Dual<ND> dmin_tie(const Dual<ND> &a, const Dual<ND> &b) {
  return a.v < b.v ? a : (b.v < a.v ? b : dhalf_tie(a, b));
}

// One candidate of min_enclosing_box.py: the box with a side along the line through corners i < j.
// w = the range of the projections of all 8 corners onto the line (:116-139), h = the range of the
// distances of the other 6 from it (:87-113); every expression in the reference's order.  A max or
// min over a dimension takes the first of equal entries in the reference's order of the points
// (the line's two, then the others ascending), which decides whose derivative an exact tie gets.
template <int ND>
__device__ __forceinline__ void enclosing_candidate(const Dual<ND> (&px)[8], const Dual<ND> (&py)[8],
                                                    int i, int j, Dual<ND> &w, Dual<ND> &h) {
  typedef Dual<ND> D;
  D x1 = px[0], y1 = py[0], x2 = px[1], y2 = py[1];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    if (k == i) { x1 = px[k]; y1 = py[k]; }
    if (k == j) { x2 = px[k]; y2 = py[k]; }
  }
  const D dx = x2 - x1, dy = y2 - y1;
  const D slope = dy / (dx + 1e-8f);
  D nrm;   // |(1, slope)|: only its value is read
  nrm.v = sqrtf(slope.v * slope.v + 1.f);
  const D num = dsqrt(dy * dy + dx * dx + 1e-14f);
  const float inf = __builtin_inff();
  // projections on values; the two corners that give the range keep their derivatives
  float pmax = (x1.v + y1.v * slope.v) / nrm.v, pmin = pmax;
  D xa = x1, ya = y1, xb = x1, yb = y1;
  {
    const float pr = (x2.v + y2.v * slope.v) / nrm.v;
    if (pr > pmax) { pmax = pr; xa = x2; ya = y2; }
    if (pr < pmin) { pmin = pr; xb = x2; yb = y2; }
  }
  D dmx(-inf), dmn(inf), amx(-1.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k == i || k == j) continue;
    const float pr = (px[k].v + py[k].v * slope.v) / nrm.v;
    if (pr > pmax) { pmax = pr; xa = px[k]; ya = py[k]; }
    if (pr < pmin) { pmin = pr; xb = px[k]; yb = py[k]; }
    const D d = (dy * px[k] - dx * py[k] + x2 * y1 - y2 * x1) / num;
    const D a = dabs(d);
    if (d.v > dmx.v) dmx = d;
    if (d.v < dmn.v) dmn = d;
    if (a.v > amx.v) amx = a;
  }
  // w = proj(a) - proj(b) = (ex + slope * ey) / nrm with e = a - b.  Its derivative is taken of
  // that one quotient with the slope terms collected, (ex' + slope ey') / nrm + slope' (ey - slope
  // ex) / nrm^3: the same derivative as of the two projections one by one, without the
  // cancellation between slope' ey / nrm and w nrm' / nrm, each ~1e8 x the result on an edge
  // that is vertical (slope = dy / 1e-8).
  w.v = pmax - pmin;
  {
    const D ex = xa - xb, ey = ya - yb;
    const float t = (ey.v - slope.v * ex.v) / (nrm.v * nrm.v);
#pragma unroll
    for (int c = 0; c < ND; ++c) w.d[c] = ((ex.d[c] + slope.v * ey.d[c]) + slope.d[c] * t) / nrm.v;
  }
  h = dmax_tie(dmx - dmn, amx);
}

// ENCLOSING 0 "smallest": the 24 candidate areas on values only, the first minimum wins (area
// + 1e8 where it is exactly 0), then the winner's (w, h) again with derivatives.  1 "aligned":
// the x and y ranges of the corners, per box first and then across (oriented_iou_loss.py:166-194).
template <int ND, int ENCLOSING>
__device__ __forceinline__ void enclosing_box(const PairGeom<ND> &g, Dual<ND> &w, Dual<ND> &h) {
  typedef Dual<ND> D;
  if (ENCLOSING == 1) {
    D x1mx = g.c1x[0], x1mn = g.c1x[0], y1mx = g.c1y[0], y1mn = g.c1y[0];
    D x2mx = g.c2x[0], x2mn = g.c2x[0], y2mx = g.c2y[0], y2mn = g.c2y[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (g.c1x[k].v > x1mx.v) x1mx = g.c1x[k];
      if (g.c1x[k].v < x1mn.v) x1mn = g.c1x[k];
      if (g.c1y[k].v > y1mx.v) y1mx = g.c1y[k];
      if (g.c1y[k].v < y1mn.v) y1mn = g.c1y[k];
      if (g.c2x[k].v > x2mx.v) x2mx = g.c2x[k];
      if (g.c2x[k].v < x2mn.v) x2mn = g.c2x[k];
      if (g.c2y[k].v > y2mx.v) y2mx = g.c2y[k];
      if (g.c2y[k].v < y2mn.v) y2mn = g.c2y[k];
    }
    w = dmax_tie(x1mx, x2mx) - dmin_tie(x1mn, x2mn);
    h = dmax_tie(y1mx, y2mx) - dmin_tie(y1mn, y2mn);
    return;
  }
  D px[8], py[8];
  Dual<0> vx[8], vy[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    px[k] = g.c1x[k]; py[k] = g.c1y[k]; px[4 + k] = g.c2x[k]; py[4 + k] = g.c2y[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) { vx[k].v = px[k].v; vy[k].v = py[k].v; }
  float best = __builtin_inff();
  int bi = 0, bj = 1;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = i + 1; j < 8; ++j) {
      if ((i == 0 && j == 2) || (i == 1 && j == 3) || (i == 5 && j == 7) || (i == 4 && j == 6))
        continue;   // a diagonal of one box is never a hull edge
      Dual<0> cw, ch;
      enclosing_candidate(vx, vy, i, j, cw, ch);
      float area = cw.v * ch.v;
      if (area == 0.f) area += 1e8f;
      if (area < best) { best = area; bi = i; bj = j; }
    }
  }
  enclosing_candidate(px, py, bi, bj, w, h);
}

template <int ND, bool SPLIT, int ENCLOSING>
__global__ __launch_bounds__(64) void giou3d_kernel(int n, const float *__restrict__ box1,
                                                    const float *__restrict__ box2, int kind,
                                                    float *__restrict__ loss,
                                                    float *__restrict__ iou,
                                                    float *__restrict__ jac) {
  typedef Dual<ND> D;
  const int gid = blockIdx.x * 64 + threadIdx.x;
  const int i = SPLIT ? gid >> 3 : gid;
  const int comp = gid & 7;
  if (i >= n || (SPLIT && comp == 7)) return;
  PairGeom<ND> g;
  pair_body<ND, SPLIT>(box1 + (size_t)i * 7, box2 + (size_t)i * 7, comp, g);
  D w, h;
  enclosing_box<ND, ENCLOSING>(g, w, h);
  D zr = dmax_tie(g.zmax1, g.zmax2) - dmin_tie(g.zmin1, g.zmin2);
  if (zr.v < 0.f) zr = D(0.f);  // clamp_min(0)
  D extra;
  if (kind == 0) {
    const D vc = zr * w * h;
    extra = (vc - g.u3d) / vc;
  } else {
    const D xo = g.b1[0] - g.b2[0], yo = g.b1[1] - g.b2[1], zo = g.b1[2] - g.b2[2];
    const D d2 = xo * xo + yo * yo + zo * zo;
    const D c2 = w * w + h * h + zr * zr;
    extra = d2 / c2;
  }
  const D out = -g.iou3d + 1.f + extra;   // 1. - iou3d + extra
  if (SPLIT) {
    if (comp == 0) {
      loss[i] = out.v;
      if (iou) iou[i] = g.iou3d.v;
    }
    jac[(size_t)i * 7 + comp] = out.d[0];
    return;
  }
  loss[i] = out.v;
  if (iou) iou[i] = g.iou3d.v;
  if (ND > 0) {
#pragma unroll
    for (int k = 0; k < ND; ++k) jac[(size_t)i * 7 + k] = out.d[k];
  }
}

}  // namespace nesie

using namespace nesie;

extern "C" int nesie_iou3d_forward(int n, const float *box1, const float *box2, float *iou,
                                   float *jac, void *stream) {
  const char *W = "iou3d_forward";
  NESIE_REQUIRE(n >= 0, W);
  if (n == 0) return NESIE_OK;
  NESIE_REQUIRE(box1 && box2 && iou, W);
  if (jac)
    hipLaunchKernelGGL((iou3d_kernel<1, true>), dim3(cdiv((long long)n * 8, 64)), dim3(64), 0,
                       (hipStream_t)stream, n, box1, box2, iou, jac);
  else
    hipLaunchKernelGGL((iou3d_kernel<0, false>), dim3(cdiv(n, 64)), dim3(64), 0,
                       (hipStream_t)stream, n, box1, box2, iou, jac);
  return check_launch(W);
}

template <int ENCLOSING>
static void launch_giou3d(int n, const float *box1, const float *box2, int kind, float *loss,
                          float *iou, float *jac, hipStream_t stream) {
  if (jac)
    hipLaunchKernelGGL((giou3d_kernel<1, true, ENCLOSING>), dim3(cdiv((long long)n * 8, 64)),
                       dim3(64), 0, stream, n, box1, box2, kind, loss, iou, jac);
  else
    hipLaunchKernelGGL((giou3d_kernel<0, false, ENCLOSING>), dim3(cdiv(n, 64)), dim3(64), 0,
                       stream, n, box1, box2, kind, loss, iou, jac);
}

extern "C" int nesie_giou3d_forward(int n, const float *box1, const float *box2, int kind,
                                    int enclosing, float *loss, float *iou, float *jac,
                                    void *stream) {
  const char *W = "giou3d_forward";
  NESIE_REQUIRE(n >= 0 && (kind == 0 || kind == 1) && (enclosing == 0 || enclosing == 1), W);
  if (n == 0) return NESIE_OK;
  NESIE_REQUIRE(box1 && box2 && loss, W);
  if (enclosing == 0) launch_giou3d<0>(n, box1, box2, kind, loss, iou, jac, (hipStream_t)stream);
  else launch_giou3d<1>(n, box1, box2, kind, loss, iou, jac, (hipStream_t)stream);
  return check_launch(W);
}
