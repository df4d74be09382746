// Rotated BEV overlap area of two (x1, y1, x2, y2, angle) rectangles, shared by
// boxes_overlap_bev (postprocess.hip) and the BEV NMS (bev_nms.hip).
#pragma once
#include "common.h"
#include <math.h>

namespace nesie {

// Edge-edge crossings, corners of one inside the other (1e-5 slack), angular order about the
// mean point, fan area -- the construction of iou3d_kernel.cu:127-238 with its constants.  cos / sin / atan2
// are taken in double and rounded to float (the canonical form shared with the oracle; the
// reference's device cosf / sinf / atan2f lie within their own error of it).
struct P2 { float x, y; };

__device__ __forceinline__ float cross3(const P2 &p1, const P2 &p2, const P2 &p0) {
  return __fsub_rn(__fmul_rn(__fsub_rn(p1.x, p0.x), __fsub_rn(p2.y, p0.y)),
                   __fmul_rn(__fsub_rn(p2.x, p0.x), __fsub_rn(p1.y, p0.y)));
}

__device__ __forceinline__ bool spans_touch(const P2 &p1, const P2 &p2, const P2 &q1,
                                            const P2 &q2) {
  return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
         fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

// crossing of segment p0-p1 with q0-q1 (iou3d_kernel.cu:80-111)
__device__ __forceinline__ bool edge_crossing(const P2 &p1, const P2 &p0, const P2 &q1,
                                              const P2 &q0, P2 &ans) {
  if (!spans_touch(p0, p1, q0, q1)) return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0);
  const float s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(__fmul_rn(s1, s2) > 0.f && __fmul_rn(s3, s4) > 0.f)) return false;
  const float s5 = cross3(q1, p1, p0);
  const float den = __fsub_rn(s5, s1);
  if (fabsf(den) > 1e-8f) {
    ans.x = __fdiv_rn(__fsub_rn(__fmul_rn(s5, q0.x), __fmul_rn(s1, q1.x)), den);
    ans.y = __fdiv_rn(__fsub_rn(__fmul_rn(s5, q0.y), __fmul_rn(s1, q1.y)), den);
  } else {
    const float a0 = __fsub_rn(p0.y, p1.y), b0 = __fsub_rn(p1.x, p0.x);
    const float c0 = __fsub_rn(__fmul_rn(p0.x, p1.y), __fmul_rn(p1.x, p0.y));
    const float a1 = __fsub_rn(q0.y, q1.y), b1 = __fsub_rn(q1.x, q0.x);
    const float c1 = __fsub_rn(__fmul_rn(q0.x, q1.y), __fmul_rn(q1.x, q0.y));
    const float D = __fsub_rn(__fmul_rn(a0, b1), __fmul_rn(a1, b0));
    ans.x = __fdiv_rn(__fsub_rn(__fmul_rn(b0, c1), __fmul_rn(b1, c0)), D);
    ans.y = __fdiv_rn(__fsub_rn(__fmul_rn(a1, c0), __fmul_rn(a0, c1)), D);
  }
  return true;
}

struct Rect {
  float x1, y1, x2, y2, cx, cy, cosa, sina;
  P2 c[5];
};

__device__ __forceinline__ P2 spin(float px, float py, float cx, float cy, float c, float s) {
  const float dx = __fsub_rn(px, cx), dy = __fsub_rn(py, cy);
  P2 r;
  r.x = __fadd_rn(__fadd_rn(__fmul_rn(dx, c), __fmul_rn(dy, s)), cx);
  r.y = __fadd_rn(__fadd_rn(__fmul_rn(-dx, s), __fmul_rn(dy, c)), cy);
  return r;
}

__device__ __forceinline__ void load_rect(const float *b, Rect &r) {
  r.x1 = b[0]; r.y1 = b[1]; r.x2 = b[2]; r.y2 = b[3];
  r.cx = __fdiv_rn(__fadd_rn(r.x1, r.x2), 2.f);
  r.cy = __fdiv_rn(__fadd_rn(r.y1, r.y2), 2.f);
  r.cosa = (float)cos((double)b[4]);
  r.sina = (float)sin((double)b[4]);
  r.c[0] = spin(r.x1, r.y1, r.cx, r.cy, r.cosa, r.sina);
  r.c[1] = spin(r.x2, r.y1, r.cx, r.cy, r.cosa, r.sina);
  r.c[2] = spin(r.x2, r.y2, r.cx, r.cy, r.cosa, r.sina);
  r.c[3] = spin(r.x1, r.y2, r.cx, r.cy, r.cosa, r.sina);
  r.c[4] = r.c[0];
}

// p inside the rotated rectangle r: turned back by cos(-angle), sin(-angle) (:54-78)
__device__ __forceinline__ bool inside_rect(const Rect &r, const P2 &p) {
  const float M = 1e-5f;
  const P2 q = spin(p.x, p.y, r.cx, r.cy, r.cosa, -r.sina);
  return q.x > __fsub_rn(r.x1, M) && q.x < __fadd_rn(r.x2, M) && q.y > __fsub_rn(r.y1, M) &&
         q.y < __fadd_rn(r.y2, M);
}

// overlap area of A and B: box_overlap of iou3d_kernel.cu:127-238, |fan area| / 2 taken in
// double and rounded to float as there
__device__ __forceinline__ float bev_overlap(const Rect &A, const Rect &B) {
  P2 pts[16];
  float ang[16];
  int cnt = 0;
  float sx = 0.f, sy = 0.f;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 hit;
      if (edge_crossing(A.c[i + 1], A.c[i], B.c[j + 1], B.c[j], hit)) {
        sx = __fadd_rn(sx, hit.x); sy = __fadd_rn(sy, hit.y);
        pts[cnt++] = hit;
      }
    }
  for (int k = 0; k < 4; ++k) {
    if (inside_rect(A, B.c[k])) {
      sx = __fadd_rn(sx, B.c[k].x); sy = __fadd_rn(sy, B.c[k].y);
      pts[cnt++] = B.c[k];
    }
    if (inside_rect(B, A.c[k])) {
      sx = __fadd_rn(sx, A.c[k].x); sy = __fadd_rn(sy, A.c[k].y);
      pts[cnt++] = A.c[k];
    }
  }
  float area = 0.f;
  if (cnt > 0) {
    const float mx = __fdiv_rn(sx, (float)cnt), my = __fdiv_rn(sy, (float)cnt);
    for (int i = 0; i < cnt; ++i)
      ang[i] = (float)atan2((double)__fsub_rn(pts[i].y, my), (double)__fsub_rn(pts[i].x, mx));
    // stable ascending order by angle (the reference's adjacent-swap passes)
    for (int i = 1; i < cnt; ++i) {
      const P2 v = pts[i];
      const float av = ang[i];
      int j = i - 1;
      while (j >= 0 && ang[j] > av) { pts[j + 1] = pts[j]; ang[j + 1] = ang[j]; --j; }
      pts[j + 1] = v; ang[j + 1] = av;
    }
    for (int k = 0; k + 1 < cnt; ++k) {
      const float ax = __fsub_rn(pts[k].x, pts[0].x), ay = __fsub_rn(pts[k].y, pts[0].y);
      const float bx = __fsub_rn(pts[k + 1].x, pts[0].x), by = __fsub_rn(pts[k + 1].y, pts[0].y);
      area = __fadd_rn(area, __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx)));
    }
  }
  return (float)((double)fabsf(area) / 2.0);
}

}  // namespace nesie
