// The canonical point-in-box test of the roiaware_pool3d family, shared by points_in_boxes.hip
// and roiaware_pool3d.hip (reference mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49,
// roiaware_pool3d_kernel.cu:14-44).  A LiDAR-frame box (cx, cy, z_bottom, w, l, h, rz) is
// expanded ONCE into (cx, cy, cz_mid, l/2, w/2, h/2, cos, sin): cos / sin of (float)(rz + pi/2)
// are evaluated in double and rounded to float, the form shared with oracle/nesie_oracle.c and
// tests/_np_ref.points_in_boxes (the reference's device cosf / sinf lie within their own 2-ulp
// error of it).  The mixed float / double comparisons of the reference are kept: z window and half
// extents in double, x / y strict, z inclusive; products and sums fp32 without contraction.
#pragma once
#include "common.h"
#include <math.h>

namespace nesie {

struct PibBox {
  float cx, cy, czm;       // centre, z already shifted to mid height
  double hl, hw, hh;       // half length, half width, half height
  float cosa, sina;
};

// (cx, cy, z_bottom) and the sizes along the box's own x (l), y (w) and z (h)
__device__ __forceinline__ PibBox pib_expand(float cx, float cy, float cz, float w, float l,
                                             float h, float rz) {
  PibBox q;
  q.cx = cx; q.cy = cy;
  q.czm = (float)((double)cz + (double)h / 2.0);  // cz += h / 2.0
  q.hl = (double)l / 2.0; q.hw = (double)w / 2.0; q.hh = (double)h / 2.0;
  const float rot_angle = (float)((double)rz + M_PI / 2);
  q.cosa = (float)cos((double)rot_angle);
  q.sina = (float)sin((double)rot_angle);
  return q;
}

// a LiDAR-frame row (x, y, z_bottom, w, l, h, rz)
__device__ __forceinline__ PibBox pib_expand(const float *bx) {
  return pib_expand(bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], bx[6]);
}

// the test; lx, ly receive the point in the box's own frame when the z window holds it
__device__ __forceinline__ bool pib_inside(const PibBox &q, float x, float y, float z, float &lx,
                                           float &ly) {
  if ((double)fabsf(__fsub_rn(z, q.czm)) > q.hh) return false;
  const float sx = __fsub_rn(x, q.cx), sy = __fsub_rn(y, q.cy);
  lx = __fadd_rn(__fmul_rn(sx, q.cosa), __fmul_rn(sy, -q.sina));
  ly = __fadd_rn(__fmul_rn(sx, q.sina), __fmul_rn(sy, q.cosa));
  return ((double)lx > -q.hl) & ((double)lx < q.hl) & ((double)ly > -q.hw) & ((double)ly < q.hw);
}

__device__ __forceinline__ bool pib_inside(const PibBox &q, float x, float y, float z) {
  float lx, ly;
  return pib_inside(q, x, y, z, lx, ly);
}

}  // namespace nesie
