// The arithmetic of one axis-aligned box pair (aa_iou3d.hip): value and Jacobians, in the reference's
// order of operations (iou3d_calculator.py:272-320) and with torch autograd's subgradients.  Host and
// device: a CPU build can check it against the recorded reference results.
#pragma once
#include <hip/hip_runtime.h>

namespace nesie {

#define AA_HD __host__ __device__ __forceinline__

// torch.max / torch.min of two tensors propagate a NaN of either side
AA_HD float tmax(float x, float y) { return (x > y || x != x) ? x : y; }
AA_HD float tmin(float x, float y) { return (x < y || x != x) ? x : y; }
AA_HD float clamp0(float x) { return x < 0.f ? 0.f : x; }
// the share of the gradient of max(x, y) that goes to x (of min(y, x) that goes to y, mirrored)
AA_HD float hi_share(float x, float y) { return x > y ? 1.f : (x == y ? 0.5f : 0.f); }
AA_HD float lo_share(float x, float y) { return hi_share(y, x); }

// The value of one pair and, where asked for, d value / d a (j1) and d value / d b (j2).
template <bool J1, bool J2>
AA_HD float aa_pair(const float (&a)[6], const float (&b)[6], int mode, float eps, float (&j1)[6],
                    float (&j2)[6]) {
  float da[3], db[3], raw[3], wh[3], eraw[3] = {0.f, 0.f, 0.f}, ew[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    da[k] = a[3 + k] - a[k];
    db[k] = b[3 + k] - b[k];
    raw[k] = tmin(a[3 + k], b[3 + k]) - tmax(a[k], b[k]);
    wh[k] = clamp0(raw[k]);
  }
  const float area1 = da[0] * da[1] * da[2];
  const float area2 = db[0] * db[1] * db[2];
  const float overlap = wh[0] * wh[1] * wh[2];
  const float union0 = area1 + area2 - overlap;
  const float uni = tmax(union0, eps);
  const float iou = overlap / uni;
  float value = iou, enc0 = 0.f, enc = 1.f, gap = 0.f;
  if (mode == 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      eraw[k] = tmax(a[3 + k], b[3 + k]) - tmin(a[k], b[k]);
      ew[k] = clamp0(eraw[k]);
    }
    enc0 = ew[0] * ew[1] * ew[2];
    enc = tmax(enc0, eps);
    gap = (enc - uni) / enc;
    value = iou - gap;
  }
  if (!J1 && !J2) return value;

  // backwards through the same graph
  float g_overlap = 1.f / uni;
  float g_union = -(iou / uni);
  float g_enc0 = 0.f;
  if (mode == 1) {
    const float g_num = -1.f / enc;        // d value / d (enc - uni)
    g_union -= g_num;
    g_enc0 = (gap / enc + g_num) * hi_share(enc0, eps);
  }
  const float g_union0 = g_union * hi_share(union0, eps);
  g_overlap -= g_union0;                   // union0 = area1 + area2 - overlap
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int p = (k + 1) % 3, q = (k + 2) % 3;
    const float g_wh = raw[k] >= 0.f ? g_overlap * (wh[p] * wh[q]) : 0.f;
    float g_ew = 0.f;
    if (mode == 1) g_ew = eraw[k] >= 0.f ? g_enc0 * (ew[p] * ew[q]) : 0.f;
    if (J1) {
      const float g_d = g_union0 * (da[p] * da[q]);
      float hi = g_wh * lo_share(a[3 + k], b[3 + k]) + g_d;    // rb = min(a.hi, b.hi)
      float lo = -(g_wh * hi_share(a[k], b[k])) - g_d;         // lt = max(a.lo, b.lo)
      if (mode == 1) {
        hi += g_ew * hi_share(a[3 + k], b[3 + k]);
        lo -= g_ew * lo_share(a[k], b[k]);
      }
      j1[3 + k] = hi;
      j1[k] = lo;
    }
    if (J2) {
      const float g_d = g_union0 * (db[p] * db[q]);
      float hi = g_wh * lo_share(b[3 + k], a[3 + k]) + g_d;
      float lo = -(g_wh * hi_share(b[k], a[k])) - g_d;
      if (mode == 1) {
        hi += g_ew * hi_share(b[3 + k], a[3 + k]);
        lo -= g_ew * lo_share(b[k], a[k]);
      }
      j2[3 + k] = hi;
      j2[k] = lo;
    }
  }
  return value;
}

#undef AA_HD

}  // namespace nesie
