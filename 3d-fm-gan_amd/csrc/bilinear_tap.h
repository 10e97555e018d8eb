// The two taps of one output index of F.interpolate(mode='bilinear', align_corners=False) by aten's fp32 rule, shared
// by the Inception input stage and the face crop: one definition, so a forward and the backward that inverts it can
// never disagree on a tap.
//   scale = (float)in / (float)out                                  one fp32 division, the caller's
//   src   = max(fmaf(scale, d + 0.5f, -0.5f), 0.f)                   ONE rounding: aten's kernels contract it
//   i0    = (int)src;  i1 = i0 + (i0 < s - 1);  l1 = src - i0;  l0 = 1.f - l1
#pragma once
#include "common.h"

struct BilinearTap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ BilinearTap bilinear_tap(float scale, int d, int s) {
  float src = __fmaf_rn(scale, (float)d + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  BilinearTap t;
  t.i0 = (int)src;
  t.i1 = t.i0 + (t.i0 < s - 1 ? 1 : 0);
  t.l1 = __fsub_rn(src, (float)t.i0);
  t.l0 = __fsub_rn(1.f, t.l1);
  return t;
}
