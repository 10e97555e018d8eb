// The arithmetic and the accesses that produce an input of the LPIPS trunk from an image (lpips ScalingLayer after a
// bilinear reduction by f = 1 / 2 / 4 at align_corners=False), shared by the input stage of the perceptual path length
// (ppl_input.hip) and the image stage of the projection criterion (projection_loss.hip): one definition of each
// association, so the two stages give the trunk the same bits by construction.  The library is built with
// -ffp-contract=on and the pragma is scoped to a function: every helper that multiplies and adds carries its own.
#pragma once
#include "common.h"

constexpr int LPIPS_IN_PIX = 4;      // adjacent output pixels a lane owns: 12 floats of NHWC storage

// first tap row (and column) inside an f x f cell: source index f*d + f/2 - 0.5, both weights 1/2
constexpr int lpips_in_first_tap(int f) { return f / 2 - (f > 1 ? 1 : 0); }

__device__ __forceinline__ float lpips_in_half(float a, float b) {
#pragma clang fp contract(off)
  return 0.5f * a + 0.5f * b;
}

// 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d): columns inside a row first
__device__ __forceinline__ float lpips_in_quad(float a, float b, float c, float d) {
  return lpips_in_half(lpips_in_half(a, b), lpips_in_half(c, d));
}

// IEEE subtraction, correctly rounded division
__device__ __forceinline__ float lpips_in_scaled(float v, float shift, float scale) {
  const float u = v - shift;
  return u / scale;
}

// W contiguous floats as 16-byte pieces; dword alignment suffices
template <int W>
__device__ __forceinline__ void lpips_in_load(const float* __restrict__ p, float (&v)[W]) {
  static_assert(W % 4 == 0, "16-byte pieces");
#pragma unroll
  for (int q = 0; q < W / 4; ++q) {
    const f32x4_u a = *reinterpret_cast<const f32x4_u*>(p + 4 * q);
    v[4 * q] = a.x, v[4 * q + 1] = a.y, v[4 * q + 2] = a.z, v[4 * q + 3] = a.w;
  }
}

// One 16-byte piece (dword alignment) of a lane's 12 floats o[3*j + c] (channel c of pixel j: 48 contiguous bytes of
// NHWC storage); the caller's loop over the three pieces is unrolled in the kernel.
__device__ __forceinline__ void lpips_in_store4(float* dst, const float* o) {
  const f32x4_u s = {o[0], o[1], o[2], o[3]};
  *reinterpret_cast<f32x4_u*>(dst) = s;
}
