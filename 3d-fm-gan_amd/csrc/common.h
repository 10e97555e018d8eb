// Shared helpers for the libfmgan_hip.so sources (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "fmgan_hip.h"

#define FMGAN_WAVE 64
#define FMGAN_NUM_XCD 8

// Compute units of the current device, asked once per device (MI355X: 256); feeds the grid caps and the split-K
// model.  Without a device (host-logic calls in the CPU test-suite) the MI355X value is assumed, so host-only entry
// points such as fmgan_modconv2d_workspace_bytes() answer the same on both boxes.
static inline int fmgan_num_cu() {
  static int cached[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) {
    (void)hipGetLastError();
    return 256;
  }
  int v = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    v = 256;
  }
  __atomic_store_n(&cached[dev], v, __ATOMIC_RELAXED);
  return v;
}
#define FMGAN_NUM_CU fmgan_num_cu()

static inline int fmgan_check_launch() {
  return hipGetLastError() == hipSuccess ? FMGAN_OK : FMGAN_ELAUNCH;
}

// Blocks are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Map the
// hardware block id to a logical id so each XCD walks one contiguous chunk of the
// logical grid: tiles that share halo rows / operand panels then share an L2.
// Bijective for any grid size (cdna_hip_programming.md §5 "XCD swizzle must be bijective").
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
  const unsigned q = nblk / FMGAN_NUM_XCD, r = nblk % FMGAN_NUM_XCD;
  const unsigned xcd = bid % FMGAN_NUM_XCD, slot = bid / FMGAN_NUM_XCD;
  const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

template <typename T> struct AccT { using type = float; };
template <> struct AccT<double> { using type = double; };

template <typename T> __device__ __forceinline__ typename AccT<T>::type to_acc(T v) {
  return static_cast<typename AccT<T>::type>(v);
}
template <> __device__ __forceinline__ float to_acc<__half>(__half v) { return __half2float(v); }

template <typename T> __device__ __forceinline__ T from_acc(typename AccT<T>::type v) {
  return static_cast<T>(v);
}
template <> __device__ __forceinline__ __half from_acc<__half>(float v) { return __float2half(v); }

// The activation of fused_bias_act, shared by fused_bias_act.hip and act16.hip so that the 16-bit kernels apply the
// very expression of the fp32 ones.  code = act*10 + grad  (op/fused_bias_act_kernel.cu:36-45)
template <typename A> __device__ __forceinline__ A act_apply(A x, A ref, int code, A alpha) {
  switch (code) {
    case 12: return A(0);
    case 30: return (x > A(0)) ? x : x * alpha;
    case 31: return (ref > A(0)) ? x : x * alpha;
    case 32: return A(0);
    default: return x;  // 10, 11 and anything else: linear
  }
}

// 4-byte-aligned vector types: global_load/store_dwordx{2,4} need only dword alignment
// on gfx950, and rows of 2H+1 floats are never 16-byte aligned.
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Four consecutive floats at p + i of a run of n.  VEC: one 16-byte access (the caller has checked alignment and
// n % 4 == 0); otherwise four bounded scalar accesses, 0 past the end: the same values in the same lanes.
template <bool VEC, typename I>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, I i, I n) {
  if constexpr (VEC) {
    return *reinterpret_cast<const f32x4*>(p + i);
  } else {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < n) v.x = p[i];
    if (i + 1 < n) v.y = p[i + 1];
    if (i + 2 < n) v.z = p[i + 2];
    if (i + 3 < n) v.w = p[i + 3];
    return v;
  }
}

template <bool VEC, typename I>
__device__ __forceinline__ void store4(float* __restrict__ p, I i, I n, f32x4 v) {
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(p + i) = v;
  } else {
    if (i < n) p[i] = v.x;
    if (i + 1 < n) p[i + 1] = v.y;
    if (i + 2 < n) p[i + 2] = v.z;
    if (i + 3 < n) p[i + 3] = v.w;
  }
}

// grid.x of a stage that walks `work` block-sized pieces per sample: no block without work, about 8 blocks per CU over
// the batch, at most `max_blocks`.
static inline int fmgan_stage_blocks(long long work, int batch, int max_blocks) {
  long long gx = work;
  const long long want = ((long long)FMGAN_NUM_CU * 8 + batch - 1) / batch;
  if (gx > want) gx = want;
  if (gx > max_blocks) gx = max_blocks;
  return (int)(gx < 1 ? 1 : gx);
}
