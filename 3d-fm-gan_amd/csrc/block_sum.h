// Fixed-order sums over a wave and over a block: one definition of the association, so the kernels that leave per-block
// partials (the metric, LPIPS-distance and projection stages) add in the same order by construction.  No atomics: the
// result is bit-reproducible run to run.  `acc` is maybe_undef as __shfl_xor's own argument is: the value is frozen at
// the kernel's call, where a hand-written butterfly would freeze it.
#pragma once
#include "common.h"

// xor butterfly over the 64 lanes, distances 32 .. 1: every lane ends with the same bits.
__device__ __forceinline__ float wave_sum_xor(__attribute__((maybe_undef)) float acc) {
#pragma unroll
  for (int m = FMGAN_WAVE / 2; m > 0; m >>= 1) acc += __shfl_xor(acc, m, FMGAN_WAVE);
  return acc;
}

// Sum of `acc` over a block of WAVES waves: the butterfly, lane 0 of each wave into red[WAVES] (shared memory), a
// barrier, then the waves in order.  Called by every thread of the block; thread 0 uses the value.  There is no barrier
// after the read of `red`: a caller that writes `red` again places its own.  fba_bwd_bias_f32 and face_region_f32 sum
// inside a loop over planes / samples and keep this sequence spelled out: inlined there, the helper changes the order
// in which the loop's invariants are hoisted, and with it the kernels' instruction schedule.
template <int WAVES>
__device__ __forceinline__ float block_sum_ordered(__attribute__((maybe_undef)) float acc, float* red) {
  static_assert(WAVES == 2 || WAVES == 4, "two or four waves");
  acc = wave_sum_xor(acc);
  if ((threadIdx.x & (FMGAN_WAVE - 1)) == 0) red[threadIdx.x / FMGAN_WAVE] = acc;
  __syncthreads();
  if constexpr (WAVES == 2) return red[0] + red[1];
  else return (red[0] + red[1]) + (red[2] + red[3]);
}
