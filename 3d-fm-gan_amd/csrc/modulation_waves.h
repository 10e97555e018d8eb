// Per-wave bodies of the modulation arithmetic, shared by the per-layer kernels (linear.hip, modconv_prep.hip) and the
// whole-network style bank (style_bank.hip): one definition of each summation chain, so the bank's bits equal the
// per-layer launches' by construction.  Every function is called by all 64 lanes of a wave with wave-uniform arguments.
#pragma once
#include "block_sum.h"

// sum_k wn[k] * x[k] (COMOD: x[k] = xb[k] * pb[k], rounded to fp32 first, i.e. the elementwise product a caller would
// have materialised): lane-strided fma chain, then the butterfly.  The bias is the caller's.
template <bool COMOD>
__device__ __forceinline__ float equal_linear_wave(const float* __restrict__ wn, const float* __restrict__ xb,
                                                   const float* __restrict__ pb, int k_in, int lane) {
  float acc = 0.f;
  for (int k = lane; k < k_in; k += 64) {
    float x = xb[k];
    if constexpr (COMOD) x = __fmul_rn(x, pb[k]);
    acc = fmaf(wn[k], x, acc);
  }
  return wave_sum_xor(acc);
}

// sum_k wn[k] * x[k] over the concatenation x = [va (k_a floats) | vb (k_b floats)], never materialised: the SAME
// lane-strided fma chain over the concatenated index (lane l takes k = l, l + 64, ..., crossing from va into vb wherever
// k_a falls) and the same butterfly, so the bits equal equal_linear_wave<false> on the concatenated row.  Scalar loads
// only: k_a is arbitrary, so vb's elements have no alignment relative to the lane stride.  The bias is the caller's.
__device__ __forceinline__ float equal_linear_concat_wave(const float* __restrict__ wn, const float* __restrict__ va,
                                                          const float* __restrict__ vb, int k_a, int k_b, int lane) {
  float acc = 0.f;
  const int k_in = k_a + k_b;
  for (int k = lane; k < k_in; k += 64) {
    const float x = k < k_a ? va[k] : vb[k - k_a];
    acc = fmaf(wn[k], x, acc);
  }
  return wave_sum_xor(acc);
}

// Demodulation of one output channel.  PRE: wo is the channel's row of per-(o,i) squared-tap sums [cin]; otherwise its
// raw taps [cin][ktaps].  Up to DEMOD_MAXJ * 64 input channels are held in registers across the samples of a wave.
constexpr int DEMOD_MAXJ = 8;

__device__ __forceinline__ bool demod_cached(int cin) { return cin <= 64 * DEMOD_MAXJ; }

template <bool PRE>
__device__ __forceinline__ float demod_tap_sq(const float* __restrict__ wo, int i, int ktaps) {
  float q = 0.f;
  if constexpr (PRE) q = wo[i];
  else
    for (int t = 0; t < ktaps; ++t) { const float w = wo[i * ktaps + t]; q = fmaf(w, w, q); }
  return q;
}

template <bool PRE>
__device__ __forceinline__ void demod_load_wsq(const float* __restrict__ wo, int cin, int ktaps, int lane,
                                               float (&wsq)[DEMOD_MAXJ]) {
#pragma unroll
  for (int j = 0; j < DEMOD_MAXJ; ++j) {
    const int i = lane + 64 * j;
    wsq[j] = i < cin ? demod_tap_sq<PRE>(wo, i, ktaps) : 0.f;
  }
}

// 1 / sqrt(scale^2 * sum_i wsq[o,i] * style[i]^2 + eps); `wsq` is read when demod_cached(cin), `wo` otherwise.
template <bool PRE>
__device__ __forceinline__ float demod_wave(const float* __restrict__ wo, const float (&wsq)[DEMOD_MAXJ],
                                            const float* __restrict__ sb, int cin, int ktaps, float scale, float eps,
                                            int lane) {
  float acc = 0.f;
  if (demod_cached(cin)) {
#pragma unroll
    for (int j = 0; j < DEMOD_MAXJ; ++j) {
      const int i = lane + 64 * j;
      if (i < cin) { const float m = sb[i]; acc = fmaf(wsq[j], m * m, acc); }
    }
  } else {
    for (int i = lane; i < cin; i += 64) {
      const float q = demod_tap_sq<PRE>(wo, i, ktaps);
      const float m = sb[i];
      acc = fmaf(q, m * m, acc);
    }
  }
  acc = wave_sum_xor(acc);
  return 1.0f / sqrtf(scale * scale * acc + eps);
}
