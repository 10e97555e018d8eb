// What the kernel families on v_mfma_f32_32x32x16_bf16 share: modconv_bf16.hip (modconv_mfma_bf16, modconv_mfma_bf16x3
// and the two weight-prep kernels) and conv3x3_x3.hip (conv3x3_mfma_bf16x3).
//
// The prepared weight image all three read.  From the fp32 MFMA layout wt[k][tap][m] = scale * W
// (fmgan_modconv_weight_prep_f32, any kind: k = the conv's input channel, m = its output channel):
//     wtb[chunk = k/16][piece][tap][k-half = (k%16)/8][m (padded to a multiple of 32)][j = k%8]      bf16, zero padded
// with one piece (bf16: bf16(wt), one rounding of the already scaled weight) or three (split operands: hi, mid, lo with
// hi + mid + lo = wt exactly).  A (chunk, piece, tap, k-half) row of 32 channels is 32 consecutive 16-byte slots: lane
// l (r = l & 31, h = l >> 5) of an MFMA reads slot r of k-half h as its A operand.
#pragma once
#include "common.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));       // 8 bf16 = one MFMA operand (4 VGPRs)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {   // RNE; lo -> bits [15:0], hi -> [31:16]
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ float bf16_to_f32(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
constexpr float BF16_MAX = 3.3895313892515355e38f;      // 0x7f7f: the largest finite bf16

// LDS-DMA (`buffer_load_dwordx4 ... lds`): 64 lanes x 16 bytes land at lds + lane * 16 (wave-uniform base) from
// rsrc base + voff (per lane, range-checked) + soff (wave-uniform); no VGPR destination.  (Device-pass guard: the host
// pass of hipcc drops the host stub of a template kernel whose body names this builtin directly — see modconv_fwd.hip.)
template <typename RSRC>
__device__ __forceinline__ void dma16_to_lds(RSRC rsrc, void* lds, unsigned voff, unsigned soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(3))) void* lds_void_ptr;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_ptr)lds, 16, voff, soff, 0, 0);
#endif
}

// The six products of a split-operand contraction, smallest first: (a piece, b piece), 0 = hi, 1 = mid, 2 = lo.
//     a * b = ah*bh + ah*bm + am*bh + am*bm + ah*bl + al*bh   + O(2^-24 |a b|)
constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};

// Host: more than 48 KB of dynamic LDS needs the opt-in once per kernel (idempotent); `done` is the caller's flag, a
// static of the launch's instantiation.
template <typename P>
void opt_in_dynamic_lds(void (*kernel)(const P), size_t lds, bool& done) {
  if (lds > 48 * 1024 && !done) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    done = true;
  }
}

}  // namespace
