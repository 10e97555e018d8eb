// Training batches straight out of device-resident image banks:
//   out[s] = ((bank[k_s][i_s] / 255) - mean) / std     uint8 HWC -> float32 CHW, for n output images s in one launch
// with the arithmetic of u8hwc_to_f32chw (image_io.hip: __fdiv_rn, __fsub_rn, __fdiv_rn), so the bits are those of
// index_select + fmgan_images_to_tensor and of torch's ((x.float() / 255) - mean) / std.
//
// Which image feeds slot s is worked out on the device.  The output is n_groups groups of `members` images; group g is
// described by value (BgGroup: bank, index source, pair swap, mul, add), and member j of it reads
//   b = j * stride;  pos = offset + (b ^ swap);  i = index[source][pos] * mul + add;  image i of bank `bank`
// so a (g_input, r_input, g_ref) triple of a dual-supervision batch is three groups over the same positions, two of them
// swapped, and an extreme-pose batch the same at stride 2.  The index lists are the epoch's, uploaded once; nothing else
// comes from the host per batch.  A slot whose bank, position or image index is out of range is skipped before any read
// of the bank: its output keeps what it held.
//
// Vector kernel: a lane owns P consecutive pixels of one image, 3P bytes loaded as whole dwords (P = 4: 3 dwords, P = 16:
// 3 dwordx4), de-interleaved with byte extracts in registers, stored as P/4 float4 per channel plane; consecutive lanes
// own consecutive runs, so a wave covers one contiguous run of the source and of each plane.  It needs every bank base
// aligned to the load width (4 / 16 bytes), H*W % P == 0 (every image then starts on that alignment, every plane on 16
// bytes) and a 16-byte aligned output; otherwise the scalar kernel runs, one pixel per lane with a guard.  All byte and
// element offsets are 64-bit: a bank of 70 000 256^2 photos has 13.8e9 bytes.
#include <climits>
#include <cstdint>

#include "common.h"

namespace {

constexpr int BG_THREADS = 256;
constexpr int BG_MAX_BANKS = 4;
constexpr int BG_MAX_GROUPS = 8;
constexpr int BG_GROUP_INTS = 5;           // bank, source, swap, mul, add
constexpr int BG_DEFAULT_PIX = 4;          // profiles/dataset.md: P = 4 against P = 16

struct BgGroup {
  int bank, source, swap, mul, add;
};

struct BgArgs {
  const unsigned char* bank[BG_MAX_BANKS];
  int count[BG_MAX_BANKS];
  const int* index[2];
  long long len[2];
  long long offset;
  int members, stride, n_groups;
  BgGroup group[BG_MAX_GROUPS];
};

typedef unsigned int bg_u32 __attribute__((may_alias));
typedef unsigned int bg_u32x4 __attribute__((ext_vector_type(4), may_alias));
typedef float bg_f32x4 __attribute__((ext_vector_type(4), may_alias));

// The source image of output slot s, or nullptr for a slot to skip.  Uniform over a block.
__device__ __forceinline__ const unsigned char* bg_source(const BgArgs& a, int s, long long image_bytes) {
  const int g = s / a.members, j = s - g * a.members;
  if (g >= a.n_groups) return nullptr;
  const BgGroup d = a.group[g];
  if (d.bank < 0 || d.bank >= BG_MAX_BANKS || d.source < 0 || d.source > 1) return nullptr;
  const unsigned char* base = a.bank[d.bank];
  const int* index = a.index[d.source];
  if (!base || !index) return nullptr;
  const long long pos = a.offset + (((long long)j * a.stride) ^ (long long)(d.swap & 1));
  if (pos < 0 || pos >= a.len[d.source]) return nullptr;
  const long long i = (long long)index[pos] * d.mul + d.add;
  if (i < 0 || i >= (long long)a.count[d.bank]) return nullptr;
  return base + i * image_bytes;
}

__device__ __forceinline__ float bg_value(unsigned int byte, float mean, float stdv) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)byte, 255.0f), mean), stdv);
}

// byte `b` (compile-time) of the little-endian dword array w
#define BG_BYTE(w, b) (((w)[(b) >> 2] >> (8 * ((b) & 3))) & 255u)

template <int P>
__global__ __launch_bounds__(BG_THREADS) void bank_gather_vec_k(BgArgs a, float* __restrict__ out, int hw, int units,
                                                                int gx, float mean, float stdv) {
  static_assert(P == 4 || P == 16, "a lane owns 4 or 16 pixels");
  constexpr int ND = 3 * P / 4;                                   // dwords per lane
  const int s = blockIdx.x / gx;
  const int u = (blockIdx.x - s * gx) * BG_THREADS + threadIdx.x;
  if (u >= units) return;
  const unsigned char* src = bg_source(a, s, 3LL * hw);
  if (!src) return;
  src += (long long)u * (3 * P);
  unsigned int w[ND];
  if constexpr (P == 4) {
#pragma unroll
    for (int q = 0; q < ND; ++q) w[q] = reinterpret_cast<const bg_u32*>(src)[q];
  } else {
#pragma unroll
    for (int q = 0; q < ND / 4; ++q) {
      const bg_u32x4 v = reinterpret_cast<const bg_u32x4*>(src)[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
  float* dst = out + (long long)s * 3 * hw + (long long)u * P;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
      bg_f32x4 v;
      v.x = bg_value(BG_BYTE(w, 3 * (4 * q) + c), mean, stdv);
      v.y = bg_value(BG_BYTE(w, 3 * (4 * q + 1) + c), mean, stdv);
      v.z = bg_value(BG_BYTE(w, 3 * (4 * q + 2) + c), mean, stdv);
      v.w = bg_value(BG_BYTE(w, 3 * (4 * q + 3) + c), mean, stdv);
      reinterpret_cast<bg_f32x4*>(dst + (long long)c * hw)[q] = v;
    }
  }
}

// one pixel per lane, any size and alignment
__global__ __launch_bounds__(BG_THREADS) void bank_gather_scalar_k(BgArgs a, float* __restrict__ out, int hw, int gx,
                                                                   float mean, float stdv) {
  const int s = blockIdx.x / gx;
  const int p = (blockIdx.x - s * gx) * BG_THREADS + threadIdx.x;
  if (p >= hw) return;
  const unsigned char* src = bg_source(a, s, 3LL * hw);
  if (!src) return;
  src += 3LL * p;
  float* dst = out + (long long)s * 3 * hw + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[(long long)c * hw] = bg_value(src[c], mean, stdv);
}

#undef BG_BYTE

}  // namespace

extern "C" int fmgan_bank_gather(const void* bank0, const void* bank1, const void* bank2, const void* bank3, int count0,
                                 int count1, int count2, int count3, int h, int w, const void* index_a, long long len_a,
                                 const void* index_b, long long len_b, long long offset, int members, int stride,
                                 const int* groups, int n_groups, float* out, float mean, float stdv,
                                 int pixels_per_lane, void* stream) {
  if (h <= 0 || w <= 0 || members < 0 || n_groups < 1 || n_groups > BG_MAX_GROUPS || (stride != 1 && stride != 2) ||
      offset < 0 || len_a < 0 || len_b < 0 || count0 < 0 || count1 < 0 || count2 < 0 || count3 < 0 || stdv == 0.f ||
      !(pixels_per_lane == 0 || pixels_per_lane == 4 || pixels_per_lane == 16))
    return FMGAN_EINVAL;
  if (members == 0) return FMGAN_OK;
  if (!groups || !out || !index_a) return FMGAN_EINVAL;
  if (((uintptr_t)index_a & 3) || ((uintptr_t)index_b & 3) || ((uintptr_t)out & 3)) return FMGAN_EINVAL;
  // element and byte offsets are long long; pixel, unit, slot and block indices are ints
  const long long hw = (long long)h * w;
  if (hw > 0x7fffffffLL / 3 - BG_THREADS * 16) return FMGAN_EOVERFLOW;
  const long long n = (long long)members * n_groups;
  if (n > 0x7fffffffLL || 3 * hw > LLONG_MAX / n) return FMGAN_EOVERFLOW;
  if (offset > LLONG_MAX / 4 || (long long)members * stride > LLONG_MAX / 4) return FMGAN_EOVERFLOW;
  BgArgs a;
  const void* banks[BG_MAX_BANKS] = {bank0, bank1, bank2, bank3};
  const int counts[BG_MAX_BANKS] = {count0, count1, count2, count3};
  uintptr_t bases = 0;
  for (int k = 0; k < BG_MAX_BANKS; ++k) {
    a.bank[k] = counts[k] > 0 ? static_cast<const unsigned char*>(banks[k]) : nullptr;
    a.count[k] = a.bank[k] ? counts[k] : 0;
    bases |= (uintptr_t)a.bank[k];
  }
  a.index[0] = static_cast<const int*>(index_a);
  a.index[1] = static_cast<const int*>(index_b);
  a.len[0] = len_a;
  a.len[1] = index_b ? len_b : 0;
  a.offset = offset;
  a.members = members;
  a.stride = stride;
  a.n_groups = n_groups;
  for (int g = 0; g < BG_MAX_GROUPS; ++g) {
    BgGroup d = {-1, 0, 0, 0, 0};                      // an unused descriptor names no bank
    if (g < n_groups) {
      const int* e = groups + g * BG_GROUP_INTS;
      d = BgGroup{e[0], e[1], e[2], e[3], e[4]};
      if (d.swap != 0 && d.swap != 1) return FMGAN_EINVAL;
    }
    a.group[g] = d;
  }
  hipStream_t hs = (hipStream_t)stream;
  const int want = pixels_per_lane ? pixels_per_lane : BG_DEFAULT_PIX;
  // the widest unit the request, the size and the pointers allow: 16 -> 4 -> scalar
  int pix = 1;
  if (((uintptr_t)out & 15) == 0) {
    if (want == 16 && hw % 16 == 0 && (bases & 15) == 0) pix = 16;
    else if (hw % 4 == 0 && (bases & 3) == 0) pix = 4;
  }
  const int units = (int)(hw / pix);
  const long long gx = (units + BG_THREADS - 1) / BG_THREADS;
  if (gx * n > 0x7fffffffLL) return FMGAN_EOVERFLOW;              // grid.x
  const dim3 grid((unsigned)(gx * n)), block(BG_THREADS);
  if (pix == 16)
    hipLaunchKernelGGL(bank_gather_vec_k<16>, grid, block, 0, hs, a, out, (int)hw, units, (int)gx, mean, stdv);
  else if (pix == 4)
    hipLaunchKernelGGL(bank_gather_vec_k<4>, grid, block, 0, hs, a, out, (int)hw, units, (int)gx, mean, stdv);
  else
    hipLaunchKernelGGL(bank_gather_scalar_k, grid, block, 0, hs, a, out, (int)hw, (int)gx, mean, stdv);
  return fmgan_check_launch();
}
