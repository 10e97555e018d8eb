// Face-regional loss of the dual-supervision G step (reference Util/training_util.py:228-256) for gfx950.
//
//   m[b,p] = (sum_c r[b,c,p]) * factor > -1          (Get_Render_Mask: torch.mean(render, dim=1) > -1)
//   loss   = mean((r*m - g*m)^2) = sum_b S[b] / (B*C*H*W),   S[b] = sum_{c,p} m * (r - g)^2
//   dL/dg  = grad_loss * 2/(B*C*H*W) * m * (g - r)            (0 exactly where m = 0; renders get no gradient)
//
// The reference spends ~10 elementwise passes over three image-sized tensors plus a device -> host -> device copy of the
// mask (`mask.type(torch.FloatTensor)`).  Here the forward reads r and g once (16 B per lane per load), the backward
// reads r, g and writes dg once; the mask is recomputed from r in registers instead of being stored.
//
// Mask decision = ATen's.  r.mean(1) on the GPU sums the C values of a pixel in fp32 in channel order (its reduction
// keeps 4 interleaved accumulators per output, so for C <= 4 each holds one value and the combine is the serial sum
// ((0 + r0) + r1) + r2 ...), then multiplies by the float factor num_outputs / numel (= 1/C).  The same operations are
// done here, so the mask is bit-identical for C <= 4; for larger C the serial sum may differ from ATen's by rounding.
//
// Mapping: lane = a group of 4 consecutive pixels of one sample (a float4 per channel plane), grid.y = samples,
// grid.x = blocks per sample (fmgan_face_region_blocks).  The scalar form (misaligned pointers or H*W % 4 != 0) walks
// the same groups with 4 bounded scalar loads, so it performs the same arithmetic in the same order: both forms give
// bit-identical partials.  Forward partial sums: per-lane serial (explicit fma), wave butterfly, 4 waves in order
// (the association of block_sum_ordered in block_sum.h, spelled out in the sample loop) -> partial[b, blockIdx.x]; no
// atomics, bit-reproducible run to run.
#include <climits>

#include "common.h"

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_MAX_BLOCKS_X = 1024;

enum { FR_LOSS = 0, FR_GRAD = 1, FR_MASK = 2 };
static_assert(FR_THREADS == 4 * FMGAN_WAVE, "the block sum below adds four waves");

__device__ __forceinline__ float fr_sq(bool m, float r, float g, float acc) {
  const float d = m ? r - g : 0.f;
  return __builtin_fmaf(d, d, acc);
}

__device__ __forceinline__ float fr_grad(bool m, float r, float g, float cf) { return m ? cf * (g - r) : 0.f; }

// CT > 0: channel count known at compile time (C = 3: the render's planes stay in registers between the mask and the
// loss); CT = 0: any C, the render is read a second time (from cache) after the mask.
template <int CT, bool VEC, int MODE>
__global__ __launch_bounds__(FR_THREADS) void face_region_f32(const float* __restrict__ r, const float* __restrict__ g,
                                                              float* __restrict__ out,
                                                              const float* __restrict__ grad_loss, int batch,
                                                              int channels, long long hw, int groups, float factor,
                                                              float coef) {
  __shared__ float red[FR_THREADS / FMGAN_WAVE];
  const int C = CT > 0 ? CT : channels;
  const long long chw = (long long)C * hw;
  float cf = 0.f;
  if constexpr (MODE == FR_GRAD) cf = grad_loss[0] * coef;
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const float* rb = r + (long long)b * chw;
    const float* gb = g + (long long)b * chw;
    float acc = 0.f;
    for (int i = blockIdx.x * FR_THREADS + threadIdx.x; i < groups; i += gridDim.x * FR_THREADS) {
      const long long p = 4LL * i;
      f32x4 rv[CT > 0 ? CT : 1];
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C; ++c) {
        const f32x4 v = load4<VEC>(rb + c * hw, p, hw);
        if constexpr (CT > 0) rv[c] = v;
        s.x = s.x + v.x; s.y = s.y + v.y; s.z = s.z + v.z; s.w = s.w + v.w;
      }
      // pixels past the end of the plane (scalar form's last group) are never in the mask
      const bool mx = p < hw && s.x * factor > -1.f;
      const bool my = p + 1 < hw && s.y * factor > -1.f;
      const bool mz = p + 2 < hw && s.z * factor > -1.f;
      const bool mw = p + 3 < hw && s.w * factor > -1.f;
      if constexpr (MODE == FR_MASK) {
        const f32x4 mv = {mx ? 1.f : 0.f, my ? 1.f : 0.f, mz ? 1.f : 0.f, mw ? 1.f : 0.f};
        store4<VEC>(out + (long long)b * hw, p, hw, mv);
      } else {
        for (int c = 0; c < C; ++c) {
          f32x4 a;
          if constexpr (CT > 0) a = rv[c];
          else a = load4<VEC>(rb + c * hw, p, hw);
          const f32x4 v = load4<VEC>(gb + c * hw, p, hw);
          if constexpr (MODE == FR_LOSS) {
            acc = fr_sq(mx, a.x, v.x, acc);
            acc = fr_sq(my, a.y, v.y, acc);
            acc = fr_sq(mz, a.z, v.z, acc);
            acc = fr_sq(mw, a.w, v.w, acc);
          } else {
            const f32x4 d = {fr_grad(mx, a.x, v.x, cf), fr_grad(my, a.y, v.y, cf), fr_grad(mz, a.z, v.z, cf),
                             fr_grad(mw, a.w, v.w, cf)};
            store4<VEC>(out + (long long)b * chw + c * hw, p, hw, d);
          }
        }
      }
    }
    if constexpr (MODE == FR_LOSS) {
      for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, FMGAN_WAVE);
      if ((threadIdx.x & (FMGAN_WAVE - 1)) == 0) red[threadIdx.x / FMGAN_WAVE] = acc;
      __syncthreads();
      if (threadIdx.x == 0) out[(long long)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
      __syncthreads();
    }
  }
}

// Grid, group count, mask factor and load form of one call; FMGAN_OK or an FMGAN_E* status.
struct FrShape {
  int gx, gy, groups;
  float factor, coef;
  bool vec;
};

int fr_shape(int batch, int channels, long long hw, uintptr_t addr_or, FrShape* sh) {
  if (batch <= 0 || channels <= 0 || hw <= 0) return FMGAN_EINVAL;
  // element offsets are long long; the group index is an int that must not wrap when the grid stride is added
  if ((long long)channels > LLONG_MAX / hw || (long long)channels * hw > LLONG_MAX / batch) return FMGAN_EOVERFLOW;
  if ((hw + 3) / 4 > 0x7fffffffLL - (long long)FR_MAX_BLOCKS_X * FR_THREADS) return FMGAN_EOVERFLOW;
  sh->groups = (int)((hw + 3) / 4);
  sh->gx = fmgan_face_region_blocks(batch, hw);
  long long gy = batch;
  const long long cap = (long long)FMGAN_NUM_CU * 32 / sh->gx;
  if (gy > cap) gy = cap > 0 ? cap : 1;
  if (gy > 65535) gy = 65535;
  sh->gy = (int)gy;
  // ATen's mean factor: static_cast<float>(num_output_elements) / numel  (= 1/C up to its rounding)
  const long long outputs = (long long)batch * hw;
  sh->factor = (float)outputs / (float)(outputs * channels);
  sh->coef = (float)(2.0 / ((double)outputs * (double)channels));      // d mean(x^2) / dx = 2x / numel
  sh->vec = (hw & 3) == 0 && (addr_or & 15) == 0;
  return FMGAN_OK;
}

template <int MODE>
int fr_launch(const float* r, const float* g, float* out, const float* grad_loss, int batch, int channels, long long hw,
              hipStream_t s) {
  if (!r || !out || (MODE != FR_MASK && !g) || (MODE == FR_GRAD && !grad_loss)) return FMGAN_EINVAL;
  // the loss writes one float per block: only r and g take part in the 16-byte load form
  const uintptr_t addr = (uintptr_t)r | (uintptr_t)g | (MODE == FR_LOSS ? 0 : (uintptr_t)out);
  FrShape sh;
  const int st = fr_shape(batch, channels, hw, addr, &sh);
  if (st != FMGAN_OK) return st;
  const dim3 grid(sh.gx, sh.gy), block(FR_THREADS);
#define FR_GO(CT, VEC)                                                                                        \
  hipLaunchKernelGGL((face_region_f32<CT, VEC, MODE>), grid, block, 0, s, r, g, out, grad_loss, batch, channels, \
                     hw, sh.groups, sh.factor, sh.coef)
  if (channels == 3) {
    if (sh.vec) FR_GO(3, true); else FR_GO(3, false);
  } else {
    if (sh.vec) FR_GO(0, true); else FR_GO(0, false);
  }
#undef FR_GO
  return fmgan_check_launch();
}

}  // namespace

extern "C" int fmgan_face_region_blocks(int batch, long long hw) {
  if (batch <= 0 || hw <= 0) return 0;
  const long long groups = (hw + 3) / 4;
  return fmgan_stage_blocks((groups + FR_THREADS - 1) / FR_THREADS, batch, FR_MAX_BLOCKS_X);
}

extern "C" int fmgan_face_region_loss_f32(const float* r, const float* g, float* partial, int batch, int channels,
                                          long long hw, void* stream) {
  return fr_launch<FR_LOSS>(r, g, partial, nullptr, batch, channels, hw, (hipStream_t)stream);
}

extern "C" int fmgan_face_region_backward_f32(const float* r, const float* g, const float* grad_loss, float* grad_g,
                                              int batch, int channels, long long hw, void* stream) {
  return fr_launch<FR_GRAD>(r, g, grad_g, grad_loss, batch, channels, hw, (hipStream_t)stream);
}

extern "C" int fmgan_render_mask_f32(const float* r, float* mask, int batch, int channels, long long hw, void* stream) {
  return fr_launch<FR_MASK>(r, nullptr, mask, nullptr, batch, channels, hw, (hipStream_t)stream);
}
