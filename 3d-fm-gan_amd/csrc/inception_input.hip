// Input stage of the FID's Inception network (reference Evaluation/inception.py:155-162) for gfx950: from the
// Generator's image batch to the channels_last input of the first convolution, in one pass.
//
//   img  [batch, 3, s, s] NCHW f32
//   v    = F.interpolate(img, size=(299, 299), mode='bilinear', align_corners=False), aten's fp32 rule:
//            scale = (float)s / 299.f                                   one fp32 division
//            src   = max(fmaf(scale, d + 0.5f, -0.5f), 0.f)              ONE rounding: aten's kernels contract it
//            i0    = (int)src;  i1 = i0 + (i0 < s - 1);  l1 = src - i0;  l0 = 1.f - l1
//            v     = h0*(w0*a + w1*b) + h1*(w0*c + w1*d)                 every product and sum rounded, no fma;
//                    a, b = img[n, ch, y0, x0 / x1], c, d = img[n, ch, y1, x0 / x1], (h0, h1) the row weights (l0, l1) of
//                    the output row, (w0, w1) those of the output column
//          s = 299: v = img (aten copies, nothing is multiplied)
//   out  = normalize ? 2*v - 1 : v                                       [batch, 299, 299, 3] dense (NHWC storage)
//
// Only tap pixels are read (a tap of weight 0 is still a tap, as in aten: its NaN reaches the output).  The ratio is not an
// integer (256: 0.856, 512: 1.712, 1024: 3.425), so the taps of adjacent outputs sit 0 .. 4 source pixels apart and nothing
// of lpips_input.h's fixed-offset vector loads applies: a lane owns one output pixel, loads its 4 taps of 3 channels as
// scalars (adjacent lanes: adjacent or near-adjacent addresses of one source row) and writes 12 contiguous bytes, a wave
// 768.  grid.x = samples * blocks per sample, one pixel per lane, no loop, no shared memory.
#include "bilinear_tap.h"

namespace {

constexpr int II_THREADS = 256;
constexpr int II_OUT = 299;

template <bool COPY>
__global__ __launch_bounds__(II_THREADS) void inception_input_f32(const float* __restrict__ img, float* __restrict__ out,
                                                                  int s, float scale, int normalize, int gx) {
  const int n = blockIdx.x / gx, blk = blockIdx.x % gx;
  const int u = blk * II_THREADS + threadIdx.x;
  if (u >= II_OUT * II_OUT) return;
  const int oy = u / II_OUT, ox = u % II_OUT;
  const long long hw = (long long)s * s;
  const float* src = img + (long long)n * 3 * hw;
  float v[3];
  if constexpr (COPY) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = src[c * hw + (long long)oy * s + ox];
  } else {
    const BilinearTap ty = bilinear_tap(scale, oy, s), tx = bilinear_tap(scale, ox, s);
    const float* r0 = src + (long long)ty.i0 * s;
    const float* r1 = src + (long long)ty.i1 * s;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = r0[c * hw + tx.i0], b = r0[c * hw + tx.i1], cc = r1[c * hw + tx.i0], d = r1[c * hw + tx.i1];
      const float top = __fadd_rn(__fmul_rn(tx.l0, a), __fmul_rn(tx.l1, b));
      const float bot = __fadd_rn(__fmul_rn(tx.l0, cc), __fmul_rn(tx.l1, d));
      v[c] = __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
    }
  }
  float* dst = out + ((long long)n * II_OUT * II_OUT + u) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = normalize ? __fsub_rn(__fmul_rn(2.f, v[c]), 1.f) : v[c];
}

// Kernel id (1: resampling, 2: s = 299, layout change only) or an FMGAN_E* status; *gx: blocks per sample.
int ii_plan(int batch, int h, int w, int* gx) {
  if (batch <= 0 || h <= 0 || w <= 0) return FMGAN_EINVAL;
  if (h != w || !(h == 256 || h == 512 || h == 1024 || h == II_OUT)) return FMGAN_EUNSUPPORTED;
  // pixel indices are ints (s <= 1024), element offsets long long; samples * blocks per sample is grid.x
  *gx = (II_OUT * II_OUT + II_THREADS - 1) / II_THREADS;
  if ((long long)*gx * batch > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  return h == II_OUT ? 2 : 1;
}

}  // namespace

extern "C" int fmgan_inception_input_select(int batch, int h, int w) {
  int gx;
  return ii_plan(batch, h, w, &gx);
}

extern "C" int fmgan_inception_input_f32(const float* img, float* out, int batch, int h, int w, int normalize,
                                         void* stream) {
  if (!img || !out) return FMGAN_EINVAL;
  int gx;
  const int id = ii_plan(batch, h, w, &gx);
  if (id <= 0) return id;
  const dim3 grid((unsigned)((long long)gx * batch)), block(II_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const float scale = (float)h / (float)II_OUT;      // rounded on the host, handed to every lane
  if (id == 2)
    hipLaunchKernelGGL(inception_input_f32<true>, grid, block, 0, st, img, out, h, scale, normalize != 0, gx);
  else
    hipLaunchKernelGGL(inception_input_f32<false>, grid, block, 0, st, img, out, h, scale, normalize != 0, gx);
  return fmgan_check_launch();
}
