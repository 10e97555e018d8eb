// Input stage of the perceptual path length (reference Evaluation/ppl.py:116-123, 191-202; lpips ScalingLayer) for
// gfx950: from the Generator's interleaved image batch to the two inputs of the channels_last VGG trunk, in one pass.
//
//   img  [2*pairs, 3, h, w] NCHW; sample 2p is the first image of pair p, sample 2p+1 the second
//   v    = the window's pixel (f = 1), or the bilinear reduction by f = 2 / 4 (F.interpolate(mode='bilinear',
//          align_corners=False) at an integer ratio: source index f*d + f/2 - 0.5, both weights 1/2), with o = f/2 - 1:
//            a, b = img[n, c, y0 + f*y + o, x0 + f*x + o (+1)],   c, d = the same columns one row below
//            v    = 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d)     in this association, no fused multiply-add
//   out  = (v - shift[c]) / scale[c]                              IEEE subtraction, correctly rounded division
//   out0 / out1 [pairs, oh, ow, 3] dense (NHWC storage of [pairs, 3, oh, ow]), oh = hc/f, ow = wc/f
//
// The composite spends five to eight launches and several intermediates on this; here only the source rows that carry a
// tap are read (all of them at f = 1 and 2, rows 4y+1 and 4y+2 at f = 4: half the image), once, and each output once.
//
// Mapping: a lane owns four adjacent output pixels of one output row of one sample: 48 contiguous output bytes, written
// as three 16-byte stores.  Its source per channel and tap row is 4 / 8 contiguous floats at f = 1 / 2 (one / two 16-byte
// loads) and four 2-float pieces 16 bytes apart at f = 4 (four 8-byte loads: nothing but taps is loaded, so no load
// reaches past the window).  The loads need dword alignment only (f32x4_u / f32x2_u): an odd x0, or o = 1 at f = 4, puts
// them off the 16-byte grid.  Lanes of a wave own consecutive units of a row: their loads cover one contiguous run of the
// source row.  grid.x = samples * blocks per sample; one unit per lane, no grid-stride loop, no shared memory.
// The vector form serves ow % 4 == 0 with no edge path at all; any other width runs the bounded form (per-pixel guards,
// scalar loads and stores, the same arithmetic in the same order: the same bits), chosen per launch, never per lane.
#include <climits>

#include "lpips_input.h"

namespace {

constexpr int PI_THREADS = 256;
constexpr int PI_PIX = LPIPS_IN_PIX;      // output pixels of a unit

template <int F, bool VEC>
__global__ __launch_bounds__(PI_THREADS) void lpips_pair_input_f32(const float* __restrict__ img,
                                                                   const float* __restrict__ shift,
                                                                   const float* __restrict__ scale,
                                                                   float* __restrict__ out0, float* __restrict__ out1,
                                                                   int h, int w, int y0, int x0, int oh, int ow,
                                                                   int units_x, int units, int gx) {
  constexpr int O = lpips_in_first_tap(F);
  const int n = blockIdx.x / gx, blk = blockIdx.x % gx;
  const int u = blk * PI_THREADS + threadIdx.x;
  if (u >= units) return;
  const int oy = u / units_x, ox = (u % units_x) * PI_PIX;
  const long long hw = (long long)h * w;
  const float* src = img + (long long)n * 3 * hw + (long long)(y0 + F * oy + O) * w + (x0 + F * ox + O);
  float* dst = ((n & 1) ? out1 : out0) + (((long long)(n >> 1) * oh + oy) * ow + ox) * 3;
  float v[3][PI_PIX];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* r0 = src + c * hw;
    const float* r1 = r0 + w;                        // read at f > 1 only
    if constexpr (VEC && F == 1) {
      lpips_in_load<PI_PIX>(r0, v[c]);
    } else if constexpr (VEC && F == 2) {
      float a[F * PI_PIX], b[F * PI_PIX];
      lpips_in_load<F * PI_PIX>(r0, a);
      lpips_in_load<F * PI_PIX>(r1, b);
#pragma unroll
      for (int j = 0; j < PI_PIX; ++j) v[c][j] = lpips_in_quad(a[F * j], a[F * j + 1], b[F * j], b[F * j + 1]);
    } else if constexpr (VEC) {
      f32x2_u a[PI_PIX], b[PI_PIX];
#pragma unroll
      for (int j = 0; j < PI_PIX; ++j) {
        a[j] = *reinterpret_cast<const f32x2_u*>(r0 + F * j);
        b[j] = *reinterpret_cast<const f32x2_u*>(r1 + F * j);
      }
#pragma unroll
      for (int j = 0; j < PI_PIX; ++j) v[c][j] = lpips_in_quad(a[j].x, a[j].y, b[j].x, b[j].y);
    } else {
#pragma unroll
      for (int j = 0; j < PI_PIX; ++j) {
        v[c][j] = 0.f;
        if (ox + j < ow) v[c][j] = F == 1 ? r0[j] : lpips_in_quad(r0[F * j], r0[F * j + 1], r1[F * j], r1[F * j + 1]);
      }
    }
  }
  const float sh[3] = {shift[0], shift[1], shift[2]}, sc[3] = {scale[0], scale[1], scale[2]};
  float o[3 * PI_PIX];
#pragma unroll
  for (int j = 0; j < PI_PIX; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * j + c] = lpips_in_scaled(v[c][j], sh[c], sc[c]);
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < 3; ++q) lpips_in_store4(dst + 4 * q, o + 4 * q);
  } else {
#pragma unroll
    for (int j = 0; j < PI_PIX; ++j)
      if (ox + j < ow) {
        dst[3 * j] = o[3 * j];
        dst[3 * j + 1] = o[3 * j + 1];
        dst[3 * j + 2] = o[3 * j + 2];
      }
  }
}

// The plan of one call: output size, units and blocks, and the kernel id (f for the vector form, 8 + f for the bounded
// one).  Returns that id, or an FMGAN_E* status.
struct PiPlan {
  int oh, ow, units_x, units, gx;
};

int pi_plan(int pairs, int h, int w, int y0, int x0, int hc, int wc, int f, PiPlan* p) {
  if (pairs <= 0 || h <= 0 || w <= 0 || y0 < 0 || x0 < 0 || hc <= 0 || wc <= 0) return FMGAN_EINVAL;
  if ((long long)y0 + hc > h || (long long)x0 + wc > w) return FMGAN_EINVAL;
  if (!(f == 1 || f == 2 || f == 4) || hc % f != 0 || wc % f != 0) return FMGAN_EUNSUPPORTED;
  // element offsets are long long; pixel, unit and block indices are ints
  const long long hw = (long long)h * w;
  if (hw > 0x7fffffffLL - PI_THREADS * PI_PIX) return FMGAN_EOVERFLOW;
  if (pairs > 0x3fffffff || 3 * hw > LLONG_MAX / (2LL * pairs)) return FMGAN_EOVERFLOW;
  p->oh = hc / f;
  p->ow = wc / f;
  p->units_x = (p->ow + PI_PIX - 1) / PI_PIX;
  p->units = p->oh * p->units_x;
  p->gx = (p->units + PI_THREADS - 1) / PI_THREADS;
  if ((long long)p->gx * 2 * pairs > 0x7fffffffLL) return FMGAN_EOVERFLOW;      // grid.x
  return p->ow % PI_PIX == 0 ? f : 8 + f;
}

}  // namespace

extern "C" int fmgan_lpips_pair_input_select(int pairs, int h, int w, int y0, int x0, int hc, int wc, int f) {
  PiPlan p;
  return pi_plan(pairs, h, w, y0, x0, hc, wc, f, &p);
}

extern "C" int fmgan_lpips_pair_input_f32(const float* img, const float* shift, const float* scale, float* out0,
                                          float* out1, int pairs, int h, int w, int y0, int x0, int hc, int wc, int f,
                                          void* stream) {
  if (pairs <= 0 || !img || !shift || !scale || !out0 || !out1) return FMGAN_EINVAL;
  PiPlan p;
  const int id = pi_plan(pairs, h, w, y0, x0, hc, wc, f, &p);
  if (id <= 0) return id;
  const dim3 grid((unsigned)((long long)p.gx * 2 * pairs)), block(PI_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define PI_GO(F, VEC)                                                                                               \
  hipLaunchKernelGGL((lpips_pair_input_f32<F, VEC>), grid, block, 0, s, img, shift, scale, out0, out1, h, w, y0, x0, \
                     p.oh, p.ow, p.units_x, p.units, p.gx)
  switch (id) {
    case 1: PI_GO(1, true); break;
    case 2: PI_GO(2, true); break;
    case 4: PI_GO(4, true); break;
    case 9: PI_GO(1, false); break;
    case 10: PI_GO(2, false); break;
    default: PI_GO(4, false); break;
  }
#undef PI_GO
  return fmgan_check_launch();
}
