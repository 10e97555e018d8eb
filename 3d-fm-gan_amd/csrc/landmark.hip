// Tensor work around the landmark networks (reference Util/landmark_util.py, Util/training_util.py:206-222) for gfx950:
// what stands between the Generator's image and the face detector / the alignment network, and between the heat maps
// and the loss and landmarks.  Five kernels, one launch each, float32, no atomics: the same input gives the same bits.
//
//   face_crop_fwd     img [N,3,H,W] in [-1,1], box [N,4] int32 (ux, uy, bx, by)  ->  out [N,3,R,R] in [0,1]
//                       canvas[c,y,x] = ((img[c, y+uy, x+ux] + 1) * 255) * 0.5 inside the image, 0 elsewhere,
//                       Hc = by - uy rows, Wc = bx - ux columns (Crop_PyTorch); the canvas is never materialised;
//                       out = bilinear(canvas -> R x R, align_corners=False) / 255, taps by bilinear_tap.h,
//                       v = h0*(w0*a + w1*b) + h1*(w0*c + w1*d), every product and sum rounded.
//                     a lane owns one output pixel (three channels): 4 taps per channel as scalar loads (adjacent lanes:
//                     adjacent or near-adjacent addresses of one source row), three coalesced stores.
//   face_crop_bwd     grad_img [N,3,H,W] from grad_out, gather form: a lane owns one image pixel, inverts the tap map to a
//                     conservative range of output rows and columns, and confirms every candidate with bilinear_tap, the
//                     forward's own function; sum in fixed order (rows, columns, row tap, column tap ascending) of
//                     (h*w) * (grad_out / 255), then (sum * 0.5) * 255: autograd's order through /255, the resampling,
//                     /2 and *255.  Pixels outside the crop get exactly 0.
//   detector_input    out[n,c] = ((img[n,2-c] + 1) * 255) * 0.5 - mean[c], mean = (104, 117, 123): Get_HeatMap_PyTorch's
//                     scaling and Batch_Img_Face_Detection's flip and subtraction.
//   distance_fwd/bwd  d[n] = sum (a - b)^2 over a sample's M elements as fixed-order partials of 4096 elements each
//                     (per-lane serial fma, block_sum_ordered);  grad_a = (2 * g[n]) * (a - b), grad_b = -grad_a.
//   landmark_decode   hm [maps,64,64] -> preds, preds_orig [maps,2] (_get_preds_fromhm_torch): one wave per map, 64
//                     values per lane as 16 coalesced 16-byte loads, (value, index) argmax by xor butterfly with the
//                     smallest flat index winning a tie (NaN counts as the largest value, as in torch.argmax), then lane
//                     0 reads the four neighbours and writes the two points.
// A box side outside [1, 2^24] gives a zero crop and a zero gradient (the tap index is an int); every image read is
// bounds-tested, so no box content can make a lane read outside img.
#include "bilinear_tap.h"
#include "block_sum.h"

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_WAVES = LM_THREADS / FMGAN_WAVE;
constexpr int LM_MAX_SIDE = 1 << 24;                 // of a crop canvas: tap indices and their float forms stay exact
constexpr int LM_MAX_IMG = 1 << 15;                  // of H, W, R: pixel indices are ints
constexpr int LM_CHUNK = 4096;                       // elements of one distance partial
constexpr int LM_MAP = 64;                           // side of a heat map the decode takes
static_assert(LM_CHUNK == LM_THREADS * 4 * 4, "four float4 per lane");
static_assert(LM_MAP * LM_MAP == FMGAN_WAVE * 4 * 16, "sixteen float4 per lane");

struct LmBox {
  int ux, uy, hc, wc;                                // hc = 0: no crop
};

__device__ __forceinline__ LmBox lm_box(const int* __restrict__ box, int n) {
  const int ux = box[4 * n], uy = box[4 * n + 1], bx = box[4 * n + 2], by = box[4 * n + 3];
  const long long hc = (long long)by - uy, wc = (long long)bx - ux;
  const bool ok = hc >= 1 && wc >= 1 && hc <= LM_MAX_SIDE && wc <= LM_MAX_SIDE;
  return {ux, uy, ok ? (int)hc : 0, ok ? (int)wc : 0};
}

// canvas value at canvas row cy, column cx of plane p (0 outside the image)
__device__ __forceinline__ float lm_canvas(const float* __restrict__ p, const LmBox& b, int cy, int cx, int H, int W) {
  const long long iy = (long long)cy + b.uy, ix = (long long)cx + b.ux;
  if (iy < 0 || iy >= H || ix < 0 || ix >= W) return 0.f;
  return __fmul_rn(__fmul_rn(__fadd_rn(p[iy * W + ix], 1.f), 255.f), 0.5f);
}

__global__ __launch_bounds__(LM_THREADS) void face_crop_fwd_f32(const float* __restrict__ img,
                                                                const int* __restrict__ box, float* __restrict__ out,
                                                                int H, int W, int R, int gx) {
  const int n = blockIdx.x / gx, u = (blockIdx.x % gx) * LM_THREADS + threadIdx.x;
  if (u >= R * R) return;
  const int oy = u / R, ox = u % R;
  const long long hw = (long long)H * W, rr = (long long)R * R;
  float* dst = out + (long long)n * 3 * rr + u;
  const LmBox b = lm_box(box, n);
  if (b.hc == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * rr] = 0.f;
    return;
  }
  const BilinearTap ty = bilinear_tap(__fdiv_rn((float)b.hc, (float)R), oy, b.hc);
  const BilinearTap tx = bilinear_tap(__fdiv_rn((float)b.wc, (float)R), ox, b.wc);
  const float* src = img + (long long)n * 3 * hw;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* p = src + c * hw;
    const float a = lm_canvas(p, b, ty.i0, tx.i0, H, W), bb = lm_canvas(p, b, ty.i0, tx.i1, H, W);
    const float cc = lm_canvas(p, b, ty.i1, tx.i0, H, W), d = lm_canvas(p, b, ty.i1, tx.i1, H, W);
    const float top = __fadd_rn(__fmul_rn(tx.l0, a), __fmul_rn(tx.l1, bb));
    const float bot = __fadd_rn(__fmul_rn(tx.l0, cc), __fmul_rn(tx.l1, d));
    const float v = __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
    dst[c * rr] = __fdiv_rn(v, 255.f);
  }
}

// Output indices d in [lo, hi] that may have canvas index c among their taps: i0 in {c - 1, c}, that is
// c - 1 <= src(d) < c + 1 with src(d) = scale * (d + 0.5) - 0.5; two indices of slack on each side cover the rounding of
// this float arithmetic (|error| < 0.1 for out <= 2^15); the caller confirms each candidate with bilinear_tap.
__device__ __forceinline__ void lm_candidates(float scale, int c, int out, int* lo, int* hi) {
  const float a = floorf(((float)c - 0.5f) / scale - 0.5f) - 2.f;
  const float b = ceilf(((float)c + 1.5f) / scale - 0.5f) + 2.f;
  *lo = a < 0.f ? 0 : (a > (float)(out - 1) ? out - 1 : (int)a);
  *hi = b < 0.f ? 0 : (b > (float)(out - 1) ? out - 1 : (int)b);
}

__global__ __launch_bounds__(LM_THREADS) void face_crop_bwd_f32(const float* __restrict__ grad_out,
                                                                const int* __restrict__ box,
                                                                float* __restrict__ grad_img, int H, int W, int R,
                                                                int gx) {
  const long long hw = (long long)H * W, rr = (long long)R * R;
  const long long u = (long long)(blockIdx.x % gx) * LM_THREADS + threadIdx.x;
  const int n = blockIdx.x / gx;
  if (u >= hw) return;
  const int iy = (int)(u / W), ix = (int)(u % W);
  float* dst = grad_img + (long long)n * 3 * hw + u;
  const LmBox b = lm_box(box, n);
  const long long cy = (long long)iy - b.uy, cx = (long long)ix - b.ux;
  float acc[3] = {0.f, 0.f, 0.f};
  if (b.hc != 0 && cy >= 0 && cy < b.hc && cx >= 0 && cx < b.wc) {
    const float sy = __fdiv_rn((float)b.hc, (float)R), sx = __fdiv_rn((float)b.wc, (float)R);
    int y_lo, y_hi, x_lo, x_hi;
    lm_candidates(sy, (int)cy, R, &y_lo, &y_hi);
    lm_candidates(sx, (int)cx, R, &x_lo, &x_hi);
    const float* go = grad_out + (long long)n * 3 * rr;
    for (int oy = y_lo; oy <= y_hi; ++oy) {
      const BilinearTap ty = bilinear_tap(sy, oy, b.hc);
      const bool y0 = ty.i0 == (int)cy, y1 = ty.i1 == (int)cy;
      if (!(y0 || y1)) continue;
      for (int ox = x_lo; ox <= x_hi; ++ox) {
        const BilinearTap tx = bilinear_tap(sx, ox, b.wc);
        const bool x0 = tx.i0 == (int)cx, x1 = tx.i1 == (int)cx;
        if (!(x0 || x1)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float g = __fdiv_rn(go[c * rr + (long long)oy * R + ox], 255.f);
          if (y0 && x0) acc[c] = __fadd_rn(acc[c], __fmul_rn(__fmul_rn(ty.l0, tx.l0), g));
          if (y0 && x1) acc[c] = __fadd_rn(acc[c], __fmul_rn(__fmul_rn(ty.l0, tx.l1), g));
          if (y1 && x0) acc[c] = __fadd_rn(acc[c], __fmul_rn(__fmul_rn(ty.l1, tx.l0), g));
          if (y1 && x1) acc[c] = __fadd_rn(acc[c], __fmul_rn(__fmul_rn(ty.l1, tx.l1), g));
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c * hw] = __fmul_rn(__fmul_rn(acc[c], 0.5f), 255.f);
}

__device__ __forceinline__ float lm_detector(float v, float mean) {
  return __fsub_rn(__fmul_rn(__fmul_rn(__fadd_rn(v, 1.f), 255.f), 0.5f), mean);
}

// VEC: a lane owns four consecutive pixels of one plane (hw % 4 == 0); otherwise one pixel.
template <bool VEC>
__global__ __launch_bounds__(LM_THREADS) void detector_input_f32(const float* __restrict__ img, float* __restrict__ out,
                                                                 long long hw, int gx) {
  const int plane = blockIdx.x / gx, c = plane % 3;
  const long long i = ((long long)(blockIdx.x % gx) * LM_THREADS + threadIdx.x) * (VEC ? 4 : 1);
  if (i >= hw) return;
  const float mean = c == 0 ? 104.f : (c == 1 ? 117.f : 123.f);
  const float* src = img + ((long long)(plane - c) + (2 - c)) * hw + i;
  float* dst = out + (long long)plane * hw + i;
  if constexpr (VEC) {
    const f32x4_u v = *reinterpret_cast<const f32x4_u*>(src);
    const f32x4_u o = {lm_detector(v.x, mean), lm_detector(v.y, mean), lm_detector(v.z, mean), lm_detector(v.w, mean)};
    *reinterpret_cast<f32x4_u*>(dst) = o;
  } else {
    *dst = lm_detector(*src, mean);
  }
}

__global__ __launch_bounds__(LM_THREADS) void heatmap_distance_fwd_f32(const float* __restrict__ a,
                                                                       const float* __restrict__ b,
                                                                       float* __restrict__ partial, long long m, int gx) {
#pragma clang fp contract(off)
  __shared__ float red[LM_WAVES];
  const int n = blockIdx.x / gx;
  const long long base = (long long)n * m, first = (long long)(blockIdx.x % gx) * LM_CHUNK + threadIdx.x * 4;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = first + (long long)k * LM_THREADS * 4;
    if (i < m) {                                           // m % 4 == 0: the whole quad is inside
      const f32x4_u va = *reinterpret_cast<const f32x4_u*>(a + base + i);
      const f32x4_u vb = *reinterpret_cast<const f32x4_u*>(b + base + i);
      const float d0 = va.x - vb.x, d1 = va.y - vb.y, d2 = va.z - vb.z, d3 = va.w - vb.w;
      acc = __builtin_fmaf(d0, d0, acc);
      acc = __builtin_fmaf(d1, d1, acc);
      acc = __builtin_fmaf(d2, d2, acc);
      acc = __builtin_fmaf(d3, d3, acc);
    }
  }
  const float sum = block_sum_ordered<LM_WAVES>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(LM_THREADS) void heatmap_distance_bwd_f32(const float* __restrict__ a,
                                                                       const float* __restrict__ b,
                                                                       const float* __restrict__ g,
                                                                       float* __restrict__ grad_a,
                                                                       float* __restrict__ grad_b, long long m, int gx) {
#pragma clang fp contract(off)
  const int n = blockIdx.x / gx;
  const long long base = (long long)n * m, first = (long long)(blockIdx.x % gx) * LM_CHUNK + threadIdx.x * 4;
  const float k2 = 2.f * g[n];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = first + (long long)k * LM_THREADS * 4;
    if (i < m) {
      const f32x4_u va = *reinterpret_cast<const f32x4_u*>(a + base + i);
      const f32x4_u vb = *reinterpret_cast<const f32x4_u*>(b + base + i);
      const f32x4_u ga = {k2 * (va.x - vb.x), k2 * (va.y - vb.y), k2 * (va.z - vb.z), k2 * (va.w - vb.w)};
      if (grad_a) *reinterpret_cast<f32x4_u*>(grad_a + base + i) = ga;
      if (grad_b) {
        const f32x4_u gb = {-ga.x, -ga.y, -ga.z, -ga.w};
        *reinterpret_cast<f32x4_u*>(grad_b + base + i) = gb;
      }
    }
  }
}

// is (v1, i1) ahead of (v2, i2) in torch.argmax's order: the larger value, NaN above everything, the smaller index on a tie
__device__ __forceinline__ bool lm_ahead(float v1, int i1, float v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 || n2) return n1 && (!n2 || i1 < i2);
  return v1 > v2 || (v1 == v2 && i1 < i2);
}

__device__ __forceinline__ float lm_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(LM_THREADS) void landmark_decode_f32(const float* __restrict__ hm,
                                                                  const float* __restrict__ center,
                                                                  const float* __restrict__ scale,
                                                                  float* __restrict__ preds,
                                                                  float* __restrict__ preds_orig, long long maps,
                                                                  int per_sample) {
#pragma clang fp contract(off)
  const long long map = (long long)blockIdx.x * LM_WAVES + threadIdx.x / FMGAN_WAVE;
  if (map >= maps) return;                                 // wave-uniform
  const int lane = threadIdx.x & (FMGAN_WAVE - 1);
  const float* p = hm + map * (LM_MAP * LM_MAP);
  float best = p[lane * 4];
  int at = lane * 4;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = (j * FMGAN_WAVE + lane) * 4;
    const f32x4_u v = *reinterpret_cast<const f32x4_u*>(p + i);
    if (lm_ahead(v.x, i, best, at)) { best = v.x; at = i; }
    if (lm_ahead(v.y, i + 1, best, at)) { best = v.y; at = i + 1; }
    if (lm_ahead(v.z, i + 2, best, at)) { best = v.z; at = i + 2; }
    if (lm_ahead(v.w, i + 3, best, at)) { best = v.w; at = i + 3; }
  }
#pragma unroll
  for (int msk = FMGAN_WAVE / 2; msk > 0; msk >>= 1) {
    const float ov = __shfl_xor(best, msk, FMGAN_WAVE);
    const int oi = __shfl_xor(at, msk, FMGAN_WAVE);
    if (lm_ahead(ov, oi, best, at)) { best = ov; at = oi; }
  }
  if (lane != 0) return;
  const int px = at % LM_MAP, py = at / LM_MAP;
  float x = (float)(px + 1), y = (float)(py + 1);
  if (px > 0 && px < LM_MAP - 1 && py > 0 && py < LM_MAP - 1) {
    x += 0.25f * lm_sign(p[at + 1] - p[at - 1]);
    y += 0.25f * lm_sign(p[at + LM_MAP] - p[at - LM_MAP]);
  }
  x -= 0.5f;
  y -= 0.5f;
  const f32x2_u pt = {x, y};
  *reinterpret_cast<f32x2_u*>(preds + map * 2) = pt;
  f32x2_u orig = {0.f, 0.f};
  if (center) {
    // inverse of transform() at resolution r = 64: (p - r * (-c / h + 0.5)) * h / r, h = 200 * scale, truncated
    const long long s = map / per_sample;
    const float h = 200.f * scale[s], r = (float)LM_MAP;
    const float tx = r * (-center[2 * s] / h + 0.5f), ty = r * (-center[2 * s + 1] / h + 0.5f);
    orig.x = truncf((x - tx) * h / r);
    orig.y = truncf((y - ty) * h / r);
  }
  *reinterpret_cast<f32x2_u*>(preds_orig + map * 2) = orig;
}

// Blocks per sample of the crop kernels (forward: over R*R outputs, backward: over H*W pixels), or an FMGAN_E* status.
int lm_crop_plan(int batch, int h, int w, int r, int* gx_fwd, int* gx_bwd) {
  if (batch <= 0 || h <= 0 || w <= 0 || r <= 0) return FMGAN_EINVAL;
  if (h > LM_MAX_IMG || w > LM_MAX_IMG || r > LM_MAX_IMG) return FMGAN_EOVERFLOW;
  const long long f = ((long long)r * r + LM_THREADS - 1) / LM_THREADS, b = ((long long)h * w + LM_THREADS - 1) / LM_THREADS;
  if (f * batch > 0x7fffffffLL || b * batch > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  *gx_fwd = (int)f;
  *gx_bwd = (int)b;
  return 1;
}

// Partials per sample of the distance, or an FMGAN_E* status.
int lm_distance_plan(int batch, long long m) {
  if (batch <= 0 || m <= 0) return FMGAN_EINVAL;
  if (m % 4 != 0) return FMGAN_EUNSUPPORTED;
  const long long gx = (m + LM_CHUNK - 1) / LM_CHUNK;
  if (gx * batch > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  return (int)gx;
}

}  // namespace

extern "C" int fmgan_face_crop_select(int batch, int h, int w, int r) {
  int f, b;
  return lm_crop_plan(batch, h, w, r, &f, &b);
}

extern "C" int fmgan_face_crop_fwd_f32(const float* img, const void* box, float* out, int batch, int h, int w, int r,
                                       void* stream) {
  if (!img || !box || !out) return FMGAN_EINVAL;
  int gf, gb;
  const int id = lm_crop_plan(batch, h, w, r, &gf, &gb);
  if (id <= 0) return id;
  hipLaunchKernelGGL(face_crop_fwd_f32, dim3((unsigned)(gf * batch)), dim3(LM_THREADS), 0, (hipStream_t)stream, img,
                     static_cast<const int*>(box), out, h, w, r, gf);
  return fmgan_check_launch();
}

extern "C" int fmgan_face_crop_bwd_f32(const float* grad_out, const void* box, float* grad_img, int batch, int h, int w,
                                       int r, void* stream) {
  if (!grad_out || !box || !grad_img) return FMGAN_EINVAL;
  int gf, gb;
  const int id = lm_crop_plan(batch, h, w, r, &gf, &gb);
  if (id <= 0) return id;
  hipLaunchKernelGGL(face_crop_bwd_f32, dim3((unsigned)(gb * batch)), dim3(LM_THREADS), 0, (hipStream_t)stream, grad_out,
                     static_cast<const int*>(box), grad_img, h, w, r, gb);
  return fmgan_check_launch();
}

extern "C" int fmgan_detector_input_f32(const float* img, float* out, int batch, long long hw, void* stream) {
  if (!img || !out || batch <= 0 || hw <= 0) return FMGAN_EINVAL;
  const bool vec = hw % 4 == 0;
  const long long gx = ((vec ? hw / 4 : hw) + LM_THREADS - 1) / LM_THREADS;
  if (gx * 3 * batch > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  const dim3 grid((unsigned)(gx * 3 * batch)), block(LM_THREADS);
  if (vec)
    hipLaunchKernelGGL(detector_input_f32<true>, grid, block, 0, (hipStream_t)stream, img, out, hw, (int)gx);
  else
    hipLaunchKernelGGL(detector_input_f32<false>, grid, block, 0, (hipStream_t)stream, img, out, hw, (int)gx);
  return fmgan_check_launch();
}

extern "C" int fmgan_heatmap_distance_blocks(int batch, long long m) {
  const int gx = lm_distance_plan(batch, m);
  return gx > 0 ? gx : 0;
}

extern "C" int fmgan_heatmap_distance_fwd_f32(const float* a, const float* b, float* partial, int batch, long long m,
                                              void* stream) {
  if (!a || !b || !partial) return FMGAN_EINVAL;
  const int gx = lm_distance_plan(batch, m);
  if (gx <= 0) return gx;
  hipLaunchKernelGGL(heatmap_distance_fwd_f32, dim3((unsigned)(gx * batch)), dim3(LM_THREADS), 0, (hipStream_t)stream, a, b,
                     partial, m, gx);
  return fmgan_check_launch();
}

extern "C" int fmgan_heatmap_distance_bwd_f32(const float* a, const float* b, const float* g, float* grad_a, float* grad_b,
                                              int batch, long long m, void* stream) {
  if (!a || !b || !g || !(grad_a || grad_b)) return FMGAN_EINVAL;
  const int gx = lm_distance_plan(batch, m);
  if (gx <= 0) return gx;
  hipLaunchKernelGGL(heatmap_distance_bwd_f32, dim3((unsigned)(gx * batch)), dim3(LM_THREADS), 0, (hipStream_t)stream, a, b,
                     g, grad_a, grad_b, m, gx);
  return fmgan_check_launch();
}

extern "C" int fmgan_landmark_decode_f32(const float* hm, const float* center, const float* scale, float* preds,
                                         float* preds_orig, int batch, int channels, int h, int w, void* stream) {
  if (!hm || !preds || !preds_orig || batch <= 0 || channels <= 0 || h <= 0 || w <= 0 || (center != nullptr) != (scale != nullptr))
    return FMGAN_EINVAL;
  if (h != LM_MAP || w != LM_MAP) return FMGAN_EUNSUPPORTED;
  const long long maps = (long long)batch * channels, gx = (maps + LM_WAVES - 1) / LM_WAVES;
  if (gx > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  hipLaunchKernelGGL(landmark_decode_f32, dim3((unsigned)gx), dim3(LM_THREADS), 0, (hipStream_t)stream, hm, center, scale,
                     preds, preds_orig, maps, channels);
  return fmgan_check_launch();
}
