// Image stage of the projection criterion (reference Evaluation/image_projection/project/__init__.py:125-129, 199-220;
// lpips ScalingLayer) for gfx950, forward and backward, one launch each.
//
//   x, target [B, 3, S, S] NCHW, S = 256 * f, f in {1, 2, 4};  mask [S, S] or none
//   forward   partial[blk] = sum over block blk's pixels of (x - t)^2 (* mask[h, w])            fixed order, no atomics
//             y[b, i, j, c] = (bilinear_f(clamp(x, -1, 1)) - shift[c]) / scale[c]               NHWC, optional
//   backward  grad_x = (k * (x - t)) * mask + 1[-1 <= x <= 1] * w_f(h, w) * (g_y[b, h/f, w/f, c] / scale[c])
//
// bilinear_f is F.interpolate(size=256, mode='bilinear', align_corners=False) at the integer ratio f: the identity at
// f = 1, and at f = 2 / 4 the mean of the 2x2 pixels at rows and columns f*i + f/2 - 1 and + 1 (both weights 1/2), built
// from lpips_in_half (lpips_input.h, shared with the PPL input stage): 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d).  Hence
// w_f = 1 at f = 1, 1/4 at f = 2, and at f = 4 1/4 on rows and columns 4i+1, 4i+2 and 0 elsewhere: every source pixel
// feeds at most one reduced pixel, and the backward is a gather.
//
// The composite spends about eight launches per direction on this (sub, pow, mean, clamp, interpolate, ScalingLayer,
// layout copy) and keeps their intermediates for autograd; here the forward reads x and target once (8 B per element,
// plus the mask and 12 B per reduced pixel of y) and the backward reads them again and writes grad_x (12 B per element,
// plus the mask and 12 B per reduced pixel of g_y).  Nothing but x and target is kept between the two.
//
// Mapping (both kernels): a lane owns four adjacent reduced pixels of one reduced row of one sample, that is an
// f x 4f window of each of the three planes: per plane and source row 4f contiguous floats (f 16-byte loads), and its
// 12 floats of y / g_y are 48 contiguous bytes (three 16-byte accesses).  Lanes of a wave own consecutive units of a
// row, so a wave covers one contiguous run of every source row it reads and of y.  grid.x = B * 128 blocks of 128
// threads, one unit per lane, no grid-stride loop.  All vector accesses need dword alignment only (f32x4_u).
// Forward sum: per-lane serial (explicit fma) over rows, planes, columns in that order, then block_sum_ordered
// (block_sum.h) over the two waves -> partial[blockIdx.x]; bit-reproducible run to run.
// A NaN in x or target reaches the sum and its own grad_x element also where mask is 0 (NaN * 0 = NaN), as in the
// reference's weighted_mse_loss, which multiplies too.
#include <climits>

#include "block_sum.h"
#include "lpips_input.h"

namespace {

constexpr int PL_THREADS = 128;
constexpr int PL_OUT = 256;                                  // the size LPIPS is evaluated at
constexpr int PL_PIX = LPIPS_IN_PIX;                         // reduced pixels of a unit
constexpr int PL_UNITS_X = PL_OUT / PL_PIX;
constexpr int PL_BLOCKS = PL_OUT * PL_UNITS_X / PL_THREADS;  // blocks per sample
constexpr int PL_MAX_BATCH = 0x7fffffff / PL_BLOCKS;         // grid.x and the partial count stay below 2^31
static_assert(PL_THREADS == 2 * FMGAN_WAVE, "the block sum below adds two waves");
static_assert(PL_OUT * PL_UNITS_X % PL_THREADS == 0, "no partial block: no bounds test in the kernels");

// torch.clamp: NaN stays NaN
__device__ __forceinline__ float pl_clamp(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

// is (row r, column j) of a lane's f x 4f window a tap of the reduction?
template <int F>
__device__ __forceinline__ constexpr bool pl_tap(int r, int j) {
  if (F < 4) return true;
  return (r == 1 || r == 2) && (j % 4 == 1 || j % 4 == 2);
}

struct PlUnit {
  int n, oy, ox;
};

__device__ __forceinline__ PlUnit pl_unit() {
  const int n = blockIdx.x / PL_BLOCKS, u = (blockIdx.x % PL_BLOCKS) * PL_THREADS + threadIdx.x;
  return {n, u / PL_UNITS_X, (u % PL_UNITS_X) * PL_PIX};
}

template <int F>
__global__ __launch_bounds__(PL_THREADS) void projection_loss_fwd_f32(const float* __restrict__ x,
                                                                      const float* __restrict__ target,
                                                                      const float* __restrict__ mask,
                                                                      const float* __restrict__ shift,
                                                                      const float* __restrict__ scale,
                                                                      float* __restrict__ partial,
                                                                      float* __restrict__ y) {
#pragma clang fp contract(off)
  constexpr int S = PL_OUT * F, W = PL_PIX * F;
  constexpr int R0 = lpips_in_first_tap(F);
  __shared__ float red[PL_THREADS / FMGAN_WAVE];
  const PlUnit un = pl_unit();
  const long long hw = (long long)S * S;
  const long long win = (long long)(F * un.oy) * S + F * un.ox;
  const float* xs = x + (long long)un.n * 3 * hw + win;
  const float* ts = target + (long long)un.n * 3 * hw + win;
  float acc = 0.f;
  float row[2][3][PL_PIX];                                   // 0.5*a + 0.5*b of the two tap rows
#pragma unroll
  for (int r = 0; r < F; ++r) {
    float m[W];
    if (mask) lpips_in_load<W>(mask + win + r * S, m);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float xv[W], tv[W];
      lpips_in_load<W>(xs + c * hw + r * S, xv);
      lpips_in_load<W>(ts + c * hw + r * S, tv);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float d = xv[j] - tv[j];
        acc = mask ? __builtin_fmaf(d * d, m[j], acc) : __builtin_fmaf(d, d, acc);
      }
      if (F == 1) {
#pragma unroll
        for (int j = 0; j < PL_PIX; ++j) row[0][c][j] = pl_clamp(xv[j]);
      } else if (r == R0 || r == R0 + 1) {
#pragma unroll
        for (int j = 0; j < PL_PIX; ++j)
          // lpips_in_half, spelled out: each clamp stays next to its product
          row[r - R0][c][j] = 0.5f * pl_clamp(xv[F * j + R0]) + 0.5f * pl_clamp(xv[F * j + R0 + 1]);
      }
    }
  }
  if (y) {
    float o[3 * PL_PIX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sh = shift[c], sc = scale[c];
#pragma unroll
      for (int j = 0; j < PL_PIX; ++j) {
        const float v = F == 1 ? row[0][c][j] : lpips_in_half(row[0][c][j], row[1][c][j]);
        o[3 * j + c] = lpips_in_scaled(v, sh, sc);
      }
    }
    float* dst = y + (((long long)un.n * PL_OUT + un.oy) * PL_OUT + un.ox) * 3;
#pragma unroll
    for (int q = 0; q < 3; ++q) lpips_in_store4(dst + 4 * q, o + 4 * q);
  }
  const float sum = block_sum_ordered<2>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

template <int F>
__global__ __launch_bounds__(PL_THREADS) void projection_loss_bwd_f32(const float* __restrict__ x,
                                                                      const float* __restrict__ target,
                                                                      const float* __restrict__ mask,
                                                                      const float* __restrict__ g_y,
                                                                      const float* __restrict__ k,
                                                                      const float* __restrict__ scale,
                                                                      float* __restrict__ grad_x) {
#pragma clang fp contract(off)
  constexpr int S = PL_OUT * F, W = PL_PIX * F;
  const PlUnit un = pl_unit();
  const long long hw = (long long)S * S;
  const long long win = (long long)(F * un.oy) * S + F * un.ox;
  const long long base = (long long)un.n * 3 * hw + win;
  const float kk = k[0];
  float term[3][PL_PIX];                                     // w_f * (g_y / scale) of the unit's reduced pixels
  if (g_y) {
    float o[3 * PL_PIX];
    lpips_in_load<3 * PL_PIX>(g_y + (((long long)un.n * PL_OUT + un.oy) * PL_OUT + un.ox) * 3, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sc = scale[c];
#pragma unroll
      for (int j = 0; j < PL_PIX; ++j) {
        const float q = o[3 * j + c] / sc;
        term[c][j] = F == 1 ? q : 0.25f * q;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < F; ++r) {
    float m[W];
    if (mask) lpips_in_load<W>(mask + win + r * S, m);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float xv[W], tv[W];
      lpips_in_load<W>(x + base + c * hw + r * S, xv);
      lpips_in_load<W>(target + base + c * hw + r * S, tv);
      float* dst = grad_x + base + c * hw + r * S;
#pragma unroll
      for (int q = 0; q < W / 4; ++q) {
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = 4 * q + e;
          float v = kk * (xv[j] - tv[j]);
          if (mask) v = v * m[j];
          if (pl_tap<F>(r, j) && g_y) v = v + (xv[j] >= -1.f && xv[j] <= 1.f ? term[c][j / F] : 0.f);
          g[e] = v;
        }
        const f32x4_u s = {g[0], g[1], g[2], g[3]};
        *reinterpret_cast<f32x4_u*>(dst + 4 * q) = s;
      }
    }
  }
}

// The plan of one call: the kernel id (f), or an FMGAN_E* status.
int pl_plan(int batch, int h, int w, int f) {
  if (batch <= 0 || h <= 0 || w <= 0 || f <= 0) return FMGAN_EINVAL;
  if (h != w || !(f == 1 || f == 2 || f == 4) || h != PL_OUT * f) return FMGAN_EUNSUPPORTED;
  // element offsets are long long (at most batch * 3 * 2^20); block and unit indices are ints
  if (batch > PL_MAX_BATCH) return FMGAN_EOVERFLOW;
  return f;
}

}  // namespace

extern "C" int fmgan_projection_loss_select(int batch, int h, int w, int f) { return pl_plan(batch, h, w, f); }

extern "C" int fmgan_projection_loss_blocks(int batch, int h, int w, int f) {
  return pl_plan(batch, h, w, f) > 0 ? batch * PL_BLOCKS : 0;
}

extern "C" int fmgan_projection_loss_fwd_f32(const float* x, const float* target, const float* mask, const float* shift,
                                             const float* scale, float* partial, float* y, int batch, int h, int w,
                                             int f, void* stream) {
  if (!x || !target || !partial || (y && !(shift && scale))) return FMGAN_EINVAL;
  const int id = pl_plan(batch, h, w, f);
  if (id <= 0) return id;
  const dim3 grid((unsigned)(batch * PL_BLOCKS)), block(PL_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define PL_GO(F) \
  hipLaunchKernelGGL((projection_loss_fwd_f32<F>), grid, block, 0, s, x, target, mask, shift, scale, partial, y)
  switch (id) {
    case 1: PL_GO(1); break;
    case 2: PL_GO(2); break;
    default: PL_GO(4); break;
  }
#undef PL_GO
  return fmgan_check_launch();
}

extern "C" int fmgan_projection_loss_bwd_f32(const float* x, const float* target, const float* mask, const float* g_y,
                                             const float* k, const float* scale, float* grad_x, int batch, int h, int w,
                                             int f, void* stream) {
  if (!x || !target || !k || !grad_x || (g_y && !scale)) return FMGAN_EINVAL;
  const int id = pl_plan(batch, h, w, f);
  if (id <= 0) return id;
  const dim3 grid((unsigned)(batch * PL_BLOCKS)), block(PL_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define PL_GO(F) hipLaunchKernelGGL((projection_loss_bwd_f32<F>), grid, block, 0, s, x, target, mask, g_y, k, scale, grad_x)
  switch (id) {
    case 1: PL_GO(1); break;
    case 2: PL_GO(2); break;
    default: PL_GO(4); break;
  }
#undef PL_GO
  return fmgan_check_launch();
}
