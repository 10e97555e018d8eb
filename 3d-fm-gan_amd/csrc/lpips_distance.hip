// LPIPS distance of one VGG tap (PNetLin.forward in lpips/__init__.py: unit-normalise over channels -> squared
// difference -> 1x1 conv to one channel -> spatial mean) and its data gradients, for gfx950.
//
//   r_k = sqrt(sum_c f_k^2),  n_k = r_k + eps,  u_k = f_k / n_k                 (k = 0, 1; per pixel)
//   d[n] = (1/HW) * sum_p sum_c w_c (u0_c - u1_c)^2
//   q1_c = -2 w_c (u0_c - u1_c) g[n]/HW,  q0 = -q1
//   grad_fk_c = ( qk_c - fk_c * (sum_c' qk_c' fk_c') / (r_k n_k) ) / n_k
//
// The composite spends about ten aten passes per direction over feature-sized tensors; here the forward reads both
// features once, the backward reads both once and writes the wanted gradients once (norms and u are recomputed).
//
// Layout: f0, f1 [N, H*W, C] f32 (NHWC storage), w [C].  16 lanes share a pixel; lane j owns the channels
// 4*(j + 16 t) .. +3, t < C/64, as float4 loads, so a wave-wide load covers 4 pixels x 256 contiguous bytes and both
// features of a pixel stay in registers between the norm pass and the difference pass (64 payload registers at C = 512).
// Narrow taps take several pixels per lane and step (LdCfg::U) to keep as many loads in flight.  w stays in registers
// for the whole block.  Channel sums are xor-butterflies inside the 16-lane group: every lane of the group ends with the
// same bits.
//
// Forward sums: each lane adds its pixels' contributions in pixel order, then block_sum_ordered (block_sum.h)
// -> partial[n, blockIdx.x].  No atomics: bit-reproducible; the caller sums each row and divides by HW.
//
// 1/n_k is formed once per pixel (IEEE division) and multiplied in: one rounding more per element than the composite's
// division.  Contraction is off in the kernels, products that should fuse say so (__builtin_fmaf): u0 - u1 is then an
// exact zero for equal inputs and (u0 - u1)^2 is symmetric in its arguments bit for bit.
//
// A pixel whose f_k is exactly zero: forward u_k = 0 (as the composite's 0 / eps); backward 0 * (0 / (0 * eps)) = NaN for
// that pixel's grad_fk, which is what autograd's composite gives (sqrt backward).  No other pixel sees it.
#include "block_sum.h"

namespace {

constexpr int LD_THREADS = 256;
constexpr int LD_GROUP = 16;                       // lanes per pixel
constexpr int LD_PIX = LD_THREADS / LD_GROUP;      // pixels per block and sub-step
constexpr int LD_MAX_BLOCKS_X = 1024;
constexpr int LD_WAVES_PER_SIMD = 4;               // 4 blocks per CU: at most 512 / 4 = 128 registers
static_assert(LD_THREADS == 4 * FMGAN_WAVE, "the block sum below adds four waves");

template <int C>
struct LdCfg {
  static_assert(C % 64 == 0 && C >= 64 && C <= 512, "16 lanes x float4 per 64 channels");
  static constexpr int T = C / 64;                 // float4 per lane, pixel and feature
  static constexpr int U = T >= 4 ? 1 : 4 / T;     // pixels per lane and step: at least 8 float4 loads in flight
};

__device__ __forceinline__ float ld_group_sum(float v) {
#pragma unroll
  for (int m = LD_GROUP / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, FMGAN_WAVE);
  return v;
}

template <int T>
__device__ __forceinline__ void ld_load(f32x4 (&v)[T], const float* __restrict__ p, bool valid) {
#pragma unroll
  for (int t = 0; t < T; ++t) v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (valid) {
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = *reinterpret_cast<const f32x4*>(p + 64 * t);
  }
}

template <int T>
__device__ __forceinline__ float ld_sumsq(const f32x4 (&v)[T]) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    s = __builtin_fmaf(v[t].x, v[t].x, s);
    s = __builtin_fmaf(v[t].y, v[t].y, s);
    s = __builtin_fmaf(v[t].z, v[t].z, s);
    s = __builtin_fmaf(v[t].w, v[t].w, s);
  }
  return s;
}

template <int C>
__global__ __launch_bounds__(LD_THREADS, LD_WAVES_PER_SIMD) void lpips_dist_fwd_f32(
    const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
    float* __restrict__ partial, int hw, float eps) {
#pragma clang fp contract(off)
  constexpr int T = LdCfg<C>::T, U = LdCfg<C>::U;
  __shared__ float red[LD_THREADS / FMGAN_WAVE];
  const int j = threadIdx.x & (LD_GROUP - 1), pg = threadIdx.x / LD_GROUP;
  // the sample's base is wave-uniform; a lane's element offset inside the sample fits 32 bits (hw * C < 2^30, checked
  // on the host): one register addresses both features
  const long long sample = (long long)blockIdx.y * hw * C;
  const float* __restrict__ a0 = f0 + sample;
  const float* __restrict__ b0 = f1 + sample;
  f32x4 wv[T];
#pragma unroll
  for (int t = 0; t < T; ++t) wv[t] = *reinterpret_cast<const f32x4*>(w + 4 * j + 64 * t);
  float acc = 0.f;
  const int step = gridDim.x * (LD_PIX * U);
  for (int base = blockIdx.x * (LD_PIX * U); base < hw; base += step) {
    f32x4 a[U][T], b[U][T];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = base + u * LD_PIX + pg;
      const unsigned off = (unsigned)p * C + 4 * j;
      ld_load<T>(a[u], a0 + off, p < hw);
      ld_load<T>(b[u], b0 + off, p < hw);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // a pixel past the end holds zeros: u0 = u1 = 0, its contribution is an exact 0
      const float i0 = 1.f / (sqrtf(ld_group_sum(ld_sumsq<T>(a[u]))) + eps);
      const float i1 = 1.f / (sqrtf(ld_group_sum(ld_sumsq<T>(b[u]))) + eps);
      float d = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const f32x4 e = a[u][t] * i0 - b[u][t] * i1;
        d = __builtin_fmaf(wv[t].x, e.x * e.x, d);
        d = __builtin_fmaf(wv[t].y, e.y * e.y, d);
        d = __builtin_fmaf(wv[t].z, e.z * e.z, d);
        d = __builtin_fmaf(wv[t].w, e.w * e.w, d);
      }
      acc += d;
    }
  }
  const float sum = block_sum_ordered<4>(acc, red);
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// G0 / G1: grad_f0 / grad_f1 is wanted (its pointer is not null).
template <int C, bool G0, bool G1>
__global__ __launch_bounds__(LD_THREADS, LD_WAVES_PER_SIMD) void lpips_dist_bwd_f32(
    const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
    const float* __restrict__ grad, float* __restrict__ grad_f0, float* __restrict__ grad_f1, int hw, float eps) {
#pragma clang fp contract(off)
  constexpr int T = LdCfg<C>::T, U = LdCfg<C>::U;
  const int j = threadIdx.x & (LD_GROUP - 1), pg = threadIdx.x / LD_GROUP;
  const long long sample = (long long)blockIdx.y * hw * C;      // wave-uniform; lane offsets are 32-bit, as above
  const float* __restrict__ a0 = f0 + sample;
  const float* __restrict__ b0 = f1 + sample;
  float* __restrict__ g0 = G0 ? grad_f0 + sample : nullptr;
  float* __restrict__ g1 = G1 ? grad_f1 + sample : nullptr;
  const float k = -2.f * (grad[blockIdx.y] / (float)hw);
  f32x4 wk[T];                                     // -2 w_c g[n] / HW
#pragma unroll
  for (int t = 0; t < T; ++t) wk[t] = *reinterpret_cast<const f32x4*>(w + 4 * j + 64 * t) * k;
  const int step = gridDim.x * (LD_PIX * U);
  for (int base = blockIdx.x * (LD_PIX * U); base < hw; base += step) {
    f32x4 a[U][T], b[U][T];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = base + u * LD_PIX + pg;
      const unsigned off = (unsigned)p * C + 4 * j;
      ld_load<T>(a[u], a0 + off, p < hw);
      ld_load<T>(b[u], b0 + off, p < hw);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = base + u * LD_PIX + pg;
      const float r0 = sqrtf(ld_group_sum(ld_sumsq<T>(a[u]))), r1 = sqrtf(ld_group_sum(ld_sumsq<T>(b[u])));
      const float n0 = r0 + eps, n1 = r1 + eps;
      const float i0 = 1.f / n0, i1 = 1.f / n1;
      float da = 0.f, db = 0.f;                    // sum_c q1_c f0_c, sum_c q1_c f1_c
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const f32x4 q = wk[t] * (a[u][t] * i0 - b[u][t] * i1);
        da = __builtin_fmaf(q.x, a[u][t].x, da);
        da = __builtin_fmaf(q.y, a[u][t].y, da);
        da = __builtin_fmaf(q.z, a[u][t].z, da);
        da = __builtin_fmaf(q.w, a[u][t].w, da);
        db = __builtin_fmaf(q.x, b[u][t].x, db);
        db = __builtin_fmaf(q.y, b[u][t].y, db);
        db = __builtin_fmaf(q.z, b[u][t].z, db);
        db = __builtin_fmaf(q.w, b[u][t].w, db);
      }
      // q0 = -q1: sum_c q0_c f0_c = -da.  0 / 0 = NaN for a zero-norm pixel, as autograd's composite
      const float c0 = -ld_group_sum(da) / (r0 * n0);
      const float c1 = ld_group_sum(db) / (r1 * n1);
      // q is formed again for the stores instead of being kept across the group sums (32 registers at C = 512), once per
      // wanted gradient.  The empty statement hides from the compiler that i0r, i1r are i0, i1 (it would keep the
      // earlier q, or a * i0 and b * i1, alive otherwise); repeated per float4 and ordered against the stores, it also
      // keeps the results from being formed all at once ahead of their stores.  Without it C = 512 takes 160 registers.
      float i0r = i0, i1r = i1;
      if (p < hw) {
        const unsigned off = (unsigned)p * C + 4 * j;
        if constexpr (G1) {
#pragma unroll
          for (int t = 0; t < T; ++t) {
            asm volatile("" : "+v"(i0r), "+v"(i1r) : : "memory");
            const f32x4 q = wk[t] * (a[u][t] * i0r - b[u][t] * i1r);
            *reinterpret_cast<f32x4*>(g1 + off + 64 * t) = (q - b[u][t] * c1) * i1r;
          }
        }
        if constexpr (G0) {
#pragma unroll
          for (int t = 0; t < T; ++t) {
            asm volatile("" : "+v"(i0r), "+v"(i1r) : : "memory");
            const f32x4 q = wk[t] * (a[u][t] * i0r - b[u][t] * i1r);
            *reinterpret_cast<f32x4*>(g0 + off + 64 * t) = (-q - a[u][t] * c0) * i0r;
          }
        }
      }
    }
  }
}

bool ld_served(int channels) { return channels == 64 || channels == 128 || channels == 256 || channels == 512; }

int ld_pixels_per_step(int channels) {
  static_assert(LdCfg<256>::U == 1 && LdCfg<512>::U == 1, "the wide taps take one pixel per lane and step");
  return LD_PIX * (channels == 64 ? LdCfg<64>::U : channels == 128 ? LdCfg<128>::U : 1);
}

// Status shared by the two launches, in the order the header states.
int ld_status(bool null_ptr, int batch, int channels, int hw, uintptr_t addr_or) {
  if (batch == 0) return FMGAN_OK;
  if (null_ptr || batch < 0 || channels <= 0 || hw <= 0) return FMGAN_EINVAL;
  // grid.y; 32-bit element offsets inside a sample (the pixel index may run one grid step past hw)
  if (batch > 65535 || (long long)hw * channels >= (1LL << 30)) return FMGAN_EOVERFLOW;
  if (!ld_served(channels) || (addr_or & 15) != 0) return FMGAN_EUNSUPPORTED;
  return FMGAN_OK;
}

}  // namespace

extern "C" int fmgan_lpips_distance_blocks(int batch, int channels, int hw) {
  if (batch <= 0 || batch > 65535 || hw <= 0 || !ld_served(channels)) return 0;
  if ((long long)hw * channels >= (1LL << 30)) return 0;
  const int pix = ld_pixels_per_step(channels);
  return fmgan_stage_blocks(((long long)hw + pix - 1) / pix, batch, LD_MAX_BLOCKS_X);
}

extern "C" int fmgan_lpips_distance_f32(const float* f0, const float* f1, const float* w, float* partial, int batch,
                                        int channels, int hw, float eps, void* stream) {
  const int st = ld_status(!f0 || !f1 || !w || !partial, batch, channels, hw,
                           (uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)w);
  if (st != FMGAN_OK || batch == 0) return st;
  const dim3 grid(fmgan_lpips_distance_blocks(batch, channels, hw), batch), block(LD_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define LD_GO(C) hipLaunchKernelGGL((lpips_dist_fwd_f32<C>), grid, block, 0, s, f0, f1, w, partial, hw, eps)
  switch (channels) {
    case 64: LD_GO(64); break;
    case 128: LD_GO(128); break;
    case 256: LD_GO(256); break;
    default: LD_GO(512); break;
  }
#undef LD_GO
  return fmgan_check_launch();
}

extern "C" int fmgan_lpips_distance_backward_f32(const float* f0, const float* f1, const float* w, const float* grad,
                                                 float* grad_f0, float* grad_f1, int batch, int channels, int hw,
                                                 float eps, void* stream) {
  const int st = ld_status(!f0 || !f1 || !w || !grad || (!grad_f0 && !grad_f1), batch, channels, hw,
                           (uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)w | (uintptr_t)grad_f0 | (uintptr_t)grad_f1);
  if (st != FMGAN_OK || batch == 0) return st;
  const dim3 grid(fmgan_lpips_distance_blocks(batch, channels, hw), batch), block(LD_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define LD_GO_G(C, G0, G1) \
  hipLaunchKernelGGL((lpips_dist_bwd_f32<C, G0, G1>), grid, block, 0, s, f0, f1, w, grad, grad_f0, grad_f1, hw, eps)
#define LD_GO(C)                                   \
  do {                                             \
    if (grad_f0 && grad_f1) LD_GO_G(C, true, true); \
    else if (grad_f1) LD_GO_G(C, false, true);     \
    else LD_GO_G(C, true, false);                  \
  } while (0)
  switch (channels) {
    case 64: LD_GO(64); break;
    case 128: LD_GO(128); break;
    case 256: LD_GO(256); break;
    default: LD_GO(512); break;
  }
#undef LD_GO
#undef LD_GO_G
  return fmgan_check_launch();
}
