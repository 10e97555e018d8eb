// Per-batch metric stage of the quantitative evaluation (reference Evaluation/quant_eval.py:25-49, 100) for gfx950:
// the face-recognition network's input of one or two image batches and the per-sample L1 between them, in one pass.
//
//   gray[b,0,oy,ox] = (1/k^2) * sum_{window} g(y,x),   g = (c0*x0 + c1*x1) + c2*x2          (RGB_to_GrayScale followed by
//                                                       avg_pool2d(k, k), Util/training_util.py:130-161)
//   l1[b]           = sum_{c,y,x} |a - b| / (3*H*W)     (torch.mean(torch.abs(a - b), dim=(1,2,3)), quant_eval.py:100)
//
// The composite spends ~22 elementwise launches on an (output, photo) pair; here every element of a and b is read once.
//
// Arithmetic of g, fixed so that the result does not depend on the machine: the three products are rounded separately
// in fp32 (coefficients float(0.2989), float(0.587), float(0.114)), then added left to right; no fused multiply-add (the
// library is built with -ffp-contract=on: contraction is switched off in fi_gray below).  A window's sum is serial and
// starts from 0: rows top to bottom, columns left to right within a row; the factor 1/k^2 is a power of two (exact).
//
// Mapping: a lane owns one unit = k rows x CS columns of one sample, CS = max(4, k): 4 windows at k = 1, 2 at k = 2,
// one at k = 4 and 8, so a window is never shared between lanes and each row of a unit is one or two 16-byte loads per
// channel.  Lanes of a wave own consecutive units of a row: their loads cover consecutive 16- or 32-byte pieces.
// grid.x = batch * (blocks per sample, fmgan_face_input_blocks); one unit per lane, no grid-stride loop.
// The scalar form (misaligned pointers or W % 4 != 0) walks the same units with bounded scalar loads (0 past the end
// of a row: such columns belong to no window, and |0 - 0| adds +0 to the L1 sum), so it performs the same arithmetic in
// the same order: both forms give identical bits.
//
// L1 partial sums, fixed order, no atomics: a row of a unit is summed serially from 0 (channel 0..2, then column:
// 3*CS <= 24 terms), the k <= 8 row sums are added serially, then block_sum_ordered of block_sum.h (butterfly: 6 steps,
// four waves: 2 steps) -> partial[b, block].  Longest serial chain: 24 + 8 + 6 + 2 = 40 additions, for every image size;
// all terms are non-negative, so the relative error of a partial is at most 40 * 2^-24 = 2.4e-6.
#include <climits>

#include "block_sum.h"

namespace {

constexpr int FI_THREADS = 256;
static_assert(FI_THREADS == 4 * FMGAN_WAVE, "the block sum below adds four waves");

// (c0*r + c1*g) + c2*b with three separately rounded products
__device__ __forceinline__ float fi_gray(float r, float g, float b) {
#pragma clang fp contract(off)
  const float p0 = 0.2989f * r;
  const float p1 = 0.587f * g;
  const float p2 = 0.114f * b;
  const float s = p0 + p1;
  return s + p2;
}

__device__ __forceinline__ float fi_abs_sum(float acc, f32x4 a, f32x4 b) {
  acc = acc + __builtin_fabsf(a.x - b.x);
  acc = acc + __builtin_fabsf(a.y - b.y);
  acc = acc + __builtin_fabsf(a.z - b.z);
  return acc + __builtin_fabsf(a.w - b.w);
}

// window sums of one image's row piece: columns 4q .. 4q+3 of the unit go to window (4q + j) / K
template <int K, int NW>
__device__ __forceinline__ void fi_add_row(float (&win)[NW], int q, f32x4 c0, f32x4 c1, f32x4 c2) {
  const float g[4] = {fi_gray(c0.x, c1.x, c2.x), fi_gray(c0.y, c1.y, c2.y), fi_gray(c0.z, c1.z, c2.z),
                      fi_gray(c0.w, c1.w, c2.w)};
#pragma unroll
  for (int j = 0; j < 4; ++j) win[(4 * q + j) / K] = win[(4 * q + j) / K] + g[j];
}

template <int K, int NW, bool VEC>
__device__ __forceinline__ void fi_store(float* __restrict__ gray, long long o, int ox, int ow, const float (&win)[NW]) {
  constexpr float inv = 1.f / (K * K);
  if constexpr (VEC && NW == 4) {
    const f32x4_u v = {win[0] * inv, win[1] * inv, win[2] * inv, win[3] * inv};
    *reinterpret_cast<f32x4_u*>(gray + o) = v;
  } else if constexpr (VEC && NW == 2) {
    const f32x2_u v = {win[0] * inv, win[1] * inv};
    *reinterpret_cast<f32x2_u*>(gray + o) = v;
  } else {
#pragma unroll
    for (int j = 0; j < NW; ++j)
      if (ox + j < ow) gray[o + j] = win[j] * inv;
  }
}

// PAIR: a second image b is read; gray_a / gray_b / partial may each be null (not wanted).
template <int K, bool VEC, bool PAIR>
__global__ __launch_bounds__(FI_THREADS) void face_input_f32(const float* __restrict__ a, const float* __restrict__ b,
                                                             float* __restrict__ gray_a, float* __restrict__ gray_b,
                                                             float* __restrict__ partial, int h, int w, int units_x,
                                                             int units, int gx) {
  constexpr int CS = K > 4 ? K : 4;      // columns of a unit
  constexpr int NW = CS / K;             // windows of a unit
  constexpr int ROWS = K > 4 ? (VEC ? 2 : 1) : K;
  __shared__ float red[FI_THREADS / FMGAN_WAVE];
  const int sample = blockIdx.x / gx, blk = blockIdx.x % gx;
  const int u = blk * FI_THREADS + threadIdx.x;
  const long long hw = (long long)h * w;
  float l1 = 0.f;
  if (u < units) {
    const int oy = u / units_x, x0 = (u % units_x) * CS;
    const int ow = w / K, ox = x0 / K;
    const float* pa = a + (long long)sample * 3 * hw + (long long)oy * K * w;
    const float* pb = PAIR ? b + (long long)sample * 3 * hw + (long long)oy * K * w : nullptr;
    float wa[NW], wb[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) wa[j] = wb[j] = 0.f;
    // rows in flight: all of them up to k = 4; at k = 8 two (24 16-byte loads of a pair) or, in the scalar form, one: the
    // full unroll takes 459 registers
#pragma unroll ROWS
    for (int r = 0; r < K; ++r) {
      const float* ra = pa + (long long)r * w;
      const float* rb = PAIR ? pb + (long long)r * w : nullptr;
      f32x4 va[3][CS / 4], vb[3][CS / 4];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < CS / 4; ++q) {
          va[c][q] = load4<VEC>(ra + c * hw, x0 + 4 * q, w);
          if constexpr (PAIR) vb[c][q] = load4<VEC>(rb + c * hw, x0 + 4 * q, w);
        }
#pragma unroll
      for (int q = 0; q < CS / 4; ++q) {
        fi_add_row<K, NW>(wa, q, va[0][q], va[1][q], va[2][q]);
        if constexpr (PAIR) fi_add_row<K, NW>(wb, q, vb[0][q], vb[1][q], vb[2][q]);
      }
      if constexpr (PAIR) {
        float row = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < CS / 4; ++q) row = fi_abs_sum(row, va[c][q], vb[c][q]);
        l1 = l1 + row;
      }
    }
    const long long o = (long long)sample * (h / K) * ow + (long long)oy * ow + ox;
    if (gray_a) fi_store<K, NW, VEC>(gray_a, o, ox, ow, wa);
    if constexpr (PAIR)
      if (gray_b) fi_store<K, NW, VEC>(gray_b, o, ox, ow, wb);
  }
  if constexpr (PAIR) {
    if (partial) {                                             // uniform over the grid
      const float sum = block_sum_ordered<4>(l1, red);
      if (threadIdx.x == 0) partial[(long long)sample * gx + blk] = sum;
    }
  }
}

// Units and blocks of one call; FMGAN_OK or an FMGAN_E* status.
struct FiShape {
  int units_x, units, gx;
};

int fi_shape(int batch, int h, int w, int k, FiShape* sh) {
  if (batch <= 0 || h <= 0 || w <= 0) return FMGAN_EINVAL;
  if (!(k == 1 || k == 2 || k == 4 || k == 8) || h % k != 0 || w % k != 0) return FMGAN_EUNSUPPORTED;
  // element offsets are long long; unit and block indices are ints
  const long long hw = (long long)h * w;
  if (3 * hw > LLONG_MAX / batch) return FMGAN_EOVERFLOW;
  if (hw > 0x7fffffffLL - FI_THREADS) return FMGAN_EOVERFLOW;
  const int cs = k > 4 ? k : 4;
  sh->units_x = (w + cs - 1) / cs;
  sh->units = (h / k) * sh->units_x;
  sh->gx = (sh->units + FI_THREADS - 1) / FI_THREADS;
  if ((long long)sh->gx * batch > 0x7fffffffLL) return FMGAN_EOVERFLOW;     // grid.x
  return FMGAN_OK;
}

}  // namespace

extern "C" int fmgan_face_input_blocks(int batch, int h, int w, int k) {
  FiShape sh;
  return fi_shape(batch, h, w, k, &sh) == FMGAN_OK ? sh.gx : 0;
}

extern "C" int fmgan_face_input_f32(const float* a, const float* b, float* gray_a, float* gray_b, float* l1_partial,
                                    int batch, int h, int w, int k, void* stream) {
  if (!a || (!gray_a && !gray_b && !l1_partial) || (!b && (gray_b || l1_partial))) return FMGAN_EINVAL;
  FiShape sh;
  const int st = fi_shape(batch, h, w, k, &sh);
  if (st != FMGAN_OK) return st;
  // a second image that feeds no output is not read
  if (!gray_b && !l1_partial) b = nullptr;
  const bool vec = (w & 3) == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
  const dim3 grid((unsigned)((long long)sh.gx * batch)), block(FI_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define FI_GO(K, VEC, PAIR)                                                                                       \
  hipLaunchKernelGGL((face_input_f32<K, VEC, PAIR>), grid, block, 0, s, a, b, gray_a, gray_b, l1_partial, h, w, \
                     sh.units_x, sh.units, sh.gx)
#define FI_K(K)                                        \
  do {                                                 \
    if (b) {                                           \
      if (vec) FI_GO(K, true, true); else FI_GO(K, false, true);   \
    } else {                                           \
      if (vec) FI_GO(K, true, false); else FI_GO(K, false, false); \
    }                                                  \
  } while (0)
  switch (k) {
    case 1: FI_K(1); break;
    case 2: FI_K(2); break;
    case 4: FI_K(4); break;
    default: FI_K(8); break;
  }
#undef FI_K
#undef FI_GO
  return fmgan_check_launch();
}
