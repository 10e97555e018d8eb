// Winograd F(2x2, 3x3) transforms for the plain 3x3 modulated conv (stride 1, pad 1) — fp32.
//
// Same operator as fmgan_modconv2d_f32 mode 0 (/root/reference/stylegan2.py:250-298, restated input-modulated):
//     out[b,o,y,x] = demod[b,o] * sum_{i,ky,kx} (scale*W[o,i,ky,kx]) * (style[b,i] * in[b,i,y+ky-1,x+kx-1])   (+ fused epilogue)
// as  Y = At [ (G g Gt) . (Bt d B) ] A  per 2x2 output tile (Lavin & Gray): 16 products per tile instead of 36, i.e. 2.25x fewer
// MACs on layers whose direct form already runs at 0.84-0.88 of the fp32 matrix peak (32^2..128^2, 256-512 channels).
// Three steps, the middle one a plain batched GEMM the caller hands to the BLAS library (torch.bmm -> hipBLASLt, fp32):
//     fmgan_wino_weight_f32:  U[xi][o][i]        = (G g Gt)[xi]  of the scaled weight                    [16, cout, cin]
//     fmgan_wino_input_f32:   V[xi][i][b*T + t]  = (Bt (style[b,i] * d) B)[xi] of tile t's 4x4 input window  [16, cin, B*T]
//     (caller)                M[xi]              = U[xi] @ V[xi]                                        [16, cout, B*T]
//     fmgan_wino_output_f32:  out tile           = epilogue( demod * At M A )                             [B, cout, H, W]
// HBM-bound: the input transform writes 4x the input, the output transform reads 4x the output; measured against copies of
// those bytes plus the 16 GEMMs (profiles/r03_winograd.md) the form pays at 32^2..128^2 and not at 256^2 and above.
// Each activation transform has two kernels with the same arithmetic: one thread per strip of four tiles, 16 bytes per lane
// (the planes of the Generator; within 0.9-1.3x of a copy of the bytes, profiles/winograd_transforms.md), and one thread per
// tile for odd tile counts and unaligned tensors; fmgan_wino_select reports the choice.  Inside a Generator forward U comes
// from the live-weight refresh (live_weights.hip, same arithmetic: winograd_weight.h) and fmgan_wino_weight_f32 is not launched.
// The sums are re-associated: results differ from the direct kernel by fp32 rounding (the GPU tests hold it to the
// direct kernel's tolerance against the CPU restatement of the reference).  T = (H/2) * (W/2) tiles per sample, H and W even.
#include "common.h"
#include "winograd_weight.h"

namespace {

// A block owns 16 input x 16 output channels, one pair per thread: the nine taps are read with o fastest over the lanes
// (64-byte runs of wt[i][tap][o]) into LDS and transformed with i fastest (64-byte runs of U[xi][o][i]); blocks stride over
// the tiles.  (32 x 32 tiles, 128-byte runs, leave a 256 x 256 weight with 64 blocks for 256 CUs: twice the time.)
constexpr int WW_T = 16;

__global__ __launch_bounds__(256) void wino_weight_f32(const float* __restrict__ wt, float* __restrict__ u, int cin, int cout) {
  __shared__ float taps[9][WW_T][WW_T + 1];
  const int i_tiles = (cin + WW_T - 1) / WW_T, o_tiles = (cout + WW_T - 1) / WW_T;
  const long long tiles = (long long)i_tiles * o_tiles;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int i0 = (int)(tile % i_tiles) * WW_T, o0 = (int)(tile / i_tiles) * WW_T;
    for (int idx = threadIdx.x; idx < 9 * WW_T * WW_T; idx += 256) {
      const int ol = idx % WW_T, r = idx / WW_T, il = r / 9, t = r - il * 9;
      if (i0 + il < cin && o0 + ol < cout) taps[t][il][ol] = wt[((long long)(i0 + il) * 9 + t) * cout + o0 + ol];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < WW_T * WW_T; idx += 256) {
      const int il = idx % WW_T, ol = idx / WW_T;
      if (i0 + il < cin && o0 + ol < cout) {
        float g[3][3], uu[16];
#pragma unroll
        for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = taps[t][il][ol];
        wino_weight_transform(g, uu);
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) u[((long long)xi * cout + o0 + ol) * cin + i0 + il] = uu[xi];
      }
    }
    __syncthreads();
  }
}

// one thread per (sample, channel, tile): 16 loads of the zero-padded 4x4 window, 32 adds, 16 coalesced stores
__global__ __launch_bounds__(256) void wino_input_f32(const float* __restrict__ x, const float* __restrict__ style,
                                                      float* __restrict__ v, int batch, int c, int h, int w) {
  const int tw = w >> 1, th = h >> 1, T = tw * th;
  const long long n_cols = (long long)batch * T, total = n_cols * c;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(idx % T);
    const int ch = (int)((idx / T) % c);
    const int b = (int)(idx / ((long long)T * c));
    const int ty = t / tw, tx = t - ty * tw;
    const float* xp = x + ((long long)b * c + ch) * h * w;
    const float s = style[(long long)b * c + ch];
    float d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = 2 * ty - 1 + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xx = 2 * tx - 1 + q;
        d[r][q] = (y >= 0 && y < h && xx >= 0 && xx < w) ? xp[(long long)y * w + xx] * s : 0.f;
      }
    }
    // Bt d B,  Bt = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
    float e[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      e[r][0] = d[r][0] - d[r][2]; e[r][1] = d[r][1] + d[r][2]; e[r][2] = d[r][2] - d[r][1]; e[r][3] = d[r][1] - d[r][3];
    }
    const long long col = (long long)b * T + t;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v0 = e[0][q] - e[2][q], v1 = e[1][q] + e[2][q], v2 = e[2][q] - e[1][q], v3 = e[1][q] - e[3][q];
      v[((long long)(0 * 4 + q) * c + ch) * n_cols + col] = v0;
      v[((long long)(1 * 4 + q) * c + ch) * n_cols + col] = v1;
      v[((long long)(2 * 4 + q) * c + ch) * n_cols + col] = v2;
      v[((long long)(3 * 4 + q) * c + ch) * n_cols + col] = v3;
    }
  }
}

// one thread per (sample, output channel, tile): 16 coalesced loads, At M A, the StyledConv epilogue, two 8-byte stores
__global__ __launch_bounds__(256) void wino_output_f32(const float* __restrict__ m, const float* __restrict__ demod,
                                                       const float* __restrict__ noise, const float* __restrict__ noise_weight,
                                                       const float* __restrict__ bias, float* __restrict__ out, int batch,
                                                       int cout, int h, int w, int noise_batch, int fuse_act, float alpha,
                                                       float act_scale) {
  const int tw = w >> 1, th = h >> 1, T = tw * th;
  const long long n_cols = (long long)batch * T, total = n_cols * cout;
  const float nw = (fuse_act && noise && noise_weight) ? noise_weight[0] : 0.f;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(idx % T);
    const int o = (int)((idx / T) % cout);
    const int b = (int)(idx / ((long long)T * cout));
    const int ty = t / tw, tx = t - ty * tw;
    const long long col = (long long)b * T + t;
    float mm[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q) mm[a][q] = m[((long long)(a * 4 + q) * cout + o) * n_cols + col];
    // At M A,  At = [1 1 1 0; 0 1 -1 -1]
    float z[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      z[0][q] = mm[0][q] + mm[1][q] + mm[2][q];
      z[1][q] = mm[1][q] - mm[2][q] - mm[3][q];
    }
    const float dm = demod ? demod[(long long)b * cout + o] : 1.f;
    const float bv = (fuse_act && bias) ? bias[o] : 0.f;
    float* op = out + (((long long)b * cout + o) * h + 2 * ty) * w + 2 * tx;
    const float* np = (fuse_act && noise) ? noise + ((long long)(noise_batch == 1 ? 0 : b) * h + 2 * ty) * w + 2 * tx : nullptr;
#pragma unroll
    for (int jy = 0; jy < 2; ++jy) {
      float y0 = (z[jy][0] + z[jy][1] + z[jy][2]) * dm, y1 = (z[jy][1] - z[jy][2] - z[jy][3]) * dm;
      if (fuse_act) {
        const float n0 = np ? __fmul_rn(nw, np[jy * w]) : 0.f, n1 = np ? __fmul_rn(nw, np[jy * w + 1]) : 0.f;
        y0 = __fadd_rn(__fadd_rn(y0, n0), bv);
        y1 = __fadd_rn(__fadd_rn(y1, n1), bv);
        y0 = (y0 > 0.f ? y0 : y0 * alpha) * act_scale;
        y1 = (y1 > 0.f ? y1 : y1 * alpha) * act_scale;
      }
      f32x2_u st; st.x = y0; st.y = y1;
      *reinterpret_cast<f32x2_u*>(op + (long long)jy * w) = st;
    }
  }
}

// ---------------------------------------------------------------------------------------------- strips of four tiles
// The same two transforms with one thread per (sample, channel, tile row, strip of four horizontally adjacent tiles): every
// access to V, M, out and the noise plane is one 16-byte access per lane, and the 4 x 10 input window of a strip is two aligned
// 16-byte loads and the two edge columns per row instead of sixteen 4-byte loads at an 8-byte lane stride.  The strips of a
// tile row, and the tile rows of a plane, are neighbours in the work index, so the rows that two tile rows share and the edge
// columns that two strips share are fetched by the same block and served from its vector cache.  Each element goes through
// the very expressions of the kernels above, in their order: the results are the same bits.
// Needs (w/2) % 4 == 0 and 16-byte aligned base pointers: rows of x / out / noise then start every strip on a 16-byte
// boundary, and T = (h/2)(w/2) is a multiple of 4, so every row of V / M and every sample's first column is one as well.

// rows outside the plane read a row inside it and are zeroed by the select: no lane leaves the plane's storage
__global__ __launch_bounds__(256) void wino_input_strip_f32(const float* __restrict__ x, const float* __restrict__ style,
                                                            float* __restrict__ v, int batch, int c, int h, int w) {
  const int tw = w >> 1, th = h >> 1, T = tw * th, sw = tw >> 2;
  const long long n_cols = (long long)batch * T, total = (long long)batch * c * th * sw;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int sx = (int)(idx % sw);
    const int ty = (int)((idx / sw) % th);
    const int ch = (int)((idx / ((long long)sw * th)) % c);
    const int b = (int)(idx / ((long long)sw * th * c));
    const int x0 = 8 * sx;
    const bool left = x0 > 0, right = x0 + 8 < w;
    const float* xp = x + ((long long)b * c + ch) * h * w + x0;
    const float s = style[(long long)b * c + ch];
    float e[4][4][4];      // [window row][tile of the strip][q]: d B
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = 2 * ty - 1 + r;
      const bool in = y >= 0 && y < h;
      const float* row = xp + (long long)(in ? y : 0) * w;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(row), hi = *reinterpret_cast<const f32x4*>(row + 4);
      const float raw[10] = {row[left ? -1 : 0], lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w, row[right ? 8 : 7]};
      float d[10];
#pragma unroll
      for (int q = 0; q < 10; ++q) {
        const bool ok = in && (q > 0 || left) && (q < 9 || right);
        d[q] = ok ? raw[q] * s : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        e[r][k][0] = d[2 * k] - d[2 * k + 2]; e[r][k][1] = d[2 * k + 1] + d[2 * k + 2];
        e[r][k][2] = d[2 * k + 2] - d[2 * k + 1]; e[r][k][3] = d[2 * k + 1] - d[2 * k + 3];
      }
    }
    const long long col = (long long)b * T + (long long)ty * tw + 4 * sx;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v0, v1, v2, v3;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v0[k] = e[0][k][q] - e[2][k][q]; v1[k] = e[1][k][q] + e[2][k][q];
        v2[k] = e[2][k][q] - e[1][k][q]; v3[k] = e[1][k][q] - e[3][k][q];
      }
      *reinterpret_cast<f32x4*>(v + ((long long)(0 * 4 + q) * c + ch) * n_cols + col) = v0;
      *reinterpret_cast<f32x4*>(v + ((long long)(1 * 4 + q) * c + ch) * n_cols + col) = v1;
      *reinterpret_cast<f32x4*>(v + ((long long)(2 * 4 + q) * c + ch) * n_cols + col) = v2;
      *reinterpret_cast<f32x4*>(v + ((long long)(3 * 4 + q) * c + ch) * n_cols + col) = v3;
    }
  }
}

__global__ __launch_bounds__(256) void wino_output_strip_f32(const float* __restrict__ m, const float* __restrict__ demod,
                                                             const float* __restrict__ noise,
                                                             const float* __restrict__ noise_weight,
                                                             const float* __restrict__ bias, float* __restrict__ out, int batch,
                                                             int cout, int h, int w, int noise_batch, int fuse_act, float alpha,
                                                             float act_scale) {
  const int tw = w >> 1, th = h >> 1, T = tw * th, sw = tw >> 2;
  const long long n_cols = (long long)batch * T, total = (long long)batch * cout * th * sw;
  const float nw = (fuse_act && noise && noise_weight) ? noise_weight[0] : 0.f;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int sx = (int)(idx % sw);
    const int ty = (int)((idx / sw) % th);
    const int o = (int)((idx / ((long long)sw * th)) % cout);
    const int b = (int)(idx / ((long long)sw * th * cout));
    const long long col = (long long)b * T + (long long)ty * tw + 4 * sx;
    f32x4 mm[4][4];        // [a][q], one lane of the vector per tile of the strip
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q) mm[a][q] = *reinterpret_cast<const f32x4*>(m + ((long long)(a * 4 + q) * cout + o) * n_cols + col);
    const float dm = demod ? demod[(long long)b * cout + o] : 1.f;
    const float bv = (fuse_act && bias) ? bias[o] : 0.f;
    float* op = out + (((long long)b * cout + o) * h + 2 * ty) * w + 8 * sx;
    const float* np = (fuse_act && noise) ? noise + ((long long)(noise_batch == 1 ? 0 : b) * h + 2 * ty) * w + 8 * sx : nullptr;
#pragma unroll
    for (int jy = 0; jy < 2; ++jy) {
      float nz[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (fuse_act && np) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(np + (long long)jy * w);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(np + (long long)jy * w + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { nz[k] = __fmul_rn(nw, lo[k]); nz[4 + k] = __fmul_rn(nw, hi[k]); }
      }
      float y[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float z[4];        // row jy of At M, tile k
#pragma unroll
        for (int q = 0; q < 4; ++q)
          z[q] = jy == 0 ? mm[0][q][k] + mm[1][q][k] + mm[2][q][k] : mm[1][q][k] - mm[2][q][k] - mm[3][q][k];
        float y0 = (z[0] + z[1] + z[2]) * dm, y1 = (z[1] - z[2] - z[3]) * dm;
        if (fuse_act) {
          y0 = __fadd_rn(__fadd_rn(y0, nz[2 * k]), bv);
          y1 = __fadd_rn(__fadd_rn(y1, nz[2 * k + 1]), bv);
          y0 = (y0 > 0.f ? y0 : y0 * alpha) * act_scale;
          y1 = (y1 > 0.f ? y1 : y1 * alpha) * act_scale;
        }
        y[2 * k] = y0; y[2 * k + 1] = y1;
      }
      const f32x4 s0 = {y[0], y[1], y[2], y[3]}, s1 = {y[4], y[5], y[6], y[7]};
      *reinterpret_cast<f32x4*>(op + (long long)jy * w) = s0;
      *reinterpret_cast<f32x4*>(op + (long long)jy * w + 4) = s1;
    }
  }
}

// `tiles` 2x2 tiles in trips of at most num_CU * 32 blocks' worth; a thread takes per_thread of them
inline unsigned wino_grid(long long tiles, int per_thread = 1) {
  long long blocks = (tiles / per_thread + 255) / 256;
  const long long cap = (long long)FMGAN_NUM_CU * 32 / per_thread;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 1: the strip kernel, 0: one tile per thread.  The output transform keeps the tile kernel on rows of fewer than 32 floats:
// a strip lane stores 32 bytes of a row, so on 64-byte rows a store instruction covers every other 16 bytes of every other
// row, and the 8-byte stores of the tile kernel, contiguous over the lanes, measured faster (profiles/winograd_transforms.md).
inline int wino_kernel(bool output, int w, bool all_aligned16) {
  return ((w >> 1) & 3) == 0 && all_aligned16 && !(output && w < 32) ? 1 : 0;
}

inline int wino_sizes(int batch, int c, int h, int w) {
  return (batch < 0 || c <= 0 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) ? FMGAN_EINVAL : FMGAN_OK;
}

}  // namespace

extern "C" int fmgan_wino_select(int output, int batch, int c, int h, int w, int all_aligned16) {
  const int st = wino_sizes(batch, c, h, w);
  return st != FMGAN_OK ? st : wino_kernel(output != 0, w, all_aligned16 != 0);
}

extern "C" int fmgan_wino_weight_f32(const float* wt, float* u, int cin, int cout, void* stream) {
  if (cin <= 0 || cout <= 0) return FMGAN_EINVAL;
  if (!wt || !u) return FMGAN_EINVAL;
  long long blocks = (long long)((cin + WW_T - 1) / WW_T) * ((cout + WW_T - 1) / WW_T);
  if (blocks > (long long)FMGAN_NUM_CU * 32) blocks = (long long)FMGAN_NUM_CU * 32;
  hipLaunchKernelGGL(wino_weight_f32, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, wt, u, cin, cout);
  return fmgan_check_launch();
}

extern "C" int fmgan_wino_input_f32(const float* x, const float* style, float* v, int batch, int c, int h, int w, void* stream) {
  if (wino_sizes(batch, c, h, w) != FMGAN_OK) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!x || !style || !v) return FMGAN_EINVAL;
  const long long tiles = (long long)batch * c * (h / 2) * (w / 2);
  if (wino_kernel(false, w, aligned16(x) && aligned16(v)))
    hipLaunchKernelGGL(wino_input_strip_f32, dim3(wino_grid(tiles, 4)), dim3(256), 0, (hipStream_t)stream, x, style, v, batch, c,
                       h, w);
  else
    hipLaunchKernelGGL(wino_input_f32, dim3(wino_grid(tiles)), dim3(256), 0, (hipStream_t)stream, x, style, v, batch, c, h, w);
  return fmgan_check_launch();
}

extern "C" int fmgan_wino_output_f32(const float* m, const float* demod, const float* noise, const float* noise_weight,
                                     const float* bias, float* out, int batch, int cout, int h, int w, int noise_batch,
                                     int fuse_act, float alpha, float act_scale, void* stream) {
  if (wino_sizes(batch, cout, h, w) != FMGAN_OK) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!m || !out) return FMGAN_EINVAL;
  if (fuse_act && noise && noise_batch != 1 && noise_batch != batch) return FMGAN_EINVAL;
  const long long tiles = (long long)batch * cout * (h / 2) * (w / 2);
  if (wino_kernel(true, w, aligned16(m) && aligned16(out) && (!(fuse_act && noise) || aligned16(noise))))
    hipLaunchKernelGGL(wino_output_strip_f32, dim3(wino_grid(tiles, 4)), dim3(256), 0, (hipStream_t)stream, m, demod, noise,
                       noise_weight, bias, out, batch, cout, h, w, noise_batch, fuse_act, alpha, act_scale);
  else
    hipLaunchKernelGGL(wino_output_f32, dim3(wino_grid(tiles)), dim3(256), 0, (hipStream_t)stream, m, demod, noise, noise_weight,
                       bias, out, batch, cout, h, w, noise_batch, fuse_act, alpha, act_scale);
  return fmgan_check_launch();
}
