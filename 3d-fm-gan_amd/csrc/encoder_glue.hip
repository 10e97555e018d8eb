// Inference glue of the pSp encoder's IR / IR-SE units (psp_encoder_model/encoders/helpers.py) for gfx950: everything
// between the MIOpen convolutions of a unit except the PReLU between its two 3x3 convolutions.
//
//   bn(v)    = (v - mean[c]) * (gamma[c] * (1 / sqrt(var[c] + eps))) + beta[c]        (eval-mode BatchNorm2d)
//   bn_prelu : y = prelu(bn(x), slope[c]);  optional y_next = bn_next(y);  optional y_sub = y[:, ::s, ::s]
//   se_pool  : partial[b, k, c] = sum of r[b, rows of chunk k, :, c]
//   se_gate  : gate[b, :] = sigmoid(fc2 . relu(fc1 . bn_out(sum_k partial[b, k, :] / HW)))
//   ir_tail  : out = bn_out(r) * gate[b, c] + shortcut;  optional out_next = bn_next(out)
//              shortcut = x_in[b, s*h, s*w, c]  (MaxPool2d(1, s), read in place)  or  bn_sc(conv1x1 output)
//
// Layout: fp32, NHWC storage ([B, H, W, C], C % 4 == 0), one float4 of four channels per lane and access.  The
// per-channel BatchNorm constants are formed from the module's four vectors at the start of every block and kept in
// LDS as (mean, gamma / sqrt(var + eps), beta): nothing is cached between launches.
//
// Elementwise kernels: a work item is 1024 float4 (4 per lane, all loads issued before the first use) of one output
// row (b, h); blocks walk the items grid-stride.  An item's row index and a lane's offset inside the row are 32-bit
// (checked on the host), the row's base is a 64-bit element offset.
//
// Reductions: no atomics.  se_pool: lane (p, q) adds the pixels p, p + P, ... of its chunk in order, then the P
// pixel-lanes are added in order.  se_gate: contiguous runs of chunks in order, then the runs in order; fc1 rows as
// lane-strided sums and an xor butterfly; fc2 rows in order.  Two runs give the same bits.
#include "common.h"

namespace {

constexpr int EG_THREADS = 256;
constexpr int EG_ITEM = 4;                         // float4 per lane and work item
constexpr int EG_SEG = EG_THREADS * EG_ITEM;       // float4 per work item
constexpr int EG_MAX_C = 1024;                     // LDS tables: 3 floats per channel and BatchNorm
constexpr int EG_MAX_MID = 256;                    // se_gate: hidden width kept in LDS
constexpr int EG_GATE_THREADS = 1024;              // se_gate: one thread per channel at the widest served layer
constexpr int EG_GATE_BATCH = 8;                   // se_gate: loads in flight per lane
constexpr int EG_BLOCKS_PER_CU = 8;
static_assert(EG_MAX_C <= EG_GATE_THREADS, "se_gate: a thread per channel");
constexpr int EG_POOL_MIN_PIX = 16;                // se_pool: pixels per chunk, at least one per pixel-lane at C = 64

struct EgBn {                                      // one BatchNorm2d in eval mode; mean == nullptr: absent
  const float* mean;
  const float* var;
  const float* gamma;
  const float* beta;
  float eps;
};

// (mean, k, beta) of channel c at tab[c], tab[C + c], tab[2C + c]
__device__ __forceinline__ void eg_bn_table(float* tab, const EgBn& bn, int C) {
  for (int c = threadIdx.x; c < C; c += EG_THREADS) {
    tab[c] = bn.mean[c];
    tab[C + c] = bn.gamma[c] * (1.f / sqrtf(bn.var[c] + bn.eps));
    tab[2 * C + c] = bn.beta[c];
  }
}

__device__ __forceinline__ f32x4 eg_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void eg_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__device__ __forceinline__ f32x4 eg_bn(const float* tab, int C, int c, f32x4 v) {
  return (v - eg_ld4(tab + c)) * eg_ld4(tab + C + c) + eg_ld4(tab + 2 * C + c);
}

__device__ __forceinline__ float eg_bn1(const EgBn& bn, int c, float v) {
  return (v - bn.mean[c]) * (bn.gamma[c] * (1.f / sqrtf(bn.var[c] + bn.eps))) + bn.beta[c];
}

// x [B,H,W,C] -> y, y_next like x (either may be null), y_sub [B,Ho,Wo,C] (null: not wanted), Ho = (H-1)/s + 1.
__global__ __launch_bounds__(EG_THREADS) void eg_bn_prelu_f32(
    const float* __restrict__ x, EgBn bn, const float* __restrict__ slope, float* __restrict__ y, EgBn bn_next,
    float* __restrict__ y_next, float* __restrict__ y_sub, int rows, int H, int W, int C, int s, int nseg) {
  extern __shared__ __attribute__((aligned(16))) float tab[];                   // bn (3C), slope (C), bn_next (3C)
  float* const tab_slope = tab + 3 * C;
  float* const tab_next = tab + 4 * C;
  eg_bn_table(tab, bn, C);
  for (int c = threadIdx.x; c < C; c += EG_THREADS) tab_slope[c] = slope[c];
  if (y_next) eg_bn_table(tab_next, bn_next, C);
  __syncthreads();
  const unsigned C4 = C / 4, row4 = (unsigned)W * C4;
  const int Ho = y_sub ? (H - 1) / s + 1 : 0, Wo = y_sub ? (W - 1) / s + 1 : 0;
  const int items = rows * nseg;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int row = item / nseg, seg = item - row * nseg;
    const long long base = (long long)row * W * C;
    const int b = row / H, h = row - b * H;
    const bool sub_row = y_sub && h % s == 0;
    const long long sub_base = sub_row ? ((long long)b * Ho + h / s) * Wo * C : 0;
    f32x4 v[EG_ITEM];
#pragma unroll
    for (int k = 0; k < EG_ITEM; ++k) {
      const unsigned j = (unsigned)seg * EG_SEG + k * EG_THREADS + threadIdx.x;
      if (j < row4) v[k] = eg_ld4(x + base + 4ll * j);
    }
#pragma unroll
    for (int k = 0; k < EG_ITEM; ++k) {
      const unsigned j = (unsigned)seg * EG_SEG + k * EG_THREADS + threadIdx.x;
      if (j >= row4) continue;
      const unsigned w = j / C4;
      const int c = 4 * (int)(j - w * C4);
      const f32x4 t = eg_bn(tab, C, c, v[k]), a = eg_ld4(tab_slope + c);
      f32x4 o;
      o.x = t.x > 0.f ? t.x : a.x * t.x;
      o.y = t.y > 0.f ? t.y : a.y * t.y;
      o.z = t.z > 0.f ? t.z : a.z * t.z;
      o.w = t.w > 0.f ? t.w : a.w * t.w;
      if (y) eg_st4(y + base + 4ll * j, o);
      if (y_next) eg_st4(y_next + base + 4ll * j, eg_bn(tab_next, C, c, o));
      if (sub_row && w % s == 0) eg_st4(y_sub + sub_base + (long long)(w / s) * C + c, o);
    }
  }
}

// r, out, out_next [B,H,W,C]; gate [B,C] or null.  SC_BN: sc [B,H,W,C] is the shortcut convolution's output and bn_sc
// is applied to it; otherwise sc [B,Hs,Ws,C] is the unit's input and pixel (s*h, s*w) is read.
template <bool SC_BN>
__global__ __launch_bounds__(EG_THREADS) void eg_ir_tail_f32(
    const float* __restrict__ r, EgBn bn, const float* __restrict__ gate, const float* __restrict__ sc, EgBn bn_sc,
    float* __restrict__ out, EgBn bn_next, float* __restrict__ out_next, int rows, int H, int W, int C, int Hs, int Ws,
    int s, int nseg) {
  extern __shared__ __attribute__((aligned(16))) float tab[];                   // bn (3C), bn_sc (3C), bn_next (3C)
  float* const tab_sc = tab + 3 * C;
  float* const tab_next = tab + 6 * C;
  eg_bn_table(tab, bn, C);
  if (SC_BN) eg_bn_table(tab_sc, bn_sc, C);
  if (out_next) eg_bn_table(tab_next, bn_next, C);
  __syncthreads();
  const unsigned C4 = C / 4, row4 = (unsigned)W * C4;
  const int items = rows * nseg;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int row = item / nseg, seg = item - row * nseg;
    const long long base = (long long)row * W * C;
    const int b = row / H, h = row - b * H;
    const long long sc_base = SC_BN ? base : ((long long)b * Hs + (long long)h * s) * Ws * C;
    const float* const g = gate ? gate + (long long)b * C : nullptr;
    f32x4 v[EG_ITEM], u[EG_ITEM];
#pragma unroll
    for (int k = 0; k < EG_ITEM; ++k) {
      const unsigned j = (unsigned)seg * EG_SEG + k * EG_THREADS + threadIdx.x;
      if (j < row4) {
        v[k] = eg_ld4(r + base + 4ll * j);
        if (SC_BN || s == 1) {
          u[k] = eg_ld4(sc + sc_base + 4ll * j);
        } else {
          const unsigned w = j / C4;
          u[k] = eg_ld4(sc + sc_base + (long long)w * s * C + 4 * (j - w * C4));
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EG_ITEM; ++k) {
      const unsigned j = (unsigned)seg * EG_SEG + k * EG_THREADS + threadIdx.x;
      if (j >= row4) continue;
      const int c = 4 * (int)(j % C4);
      f32x4 t = eg_bn(tab, C, c, v[k]);
      if (g) t = t * eg_ld4(g + c);
      const f32x4 o = t + (SC_BN ? eg_bn(tab_sc, C, c, u[k]) : u[k]);
      eg_st4(out + base + 4ll * j, o);
      if (out_next) eg_st4(out_next + base + 4ll * j, eg_bn(tab_next, C, c, o));
    }
  }
}

// block (chunk k, sample b): rows [k * rpc, min(H, (k + 1) * rpc)) of r[b]; P = EG_THREADS / C4 pixel-lanes (>= 1)
__global__ __launch_bounds__(EG_THREADS) void eg_se_pool_f32(const float* __restrict__ r, float* __restrict__ partial,
                                                             int H, int W, int C, int rpc, int P) {
  __shared__ f32x4 red[EG_THREADS];
  const int C4 = C / 4;
  const int p = threadIdx.x / C4, q = threadIdx.x - p * C4;
  const int row0 = blockIdx.x * rpc, row1 = min(H, row0 + rpc);
  const int npix = (row1 - row0) * W;
  const float* const src = r + ((long long)blockIdx.y * H + row0) * W * C + 4 * q;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (p < P) {
    int i = p;
    for (; i + 3 * P < npix; i += 4 * P) {         // four loads in flight, added in pixel order
      const f32x4 a0 = eg_ld4(src + (long long)i * C), a1 = eg_ld4(src + (long long)(i + P) * C);
      const f32x4 a2 = eg_ld4(src + (long long)(i + 2 * P) * C), a3 = eg_ld4(src + (long long)(i + 3 * P) * C);
      acc = (((acc + a0) + a1) + a2) + a3;
    }
    for (; i < npix; i += P) acc = acc + eg_ld4(src + (long long)i * C);
    red[threadIdx.x] = acc;
  }
  __syncthreads();
  if (p == 0) {
    for (int k = 1; k < P; ++k) acc = acc + red[k * C4 + q];
    eg_st4(partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * C + 4 * q, acc);
  }
}

// one block per sample: partial [B, chunks, C] -> gate [B, C]; fc1 [M, C], fc2 [C, M].  The block is launch-latency
// bound: every phase issues its loads in batches of EG_GATE_BATCH before the (ordered) additions that use them.
//   1. G = EG_GATE_THREADS / C thread groups; group g adds the chunks [g * per, (g + 1) * per) of its channel in
//      order, then the G group sums are added in order; bn of the mean -> pooled[C]
//   2. one wave per fc1 row: lane-strided products, xor butterfly, relu -> hidden[M]
//   3. one thread per channel: the fc2 row in order, sigmoid
__global__ __launch_bounds__(EG_GATE_THREADS) void eg_se_gate_f32(const float* __restrict__ partial, int chunks, float hw,
                                                                  EgBn bn, const float* __restrict__ fc1,
                                                                  const float* __restrict__ fc2,
                                                                  float* __restrict__ gate, int C, int M) {
  __shared__ float part[EG_GATE_THREADS];
  __shared__ float pooled[EG_MAX_C];
  __shared__ float hidden[EG_MAX_MID];
  const float* const src = partial + (long long)blockIdx.x * chunks * C;
  const int G = EG_GATE_THREADS / C, per = (chunks + G - 1) / G;
  const int g = threadIdx.x / C, c0 = threadIdx.x - g * C;
  if (g < G) {
    const int k1 = min(chunks, (g + 1) * per);
    float s = 0.f;
    int k = g * per;
    for (; k + EG_GATE_BATCH <= k1; k += EG_GATE_BATCH) {
      float v[EG_GATE_BATCH];
#pragma unroll
      for (int u = 0; u < EG_GATE_BATCH; ++u) v[u] = src[(long long)(k + u) * C + c0];
#pragma unroll
      for (int u = 0; u < EG_GATE_BATCH; ++u) s += v[u];
    }
    for (; k < k1; ++k) s += src[(long long)k * C + c0];
    part[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < C) {
    float s = part[threadIdx.x];
    for (int q = 1; q < G; ++q) s += part[q * C + threadIdx.x];
    pooled[threadIdx.x] = eg_bn1(bn, threadIdx.x, s / hw);
  }
  __syncthreads();
  const int lane = threadIdx.x & (FMGAN_WAVE - 1), wave = threadIdx.x / FMGAN_WAVE;
  for (int j = wave; j < M; j += EG_GATE_THREADS / FMGAN_WAVE) {
    const float* const row = fc1 + (long long)j * C;
    float s = 0.f;
    int c = lane;
    for (; c + (EG_GATE_BATCH - 1) * FMGAN_WAVE < C; c += EG_GATE_BATCH * FMGAN_WAVE) {
      float v[EG_GATE_BATCH];
#pragma unroll
      for (int u = 0; u < EG_GATE_BATCH; ++u) v[u] = row[c + u * FMGAN_WAVE];
#pragma unroll
      for (int u = 0; u < EG_GATE_BATCH; ++u) s = __builtin_fmaf(v[u], pooled[c + u * FMGAN_WAVE], s);
    }
    for (; c < C; c += FMGAN_WAVE) s = __builtin_fmaf(row[c], pooled[c], s);
#pragma unroll
    for (int m = FMGAN_WAVE / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, FMGAN_WAVE);
    if (lane == 0) hidden[j] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  if (threadIdx.x < C) {
    const float* const row = fc2 + (long long)threadIdx.x * M;
    float s = 0.f;
    int j = 0;
    for (; j + EG_GATE_BATCH <= M; j += EG_GATE_BATCH) {
      float v[EG_GATE_BATCH];
#pragma unroll
      for (int u = 0; u < EG_GATE_BATCH; ++u) v[u] = row[j + u];
#pragma unroll
      for (int u = 0; u < EG_GATE_BATCH; ++u) s = __builtin_fmaf(v[u], hidden[j + u], s);
    }
    for (; j < M; ++j) s = __builtin_fmaf(row[j], hidden[j], s);
    gate[(long long)blockIdx.x * C + threadIdx.x] = 1.f / (1.f + expf(-s));
  }
}

bool eg_bn_null(const float* mean, const float* var, const float* gamma, const float* beta) {
  return !mean || !var || !gamma || !beta;
}

uintptr_t eg_bn_addr(const float* mean, const float* var, const float* gamma, const float* beta) {
  return (uintptr_t)mean | (uintptr_t)var | (uintptr_t)gamma | (uintptr_t)beta;
}

// Status shared by the launches over [batch, h, w, channels], in the order the header states.
int eg_status(bool null_ptr, int batch, int channels, int h, int w, uintptr_t addr_or) {
  if (batch == 0) return FMGAN_OK;
  if (null_ptr || batch < 0 || channels <= 0 || h <= 0 || w <= 0) return FMGAN_EINVAL;
  // 32-bit: rows, work items (rows * segments), float4 offsets inside a row; grid.y of se_pool
  const long long rows = (long long)batch * h, row4 = (long long)w * ((channels + 3) / 4);
  if (batch > 65535 || rows * ((row4 + EG_SEG - 1) / EG_SEG) >= (1LL << 31) || row4 >= (1LL << 30))
    return FMGAN_EOVERFLOW;
  if (channels % 4 != 0 || channels > EG_MAX_C || (addr_or & 15) != 0) return FMGAN_EUNSUPPORTED;
  return FMGAN_OK;
}

int eg_grid(long long items) {
  const long long cap = (long long)FMGAN_NUM_CU * EG_BLOCKS_PER_CU;
  return (int)(items < cap ? items : cap);
}

int eg_rows_per_chunk(int batch, int h, int w) {
  const int want = (4 * FMGAN_NUM_CU + batch - 1) / batch;      // ~4 blocks per CU over the batch
  int rpc = (h + want - 1) / want;
  const int min_rows = (EG_POOL_MIN_PIX + w - 1) / w;
  if (rpc < min_rows) rpc = min_rows;
  return rpc < h ? rpc : h;
}

}  // namespace

extern "C" int fmgan_bn_prelu_f32(const float* x, const float* mean, const float* var, const float* gamma,
                                  const float* beta, float eps, const float* slope, float* y, const float* next_mean,
                                  const float* next_var, const float* next_gamma, const float* next_beta, float next_eps,
                                  float* y_next, float* y_sub, int batch, int channels, int h, int w, int sub_stride,
                                  void* stream) {
  const bool bad = !x || !slope || eg_bn_null(mean, var, gamma, beta) || (!y && !y_next && !y_sub) ||
                   (y_next && eg_bn_null(next_mean, next_var, next_gamma, next_beta)) || (y_sub && sub_stride < 1);
  uintptr_t addr = (uintptr_t)x | (uintptr_t)slope | eg_bn_addr(mean, var, gamma, beta) | (uintptr_t)y |
                   (uintptr_t)y_next | (uintptr_t)y_sub;
  if (y_next) addr |= eg_bn_addr(next_mean, next_var, next_gamma, next_beta);
  const int st = eg_status(bad, batch, channels, h, w, addr);
  if (st != FMGAN_OK || batch == 0) return st;
  const int rows = batch * h, nseg = (w * (channels / 4) + EG_SEG - 1) / EG_SEG;
  const EgBn bn{mean, var, gamma, beta, eps}, bn_next{next_mean, next_var, next_gamma, next_beta, next_eps};
  hipLaunchKernelGGL(eg_bn_prelu_f32, dim3(eg_grid((long long)rows * nseg)), dim3(EG_THREADS),
                     7 * channels * sizeof(float), (hipStream_t)stream, x, bn, slope, y, bn_next, y_next, y_sub, rows, h,
                     w, channels, y_sub ? sub_stride : 1, nseg);
  return fmgan_check_launch();
}

extern "C" int fmgan_se_pool_chunks(int batch, int channels, int h, int w) {
  if (batch <= 0 || eg_status(false, batch, channels, h, w, 0) != FMGAN_OK) return 0;
  const int rpc = eg_rows_per_chunk(batch, h, w);
  return (h + rpc - 1) / rpc;
}

extern "C" int fmgan_se_pool_f32(const float* r, float* partial, int batch, int channels, int h, int w, void* stream) {
  const int st = eg_status(!r || !partial, batch, channels, h, w, (uintptr_t)r | (uintptr_t)partial);
  if (st != FMGAN_OK || batch == 0) return st;
  const int rpc = eg_rows_per_chunk(batch, h, w), chunks = (h + rpc - 1) / rpc;
  hipLaunchKernelGGL(eg_se_pool_f32, dim3(chunks, batch), dim3(EG_THREADS), 0, (hipStream_t)stream, r, partial, h, w,
                     channels, rpc, EG_THREADS / (channels / 4));
  return fmgan_check_launch();
}

extern "C" int fmgan_se_gate_f32(const float* partial, int chunks, long long hw, const float* mean, const float* var,
                                 const float* gamma, const float* beta, float eps, const float* fc1, const float* fc2,
                                 float* gate, int batch, int channels, int mid, void* stream) {
  if (batch == 0) return FMGAN_OK;
  if (!partial || !fc1 || !fc2 || !gate || eg_bn_null(mean, var, gamma, beta) || batch < 0 || channels <= 0 ||
      mid <= 0 || chunks <= 0 || hw <= 0)
    return FMGAN_EINVAL;
  if (channels % 4 != 0 || channels > EG_MAX_C || mid > EG_MAX_MID) return FMGAN_EUNSUPPORTED;
  const EgBn bn{mean, var, gamma, beta, eps};
  hipLaunchKernelGGL(eg_se_gate_f32, dim3(batch), dim3(EG_GATE_THREADS), 0, (hipStream_t)stream, partial, chunks,
                     (float)hw, bn, fc1, fc2, gate, channels, mid);
  return fmgan_check_launch();
}

extern "C" int fmgan_ir_tail_f32(const float* r, const float* mean, const float* var, const float* gamma,
                                 const float* beta, float eps, const float* gate, const float* shortcut, int sc_h,
                                 int sc_w, int sc_stride, const float* sc_mean, const float* sc_var,
                                 const float* sc_gamma, const float* sc_beta, float sc_eps, float* out,
                                 const float* next_mean, const float* next_var, const float* next_gamma,
                                 const float* next_beta, float next_eps, float* out_next, int batch, int channels, int h,
                                 int w, void* stream) {
  const bool sc_bn = sc_mean || sc_var || sc_gamma || sc_beta;
  bool bad = !r || !shortcut || !out || eg_bn_null(mean, var, gamma, beta) ||
             (sc_bn && eg_bn_null(sc_mean, sc_var, sc_gamma, sc_beta)) ||
             (out_next && eg_bn_null(next_mean, next_var, next_gamma, next_beta));
  if (batch != 0 && !bad && h > 0 && w > 0) {
    // the shortcut covers the output: as it is (convolution output), or subsampled like MaxPool2d(1, stride)
    if (sc_bn) bad = sc_stride != 1 || sc_h != h || sc_w != w;
    else bad = sc_stride < 1 || sc_h < 1 || sc_w < 1 || (sc_h - 1) / sc_stride + 1 != h || (sc_w - 1) / sc_stride + 1 != w;
  }
  uintptr_t addr = (uintptr_t)r | (uintptr_t)shortcut | (uintptr_t)out | (uintptr_t)gate | (uintptr_t)out_next |
                   eg_bn_addr(mean, var, gamma, beta);
  if (sc_bn) addr |= eg_bn_addr(sc_mean, sc_var, sc_gamma, sc_beta);
  if (out_next) addr |= eg_bn_addr(next_mean, next_var, next_gamma, next_beta);
  int st = eg_status(bad, batch, channels, h, w, addr);
  if (st == FMGAN_OK && batch != 0) st = eg_status(false, batch, channels, sc_h, sc_w, 0);   // the source's offsets
  if (st != FMGAN_OK || batch == 0) return st;
  const int rows = batch * h, nseg = (w * (channels / 4) + EG_SEG - 1) / EG_SEG;
  const EgBn bn{mean, var, gamma, beta, eps}, bn_sc{sc_mean, sc_var, sc_gamma, sc_beta, sc_eps};
  const EgBn bn_next{next_mean, next_var, next_gamma, next_beta, next_eps};
  const dim3 grid(eg_grid((long long)rows * nseg)), block(EG_THREADS);
  const size_t lds = 9 * channels * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (sc_bn)
    hipLaunchKernelGGL(eg_ir_tail_f32<true>, grid, block, lds, s, r, bn, gate, shortcut, bn_sc, out, bn_next, out_next,
                       rows, h, w, channels, sc_h, sc_w, 1, nseg);
  else
    hipLaunchKernelGGL(eg_ir_tail_f32<false>, grid, block, lds, s, r, bn, gate, shortcut, bn_sc, out, bn_next, out_next,
                       rows, h, w, channels, sc_h, sc_w, sc_stride, nseg);
  return fmgan_check_launch();
}
