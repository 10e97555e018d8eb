// The two launches the training loop adds per iteration.
//
// train_ema_f32: the EMA of a whole parameter set, dst <- decay * dst + alpha * src, in one launch.  The reference's
// `accumulate` (train_3_encoder.py:195-200) is a mul_ and an add_ per parameter: 164 - 276 aten launches per iteration
// for the Generators of 64^2 .. 1024^2, most of them over a few hundred elements.  Here a device table of
// {dst, src, numel, block_begin} is walked as live_weights_f32 walks its table: a block finds its entry by a uniform
// binary search and handles EMA_CHUNK consecutive elements of that tensor.  Pure streaming (12 bytes per element), no
// LDS, no reduction: elementwise and bit-reproducible.
//
// train_loss_row_f32: one wave gathers up to 16 scalars, each somewhere in device memory, into one row of the loss
// ledger (op/loss_log.py) — what the reference reads back with nine .item() calls per iteration.  The 16 addresses
// arrive by value in the kernel arguments; lane i picks its own with 16 uniform selects (indexing the struct by lane id
// would make the compiler copy it to scratch).
#include "common.h"

namespace {

constexpr int EMA_THREADS = 256, EMA_PER = 16, EMA_CHUNK = EMA_THREADS * EMA_PER;

// Two roundings, written out: the product, then one fused multiply-add (the file is compiled with -ffp-contract=on; the
// fma is explicit so that nothing else can be contracted into it).
__device__ __forceinline__ float ema1(float d, float s, float decay, float alpha) {
  const float dd = d * decay;
  return __builtin_fmaf(alpha, s, dd);
}

__global__ __launch_bounds__(EMA_THREADS) void train_ema_f32(const fmgan_ema_entry* __restrict__ table, int n_entries,
                                                             float decay, float alpha) {
  // entry of this block: the last one whose block_begin <= blockIdx.x (uniform binary search)
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].block_begin <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const fmgan_ema_entry e = table[lo];
  const long long base = ((long long)blockIdx.x - e.block_begin) * EMA_CHUNK;
  const long long left = e.numel - base;
  if (base < 0 || left <= 0) return;                       // a block outside its entry: nothing of it to touch
  const int n = left < EMA_CHUNK ? (int)left : EMA_CHUNK;
  float* __restrict__ dst = (float*)e.dst + base;
  const float* __restrict__ src = (const float*)e.src + base;
  // elements before dst's first 16-byte boundary; vector accesses only if src is aligned there as well
  int head = (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
  const bool vec = ((((uintptr_t)src) + 4u * (unsigned)head) & 15u) == 0;
  if (!vec || head > n) head = n;
  const int nvec = (n - head) >> 2;
  for (int i = threadIdx.x; i < head; i += EMA_THREADS) dst[i] = ema1(dst[i], src[i], decay, alpha);
  // all eight loads of a lane are issued before the first store: 128 bytes in flight per lane
  f32x4* vd = reinterpret_cast<f32x4*>(dst + head);
  const f32x4* vs = reinterpret_cast<const f32x4*>(src + head);
  f32x4 d[EMA_PER / 4], s[EMA_PER / 4];
#pragma unroll
  for (int k = 0; k < EMA_PER / 4; ++k) {
    const int v = threadIdx.x + EMA_THREADS * k;
    if (v < nvec) {
      s[k] = vs[v];
      d[k] = vd[v];
    }
  }
#pragma unroll
  for (int k = 0; k < EMA_PER / 4; ++k) {
    const int v = threadIdx.x + EMA_THREADS * k;
    if (v < nvec) {
      d[k].x = ema1(d[k].x, s[k].x, decay, alpha);
      d[k].y = ema1(d[k].y, s[k].y, decay, alpha);
      d[k].z = ema1(d[k].z, s[k].z, decay, alpha);
      d[k].w = ema1(d[k].w, s[k].w, decay, alpha);
      vd[v] = d[k];
    }
  }
  for (int i = head + 4 * nvec + threadIdx.x; i < n; i += EMA_THREADS) dst[i] = ema1(dst[i], src[i], decay, alpha);
}

__global__ __launch_bounds__(FMGAN_WAVE) void train_loss_row_f32(fmgan_loss_ptrs ptrs, int n, float* __restrict__ row) {
  const int lane = threadIdx.x;
  if (lane >= 16) return;
  const float* p = nullptr;
#pragma unroll
  for (int i = 0; i < 16; ++i) p = lane == i ? ptrs.p[i] : p;
  float v = 0.f;
  if (lane < n && p != nullptr) v = *p;
  row[lane] = v;
}

}  // namespace

extern "C" long long fmgan_ema_blocks(long long numel) {
  return numel > 0 ? (numel + EMA_CHUNK - 1) / EMA_CHUNK : 0;
}

extern "C" int fmgan_ema_f32(const fmgan_ema_entry* table_dev, int n_entries, long long total_blocks, float decay,
                             float alpha, void* stream) {
  if (n_entries < 0 || total_blocks < 0) return FMGAN_EINVAL;
  if (n_entries == 0 || total_blocks == 0) return FMGAN_OK;
  if (!table_dev) return FMGAN_EINVAL;
  if (total_blocks > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  hipLaunchKernelGGL(train_ema_f32, dim3((unsigned)total_blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream, table_dev,
                     n_entries, decay, alpha);
  return fmgan_check_launch();
}

extern "C" int fmgan_loss_row_f32(const fmgan_loss_ptrs* ptrs, int n, float* row_dev, void* stream) {
  if (!ptrs || !row_dev || n < 0 || n > 16) return FMGAN_EINVAL;
  hipLaunchKernelGGL(train_loss_row_f32, dim3(1), dim3(FMGAN_WAVE), 0, (hipStream_t)stream, *ptrs, n, row_dev);
  return fmgan_check_launch();
}
