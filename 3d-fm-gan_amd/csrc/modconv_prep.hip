// ModulatedConv2d helpers for gfx950 (MI355X): demodulation, the cached per-(o,i) weight squares and the weight
// layouts the MFMA kernels read (modconv_fwd.hip, modconv_wgrad.hip).
// Demodulation: one wave per output channel, sum over Cin by wave-shuffle butterfly.
#include "modulation_waves.h"

namespace {

// ------------------------------------------------------------------ demod
// PRE: W is the per-(o,i) sum of squared taps [cout][cin] (modconv_wsq_f32, cached with the weight) instead of the
// raw weight — the same fma chains in the same order, so both variants give identical bits.
template <bool PRE>
__global__ __launch_bounds__(256) void modconv_demod_f32(const float* __restrict__ W,
                                                         const float* __restrict__ style,
                                                         float* __restrict__ demod, int batch, int cout, int cin,
                                                         int ktaps, float scale, float eps) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= cout) return;  // wave-uniform
  const float* wo = W + (long long)o * cin * (PRE ? 1 : ktaps);
  float wsq[DEMOD_MAXJ];
  if (demod_cached(cin)) demod_load_wsq<PRE>(wo, cin, ktaps, lane, wsq);
  // PRE (inference): one wave per (output channel, sample) — the grid's y extent covers the batch, so the samples' style
  // loads are independent waves instead of `batch` dependent round trips inside one wave.  The raw-weight form keeps one
  // wave per channel (it squares nine taps per weight; repeating that per sample would cost more than it hides).
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    const float d = demod_wave<PRE>(wo, wsq, style + (long long)b * cin, cin, ktaps, scale, eps, lane);
    if (lane == 0) demod[(long long)b * cout + o] = d;
  }
}

__global__ __launch_bounds__(256) void modconv_wsq_f32(const float* __restrict__ W, float* __restrict__ wsq,
                                                       long long n, int ktaps) {
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
    float q = 0.f;
    for (int t = 0; t < ktaps; ++t) { const float w = W[idx * ktaps + t]; q = fmaf(w, w, q); }
    wsq[idx] = q;
  }
}

// ------------------------------------------------------------------ weight prep
// kind 0 (forward):                          wt[i][t][o] = scale * W[o][i][t]
// kind 1 (data-gradient of the plain conv):  wt[o][t][i] = scale * W[o][i][ktaps-1-t]   (taps flipped, roles swapped)
// kind 2 (data-gradient of the transposed):  wt[o][t][i] = scale * W[o][i][t]           (roles swapped)
__global__ __launch_bounds__(256) void modconv_weight_prep_f32(const float* __restrict__ W, float* __restrict__ wt,
                                                               int cout, int cin, int ktaps, float scale, int kind) {
  const long long total = (long long)cout * cin * ktaps;
  const int cols = kind == 0 ? cout : cin;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % cols);
    const long long rt = idx / cols;
    const int t = (int)(rt % ktaps), r = (int)(rt / ktaps);
    float v;
    if (kind == 0) v = W[((long long)c * cin + r) * ktaps + t];
    else v = W[((long long)r * cin + c) * ktaps + (kind == 1 ? ktaps - 1 - t : t)];
    wt[idx] = scale * v;
  }
}

}  // namespace

extern "C" int fmgan_modconv_demod_f32(const float* weight, const float* style, float* demod, int batch, int cout,
                                       int cin, int ktaps, float scale, float eps, void* stream) {
  if (batch < 0 || cout <= 0 || cin <= 0 || ktaps <= 0) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!weight || !style || !demod) return FMGAN_EINVAL;
  hipLaunchKernelGGL(modconv_demod_f32<false>, dim3((cout + 3) / 4), dim3(256), 0, (hipStream_t)stream, weight, style,
                     demod, batch, cout, cin, ktaps, scale, eps);
  return fmgan_check_launch();
}

extern "C" int fmgan_modconv_wsq_f32(const float* weight, float* wsq, int cout, int cin, int ktaps, void* stream) {
  if (cout <= 0 || cin <= 0 || ktaps <= 0) return FMGAN_EINVAL;
  if (!weight || !wsq) return FMGAN_EINVAL;
  const long long n = (long long)cout * cin;
  long long blocks = (n + 255) / 256;
  if (blocks > FMGAN_NUM_CU * 16) blocks = FMGAN_NUM_CU * 16;
  hipLaunchKernelGGL(modconv_wsq_f32, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, weight, wsq, n, ktaps);
  return fmgan_check_launch();
}

extern "C" int fmgan_modconv_demod_wsq_f32(const float* wsq, const float* style, float* demod, int batch, int cout,
                                           int cin, float scale, float eps, void* stream) {
  if (batch < 0 || cout <= 0 || cin <= 0) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!wsq || !style || !demod) return FMGAN_EINVAL;
  hipLaunchKernelGGL(modconv_demod_f32<true>, dim3((cout + 3) / 4, batch < 64 ? batch : 64), dim3(256), 0, (hipStream_t)stream, wsq, style, demod,
                     batch, cout, cin, 1, scale, eps);
  return fmgan_check_launch();
}

extern "C" int fmgan_modconv_weight_prep_f32(const float* weight, float* wt, int cout, int cin, int ktaps, float scale,
                                             int kind, void* stream) {
  if (cout <= 0 || cin <= 0 || ktaps <= 0) return FMGAN_EINVAL;
  if (kind < 0 || kind > 2) return FMGAN_EUNSUPPORTED;
  if (!weight || !wt) return FMGAN_EINVAL;
  const long long total = (long long)cout * cin * ktaps;
  long long blocks = (total + 255) / 256;
  if (blocks > FMGAN_NUM_CU * 16) blocks = FMGAN_NUM_CU * 16;
  hipLaunchKernelGGL(modconv_weight_prep_f32, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, weight, wt,
                     cout, cin, ktaps, scale, kind);
  return fmgan_check_launch();
}
