// Every modulated layer's style vector, and every demodulated layer's coefficients, in TWO launches per forward.
//
// The synthesis network modulates each of its convolutions with s = EqualLinear(latent[:, col]) (the reference:
// stylegan2.py:226,252) and demodulates the 3x3 ones (stylegan2.py:254-256).  Issued per layer that is one
// fmgan_equal_linear_f32 + one fmgan_modconv_demod_wsq_f32 launch (and, under co-modulation, one elementwise
// W * W+[:, col]) on the critical path between the contractions: 26 + 17 (+ 18) launches of 5-10 us at 1024^2, each far
// too small to fill the chip.  When every latent column is known before the network starts (re-animation: W+ of the
// photo is cached, W of the render frames is one small ResNet away) none of them depends on an activation, so a
// device-side table of the layers (fmgan_style_bank_entry) is walked by one launch for all styles and one for all
// demodulation coefficients.
//   style:  one wave per (entry, feature n, sample t)   s[t,n] = sum_k ws[n,k] * x[t,k] + bs[n]
//           x[t,k] = w[t,k], or fl(w[t,k] * wplus[p,col,k]) for a sliced column (p = 0 when the photo is shared)
//   demod:  one wave per (entry, channel o, sample t)   d[t,o] = 1 / sqrt(scale^2 * sum_i wsq[o,i] * s[t,i]^2 + eps)
// The per-wave bodies are those of the per-layer kernels (modulation_waves.h): identical bits.  No atomics; every output
// element has exactly one writer.  HBM/L2-bound: the style launch reads each layer's [cin, style_dim] matrix once per
// sample block (26 x 1 MB at 1024^2, L2-resident across the samples), the demod launch each [cout, cin] table.
// Grid: x = feature blocks of 4 waves (capped; a wave strides over the features beyond), y = entry, z = sample (capped at
// 64, strided beyond).
// The concatenating co-modulation modes of the 2-encoder scheme (the reference: Util/network_util.py:264-282) modulate
// with x[t] = [v[t] | wplus[p, col]] over a [cin, Dv + Dw] matrix: style_bank_concat_f32 is the same walk with the
// concatenated chain (equal_linear_concat_wave); every column is concatenated, `sliced` is not read.
#include "modulation_waves.h"

namespace {

constexpr int SB_MAX_XBLOCKS = 128;   // 512 features of 4 waves per block: the widest layer of the unpruned networks

__global__ __launch_bounds__(256) void style_bank_f32(const fmgan_style_bank_entry* __restrict__ table,
                                                      const float* __restrict__ w, const float* __restrict__ wplus,
                                                      int wplus_batch, int batch, int style_dim,
                                                      float* __restrict__ styles_out) {
  const fmgan_style_bank_entry e = table[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const float* __restrict__ ws = (const float*)e.ws;
  const float* __restrict__ bs = (const float*)e.bs;
  float* __restrict__ out = styles_out + (long long)batch * e.style_off;
  for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < e.cin; n += gridDim.x * 4) {   // wave-uniform
    const float* wn = ws + (long long)n * style_dim;
    for (int t = blockIdx.z; t < batch; t += gridDim.z) {
      const float* xb = w + (long long)t * style_dim;
      float acc;
      if (e.sliced) {
        const long long p = wplus_batch == 1 ? 0 : t;
        acc = equal_linear_wave<true>(wn, xb, wplus + (p * e.n_styles + e.col) * style_dim, style_dim, lane);
      } else {
        acc = equal_linear_wave<false>(wn, xb, nullptr, style_dim, lane);
      }
      if (lane == 0) out[(long long)t * e.cin + n] = bs ? acc + bs[n] : acc;
    }
  }
}

__global__ __launch_bounds__(256) void style_bank_concat_f32(const fmgan_style_bank_entry* __restrict__ table,
                                                             const float* __restrict__ v, const float* __restrict__ wplus,
                                                             int wplus_batch, int batch, int dv, int dw,
                                                             float* __restrict__ styles_out) {
  const fmgan_style_bank_entry e = table[blockIdx.y];
  if (e.col < 0 || e.col >= e.n_styles) return;   // block-uniform: never read outside wplus (the host refuses such a table)
  const int lane = threadIdx.x & 63;
  const float* __restrict__ ws = (const float*)e.ws;
  const float* __restrict__ bs = (const float*)e.bs;
  float* __restrict__ out = styles_out + (long long)batch * e.style_off;
  for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < e.cin; n += gridDim.x * 4) {   // wave-uniform
    const float* wn = ws + (long long)n * (dv + dw);
    for (int t = blockIdx.z; t < batch; t += gridDim.z) {
      const long long p = wplus_batch == 1 ? 0 : t;
      const float acc = equal_linear_concat_wave(wn, v + (long long)t * dv, wplus + (p * e.n_styles + e.col) * dw, dv, dw,
                                                 lane);
      if (lane == 0) out[(long long)t * e.cin + n] = bs ? acc + bs[n] : acc;
    }
  }
}

__global__ __launch_bounds__(256) void demod_bank_f32(const fmgan_style_bank_entry* __restrict__ table,
                                                      const float* __restrict__ styles, int batch,
                                                      float* __restrict__ demod_out) {
  const fmgan_style_bank_entry e = table[blockIdx.y];
  if (!e.demodulate || !e.wsq) return;   // block-uniform
  const int lane = threadIdx.x & 63;
  const float* __restrict__ style = styles + (long long)batch * e.style_off;
  float* __restrict__ out = demod_out + (long long)batch * e.demod_off;
  for (int o = blockIdx.x * 4 + (threadIdx.x >> 6); o < e.cout; o += gridDim.x * 4) {   // wave-uniform
    const float* wo = (const float*)e.wsq + (long long)o * e.cin;
    float wsq[DEMOD_MAXJ];
    if (demod_cached(e.cin)) demod_load_wsq<true>(wo, e.cin, 1, lane, wsq);
    for (int t = blockIdx.z; t < batch; t += gridDim.z) {
      const float d = demod_wave<true>(wo, wsq, style + (long long)t * e.cin, e.cin, 1, e.scale, e.eps, lane);
      if (lane == 0) out[(long long)t * e.cout + o] = d;
    }
  }
}

}  // namespace

extern "C" int fmgan_style_bank_entry_bytes(void) { return (int)sizeof(fmgan_style_bank_entry); }

extern "C" int fmgan_style_bank_f32(const fmgan_style_bank_entry* table_dev, int n_entries, const float* w,
                                    const float* wplus, int wplus_batch, int batch, int style_dim, float* styles_out,
                                    void* stream) {
  if (n_entries <= 0 || n_entries > 65535 || batch < 0 || style_dim <= 0) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!table_dev || !w || !wplus || !styles_out) return FMGAN_EINVAL;
  if (wplus_batch != 1 && wplus_batch != batch) return FMGAN_EINVAL;
  hipLaunchKernelGGL(style_bank_f32, dim3(SB_MAX_XBLOCKS, n_entries, batch < 64 ? batch : 64), dim3(256), 0,
                     (hipStream_t)stream, table_dev, w, wplus, wplus_batch, batch, style_dim, styles_out);
  return fmgan_check_launch();
}

extern "C" int fmgan_style_bank_concat_f32(const fmgan_style_bank_entry* table_dev, int n_entries, const float* v,
                                           const float* wplus, int wplus_batch, int batch, int dv, int dw,
                                           float* styles_out, void* stream) {
  if (n_entries <= 0 || n_entries > 65535 || batch < 0 || dv <= 0 || dw <= 0) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!table_dev || !v || !wplus || !styles_out) return FMGAN_EINVAL;
  if (wplus_batch != 1 && wplus_batch != batch) return FMGAN_EINVAL;
  hipLaunchKernelGGL(style_bank_concat_f32, dim3(SB_MAX_XBLOCKS, n_entries, batch < 64 ? batch : 64), dim3(256), 0,
                     (hipStream_t)stream, table_dev, v, wplus, wplus_batch, batch, dv, dw, styles_out);
  return fmgan_check_launch();
}

extern "C" int fmgan_demod_bank_f32(const fmgan_style_bank_entry* table_dev, int n_entries, const float* styles,
                                    int batch, float* demod_out, void* stream) {
  if (n_entries <= 0 || n_entries > 65535 || batch < 0) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  if (!table_dev || !styles || !demod_out) return FMGAN_EINVAL;
  hipLaunchKernelGGL(demod_bank_f32, dim3(SB_MAX_XBLOCKS, n_entries, batch < 64 ? batch : 64), dim3(256), 0,
                     (hipStream_t)stream, table_dev, styles, batch, demod_out);
  return fmgan_check_launch();
}
