// 16-bit activations in HBM: bias-activation, its one-pass backward and the up = down = 1 FIR on bf16 and
// f16 tensors, for gfx950.
//
// Under torch.autocast the MIOpen convolutions of the Discriminator and of the encoder heads produce and consume bf16;
// the fp32 kernels of fused_bias_act.hip / upfirdn2d.hip sit between them behind a widening and a narrowing cast
// kernel each.  The kernels here read and write the 2-byte elements themselves: half the bytes, no cast kernels.  They
// are streaming kernels, HBM-bound by construction:
//   * 8 elements (16 bytes) per lane per access wherever the addresses allow it, scalar 2-byte accesses for the head
//     and the tail of a run whose ends are not on a 16-byte boundary (as train_ema_f32 does for 4-byte elements);
//   * every value is widened to fp32 (exact), the arithmetic is that of the fp32 kernels in the same order, and the
//     result is narrowed ONCE, round-to-nearest-even, at the store: y16 == narrow(fp32 kernel(widen(x16)));
//   * one writer per output element, no atomics; the bias-gradient partial sums have a fixed association.
// The fp32 kernels, their names, dispatch and bits are untouched: these are additional entry points.
#include <stdlib.h>
#include "common.h"

namespace {

typedef unsigned short us;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x2_u __attribute__((ext_vector_type(2), aligned(4)));

struct BF16 {};   // tags: the element type of a kernel instantiation (the data are handled as raw 16-bit patterns)
struct F16 {};

template <typename T> struct Io;
template <> struct Io<BF16> {
  static __device__ __forceinline__ float widen(unsigned b) { return __uint_as_float(b << 16); }
  // round-to-nearest-even, NaN -> a quiet NaN: the conversion of the language, which gfx950 has as an instruction
  // (v_cvt_pk_bf16_f32) — no compare masks in scalar registers, a sixth of the integer form's vector work
  static __device__ __forceinline__ unsigned narrow(float f) {
    const __bf16 h = (__bf16)f;
    return (unsigned)__builtin_bit_cast(us, h);
  }
};
template <> struct Io<F16> {
  static __device__ __forceinline__ float widen(unsigned b) { return __half2float(__ushort_as_half((us)b)); }
  // v_cvt_f16_f32 (RNE) on the ROUNDED fp32 value.  Written as an instruction: from `__float2half(a * b)` the compiler
  // may form v_fma_mixlo_f16, which rounds the exact product to f16 directly — one rounding where the fp32 kernel
  // followed by a narrowing has two, and a different last bit now and then.
  static __device__ __forceinline__ unsigned narrow(float f) {
    unsigned r;
    asm("v_cvt_f16_f32 %0, %1" : "=v"(r) : "v"(f));
    return r & 0xffffu;
  }
};

template <typename T> __device__ __forceinline__ void widen8(const u32x4 w, float (&v)[8]) {
  v[0] = Io<T>::widen(w.x & 0xffffu); v[1] = Io<T>::widen(w.x >> 16);
  v[2] = Io<T>::widen(w.y & 0xffffu); v[3] = Io<T>::widen(w.y >> 16);
  v[4] = Io<T>::widen(w.z & 0xffffu); v[5] = Io<T>::widen(w.z >> 16);
  v[6] = Io<T>::widen(w.w & 0xffffu); v[7] = Io<T>::widen(w.w >> 16);
}

__device__ __forceinline__ u32x4 pack8(const unsigned (&h)[8]) {
  u32x4 w;
  w.x = h[0] | (h[1] << 16); w.y = h[2] | (h[3] << 16); w.z = h[4] | (h[5] << 16); w.w = h[6] | (h[7] << 16);
  return w;
}

// A run of n 2-byte elements at o (written) and a, r (read; r may be 0): `head` (< 8) elements before o's first 16-byte
// boundary, then `nvec` vectors of 8, then the tail.  Vectors only if a and r are aligned where o is; otherwise (and for
// a run that ends before the boundary) the whole run is tail.
__device__ __forceinline__ void split_run(uintptr_t o, uintptr_t a, uintptr_t r, long long n, int& head, int& nvec) {
  head = (int)(((16u - (unsigned)(o & 15u)) & 15u) >> 1);
  const bool vec = ((a + 2u * (unsigned)head) & 15u) == 0 && (r == 0 || ((r + 2u * (unsigned)head) & 15u) == 0);
  if (!vec || head > n) head = 0;
  nvec = vec && head <= n ? (int)((n - head) >> 3) : 0;
}

// ---------------------------------------------------------------- bias-activation
// CODE 30 / 31: the two codes of the training step, compiled in (31 reads ref); CODE 0: any code at run time, ref optional.
template <typename T, int CODE>
__device__ __forceinline__ unsigned fba1(unsigned xb, unsigned rb, float bias, int code, float alpha, float scale) {
  const float v = Io<T>::widen(xb) + bias;
  return Io<T>::narrow(act_apply(v, Io<T>::widen(rb), CODE ? CODE : code, alpha) * scale);
}

template <typename T, int CODE>
__device__ __forceinline__ u32x4 fba8(const u32x4 xw, const u32x4 rw, const float (&bias)[8], int code, float alpha,
                                      float scale) {
  float xv[8], rv[8];
  widen8<T>(xw, xv);
  widen8<T>(rw, rv);
  unsigned h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = Io<T>::narrow(act_apply(xv[k] + bias[k], rv[k], CODE ? CODE : code, alpha) * scale);
  return pack8(h);
}

// planes layout: `planes` runs of `step` elements, the bias a scalar per run (b[pl % size_b]); a tensor without bias is
// one run.  A block row (grid.y, grid.z) owns one run and grid.x strides it: no loop over runs, whose invariants the
// compiler would hoist into more scalar registers than eight waves per SIMD leave.  The host keeps step / 8 and planes
// within 31 bits.
template <typename T, int CODE>
__global__ __launch_bounds__(256, 8) void act16_fba(us* __restrict__ out, const us* __restrict__ x,
                                                    const float* __restrict__ b, const us* __restrict__ ref, int planes,
                                                    long long step, int size_b, int code, float alpha, float scale) {
  const bool has_ref = CODE == 31 || (CODE == 0 && ref != nullptr);
  const int tid = blockIdx.x * 256 + threadIdx.x, nthr = gridDim.x * 256;
  const long long run = (long long)blockIdx.z * gridDim.y + blockIdx.y;
  if (run < planes) {
    const int pl = (int)run;
    const float bv = b ? b[pl % size_b] : 0.f;
    const float bias[8] = {bv, bv, bv, bv, bv, bv, bv, bv};
    const us* xp = x + pl * step;
    const us* rp = has_ref ? ref + pl * step : nullptr;
    us* op = out + pl * step;
    int head, nvec;
    split_run((uintptr_t)op, (uintptr_t)xp, (uintptr_t)rp, step, head, nvec);
    if (tid < head) op[tid] = (us)fba1<T, CODE>(xp[tid], has_ref ? rp[tid] : 0u, bv, code, alpha, scale);
    const u32x4* x8 = reinterpret_cast<const u32x4*>(xp + head);
    const u32x4* r8 = reinterpret_cast<const u32x4*>(rp + head);
    u32x4* o8 = reinterpret_cast<u32x4*>(op + head);
#pragma unroll 1
    for (int v = tid; v < nvec; v += nthr) {
      u32x4 rw = {0u, 0u, 0u, 0u};
      if (has_ref) rw = r8[v];
      o8[v] = fba8<T, CODE>(x8[v], rw, bias, code, alpha, scale);
    }
#pragma unroll 1
    for (long long i = head + 8LL * nvec + tid; i < step; i += nthr)
      op[i] = (us)fba1<T, CODE>(xp[i], has_ref ? rp[i] : 0u, bv, code, alpha, scale);
  }
}

// bias innermost (step_b == 1): element i takes b[i % size_b] — the [B, C] tensors of EqualLinear(fused_lrelu).
// One modulo per vector of 8, then the index walks with a wrap.  The host keeps n within 31 bits.
template <typename T, int CODE>
__global__ __launch_bounds__(256, 8) void act16_fba_inner(us* __restrict__ out, const us* __restrict__ x,
                                                          const float* __restrict__ b, const us* __restrict__ ref, int n,
                                                          int size_b, int code, float alpha, float scale) {
  const bool has_ref = CODE == 31 || (CODE == 0 && ref != nullptr);
  const int tid = blockIdx.x * 256 + threadIdx.x, nthr = gridDim.x * 256;
  int head, nvec;
  split_run((uintptr_t)out, (uintptr_t)x, (uintptr_t)(has_ref ? ref : nullptr), n, head, nvec);
  if (tid < head) out[tid] = (us)fba1<T, CODE>(x[tid], has_ref ? ref[tid] : 0u, b[tid % size_b], code, alpha, scale);
  const u32x4* x8 = reinterpret_cast<const u32x4*>(x + head);
  const u32x4* r8 = reinterpret_cast<const u32x4*>(ref + head);
  u32x4* o8 = reinterpret_cast<u32x4*>(out + head);
#pragma unroll 1
  for (int v = tid; v < nvec; v += nthr) {
    u32x4 rw = {0u, 0u, 0u, 0u};
    if (has_ref) rw = r8[v];
    int j = (head + 8 * v) % size_b;
    float bias[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      bias[k] = b[j];
      j = j + 1 == size_b ? 0 : j + 1;
    }
    o8[v] = fba8<T, CODE>(x8[v], rw, bias, code, alpha, scale);
  }
#pragma unroll 1
  for (int i = head + 8 * nvec + tid; i < n; i += nthr)
    out[i] = (us)fba1<T, CODE>(x[i], has_ref ? ref[i] : 0u, b[i % size_b], code, alpha, scale);
}

// ---------------------------------------------------------------- backward of lrelu(x + b) * scale, one pass
// grad_in = narrow(act'(g; ref) * scale) and, per (plane, block), the fp32 sum of the STORED grad_in widened back: the
// bias gradient is the sum of what was written.  Fixed association, as fba_bwd_bias_f32: per-lane serial in index
// order (head element, vectors, tail), wave butterfly, the 4 waves in order.
template <typename T>
__device__ __forceinline__ float fba_bwd1(us* o, unsigned gb, unsigned rb, float alpha, float scale) {
  const unsigned s = Io<T>::narrow(act_apply(Io<T>::widen(gb), Io<T>::widen(rb), 31, alpha) * scale);
  *o = (us)s;
  return Io<T>::widen(s);
}

template <typename T>
__global__ __launch_bounds__(256, 8) void act16_fba_bwd(us* __restrict__ gi, float* __restrict__ partial,
                                                        const us* __restrict__ g, const us* __restrict__ ref, int planes,
                                                        int hw, float alpha, float scale) {
  __shared__ float red[4];
  const int tid = blockIdx.x * 256 + threadIdx.x, nthr = gridDim.x * 256;
#pragma unroll 1
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const us* gp = g + (long long)pl * hw;
    const us* rp = ref + (long long)pl * hw;
    us* op = gi + (long long)pl * hw;
    int head, nvec;
    split_run((uintptr_t)op, (uintptr_t)gp, (uintptr_t)rp, hw, head, nvec);
    float acc = 0.f;
    if (tid < head) acc += fba_bwd1<T>(op + tid, gp[tid], rp[tid], alpha, scale);
    const u32x4* g8 = reinterpret_cast<const u32x4*>(gp + head);
    const u32x4* r8 = reinterpret_cast<const u32x4*>(rp + head);
    u32x4* o8 = reinterpret_cast<u32x4*>(op + head);
#pragma unroll 1
    for (int v = tid; v < nvec; v += nthr) {
      float gv[8], rv[8], w[8];
      widen8<T>(g8[v], gv);
      widen8<T>(r8[v], rv);
      unsigned h[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        h[k] = Io<T>::narrow(act_apply(gv[k], rv[k], 31, alpha) * scale);
        w[k] = Io<T>::widen(h[k]);
      }
      o8[v] = pack8(h);
      acc += ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
    }
#pragma unroll 1
    for (int i = head + 8 * nvec + tid; i < hw; i += nthr) acc += fba_bwd1<T>(op + i, gp[i], rp[i], alpha, scale);
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)pl * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- FIR, up = down = 1, minor = 1, <= 4x4 taps
// out[n,oy,ox] = sum_{ky,kx} kflip[ky,kx] * in[n, oy + ky - pad_y0, ox + kx - pad_x0], zero outside the plane, summed
// with fmaf in tap order (ky outer, kx inner, ascending) from 0.
//
// A kh x kw FIR is placed in the bottom-right corner of a 4x4 one (pads grown by 4 - kh, 4 - kw; absent taps are
// skipped by uniform branches, not multiplied by zero), so one window shape serves every size.  A lane owns 8 consecutive
// output columns and marches down `th` output rows.  Per input row it fetches the 11 columns under its taps ONCE, as 6 packed dwords; the
// last four rows stay in registers PACKED (24 VGPRs; widened they would be 44) and rotate through the statically
// unrolled loop, so an input row is read once per row tile and nothing moves between registers.  An output row widens
// its four window rows on the fly.
// The 11 columns start anywhere (pad 1: on an odd element), so they are fetched as the 12 elements from the even
// address at or below them — one dwordx4 and one dwordx2 that need dword alignment only — and shifted by one element
// with v_alignbit when the start is odd.  Lanes whose 24 bytes would leave the tensor (its first and last rows only)
// fetch element-wise.  Columns outside the row are cleared in the packed words (edge lanes only).
struct Fir16Params {
  long long items;      // major * tiles_y * groups: one lane each
  long long total_in;   // major * in_h * in_w
  int in_h, in_w, out_h, out_w;
  int pad_x0, pad_y0;   // of the embedded 4x4 FIR
  int kh, kw;
  int th, tiles_y, groups;
};

struct Row16 { unsigned w[6]; };   // 12 packed elements; element j of the window = half (j & 1) of w[j >> 1]

template <typename T> __device__ __forceinline__ float row_elem(const Row16& r, int j) {
  return Io<T>::widen((j & 1) ? r.w[j >> 1] >> 16 : r.w[j >> 1] & 0xffffu);
}

// the window row of input row iy of the plane that starts `base` elements into `in`: columns cx0 .. cx0 + 10, zero
// where the row or a column is outside.  Addresses are `in` plus an element index, so the fetches are global loads.
// Conditions on colmask do not change from row to row; the empty asm makes the value opaque here, so that the compiler
// builds their lane masks where an edge lane needs them and does not keep one scalar register pair per column alive
// through the row loop.
__device__ __forceinline__ Row16 fir_load_row(const us* __restrict__ in, long long base, int iy, int cx0,
                                              unsigned colmask, int in_h, int in_w, long long total_in) {
  Row16 r;
#pragma unroll
  for (int j = 0; j < 6; ++j) r.w[j] = 0u;
  asm volatile("" : "+v"(colmask));
  if (iy < 0 || iy >= in_h || colmask == 0u) return r;
  const long long a0 = base + (long long)iy * in_w + cx0;          // window column 0, in elements from `in` (an edge: < 0)
  const unsigned par = (unsigned)(((uintptr_t)in >> 1) + (unsigned long long)a0) & 1u;
  const long long e = a0 - par;                                    // the even (dword-aligned) address at or below it
  if (e >= 0 && e + 12 <= total_in) {
    const u32x4_u w0 = *reinterpret_cast<const u32x4_u*>(in + e);
    const u32x2_u w1 = *reinterpret_cast<const u32x2_u*>(in + e + 8);
    const unsigned sh = par * 16u;
    r.w[0] = __builtin_amdgcn_alignbit(w0.y, w0.x, sh);
    r.w[1] = __builtin_amdgcn_alignbit(w0.z, w0.y, sh);
    r.w[2] = __builtin_amdgcn_alignbit(w0.w, w0.z, sh);
    r.w[3] = __builtin_amdgcn_alignbit(w1.x, w0.w, sh);
    r.w[4] = __builtin_amdgcn_alignbit(w1.y, w1.x, sh);
    r.w[5] = __builtin_amdgcn_alignbit(0u, w1.y, sh);
    if (colmask != 0x7ffu) {
#pragma unroll
      for (int j = 0; j < 6; ++j)
        r.w[j] &= ((colmask >> (2 * j) & 1u) ? 0xffffu : 0u) | ((colmask >> (2 * j + 1) & 1u) ? 0xffff0000u : 0u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 11; ++j) {                                 // branch-free: an absent column reads in[0] and drops it
      const bool ok = colmask >> j & 1u;
      const unsigned v = in[ok ? a0 + j : 0];
      r.w[j >> 1] |= (ok ? v : 0u) << (16 * (j & 1));
    }
  }
  return r;
}

// 8 outputs at element index o of `out`.  A whole group goes out as 16 bytes: one dwordx4 where the address is
// dword-aligned, else (odd output widths: every second row) a 2-byte element, a dwordx2, a dword and a 2-byte element.
// The last group of a row stores its `nst` < 8 columns one by one (nst opaque, as colmask above).
__device__ __forceinline__ void fir_store_row(us* __restrict__ out, long long o, const unsigned (&h)[8], int nst) {
  us* q = out + o;
  if (nst >= 8) {
    if (((((uintptr_t)out >> 1) + (unsigned long long)o) & 1u) == 0) {
      *reinterpret_cast<u32x4_u*>(q) = pack8(h);
    } else {
      u32x2_u m;
      m.x = h[1] | (h[2] << 16); m.y = h[3] | (h[4] << 16);
      q[0] = (us)h[0];
      *reinterpret_cast<u32x2_u*>(q + 1) = m;
      *reinterpret_cast<unsigned*>(q + 5) = h[5] | (h[6] << 16);
      q[7] = (us)h[7];
    }
  } else {
    asm volatile("" : "+v"(nst));
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < nst) q[c] = (us)h[c];
  }
}

// fmaf(tap, x, acc) with the tap read from its scalar register.  Left to the compiler, pairs of these become
// v_pk_fma_f32, whose operands are VGPR pairs: the 16 taps would take 32 VGPRs and push the kernel into scratch.
__device__ __forceinline__ float fma_tap(float tap, float x, float acc) {
  asm("v_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "s"(tap), "v"(x));
  return acc;
}

template <typename T>
__global__ __launch_bounds__(256, 8) void ufd16_fir(const us* __restrict__ in, const float* __restrict__ kern,
                                                    us* __restrict__ out, const Fir16Params p) {
  // k[ky*4 + kx] of the embedded, flipped FIR: kernel[3 - ky][3 - kx] where that tap exists (uniform: scalar registers)
  float k[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int ry = 3 - (t >> 2), rx = 3 - (t & 3);
    k[t] = (ry < p.kh && rx < p.kw) ? kern[ry * p.kw + rx] : 0.f;
  }
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= p.items) return;
  const int g = (int)(item % p.groups);
  const long long t2 = item / p.groups;
  const int ty = (int)(t2 % p.tiles_y);
  const long long pl = t2 / p.tiles_y;
  const int ox0 = g * 8, oy0 = ty * p.th;
  const int cx0 = ox0 - p.pad_x0;                                  // input column under tap column 0 of output ox0
  const long long base = pl * p.in_h * p.in_w;                     // the plane, in elements from `in`
  long long orow = (pl * p.out_h + oy0) * p.out_w + ox0;           // output row of the tile in elements from `out`, advanced
                                                                   // as rows are stored
  unsigned colmask = 0;                                            // bit j: column cx0 + j lies in the row
#pragma unroll
  for (int j = 0; j < 11; ++j) colmask |= (cx0 + j >= 0 && cx0 + j < p.in_w) ? (1u << j) : 0u;
  const int nst = p.out_w - ox0;                                   // columns of this group that exist (>= 8: all)
  const int iy0 = oy0 - p.pad_y0;
  const int rows = min(p.th, p.out_h - oy0);                       // output rows of this lane's tile (the last tile: fewer)

  // th is a multiple of 4: th + 3 input rows, walked in groups of 4 with uniform bounds; lanes of a short last tile
  // keep loading (rows below the plane are zeros without a load) and skip the stores.
  Row16 win[4];
#pragma unroll 1
  for (int q = 0; q < p.th + 3; q += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = q + u;                                         // input row t of the tile: output row t - ky by tap row ky
      if (u == 3 && t >= p.th + 3) break;
      win[u] = fir_load_row(in, base, iy0 + t, cx0, colmask, p.in_h, p.in_w, p.total_in);
      if (t >= 3 && t - 3 < rows) {                                // output row t - 3: tap row ky sits in slot (u + 1 + ky) & 3
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
          if (3 - ky < p.kh) {
            const Row16& r = win[(u + 1 + ky) & 3];
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
              if (3 - kx < p.kw) {
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = fma_tap(k[ky * 4 + kx], row_elem<T>(r, c + kx), acc[c]);
              }
            }
          }
        }
        unsigned h[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = Io<T>::narrow(acc[c]);
        fir_store_row(out, orow, h, nst);
        orow += p.out_w;
      }
    }
  }
}

// ---------------------------------------------------------------- generic upfirdn2d, 16-bit data, fp32 taps
// One output per thread, any up / down / pad / kernel size / minor: ufd_generic of upfirdn2d.hip with 2-byte loads.
struct Ufd16Params {
  int in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, out_h, out_w;
};

template <typename T>
__global__ __launch_bounds__(256) void ufd16_generic(const us* __restrict__ in, const float* __restrict__ kern,
                                                     us* __restrict__ out, const Ufd16Params p, const long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int mi = (int)(idx % p.minor);
    long long t = idx / p.minor;
    const int ox = (int)(t % p.out_w);
    t /= p.out_w;
    const int oy = (int)(t % p.out_h);
    const long long mj = t / p.out_h;
    const int by = oy * p.down_y - p.pad_y0;
    const int bx = ox * p.down_x - p.pad_x0;
    const us* pin = in + mj * p.in_h * p.in_w * p.minor + mi;
    float v = 0.f;
    for (int ky = 0; ky < p.kh; ++ky) {
      const int uy = by + ky;
      if (uy < 0 || (uy % p.up_y) != 0) continue;
      const int iy = uy / p.up_y;
      if (iy >= p.in_h) continue;
      for (int kx = 0; kx < p.kw; ++kx) {
        const int ux = bx + kx;
        if (ux < 0 || (ux % p.up_x) != 0) continue;
        const int ix = ux / p.up_x;
        if (ix >= p.in_w) continue;
        v = __builtin_fmaf(Io<T>::widen(pin[((long long)iy * p.in_w + ix) * p.minor]),
                           kern[(p.kh - 1 - ky) * p.kw + (p.kw - 1 - kx)], v);
      }
    }
    out[idx] = (us)Io<T>::narrow(v);
  }
}

// ---------------------------------------------------------------- host
constexpr long long IDX_MAX = 0x7f000000LL;
bool dtype16(int dtype) { return dtype == FMGAN_F16 || dtype == FMGAN_BF16; }
bool odd(const void* p) { return ((uintptr_t)p & 1u) != 0; }

// 1: planes kernel (bias per run), 2: bias-innermost kernel, 3: planes kernel over the whole tensor as one run (no bias)
int fba_plan(int dtype, long long size_x, int size_b, int step_b, int act, int grad) {
  if (!dtype16(dtype)) return FMGAN_EUNSUPPORTED;
  if (size_x < 0 || size_b < 0 || step_b <= 0) return FMGAN_EINVAL;
  const int code = act * 10 + grad;
  if (code != 10 && code != 11 && code != 12 && code != 30 && code != 31 && code != 32) return FMGAN_EUNSUPPORTED;
  // 32-bit loop counters that advance by the grid's thread count (< 2^22): kept below IDX_MAX
  if (size_b == 0) return size_x / 8 > IDX_MAX ? FMGAN_EOVERFLOW : 3;
  if (step_b == 1) return size_x > IDX_MAX ? FMGAN_EOVERFLOW : 2;
  if (size_x % step_b) return FMGAN_EINVAL;
  return size_x / step_b > IDX_MAX ? FMGAN_EOVERFLOW : 1;
}

template <typename T, int CODE>
void launch_fba(int kind, const void* x, const float* bias, const void* ref, void* out, long long size_x, int size_b,
                int step_b, int code, float alpha, float scale, hipStream_t s) {
  const long long cap = (long long)FMGAN_NUM_CU * 32;
  if (kind == 2) {
    long long blocks = (size_x + 2047) / 2048;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((act16_fba_inner<T, CODE>), dim3((unsigned)blocks), dim3(256), 0, s, (us*)out, (const us*)x, bias,
                       (const us*)ref, (int)size_x, size_b, code, alpha, scale);
    return;
  }
  const long long planes = kind == 1 ? size_x / step_b : 1, step = kind == 1 ? step_b : size_x;
  long long gx = (step + 2047) / 2048;
  const long long gx_cap = planes == 1 ? cap : 64;
  if (gx > gx_cap) gx = gx_cap;
  const long long gy = planes < 65535 ? planes : 65535, gz = (planes + gy - 1) / gy;   // planes <= IDX_MAX: gz < 65536
  hipLaunchKernelGGL((act16_fba<T, CODE>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0, s, (us*)out, (const us*)x,
                     kind == 1 ? bias : nullptr, (const us*)ref, (int)planes, step, size_b > 0 ? size_b : 1, code, alpha, scale);
}

template <typename T>
void launch_fba_t(int kind, const void* x, const float* bias, const void* ref, void* out, long long size_x, int size_b,
                  int step_b, int code, float alpha, float scale, hipStream_t s) {
  if (code == 30) launch_fba<T, 30>(kind, x, bias, nullptr, out, size_x, size_b, step_b, code, alpha, scale, s);
  else if (code == 31 && ref) launch_fba<T, 31>(kind, x, bias, ref, out, size_x, size_b, step_b, code, alpha, scale, s);
  else launch_fba<T, 0>(kind, x, bias, ref, out, size_x, size_b, step_b, code, alpha, scale, s);
}

struct Ufd16Plan {
  int kernel;          // 1: ufd16_fir, 0: ufd16_generic
  Ufd16Params g;
  Fir16Params f;
  long long total;
  unsigned blocks;
};

int ufd16_plan(int dtype, long long major, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x,
               int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, Ufd16Plan& pl) {
  pl = Ufd16Plan{};
  if (!dtype16(dtype)) return FMGAN_EUNSUPPORTED;
  if (major < 0 || in_h <= 0 || in_w <= 0 || minor <= 0 || kh <= 0 || kw <= 0) return FMGAN_EINVAL;
  if (up_x <= 0 || up_y <= 0 || down_x <= 0 || down_y <= 0) return FMGAN_EINVAL;
  int out_h = 0, out_w = 0;
  fmgan_upfirdn2d_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, &out_h, &out_w);
  if (out_h <= 0 || out_w <= 0) return FMGAN_EINVAL;
  if ((long long)in_h * in_w * minor > 0x7fffffffLL || (long long)out_h * out_w * minor > 0x7fffffffLL ||
      major > 0x7fffffffLL)
    return FMGAN_EOVERFLOW;
  if (abs(pad_x0) > (1 << 24) || abs(pad_y0) > (1 << 24)) return FMGAN_EINVAL;
  const long long cap = (long long)FMGAN_NUM_CU * 32;
  pl.g = Ufd16Params{in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, out_h, out_w};
  if (minor == 1 && up_x == 1 && up_y == 1 && down_x == 1 && down_y == 1 && kh <= 4 && kw <= 4) {
    pl.kernel = 1;
    Fir16Params& f = pl.f;
    f.in_h = in_h; f.in_w = in_w; f.out_h = out_h; f.out_w = out_w;
    f.pad_x0 = pad_x0 + (4 - kw); f.pad_y0 = pad_y0 + (4 - kh);
    f.kh = kh; f.kw = kw;
    f.groups = (out_w + 7) / 8;
    // the tallest row tile (halo re-read 3 / th, from L2) that still gives every CU 32 waves
    f.th = 32;
    while (f.th > 4 && (major > 0 ? major : 1) * f.groups * ((out_h + f.th - 1) / f.th) < cap * 64) f.th >>= 1;
    f.tiles_y = (out_h + f.th - 1) / f.th;
    f.items = major * f.tiles_y * f.groups;
    f.total_in = major * in_h * in_w;
    if ((f.items + 255) / 256 > 0x7fffffffLL) return FMGAN_EOVERFLOW;
    pl.blocks = (unsigned)((f.items + 255) / 256);
    return FMGAN_OK;
  }
  pl.kernel = 0;
  pl.total = major * out_h * out_w * minor;
  const long long blocks = (pl.total + 255) / 256;
  pl.blocks = (unsigned)(blocks < cap ? blocks : cap);
  return FMGAN_OK;
}

template <typename T>
void launch_ufd16(const Ufd16Plan& pl, const void* in, const float* kern, void* out, hipStream_t s) {
  const dim3 g(pl.blocks), b(256);
  if (pl.kernel == 0) hipLaunchKernelGGL(ufd16_generic<T>, g, b, 0, s, (const us*)in, kern, (us*)out, pl.g, pl.total);
  else hipLaunchKernelGGL(ufd16_fir<T>, g, b, 0, s, (const us*)in, kern, (us*)out, pl.f);
}

}  // namespace

extern "C" int fmgan_act16_fba_select(int dtype, long long size_x, int size_b, int step_b, int act, int grad) {
  return fba_plan(dtype, size_x, size_b, step_b, act, grad);
}

extern "C" int fmgan_act16_fba(int dtype, const void* x, const float* bias, const void* refer, void* out,
                               long long size_x, int size_b, int step_b, int act, int grad, float alpha, float scale,
                               void* stream) {
  if (!bias) size_b = 0;
  const int kind = fba_plan(dtype, size_x, size_b, step_b, act, grad);
  if (kind < 0) return kind;
  if (size_x == 0) return FMGAN_OK;
  if (!x || !out || odd(x) || odd(out) || odd(refer) || ((uintptr_t)bias & 3u)) return FMGAN_EINVAL;
  const int code = act * 10 + grad;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FMGAN_BF16) launch_fba_t<BF16>(kind, x, bias, refer, out, size_x, size_b, step_b, code, alpha, scale, s);
  else launch_fba_t<F16>(kind, x, bias, refer, out, size_x, size_b, step_b, code, alpha, scale, s);
  return fmgan_check_launch();
}

// blocks per plane (= columns of the partial array) of fmgan_act16_fba_bwd; 0: arguments it does not serve
extern "C" int fmgan_act16_fba_bwd_blocks(long long planes, int hw) {
  if (planes <= 0 || hw <= 0 || planes > 0x7f000000LL || hw > 0x7f000000) return 0;
  int gx = (hw + 8191) / 8192;                 // >= 4 vectors of 8 per lane
  if (gx > 64) gx = 64;
  return gx;
}

extern "C" int fmgan_act16_fba_bwd(int dtype, const void* grad_out, const void* ref_out, void* grad_in, float* partial,
                                   long long planes, int hw, float alpha, float scale, void* stream) {
  if (!dtype16(dtype)) return FMGAN_EUNSUPPORTED;
  if (planes < 0 || hw <= 0) return FMGAN_EINVAL;
  if (planes == 0) return FMGAN_OK;
  if (planes > 0x7f000000LL || hw > 0x7f000000) return FMGAN_EOVERFLOW;
  if (!grad_out || !ref_out || !grad_in || !partial || odd(grad_out) || odd(ref_out) || odd(grad_in) ||
      ((uintptr_t)partial & 3u))
    return FMGAN_EINVAL;
  const int gx = fmgan_act16_fba_bwd_blocks(planes, hw);
  long long gy = planes;
  const long long cap = (long long)FMGAN_NUM_CU * 32 / gx;
  if (gy > cap) gy = cap > 0 ? cap : 1;
  if (gy > 65535) gy = 65535;
  const dim3 g((unsigned)gx, (unsigned)gy), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == FMGAN_BF16)
    hipLaunchKernelGGL(act16_fba_bwd<BF16>, g, b, 0, s, (us*)grad_in, partial, (const us*)grad_out, (const us*)ref_out,
                       (int)planes, hw, alpha, scale);
  else
    hipLaunchKernelGGL(act16_fba_bwd<F16>, g, b, 0, s, (us*)grad_in, partial, (const us*)grad_out, (const us*)ref_out,
                       (int)planes, hw, alpha, scale);
  return fmgan_check_launch();
}

extern "C" int fmgan_ufd16_select(int dtype, int major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                                  int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                                  int pad_y1) {
  Ufd16Plan pl;
  const int st = ufd16_plan(dtype, major, in_h, in_w, minor, kernel_h, kernel_w, up_x, up_y, down_x, down_y, pad_x0,
                            pad_x1, pad_y0, pad_y1, pl);
  return st != FMGAN_OK ? st : pl.kernel;
}

extern "C" int fmgan_ufd16(int dtype, const void* input, const float* kernel, void* out, int major, int in_h, int in_w,
                           int minor, int kernel_h, int kernel_w, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                           int pad_x1, int pad_y0, int pad_y1, void* stream) {
  Ufd16Plan pl;
  const int st = ufd16_plan(dtype, major, in_h, in_w, minor, kernel_h, kernel_w, up_x, up_y, down_x, down_y, pad_x0,
                            pad_x1, pad_y0, pad_y1, pl);
  if (st != FMGAN_OK || major == 0) return st;
  if (!input || !kernel || !out || odd(input) || odd(out) || ((uintptr_t)kernel & 3u)) return FMGAN_EINVAL;
  if (dtype == FMGAN_BF16) launch_ufd16<BF16>(pl, input, kernel, out, (hipStream_t)stream);
  else launch_ufd16<F16>(pl, input, kernel, out, (hipStream_t)stream);
  return fmgan_check_launch();
}
