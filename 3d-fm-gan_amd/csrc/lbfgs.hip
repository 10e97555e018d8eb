// L-BFGS on flat float32 state with the direction computed in Gram space (Evaluation/image_projection/LBFGS.py, the
// fused path of FullBatchLBFGS.step; include/fmgan_hip.h has the contract).
//
//   lbfgs_pair       one pass: gradients (through the segment table) -> g, the candidate pair s = t d, y = g - g_prev
//                    into the ring's spare slot, and per-block float64 partials of every product the Gram matrix needs
//   lbfgs_coeffs     one block: finalises the partials, accepts or rejects the pair, updates G and the ring, runs the
//                    two-loop recursion on coefficient vectors in R^(2k+1)
//   lbfgs_direction  one pass: d = sum coefficient * basis vector, g_prev = g, partials of g.d
//   lbfgs_update     param += a d through the table
//   lbfgs_gather     gradients -> flat g_new, partials of g_new.d
//   lbfgs_reduce     one block: the partials of a scalar product, added in a fixed order, into the scalar record
//
// Every sum is float64, added in a fixed order (lane products in element order, the xor butterfly of block_sum.h widened
// to double, the waves as (0 + 1) + (2 + 3), the blocks in order): no atomics, two runs give the same bits.
#include "common.h"

#define LB_THREADS 256
#define LB_WAVES (LB_THREADS / FMGAN_WAVE)
#define LB_PER_LANE 8                                  // elements a lane of lbfgs_pair keeps in registers
#define LB_TILE (LB_THREADS * LB_PER_LANE)
#define LB_MAX_M 32
#define LB_MAX_SEG 64
#define LB_MAX_Q (6 * LB_MAX_M + 7)
#define LB_MAX_K (2 * LB_MAX_M + 1)
#define LB_STREAM_BLOCKS 2048                          // grid cap of the passes that leave one partial per block
#define LBC_THREADS 1024                               // lbfgs_coeffs: one block
#define LBC_PARTS 8                                    // ... whose threads add the partial rows in 8 interleaved parts

// int state: [0] head slot, [1] live pairs, [2 ..] the live slots, oldest first.
// record (double): [0] accepted, [1] H_diag, [2] ys, [3] sBs, [4] g.d, [5] g_new.d, [6] g.g, [7] yy.
enum { REC_ACCEPTED = 0, REC_HDIAG, REC_YS, REC_SBS, REC_GTD, REC_GTD_NEW, REC_GG, REC_YY };

struct LbSegs {
  float* param[LB_MAX_SEG];
  const float* grad[LB_MAX_SEG];
  long long end[LB_MAX_SEG];      // flat offset one past the segment's last element
  int nseg;
};

__device__ __forceinline__ double wave_sum_xor_f64(double acc) {
#pragma unroll
  for (int m = FMGAN_WAVE / 2; m > 0; m >>= 1) acc += __shfl_xor(acc, m, FMGAN_WAVE);
  return acc;
}

// block_sum.h's association in double; every thread calls it, thread 0 uses the value.
__device__ __forceinline__ double block_sum_ordered_f64(double acc, double* red) {
  acc = wave_sum_xor_f64(acc);
  if ((threadIdx.x & (FMGAN_WAVE - 1)) == 0) red[threadIdx.x / FMGAN_WAVE] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Segment of flat element e, searched upwards from `seg` (the elements of a tile ascend; empty segments are passed).
__device__ __forceinline__ int seg_of(const LbSegs& segs, long long e, int seg) {
  while (seg < segs.nseg - 1 && e >= segs.end[seg]) ++seg;
  return seg;
}

__device__ __forceinline__ int seg_first(const LbSegs& segs, long long e) {
  int lo = 0, hi = segs.nseg - 1;       // first segment whose end is beyond e
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e >= segs.end[mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long seg_begin(const LbSegs& segs, int seg) { return seg == 0 ? 0 : segs.end[seg - 1]; }

// f(i, e, seg, offset in the segment) for the elements e = base + i * LB_THREADS + threadIdx.x < n of the tile at `base`,
// i ascending.  A tile inside one segment (all but a few of them: the noise maps are large) takes the segment from the
// block's own search, a uniform value; only a tile that straddles segments searches per element.
template <typename F>
__device__ __forceinline__ void for_tile_elements(const LbSegs& segs, long long base, long long n, F f) {
  const int seg0 = seg_first(segs, base);
  const long long lim = base + LB_TILE < n ? base + LB_TILE : n;
  if (lim <= segs.end[seg0]) {
    const long long begin = seg_begin(segs, seg0);
#pragma unroll
    for (int i = 0; i < LB_PER_LANE; ++i) {
      const long long e = base + i * LB_THREADS + threadIdx.x;
      if (e < n) f(i, e, seg0, e - begin);
    }
  } else {
    int seg = seg0;
#pragma unroll
    for (int i = 0; i < LB_PER_LANE; ++i) {
      const long long e = base + i * LB_THREADS + threadIdx.x;
      if (e < n) {
        seg = seg_of(segs, e, seg);
        f(i, e, seg, e - seg_begin(segs, seg));
      }
    }
  }
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_pair(const LbSegs segs, float* __restrict__ g,
                                                         const float* __restrict__ g_prev, const float* __restrict__ d,
                                                         float* __restrict__ S, float* __restrict__ Y,
                                                         const int* __restrict__ ist, double* __restrict__ partial,
                                                         long long n, int m, float t, int has_pair) {
  __shared__ double red[LB_MAX_Q][LB_WAVES];
  const int tid = threadIdx.x, lane = tid & (FMGAN_WAVE - 1), wave = tid / FMGAN_WAVE;
  const int slots = m + 1, head = ist[0], count = ist[1], cand = (head + 1) % slots, Q = 6 * m + 7, T = 6 * m;
  const long long base = (long long)blockIdx.x * LB_TILE;
  float gv[LB_PER_LANE], sv[LB_PER_LANE], yv[LB_PER_LANE];
  double a_ss = 0, a_sy = 0, a_yy = 0, a_sg = 0, a_yg = 0, a_gg = 0, a_sp = 0;
#pragma unroll
  for (int i = 0; i < LB_PER_LANE; ++i) gv[i] = sv[i] = yv[i] = 0.f;
  for_tile_elements(segs, base, n, [&](int i, long long e, int seg, long long off) {
    const float* gp = segs.grad[seg];
    gv[i] = gp ? gp[off] : 0.f;
    g[e] = gv[i];
    if (has_pair) {
      const float gpv = g_prev[e];
      sv[i] = t * d[e];
      yv[i] = gv[i] - gpv;
      S[(long long)cand * n + e] = sv[i];
      Y[(long long)cand * n + e] = yv[i];
      a_sp += (double)sv[i] * (double)gpv;
    }
  });
#pragma unroll
  for (int i = 0; i < LB_PER_LANE; ++i) {
    a_ss += (double)sv[i] * (double)sv[i];
    a_sy += (double)sv[i] * (double)yv[i];
    a_yy += (double)yv[i] * (double)yv[i];
    a_sg += (double)sv[i] * (double)gv[i];
    a_yg += (double)yv[i] * (double)gv[i];
    a_gg += (double)gv[i] * (double)gv[i];
  }
  double tail[7] = {a_ss, a_sy, a_yy, a_sg, a_yg, a_gg, a_sp};
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const double v = wave_sum_xor_f64(tail[q]);
    if (lane == 0) red[T + q][wave] = v;
  }
  // the history on the outside: each live slot is read once, against the tile held in registers
  for (int j = 0; j < count; ++j) {
    const int slot = (head - count + 1 + j + slots) % slots;
    const float* __restrict__ sj = S + (long long)slot * n;
    const float* __restrict__ yj = Y + (long long)slot * n;
    double acc[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < LB_PER_LANE; ++i) {
      const long long e = base + i * LB_THREADS + tid;
      float a = 0.f, b = 0.f;
      if (e < n) {
        a = sj[e];
        b = yj[e];
      }
      acc[0] += (double)a * (double)sv[i];
      acc[1] += (double)a * (double)yv[i];
      acc[2] += (double)a * (double)gv[i];
      acc[3] += (double)b * (double)sv[i];
      acc[4] += (double)b * (double)yv[i];
      acc[5] += (double)b * (double)gv[i];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double v = wave_sum_xor_f64(acc[q]);
      if (lane == 0) red[6 * j + q][wave] = v;
    }
  }
  __syncthreads();
  for (int q = tid; q < Q; q += LB_THREADS) {
    const bool live = q >= T || q < 6 * count;
    partial[(long long)blockIdx.x * Q + q] = live ? (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]) : 0.0;
  }
}

__global__ __launch_bounds__(LBC_THREADS) void lbfgs_coeffs(const double* __restrict__ partial, int nblocks, int m,
                                                           double* __restrict__ G, int* __restrict__ ist,
                                                           double* __restrict__ rec, double* __restrict__ coef, float t,
                                                           float eps, int has_pair) {
  __shared__ double sum[LB_MAX_Q];
  __shared__ double part[LBC_PARTS][LB_MAX_Q];
  __shared__ double Gc[LB_MAX_K * LB_MAX_K];
  __shared__ double qv[LB_MAX_K], rv[LB_MAX_K], al[LB_MAX_M], rho[LB_MAX_M];
  __shared__ int slot[LB_MAX_M];
  __shared__ int live;
  const int tid = threadIdx.x, Q = 6 * m + 7, T = 6 * m, slots = m + 1, D = 2 * slots + 1, gI = 2 * slots;
  // rows p, p + 8, p + 16, ... of the partials in part p, then the parts in order: a fixed order
  for (int idx = tid; idx < Q * LBC_PARTS; idx += LBC_THREADS) {
    const int q = idx % Q, p = idx / Q;
    double a = 0;
#pragma unroll 8
    for (int b = p; b < nblocks; b += LBC_PARTS) a += partial[(long long)b * Q + q];
    part[p][q] = a;
  }
  for (int i = tid; i < D; i += LBC_THREADS) coef[i] = 0.0;
  __syncthreads();
  if (tid < Q) {
    double a = part[0][tid];
#pragma unroll
    for (int p = 1; p < LBC_PARTS; ++p) a += part[p][tid];
    sum[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    int head = ist[0], count = ist[1];
    const int cand = (head + 1) % slots;
    for (int i = 0; i < count; ++i) {
      const int sl = (head - count + 1 + i + slots) % slots;
      G[gI * D + sl] = G[sl * D + gI] = sum[6 * i + 2];
      G[gI * D + slots + sl] = G[(slots + sl) * D + gI] = sum[6 * i + 5];
    }
    G[gI * D + gI] = sum[T + 5];
    const double ys = sum[T + 1], yy = sum[T + 2], sBs = -(double)t * sum[T + 6];
    const bool accepted = has_pair && ys > (double)eps * sBs;
    if (accepted) {
      const int cs = cand, cy = slots + cand;
      for (int i = 0; i < count; ++i) {
        const int sl = (head - count + 1 + i + slots) % slots;
        G[cs * D + sl] = G[sl * D + cs] = sum[6 * i + 0];
        G[cy * D + sl] = G[sl * D + cy] = sum[6 * i + 1];
        G[cs * D + slots + sl] = G[(slots + sl) * D + cs] = sum[6 * i + 3];
        G[cy * D + slots + sl] = G[(slots + sl) * D + cy] = sum[6 * i + 4];
      }
      G[cs * D + cs] = sum[T + 0];
      G[cs * D + cy] = G[cy * D + cs] = ys;
      G[cy * D + cy] = yy;
      G[cs * D + gI] = G[gI * D + cs] = sum[T + 3];
      G[cy * D + gI] = G[gI * D + cy] = sum[T + 4];
      head = cand;
      count = count < m ? count + 1 : m;
      rec[REC_HDIAG] = ys / yy;
    }
    ist[0] = head;
    ist[1] = count;
    for (int i = 0; i < count; ++i) ist[2 + i] = slot[i] = (head - count + 1 + i + slots) % slots;
    live = count;
    rec[REC_ACCEPTED] = accepted ? 1.0 : 0.0;
    rec[REC_YS] = has_pair ? ys : 0.0;
    rec[REC_SBS] = has_pair ? sBs : 0.0;
    rec[REC_YY] = has_pair ? yy : 0.0;
    rec[REC_GG] = sum[T + 5];
  }
  __syncthreads();
  const int k = live, K = 2 * k + 1;
  // the live part of G in the order s_1..s_k, y_1..y_k, g
  for (int idx = tid; idx < K * K; idx += LBC_THREADS) {
    const int a = idx / K, b = idx % K;
    const int ra = a < k ? slot[a] : a < 2 * k ? slots + slot[a - k] : gI;
    const int rb = b < k ? slot[b] : b < 2 * k ? slots + slot[b - k] : gI;
    Gc[idx] = G[ra * D + rb];
  }
  __syncthreads();
  if (tid == 0) {
    for (int j = 0; j < K; ++j) qv[j] = 0.0;
    qv[2 * k] = -1.0;
    for (int i = 0; i < k; ++i) rho[i] = 1.0 / Gc[i * K + k + i];
    for (int i = k - 1; i >= 0; --i) {
      double a = 0;
      for (int j = 0; j < K; ++j) a += Gc[i * K + j] * qv[j];
      al[i] = a * rho[i];
      qv[k + i] -= al[i];
    }
    const double gamma = rec[REC_HDIAG];
    for (int j = 0; j < K; ++j) rv[j] = gamma * qv[j];
    for (int i = 0; i < k; ++i) {
      double b = 0;
      for (int j = 0; j < K; ++j) b += Gc[(k + i) * K + j] * rv[j];
      rv[i] += al[i] - b * rho[i];
    }
    for (int i = 0; i < k; ++i) {
      coef[slot[i]] = rv[i];
      coef[slots + slot[i]] = rv[k + i];
    }
    coef[gI] = rv[2 * k];
  }
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_direction(const double* __restrict__ coef, const int* __restrict__ ist,
                                                              const float* __restrict__ S, const float* __restrict__ Y,
                                                              const float* __restrict__ g, float* __restrict__ g_prev,
                                                              float* __restrict__ d, double* __restrict__ partial,
                                                              long long n, int m) {
  __shared__ double red[LB_WAVES];
  const int slots = m + 1, k = ist[1];
  const double cg = coef[2 * slots];
  double gd = 0;
  for (long long e = (long long)blockIdx.x * LB_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * LB_THREADS) {
    const float gv = g[e];
    double acc = cg * (double)gv;
    for (int i = 0; i < k; ++i) {
      const int sl = ist[2 + i];
      acc += coef[sl] * (double)S[(long long)sl * n + e];
      acc += coef[slots + sl] * (double)Y[(long long)sl * n + e];
    }
    const float dv = (float)acc;
    d[e] = dv;
    g_prev[e] = gv;
    gd += (double)gv * (double)dv;
  }
  gd = block_sum_ordered_f64(gd, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = gd;
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_update(const LbSegs segs, const float* __restrict__ d, float a,
                                                           long long n) {
  for (long long base = (long long)blockIdx.x * LB_TILE; base < n; base += (long long)gridDim.x * LB_TILE)
    for_tile_elements(segs, base, n, [&](int, long long e, int seg, long long off) {
      float* p = segs.param[seg] + off;
      *p = __builtin_fmaf(a, d[e], *p);
    });
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_gather(const LbSegs segs, float* __restrict__ g_new,
                                                           const float* __restrict__ d, double* __restrict__ partial,
                                                           long long n) {
  __shared__ double red[LB_WAVES];
  double gd = 0;
  for (long long base = (long long)blockIdx.x * LB_TILE; base < n; base += (long long)gridDim.x * LB_TILE)
    for_tile_elements(segs, base, n, [&](int, long long e, int seg, long long off) {
      const float* gp = segs.grad[seg];
      const float gv = gp ? gp[off] : 0.f;
      g_new[e] = gv;
      gd += (double)gv * (double)d[e];
    });
  gd = block_sum_ordered_f64(gd, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = gd;
}

__global__ __launch_bounds__(LB_THREADS) void lbfgs_reduce(const double* __restrict__ partial, int nblocks,
                                                           double* __restrict__ out) {
  __shared__ double red[LB_WAVES];
  double a = 0;
  for (int b = threadIdx.x; b < nblocks; b += LB_THREADS) a += partial[b];
  a = block_sum_ordered_f64(a, red);
  if (threadIdx.x == 0) *out = a;
}

// ---------------------------------------------------------------------------------------------- host side
static int lb_segs(const long long* table, int nseg, long long n, LbSegs* out) {
  if (!table || nseg < 1 || nseg > LB_MAX_SEG || n <= 0) return FMGAN_EINVAL;
  long long end = 0;
  for (int i = 0; i < nseg; ++i) {
    const long long numel = table[3 * i + 2];
    if (numel < 0 || (numel > 0 && !table[3 * i])) return FMGAN_EINVAL;
    end += numel;
    out->param[i] = (float*)(uintptr_t)table[3 * i];
    out->grad[i] = (const float*)(uintptr_t)table[3 * i + 1];
    out->end[i] = end;
  }
  out->nseg = nseg;
  return end == n ? FMGAN_OK : FMGAN_EINVAL;
}

static int lb_stream_blocks(long long n, int per_block) {
  const long long b = (n + per_block - 1) / per_block;
  return (int)(b < LB_STREAM_BLOCKS ? b : LB_STREAM_BLOCKS);
}

extern "C" long long fmgan_lbfgs_pair_blocks(long long n) {
  if (n <= 0) return 0;
  const long long b = (n + LB_TILE - 1) / LB_TILE;
  return b > 0x7fffffffLL ? 0 : b;
}

extern "C" int fmgan_lbfgs_pair_f32(const long long* segs, int nseg, float* g, const float* g_prev, const float* d,
                                    float* S, float* Y, const void* state, double* partial, long long n, int m, float t,
                                    int has_pair, void* stream) {
  LbSegs tab;
  const int st = lb_segs(segs, nseg, n, &tab);
  if (st != FMGAN_OK) return st;
  if (!g || !g_prev || !d || !S || !Y || !state || !partial) return FMGAN_EINVAL;
  if (m < 1 || m > LB_MAX_M) return FMGAN_EUNSUPPORTED;
  const long long blocks = fmgan_lbfgs_pair_blocks(n);
  if (blocks <= 0) return FMGAN_EOVERFLOW;
  hipLaunchKernelGGL(lbfgs_pair, dim3((unsigned)blocks), dim3(LB_THREADS), 0, (hipStream_t)stream, tab, g, g_prev, d, S, Y,
                     (const int*)state, partial, n, m, t, has_pair ? 1 : 0);
  return fmgan_check_launch();
}

extern "C" int fmgan_lbfgs_coeffs_f64(const double* partial, double* G, void* state, double* record, double* coef,
                                      long long n, int m, float t, float eps, int has_pair, void* stream) {
  if (!partial || !G || !state || !record || !coef || n <= 0) return FMGAN_EINVAL;
  if (m < 1 || m > LB_MAX_M) return FMGAN_EUNSUPPORTED;
  const long long blocks = fmgan_lbfgs_pair_blocks(n);
  if (blocks <= 0) return FMGAN_EOVERFLOW;
  hipLaunchKernelGGL(lbfgs_coeffs, dim3(1), dim3(LBC_THREADS), 0, (hipStream_t)stream, partial, (int)blocks, m, G, (int*)state,
                     record, coef, t, eps, has_pair ? 1 : 0);
  return fmgan_check_launch();
}

extern "C" int fmgan_lbfgs_direction_f32(const double* coef, const void* state, const float* S, const float* Y,
                                         const float* g, float* g_prev, float* d, double* partial, double* record,
                                         long long n, int m, void* stream) {
  if (!coef || !state || !S || !Y || !g || !g_prev || !d || !partial || !record || n <= 0) return FMGAN_EINVAL;
  if (m < 1 || m > LB_MAX_M) return FMGAN_EUNSUPPORTED;
  const int blocks = lb_stream_blocks(n, LB_THREADS);
  hipLaunchKernelGGL(lbfgs_direction, dim3(blocks), dim3(LB_THREADS), 0, (hipStream_t)stream, coef, (const int*)state, S, Y, g, g_prev,
                     d, partial, n, m);
  hipLaunchKernelGGL(lbfgs_reduce, dim3(1), dim3(LB_THREADS), 0, (hipStream_t)stream, (const double*)partial, blocks,
                     record + REC_GTD);
  return fmgan_check_launch();
}

extern "C" int fmgan_lbfgs_update_f32(const long long* segs, int nseg, const float* d, float a, long long n,
                                      void* stream) {
  LbSegs tab;
  const int st = lb_segs(segs, nseg, n, &tab);
  if (st != FMGAN_OK) return st;
  if (!d) return FMGAN_EINVAL;
  hipLaunchKernelGGL(lbfgs_update, dim3(lb_stream_blocks(n, LB_TILE)), dim3(LB_THREADS), 0, (hipStream_t)stream, tab, d, a, n);
  return fmgan_check_launch();
}

extern "C" int fmgan_lbfgs_gather_f32(const long long* segs, int nseg, float* g_new, const float* d, double* partial,
                                      double* record, long long n, void* stream) {
  LbSegs tab;
  const int st = lb_segs(segs, nseg, n, &tab);
  if (st != FMGAN_OK) return st;
  if (!g_new || !d || !partial || !record) return FMGAN_EINVAL;
  const int blocks = lb_stream_blocks(n, LB_TILE);
  hipLaunchKernelGGL(lbfgs_gather, dim3(blocks), dim3(LB_THREADS), 0, (hipStream_t)stream, tab, g_new, d, partial, n);
  hipLaunchKernelGGL(lbfgs_reduce, dim3(1), dim3(LB_THREADS), 0, (hipStream_t)stream, (const double*)partial, blocks,
                     record + REC_GTD_NEW);
  return fmgan_check_launch();
}
