// Weight gradients of the modulated convolutions for gfx950 (MI355X), on v_mfma_f32_32x32x2_f32 (exact fp32, as the
// forward kernel of modconv_fwd.hip): a 32 x 32 tile for the narrow plain layers and a 64 x 64 tile for every mode.
#include "common.h"

namespace {

// ------------------------------------------------------------------ weight gradient of the plain conv (MFMA)
// gw[o,i,ky,kx] = sum_{b,y,x} (d[b,o] * go[b,o,y,x]) * (s[b,i] * x[b,i,y+ky-1,x+kx-1])
// GEMM with M = Cout (A rows), N = Cin (B columns), K = pixels; the 9 taps are 9 accumulators that share the A
// operand and read B at 9 constant offsets of the staged halo patch.  A block owns a 32(o) x 32(i) tile; its four
// waves take the four 32-pixel quarters of each 128-pixel tile (so a chunk is 16 K-steps x 9 MFMAs per wave) and are
// summed through LDS at the end; the pixel range is split over blocks (fixed-order finish, no atomics).
struct WGParams {
  const float* go; const float* d; const float* x; const float* s; float* partial;
  int batch, cin, cout, h, w;
  int tw_log2, th, tiles_x, tiles_y, ntiles, ksplit, tiles_per_split, o_tiles, i_tiles;
};

__global__ __launch_bounds__(256, 2) void modconv_wgrad_f32(const WGParams p) {
  constexpr int SA = 129;                      // Gz row stride (128 pixels + 1: conflict-free across o)
  extern __shared__ float smem[];
  const int TW = 1 << p.tw_log2, PWP = TW + 2, PH = p.th + 2;
  const int SB = PH * PWP + 1 + ((PH * PWP) & 1);   // odd stride: conflict-free across i
  float* Gz = smem;                            // [32][SA]
  float* Us = smem + 32 * SA;                  // [32][SB]
  // wave index as an SGPR: LDS-DMA destinations (M0), piece guards and tile offsets derived from it stay scalar
  // (left in a VGPR, every `buffer_load ... lds` sat in a waterfall loop with v_readfirstlane)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;
  const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int o_tile = lb % p.o_tiles;
  const int i_tile = (lb / p.o_tiles) % p.i_tiles;
  const int ks = lb / (p.o_tiles * p.i_tiles);
  const int o0 = o_tile * 32, i0 = i_tile * 32;
  const int hw = p.h * p.w;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int t_begin = ks * p.tiles_per_split, t_end = min(p.ntiles, t_begin + p.tiles_per_split);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int tx = tile % p.tiles_x;
    const int ty = (tile / p.tiles_x) % p.tiles_y;
    const int b = tile / (p.tiles_x * p.tiles_y);
    const int y0 = ty * p.th, x0 = tx * TW;
    __syncthreads();
    // A: 32 output channels x 128 pixels of d*go
    for (int idx = tid; idx < 32 * 128; idx += 256) {
      const int o = idx >> 7, pix = idx & 127;
      const int y = y0 + (pix >> p.tw_log2), x = x0 + (pix & (TW - 1));
      float v = 0.f;
      if (o0 + o < p.cout && y < p.h && x < p.w) {
        const long long ch = (long long)b * p.cout + o0 + o;
        v = p.go[ch * hw + y * p.w + x];
        if (p.d) v *= p.d[ch];
      }
      Gz[o * SA + pix] = v;
    }
    // B: 32 input channels x halo patch of s*x
    const int patch = PH * PWP;
    for (int idx = tid; idx < 32 * patch; idx += 256) {
      const int i = idx / patch, q = idx - i * patch;
      const int y = y0 + q / PWP - 1, x = x0 + q % PWP - 1;
      float v = 0.f;
      if (i0 + i < p.cin && y >= 0 && y < p.h && x >= 0 && x < p.w) {
        const long long ch = (long long)b * p.cin + i0 + i;
        v = p.x[ch * hw + y * p.w + x] * p.s[ch];
      }
      Us[i * SB + q] = v;
    }
    __syncthreads();
    const float* ga = Gz + l31 * SA + wave * 32 + khalf;
    const float* ub = Us + l31 * SB;
    float a_cur, b_cur[9], a_nxt = 0.f, b_nxt[9];
    auto fetch = [&](float& a, float (&bb)[9], int j) {
      const int pix = wave * 32 + 2 * j + khalf;
      const int off = (pix >> p.tw_log2) * PWP + (pix & (TW - 1));
      a = ga[2 * j];
#pragma unroll
      for (int t = 0; t < 9; ++t) bb[t] = ub[off + (t / 3) * PWP + (t % 3)];
    };
    fetch(a_cur, b_cur, 0);
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      __builtin_amdgcn_sched_barrier(0);
      if (j + 1 < 16) fetch(a_nxt, b_nxt, j + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[t], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
#pragma unroll
      for (int t = 0; t < 9; ++t) b_cur[t] = b_nxt[t];
    }
  }
  // sum the four waves through LDS, one tap at a time, and write the block's partial slab [ks][t][o][i]
  float* red = smem;   // [4][32][33]
  float* slab = p.partial + (long long)ks * 9 * p.cout * p.cin;
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = (r & 3) + 8 * (r >> 2) + 4 * khalf;
      red[(wave * 32 + o) * 33 + l31] = acc[t][r];
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += 256) {
      const int o = e >> 5, i = e & 31;
      const float v = red[o * 33 + i] + red[(32 + o) * 33 + i] + red[(64 + o) * 33 + i] + red[(96 + o) * 33 + i];
      if (o0 + o < p.cout && i0 + i < p.cin) slab[((long long)t * p.cout + o0 + o) * p.cin + i0 + i] = v;
    }
  }
}

// gw[o][i][t] = scale * sum_ks partial[ks][t][o][i]
__global__ __launch_bounds__(256) void modconv_wgrad_finish_f32(const float* __restrict__ partial, float* __restrict__ gw,
                                                                int cout, int cin, int ksplit, float scale) {
  const int total = cout * cin * 9;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int t = idx % 9, oi = idx / 9;
    float v = 0.f;
    for (int ks = 0; ks < ksplit; ++ks) v += partial[((long long)ks * 9 + t) * cout * cin + oi];
    gw[idx] = v * scale;
  }
}


// ---- 64 x 64 weight-gradient tile (round 2).  The 32 x 32 kernel above spends most of its time filling LDS: every
// 144 MFMAs of a wave need a new 128-pixel tile, and a block re-reads gz / u for a quarter of the output a 64 x 64 tile
// covers.  Here a block owns 64 (o) x 64 (i), its four waves the four 32 x 32 quadrants, and ALL of them walk the same
// 2 x TW pixels per step: 2 TW/2... = TW K-steps x 9 MFMAs = 288 MFMAs per wave between two barriers (TW = 32), with the
// pixel pair of an MFMA (its K = 2) taken from the two rows — so consecutive K-steps move one pixel along x and the
// 3 x 3 window of the shifted operand slides: 3 new LDS reads per step instead of 9 (+1 for gz): 4 reads per 9 MFMAs.
struct WG64Params {
  // R[t][a][b] = sum_{n,y,x} (sa[n,a] * A[n,a,y,x]) * (sb[n,b] * B[n,b, SP*y + ky - ORG, SP*x + kx - ORG])
  //   SP = 1, ORG = 1: plain conv        A = go [cout, h, w],          B = x  [cin, h, w]         gw[o=a][i=b]
  //   SP = 2, ORG = 0: transposed conv   A = x  [cin, h, w],           B = go [cout, 2h+1, 2w+1]  gw[o=b][i=a]
  //   SP = 2, ORG = 0: stride-2 conv     A = go [cout, h', w'],        B = x  [cin, h, w]         gw[o=a][i=b]
  const float* A; const float* sa; const float* B; const float* sb; float* partial;
  int batch, ca, cb, ha, wa, hb, wb;
  int tiles_x, tiles_y, ntiles, ksplit, tiles_per_split, a_tiles, b_tiles;
};

template <int TWL2, int SP>
__global__ __launch_bounds__(256, 2) void modconv_wgrad64_f32(const WG64Params p) {
  constexpr int TW = 1 << TWL2, ORG = SP == 1 ? 1 : 0;
  constexpr int PA = 2 * TW + 1;                          // odd pitches: conflict-free over channels
  constexpr int BR = SP + 3, PWP = SP * (TW - 1) + 3;     // rows / columns of the shifted operand's patch
  constexpr int PB = (BR * PWP) | 1;
  // per thread: float4 of A; of B: float4 of the row interiors + the scalars left over
  constexpr int NA4 = 64 * 2 * TW / 4 / 256;
  constexpr int RV = SP == 1 ? TW / 4 : PWP / 4;          // float4 per patch row (SP 1: the aligned interior x0 .. x0+TW-1)
  constexpr int RS = PWP - 4 * RV;                        // scalars per patch row (SP 1: the two halo columns)
  constexpr int NB4 = (64 * BR * RV + 255) / 256, NBS = (64 * BR * RS + 255) / 256;
  extern __shared__ float smem[];
  float* As = smem;               // [64][PA]
  float* Bs = smem + 64 * PA;     // [64][PB]
  // wave index as an SGPR: LDS-DMA destinations (M0), piece guards and tile offsets derived from it stay scalar
  // (left in a VGPR, every `buffer_load ... lds` sat in a waterfall loop with v_readfirstlane)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5;
  const int aq = wave >> 1, bq = wave & 1;
  const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int a_tile = lb % p.a_tiles;
  const int b_tile = (lb / p.a_tiles) % p.b_tiles;
  const int ks = lb / (p.a_tiles * p.b_tiles);
  const int a0 = a_tile * 64, b0 = b_tile * 64;
  const long long hwa = (long long)p.ha * p.wa, hwb = (long long)p.hb * p.wb;
  // A rows start 16-byte aligned and a float4 never straddles the right edge (B is read with dword-aligned vectors)
  const bool vec = (p.wa & 3) == 0 && (((uintptr_t)p.A) & 15) == 0 && (((uintptr_t)p.B) & 3) == 0;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // ---- staging plan: everything a tile step needs is loaded into registers while the previous step is on the
  // matrix pipe and written to LDS after the barrier (the forward kernel's register pipeline)
  f32x4 a4[NA4], b4[NB4];
  float bs[NBS], sa_n = 1.f, sb_n = 1.f, sa_lane = 1.f, sb_lane = 1.f;
  const int my_a = a0 + aq * 32 + l31, my_b = b0 + bq * 32 + l31;
  auto decode = [&](int tile, int& n, int& y0, int& x0) {
    const int tx = tile % p.tiles_x;
    const int ty = (tile / p.tiles_x) % p.tiles_y;
    n = tile / (p.tiles_x * p.tiles_y);
    y0 = ty * 2; x0 = tx * TW;
  };
  // patch (row r, column c) of the shifted operand <-> its pixel
  auto issue = [&](int tile) {
    int n, y0, x0;
    decode(tile, n, y0, x0);
    sa_n = (p.sa && my_a < p.ca) ? p.sa[(long long)n * p.ca + my_a] : (my_a < p.ca ? 1.f : 0.f);
    sb_n = (p.sb && my_b < p.cb) ? p.sb[(long long)n * p.cb + my_b] : (my_b < p.cb ? 1.f : 0.f);
    if (!vec) return;
#pragma unroll
    for (int k = 0; k < NA4; ++k) {
      const int q = tid + 256 * k;
      const int a = q / (2 * TW / 4), rem = q % (2 * TW / 4);
      const int y = y0 + rem / (TW / 4), x = x0 + 4 * (rem % (TW / 4));
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (a0 + a < p.ca && y < p.ha && x < p.wa)
        v = *reinterpret_cast<const f32x4*>(p.A + ((long long)n * p.ca + a0 + a) * hwa + (long long)y * p.wa + x);
      a4[k] = v;
    }
    const int by0 = SP * y0 - ORG, bx0 = SP * x0 - ORG;
#pragma unroll
    for (int k = 0; k < NB4; ++k) {
      const int q = tid + 256 * k;
      const int b = q / (BR * RV), rem = q % (BR * RV);
      const int y = by0 + rem / RV, c = (SP == 1 ? 1 : 0) + 4 * (rem % RV), x = bx0 + c;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (q < 64 * BR * RV && b0 + b < p.cb && y >= 0 && y < p.hb) {
        const float* src = p.B + ((long long)n * p.cb + b0 + b) * hwb + (long long)y * p.wb + x;
        if (x >= 0 && x + 3 < p.wb) {
          const f32x4_u t = *reinterpret_cast<const f32x4_u*>(src);
          v.x = t.x; v.y = t.y; v.z = t.z; v.w = t.w;
        } else {
          if (x + 0 >= 0 && x + 0 < p.wb) v.x = src[0];
          if (x + 1 >= 0 && x + 1 < p.wb) v.y = src[1];
          if (x + 2 >= 0 && x + 2 < p.wb) v.z = src[2];
          if (x + 3 >= 0 && x + 3 < p.wb) v.w = src[3];
        }
      }
      b4[k] = v;
    }
#pragma unroll
    for (int k = 0; k < NBS; ++k) {
      const int q = tid + 256 * k;
      const int b = q / (BR * RS), rem = q % (BR * RS);
      const int r = rem / RS, e = rem % RS;
      // SP 1: the two halo columns 0 and TW+1; SP 2: the column(s) after the last float4
      const int c = SP == 1 ? (e ? TW + 1 : 0) : 4 * RV + e;
      const int y = by0 + r, x = bx0 + c;
      bs[k] = (q < 64 * BR * RS && b0 + b < p.cb && y >= 0 && y < p.hb && x >= 0 && x < p.wb)
                  ? p.B[((long long)n * p.cb + b0 + b) * hwb + (long long)y * p.wb + x] : 0.f;
    }
  };
  auto commit = [&](int tile) {
    sa_lane = sa_n; sb_lane = sb_n;
    if (vec) {
#pragma unroll
      for (int k = 0; k < NA4; ++k) {
        const int q = tid + 256 * k;
        const int a = q / (2 * TW / 4), rem = q % (2 * TW / 4);
        float* dst = As + a * PA + 4 * rem;                // (row r, column 4*c4) = r*TW + 4*c4 = 4*rem
        dst[0] = a4[k].x; dst[1] = a4[k].y; dst[2] = a4[k].z; dst[3] = a4[k].w;
      }
#pragma unroll
      for (int k = 0; k < NB4; ++k) {
        const int q = tid + 256 * k;
        if (q < 64 * BR * RV) {
          const int b = q / (BR * RV), rem = q % (BR * RV);
          float* dst = Bs + b * PB + (rem / RV) * PWP + (SP == 1 ? 1 : 0) + 4 * (rem % RV);
          dst[0] = b4[k].x; dst[1] = b4[k].y; dst[2] = b4[k].z; dst[3] = b4[k].w;
        }
      }
#pragma unroll
      for (int k = 0; k < NBS; ++k) {
        const int q = tid + 256 * k;
        if (q < 64 * BR * RS) {
          const int b = q / (BR * RS), rem = q % (BR * RS);
          const int r = rem / RS, e = rem % RS;
          Bs[b * PB + r * PWP + (SP == 1 ? (e ? TW + 1 : 0) : 4 * RV + e)] = bs[k];
        }
      }
      return;
    }
    // widths that are no multiple of 4 / unaligned tensors: guarded scalar fill, not prefetched
    int n, y0, x0;
    decode(tile, n, y0, x0);
    for (int idx = tid; idx < 64 * 2 * TW; idx += 256) {
      const int a = idx / (2 * TW), rc = idx - a * 2 * TW;
      const int y = y0 + (rc >> TWL2), x = x0 + (rc & (TW - 1));
      float v = 0.f;
      if (a0 + a < p.ca && y < p.ha && x < p.wa) v = p.A[((long long)n * p.ca + a0 + a) * hwa + (long long)y * p.wa + x];
      As[a * PA + rc] = v;
    }
    for (int idx = tid; idx < 64 * BR * PWP; idx += 256) {
      const int b = idx / (BR * PWP), q = idx - b * BR * PWP;
      const int y = SP * y0 - ORG + q / PWP, x = SP * x0 - ORG + q % PWP;
      float v = 0.f;
      if (b0 + b < p.cb && y >= 0 && y < p.hb && x >= 0 && x < p.wb)
        v = p.B[((long long)n * p.cb + b0 + b) * hwb + (long long)y * p.wb + x];
      Bs[b * PB + q] = v;
    }
  };

  const float* ga = As + (aq * 32 + l31) * PA + khalf * TW;
  const float* ub = Bs + (bq * 32 + l31) * PB + SP * khalf * PWP;
  const int t_begin = ks * p.tiles_per_split, t_end = min(p.ntiles, t_begin + p.tiles_per_split);
  if (t_begin < t_end) issue(t_begin);
  for (int tile = t_begin; tile < t_end; ++tile) {
    __syncthreads();                       // every wave is done reading the previous step
    commit(tile);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    if (tile + 1 < t_end) issue(tile + 1);  // in flight during this step's MFMAs
    // K-step j: A pixel (y0 + khalf, x0 + j); tap (ky, kx) reads patch row SP*khalf + ky, column SP*j + kx.
    // The 3-column window slides by SP columns per step: column c lives in slot c % 3.
    float win[3][3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int c = 0; c < 3; ++c) win[ky][c] = ub[ky * PWP + c] * sb_lane;
    float a_cur = ga[0] * sa_lane, a_nxt = 0.f;
#pragma unroll
    for (int j = 0; j < TW; ++j) {
      __builtin_amdgcn_sched_barrier(0);
      float nw[3][SP];
      if (j + 1 < TW) {                    // operands of step j + 1 while step j is on the matrix pipe
        a_nxt = ga[j + 1];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int e = 0; e < SP; ++e) nw[ky][e] = ub[ky * PWP + SP * j + 3 + e];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
          acc[ky * 3 + kx] =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, win[ky][(SP * j + kx) % 3], acc[ky * 3 + kx], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (j + 1 < TW) {
        a_cur = a_nxt * sa_lane;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int e = 0; e < SP; ++e) win[ky][(SP * j + e) % 3] = nw[ky][e] * sb_lane;   // columns SP*j .. leave, SP*j+3 .. enter
      }
    }
  }
  float* slab = p.partial + (long long)ks * 9 * p.ca * p.cb;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int a = a0 + aq * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      if (a < p.ca && my_b < p.cb) slab[((long long)t * p.ca + a) * p.cb + my_b] = acc[t][r];
    }
}

// gw[o][i][t] = scale * sum_ks partial[ks][t][a][b];  transposed: (a, b) = (i, o), else (o, i)
__global__ __launch_bounds__(256) void modconv_wgrad64_finish_f32(const float* __restrict__ partial, float* __restrict__ gw,
                                                                  int cout, int cin, int ksplit, float scale, int transposed) {
  const int total = cout * cin * 9;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int t = idx % 9, oi = idx / 9;
    const int o = oi / cin, i = oi - o * cin;
    const long long ab = transposed ? (long long)i * cout + o : (long long)o * cin + i;
    float v = 0.f;
    for (int ks = 0; ks < ksplit; ++ks) v += partial[((long long)ks * 9 + t) * cout * cin + ab];
    gw[idx] = v * scale;
  }
}

// ---- the plan: which kernel, which pixel tile, which split over pixels.  ONE decision, made here, for the launch, for the
// workspace query and for fmgan_modconv_wgrad_select (the launch's plan with the launch left out).
// mode 0: plain conv; 1: transposed stride-2 conv (x [h,w], go [2h+1,2w+1]); 2: stride-2 valid conv (x [h,w], go [(h-3)/2+1, ..])
struct WGPlan {
  int family;                    // 0: declined (the host keeps MIOpen's wgrad); 32 / 64: the channel tile of the kernel
  int tw_log2, sp;               // 64: modconv_wgrad64_f32<tw_log2, sp>;  32: WGParams::tw_log2, sp = 1
  int ca, ha, wa, cb, hb, wb;    // channels and plane of the unshifted operand A and of the shifted one B (WG64Params);
                                 // for the 32 x 32 tile A = go, B = x
  int th;                        // rows of a pixel tile: 2 (64), 128 / TW (32)
  int tiles_x, tiles_y, ntiles, a_tiles, b_tiles, ksplit, tiles_per_split;
};

inline WGPlan wgrad_plan(int batch, int cin, int cout, int h, int w, int mode) {
  WGPlan pl{};
  const bool wide = cin >= 48 && cout >= 48;               // 64 x 64 tile; narrower layers: the 32 x 32 tile, plain conv only
  if (!wide && mode != 0) return pl;
  if (mode == 0) {
    pl.ca = cout; pl.ha = h; pl.wa = w;
    pl.cb = cin; pl.hb = h; pl.wb = w;
  } else if (mode == 1) {
    pl.ca = cin; pl.ha = h; pl.wa = w;
    pl.cb = cout; pl.hb = 2 * h + 1; pl.wb = 2 * w + 1;
  } else {
    if (h < 3 || w < 3) return pl;
    pl.ca = cout; pl.ha = (h - 3) / 2 + 1; pl.wa = (w - 3) / 2 + 1;
    pl.cb = cin; pl.hb = h; pl.wb = w;
  }
  if (pl.wa < 16) return pl;                               // narrow / tiny layers: the host keeps MIOpen's wgrad
  const int tile = wide ? 64 : 32;
  pl.tw_log2 = (mode == 0 && pl.wa >= 32) ? 5 : 4;
  pl.sp = mode == 0 ? 1 : 2;
  const int TW = 1 << pl.tw_log2;
  pl.th = wide ? 2 : 128 / TW;
  pl.tiles_x = (pl.wa + TW - 1) / TW;
  pl.tiles_y = (pl.ha + pl.th - 1) / pl.th;
  pl.ntiles = batch * pl.tiles_x * pl.tiles_y;
  pl.a_tiles = (pl.ca + tile - 1) / tile;
  pl.b_tiles = (pl.cb + tile - 1) / tile;
  const int pairs = pl.a_tiles * pl.b_tiles;
  // 64: ~2 rounds of 2 blocks per CU, at least 4 tile steps per block;  32: ~3 rounds of 2 blocks per CU
  int ks = (FMGAN_NUM_CU * (wide ? 4 : 6) + pairs - 1) / pairs;
  const int max_ks = wide ? (pl.ntiles / 4 > 0 ? pl.ntiles / 4 : 1) : pl.ntiles;
  if (ks > max_ks) ks = max_ks;
  if (ks < 1) ks = 1;
  pl.tiles_per_split = (pl.ntiles + ks - 1) / ks;
  pl.ksplit = (pl.ntiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
  pl.family = tile;
  return pl;
}

// What the entry points answer before they plan: bad sizes, unknown mode; then (wgrad_range) the 32-bit index ranges.
inline int wgrad_sizes(int batch, int cin, int cout, int h, int w, int mode) {
  if (batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return FMGAN_EINVAL;
  if (mode < 0 || mode > 2) return FMGAN_EUNSUPPORTED;
  return FMGAN_OK;
}

inline int wgrad_range(int batch, int cin, int cout, int h, int w, int mode) {
  // go is the largest tensor of the transposed conv: [batch, cout, 2h+1, 2w+1]
  const long long big_hw = mode == 1 ? (long long)(2 * h + 1) * (2 * w + 1) : (long long)h * w;
  if ((long long)batch * (cin > cout ? cin : cout) * big_hw >= (1LL << 40)) return FMGAN_EOVERFLOW;
  if (big_hw >= (1LL << 31) || cin > (1 << 20) || cout > (1 << 20)) return FMGAN_EOVERFLOW;
  return FMGAN_OK;
}

inline long long wgrad_workspace(const WGPlan& pl) {
  return (long long)pl.ksplit * 9 * pl.ca * pl.cb * (long long)sizeof(float);
}

template <int TWL2, int SP>
inline void wgrad64_launch(const WG64Params& q, long long nblk, hipStream_t s) {
  constexpr int TW = 1 << TWL2;
  constexpr int PB = ((SP + 3) * (SP * (TW - 1) + 3)) | 1;
  const size_t lds = sizeof(float) * 64 * ((2 * TW + 1) + PB);
  hipLaunchKernelGGL((modconv_wgrad64_f32<TWL2, SP>), dim3((unsigned)nblk), dim3(256), lds, s, q);
}

}  // namespace

extern "C" long long fmgan_modconv_wgrad_mode_workspace_bytes(int batch, int cin, int cout, int h, int w, int mode) {
  if (wgrad_sizes(batch, cin, cout, h, w, mode) != FMGAN_OK) return 0;
  const WGPlan pl = wgrad_plan(batch, cin, cout, h, w, mode);
  return pl.family ? wgrad_workspace(pl) : 0;
}

extern "C" long long fmgan_modconv_wgrad_workspace_bytes(int batch, int cin, int cout, int h, int w) {
  return fmgan_modconv_wgrad_mode_workspace_bytes(batch, cin, cout, h, w, 0);
}

extern "C" int fmgan_modconv_wgrad_select(int batch, int cin, int cout, int h, int w, int mode, int aligned16, int* family,
                                          int* tw, int* sp, int* ksplit, int* tiles_per_split, int* ntiles, int* vec) {
  WGPlan pl{};
  int st = wgrad_sizes(batch, cin, cout, h, w, mode);
  if (st == FMGAN_OK) st = wgrad_range(batch, cin, cout, h, w, mode);
  if (st == FMGAN_OK) {
    pl = wgrad_plan(batch, cin, cout, h, w, mode);
    if (!pl.family) st = FMGAN_EUNSUPPORTED;
    else if ((long long)pl.a_tiles * pl.b_tiles * pl.ksplit > 0x7fffffffLL) st = FMGAN_EOVERFLOW;
  }
  const bool ok = st == FMGAN_OK;
  if (family) *family = ok ? pl.family : 0;
  if (tw) *tw = ok ? 1 << pl.tw_log2 : 0;
  if (sp) *sp = ok ? pl.sp : 0;
  if (ksplit) *ksplit = ok ? pl.ksplit : 0;
  if (tiles_per_split) *tiles_per_split = ok ? pl.tiles_per_split : 0;
  if (ntiles) *ntiles = ok ? pl.ntiles : 0;
  // the 64 x 64 kernels' own `vec` predicate (its third term, a dword-aligned B, holds for every float tensor)
  if (vec) *vec = ok && pl.family == 64 && (pl.wa & 3) == 0 && aligned16 ? 1 : 0;
  return st;
}

extern "C" int fmgan_modconv_wgrad_mode_f32(const float* go, const float* demod, const float* x, const float* style,
                                            float* gw, int batch, int cin, int cout, int h, int w, int mode, float scale,
                                            void* workspace, long long workspace_bytes, void* stream) {
  int st = wgrad_sizes(batch, cin, cout, h, w, mode);
  if (st != FMGAN_OK) return st;
  if (!go || !x || !style || !gw || !workspace) return FMGAN_EINVAL;
  st = wgrad_range(batch, cin, cout, h, w, mode);
  if (st != FMGAN_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const WGPlan pl = wgrad_plan(batch, cin, cout, h, w, mode);
  if (!pl.family) return FMGAN_EUNSUPPORTED;               // narrow / tiny layers: the host keeps MIOpen's wgrad
  if (workspace_bytes < wgrad_workspace(pl)) return FMGAN_EINVAL;
  const long long nblk = (long long)pl.a_tiles * pl.b_tiles * pl.ksplit;
  if (nblk > 0x7fffffffLL) return FMGAN_EOVERFLOW;
  int fb = (cout * cin * 9 + 255) / 256;
  if (fb > FMGAN_NUM_CU * 16) fb = FMGAN_NUM_CU * 16;
  if (pl.family == 64) {
    WG64Params q{};
    if (mode == 1) { q.A = x; q.sa = style; q.B = go; q.sb = demod; }
    else { q.A = go; q.sa = demod; q.B = x; q.sb = style; }
    q.partial = (float*)workspace;
    q.batch = batch; q.ca = pl.ca; q.cb = pl.cb; q.ha = pl.ha; q.wa = pl.wa; q.hb = pl.hb; q.wb = pl.wb;
    q.tiles_x = pl.tiles_x; q.tiles_y = pl.tiles_y; q.ntiles = pl.ntiles; q.ksplit = pl.ksplit;
    q.tiles_per_split = pl.tiles_per_split; q.a_tiles = pl.a_tiles; q.b_tiles = pl.b_tiles;
    if (pl.sp == 1) {
      if (pl.tw_log2 == 5) wgrad64_launch<5, 1>(q, nblk, s); else wgrad64_launch<4, 1>(q, nblk, s);
    } else {
      wgrad64_launch<4, 2>(q, nblk, s);
    }
    st = fmgan_check_launch();
    if (st != FMGAN_OK) return st;
    hipLaunchKernelGGL(modconv_wgrad64_finish_f32, dim3(fb), dim3(256), 0, s, (const float*)workspace, gw, cout, cin,
                       pl.ksplit, scale, mode == 1 ? 1 : 0);
    return fmgan_check_launch();
  }
  WGParams p{};
  p.go = go; p.d = demod; p.x = x; p.s = style; p.partial = (float*)workspace;
  p.batch = batch; p.cin = cin; p.cout = cout; p.h = h; p.w = w;
  p.tw_log2 = pl.tw_log2; p.th = pl.th; p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles;
  p.ksplit = pl.ksplit; p.tiles_per_split = pl.tiles_per_split; p.o_tiles = pl.a_tiles; p.i_tiles = pl.b_tiles;
  const int TW = 1 << p.tw_log2;
  const int patch = (p.th + 2) * (TW + 2);
  const int SB = patch + 1 + (patch & 1);
  size_t lds = sizeof(float) * (32 * 129 + 32 * (size_t)SB);
  if (lds < sizeof(float) * 4 * 32 * 33) lds = sizeof(float) * 4 * 32 * 33;
  hipLaunchKernelGGL(modconv_wgrad_f32, dim3((unsigned)nblk), dim3(256), lds, s, p);
  st = fmgan_check_launch();
  if (st != FMGAN_OK) return st;
  hipLaunchKernelGGL(modconv_wgrad_finish_f32, dim3(fb), dim3(256), 0, s, (const float*)workspace, gw, cout, cin,
                     p.ksplit, scale);
  return fmgan_check_launch();
}

extern "C" int fmgan_modconv_wgrad_f32(const float* go, const float* demod, const float* x, const float* style,
                                       float* gw, int batch, int cin, int cout, int h, int w, float scale,
                                       void* workspace, long long workspace_bytes, void* stream) {
  if (w > 0 && w < 16) return FMGAN_EUNSUPPORTED;           // tiny layers: negligible FLOPs, the host keeps MIOpen's wgrad
  return fmgan_modconv_wgrad_mode_f32(go, demod, x, style, gw, batch, cin, cout, h, w, 0, scale, workspace,
                                      workspace_bytes, stream);
}
