// conv3x3_mfma_bf16x3: a plain 3x3 / pad 1 convolution at stride 1 or 2 with fp32 tensors, each operand split into
// three bf16 pieces and six v_mfma_f32_32x32x16_bf16 per product (bf16_mfma.h; the contraction of modconv_mfma_bf16x3 in
// modconv_bf16.hip, whose comment has the error bound).  No style and no demodulation.  This family IS on the default
// inference path of the pSp encoder: the first convolution of the fine style heads and the body's 3x3 convolutions whose
// output is at least 32 wide (at a 256^2 photo: both convolutions of units 0-5 and conv1 of unit 6, thirteen of
// sixteen; helpers.py body_x3_serves is the rule, FMGAN_PSP_BODY_X3=0 the switch; DESIGN 3.3c / 3.4d,
// profiles/psp_body_x3.md), and — on the narrow-tile members conv3x3_tail_x3 below — the heads' convolutions with an
// output 9 .. 16 wide (psp_encoders.py TAIL_X3_WIDTHS; FMGAN_PSP_TAIL_X3=0 gives MIOpen back; profiles/psp_tail_x3.md).
// The default pairs1024 / pairs256 figures of bench.py have all of these on this contraction.
//
// Stride 2 first.  The first convolution of a pSp style head (psp_encoders.py GradualStyleBlock): out = LeakyReLU(conv(in, W) + bias), NCHW
// in, NCHW or NHWC out (the MIOpen tail of the head reads NHWC), no style and no demodulation (nothing to multiply: compiled out), the six-product contraction of
// modconv_mfma_bf16x3 with a fixed summation order (no split-K, no atomics: two calls give the same bits).
//   * tile: 64 output channels x (4 rows x 32 columns) output positions per block; waves 2 x 2: wave (wm, wn) holds
//     channels 32*wm.. and rows 2*wn, 2*wn+1.  A 256-position tile as the modulated kernel's would need a 17 x 65 input patch (106 KB in
//     three pieces): one block per CU.  This one keeps 9 x 65 = 55 KB and two blocks per CU, and 512 blocks at the heads'
//     shape (512 -> 512, 64^2 -> 32^2, B = 8).
//   * patch: input rows 2*y0-1 .. 2*y0+7, columns 2*x0-1 .. 2*x0+63 (origin -1 = the pad; outside the image the loads
//     are parked out of range and read zeros), laid out per row as [even patch columns (33)][odd (32)] so that the 32
//     lanes of a tap (input columns 2*x + kx - 1: a stride of two) read consecutive 16-byte slots as the plain mode does;
//   * weights: NOT through LDS.  Each wave fetches its own 32 rows of the prepared image (modconv_weight_to_bf16x3) one
//     tap ahead with one 16-byte buffer load per piece — the image is laid out as the MFMA operand, consecutive lanes on
//     consecutive slots — which leaves the LDS to the patch.
//   * special values: a finite activation beyond the largest bf16 is clamped for its high piece (the residual goes to
//     mid + lo, still exact).  Inf or NaN cannot be split — (Inf, 0, 0) times a finite (bh, 0, 0) would give Inf*0 —
//     so a block that meets one among ITS operands (patch or weight rows; found while staging, no extra pass) recomputes
//     its tile with plain fp32 FMAs in a fixed order: the non-finite outputs are those of the fp32 products.
//
// The family (template arguments of conv3x3_mfma_bf16x3; the contraction and its summation order are the same in all):
//   * S = 2 (above) or 1: the stride-1 patch is the plain one, rows y0-1 .. y0+4 and columns x0-1 .. x0+32 in order
//     (6 x 34 = 19 KB in three pieces, a third of the stride-2 one), one LDS slot per thread; same 64 x (4 x 32) tile,
//     built for three blocks per CU (the registers then set the limit, not the LDS);
//   * NHWC_IN: the input is channels_last storage in[b][y][x][i].  A slot's 16 channels are 64 contiguous bytes: four
//     16-byte loads (by four neighbouring lanes) instead of sixteen 4-byte ones a plane apart.  Needs cin % 4 == 0 (a
//     quad is inside cin or outside: outside it is parked out of range like the padding) and a 16-byte aligned input;
//   * EPI: none (plain store) / bias + LeakyReLU(alpha) / per-channel PReLU v > 0 ? v : slope[o] * v without bias
//     (aten's prelu arithmetic on the accumulator value: the fused result is conv followed by aten PReLU).  The fp32
//     recomputation of a block with Inf / NaN operands applies the same epilogue.
// The encoder body's 3x3 convolutions (helpers._fused_unit: conv1 with the PReLU epilogue, conv2 with none, both
// channels_last in and out) and the style heads' first convolution (stride 2, LeakyReLU) run on it.
#include "bf16_mfma.h"

namespace {

enum { C3_NONE = 0, C3_LRELU = 1, C3_PRELU = 2 };

struct C3Params {
  const float* in; const unsigned short* wt; const float* aux; float* out;     // aux: bias (C3_LRELU) or slope (C3_PRELU)
  int batch, cin, cout, h, w, oh, ow;
  int tiles_x, tiles_y, o_tiles, mp;
  float alpha;
  int stride, epi;
  int in_nhwc, out_nhwc;                                 // 0: [b][c][y][x]; 1: [b][y][x][c] (channels_last storage)
};

// A block is four waves, WM on channel groups of 32 by WN on position groups; a wave holds RNP position groups of one
// MFMA's 32 position lanes each, and a position group is 32 / TW output rows of TW columns (one row of 32 by default).
// A_RING: 0, a wave fetches its weights one tap ahead (two blocks per CU cover the rest of the latency); a divisor of 9
// (the narrow tiles, whose grids leave one block per CU or fewer, use 9): a ring of that many taps' weights, fetched
// A_RING - 1 taps ahead across chunk boundaries.
template <int S, int TW_ = 32, int BM_ = 64, int RNP_ = 2, int A_RING_ = 0>
struct C3Tile {
  static constexpr int BM = BM_, TW = TW_, RNP = RNP_, A_RING = A_RING_;
  static_assert(A_RING == 0 || 9 % A_RING == 0, "a tap keeps its ring slot from chunk to chunk");
  static constexpr int WM = BM / 32, WN = 4 / WM, RPG = 32 / TW, TH = WN * RNP * RPG;
  static constexpr int TW_LOG2 = TW == 32 ? 5 : TW == 16 ? 4 : 3, NPOS = TH * TW, NPOS_LOG2 = NPOS == 128 ? 7 : 6;
  static_assert((WM == 1 || WM == 2) && (TW == 32 || TW == 16 || TW == 8) && (NPOS == 128 || NPOS == 64), "tile");
  static constexpr int PH = S * (TH - 1) + 3, PWP = S * (TW - 1) + 3, EVEN = (PWP + 1) / 2;
  static constexpr int PLANE = PH * PWP;
  static constexpr size_t LDS = (size_t)(3 * 2 * PLANE) * 16;
  static constexpr int BLOCKS_PER_CU = S == 1 ? 3 : 2;
};

// the launch's plan; false when the shape is not served (stride, channels_last width, 32-bit buffer ranges, grid size)
template <class Tile>
bool c3_plan_tile(C3Params& p) {
  if (p.batch <= 0 || p.cin <= 0 || p.cout <= 0 || p.h <= 0 || p.w <= 0) return false;
  if (p.stride != 1 && p.stride != 2) return false;
  if (p.in_nhwc && (p.cin & 3)) return false;                                               // 16-byte channel quads
  p.oh = (p.h - 1) / p.stride + 1; p.ow = (p.w - 1) / p.stride + 1;
  p.mp = (p.cout + 31) / 32 * 32;
  p.tiles_x = (p.ow + Tile::TW - 1) / Tile::TW;
  p.tiles_y = (p.oh + Tile::TH - 1) / Tile::TH;
  p.o_tiles = (p.cout + Tile::BM - 1) / Tile::BM;
  // one sample's input, either layout: the largest byte offset a lane forms is below cin * h * w * 4
  if ((long long)p.cin * p.h * p.w * 4 >= 0xFFFFFFF0LL) return false;
  if ((long long)((p.cin + 15) / 16) * 54 * p.mp * 16 >= 0xFFFFFFF0LL) return false;       // the weight image
  if ((long long)p.o_tiles * p.tiles_x * p.tiles_y * p.batch > 0x7fffffffLL) return false;
  if ((long long)p.batch * p.cout * p.oh * p.ow > (1LL << 40)) return false;
  return true;
}
bool c3_plan(C3Params& p) { return c3_plan_tile<C3Tile<1>>(p); }                             // (the output tile of both strides)

// One block's tile; the body of every kernel of this file.
template <class Tile, int S, bool NHWC_IN, int EPI>
__device__ __forceinline__ void c3_block(const C3Params p) {
  constexpr int BM = Tile::BM, TW = Tile::TW, PWP = Tile::PWP, EVEN = Tile::EVEN, PLANE = Tile::PLANE;
  constexpr int RNP = Tile::RNP, RPG = Tile::RPG, WM = Tile::WM;
  // staging units per thread and floats per unit.  A thread owns whole slots: 16 channels a plane apart (NCHW input) or
  // as four 16-byte loads (channels_last input, stride 1: 204 slots, the staging is a small part of the block's work).
  // QUAD (channels_last input, stride 2: 585 slots for the same products): four lanes share a slot, each on one 16-byte
  // channel quad of its 64 contiguous bytes, so that one load instruction of a wave covers 16 whole slots — a lane on a
  // whole slot of its own, 64 lanes 4 KB apart, measured 20 % slower than the NCHW staging at the heads' shape.  (At
  // stride 1 the QUAD form spills at three blocks per CU.)
  constexpr bool QUAD = NHWC_IN && S == 2;
  constexpr int NU = QUAD ? (4 * PLANE + 255) / 256 : (PLANE + 255) / 256, NV = QUAD ? 4 : 16;
  static_assert(NU <= 16, "one staging unit per issue_x call");
  extern __shared__ u32x4 smem_q[];
  u32x4* Xs = smem_q;                                   // [3 pieces][2 k-halves][PLANE]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, khalf = lane >> 5, wm = wave & (WM - 1), wn = wave >> (WM - 1);
  const int lr = l31 >> Tile::TW_LOG2, lc = l31 & (TW - 1);      // this lane's row and column in its position group
  const int kq = tid & 3;                                // QUAD: this lane's channel quad of its slots
  unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  const int o_tile = lb % p.o_tiles; lb /= p.o_tiles;
  const int tx_i = lb % p.tiles_x; lb /= p.tiles_x;
  const int ty_i = lb % p.tiles_y;
  const int b = lb / p.tiles_y;
  const int o0 = o_tile * BM, x0 = tx_i * TW, y0 = ty_i * Tile::TH;
  const int hw = p.h * p.w;
  const float* in_b = p.in + (long long)b * p.cin * hw;

  // Two accumulators per position row: the hi*hi products in one, the five correction products (2^-8 and 2^-16 of
  // them) in the other, added once at the end — the corrections are then rounded at their own magnitude, and the main
  // chain is one step per (chunk, tap) instead of six.
  f32x16 acc[RNP], acc_lo[RNP];
#pragma unroll
  for (int g = 0; g < RNP; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[g][r] = 0.f; acc_lo[g][r] = 0.f; }

  constexpr unsigned PARK = 0xFFFFFFF0u;
  const unsigned x_bytes = (unsigned)((long long)p.cin * hw * 4);
  const unsigned mp16 = (unsigned)p.mp * 16u;
  const unsigned w_bytes = (unsigned)((p.cin + 15) >> 4) * 54u * mp16;
  const auto rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in_b), 0, x_bytes, 0x00020000);
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(p.wt), 0, w_bytes, 0x00020000);
  unsigned xvo[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int q = QUAD ? (tid + 256 * u) >> 2 : tid + 256 * u;      // the LDS slot: row r, then (S = 2) even patch columns, then odd
    const int r = q / PWP, t = q - r * PWP;
    const int c = S == 1 ? t : (t < EVEN ? 2 * t : 2 * (t - EVEN) + 1);
    const int y = S * y0 + r - 1, x = S * x0 + c - 1;
    const bool inside = q < PLANE && y >= 0 && y < p.h && x >= 0 && x < p.w;
    const unsigned pos_bytes = NHWC_IN ? 4u * (unsigned)p.cin : 4u;
    xvo[u] = inside ? (unsigned)(y * p.w + x) * pos_bytes + (QUAD ? 16u * (unsigned)kq : 0u) : PARK;
  }
  const int arow = o0 + wm * 32 + l31;                   // this lane's weight row (a 32-row group lies wholly inside mp or not)
  const unsigned avo = arow < p.mp ? (unsigned)(khalf * p.mp + arow) * 16u : PARK;

  float xv[NU][NV];
  auto issue_x = [&](int i0, int kc) {
    if constexpr (QUAD) {                                // staging unit kc: channels i0 + 4*kq .. + 3 of its slot (past cin: parked, zeros)
      if (kc < NU) {
        const unsigned vo = i0 + 4 * kq < p.cin ? xvo[kc] : PARK;
        const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, vo, (unsigned)(i0 * 4), 0));
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[kc][e] = __uint_as_float(v[e]);
      }
    } else if constexpr (NHWC_IN) {                      // channels i0 + kc .. + 3 of the patch, once per quad (past cin: parked)
      if ((kc & 3) == 0) {
        const bool inside = i0 + kc < p.cin;
        const unsigned soff = inside ? (unsigned)((i0 + kc) * 4) : 0u;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, inside ? xvo[u] : PARK, soff, 0));
#pragma unroll
          for (int e = 0; e < 4; ++e) xv[u][kc + e] = __uint_as_float(v[e]);
        }
      }
    } else {                                             // channel i0 + kc of the patch (past cin: channel 0, dropped in commit_x)
      const unsigned soff = i0 + kc < p.cin ? (unsigned)((i0 + kc) * hw * 4) : 0u;
#pragma unroll
      for (int u = 0; u < NU; ++u)
        xv[u][kc] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_x, xvo[u], soff, 0));
    }
  };
  float xflag = 0.f;                                     // NaN once an activation of this block's patch is Inf or NaN
  // two activations as their three bf16 pieces (hi clamped to the largest finite bf16: the residual stays exact)
  auto split2 = [&](float v0, float v1, unsigned& h01, unsigned& m01, unsigned& l01) {
    xflag = __builtin_fmaf(v0, 0.f, xflag);
    xflag = __builtin_fmaf(v1, 0.f, xflag);
    h01 = pack_bf16(__builtin_amdgcn_fmed3f(v0, -BF16_MAX, BF16_MAX), __builtin_amdgcn_fmed3f(v1, -BF16_MAX, BF16_MAX));
    const float r0 = v0 - __uint_as_float(h01 << 16), r1 = v1 - __uint_as_float(h01 & 0xffff0000u);
    m01 = pack_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(m01 << 16), s1 = r1 - __uint_as_float(m01 & 0xffff0000u);
    l01 = pack_bf16(s0, s1);
  };
  auto commit_x = [&](int i0) {
    if constexpr (QUAD) {                                // a quad is half of a k-half's 16-byte slot: 8-byte LDS writes
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int q = (tid + 256 * u) >> 2;
        if (q < PLANE) {
          unsigned h[2], m[2], l[2];
          split2(xv[u][0], xv[u][1], h[0], m[0], l[0]);
          split2(xv[u][2], xv[u][3], h[1], m[1], l[1]);
          u32x2* dst = reinterpret_cast<u32x2*>(Xs + (kq >> 1) * PLANE + q) + (kq & 1);
          u32x2 ph = {h[0], h[1]}, pm = {m[0], m[1]}, pl = {l[0], l[1]};
          dst[0] = ph; dst[4 * PLANE] = pm; dst[8 * PLANE] = pl;       // a piece is 2 * PLANE slots
        }
      }
    } else {
      if (i0 + 16 > p.cin) {                             // the partial last chunk: zeros past cin
#pragma unroll
        for (int kc = 0; kc < 16; ++kc)
          if (i0 + kc >= p.cin) {
#pragma unroll
            for (int u = 0; u < NU; ++u) xv[u][kc] = 0.f;
          }
      }
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int q = tid + 256 * u;
        if (q < PLANE) {
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            unsigned h[4], m[4], l[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) split2(xv[u][8 * hh + 2 * e], xv[u][8 * hh + 2 * e + 1], h[e], m[e], l[e]);
            u32x4 ph = {h[0], h[1], h[2], h[3]}, pm = {m[0], m[1], m[2], m[3]}, pl = {l[0], l[1], l[2], l[3]};
            Xs[(0 * 2 + hh) * PLANE + q] = ph;
            Xs[(1 * 2 + hh) * PLANE + q] = pm;
            Xs[(2 * 2 + hh) * PLANE + q] = pl;
          }
        }
      }
    }
  };

  int pbase[RNP];
#pragma unroll
  for (int g = 0; g < RNP; ++g) pbase[g] = khalf * PLANE + S * ((wn * RNP + g) * RPG + lr) * PWP + lc;

  struct Ops { u32x4 a[3]; bf16x8 b[3][RNP]; };
  auto fetch_a = [&](Ops& o, unsigned soff_chunk, int t) {
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
      o.a[pc] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, avo, soff_chunk + (unsigned)(pc * 18 + t * 2) * mp16, 0));
  };
  auto fetch_b = [&](Ops& o, int t) {
    const int ky = t / 3, kx = t - 3 * ky;
    const int off = S == 1 ? ky * PWP + kx : ky * PWP + (kx & 1) * EVEN + (kx >> 1);     // patch column S*lc + kx
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
      for (int g = 0; g < RNP; ++g) o.b[pc][g] = __builtin_bit_cast(bf16x8, Xs[pc * 2 * PLANE + pbase[g] + off]);
  };
  unsigned wflag = 0;                                    // bits 15 / 31 once a high weight piece of this wave's rows is Inf or NaN

  const int chunks = (p.cin + 15) >> 4;
#pragma unroll
  for (int kc = 0; kc < 16; ++kc) issue_x(0, kc);
  if constexpr (Tile::A_RING != 0) {
    // Weights A_RING - 1 taps ahead: tap t of every chunk lives in ring slot t % A_RING (A_RING divides 9), refilled for
    // tap t + A_RING - 1 — of the next chunk past tap 8 — once tap t - 1 has used it.  Same products in the same order.
    constexpr int AR = Tile::A_RING, AD = AR - 1;
    Ops ring[AR];                          // (.a only; the patch operands alternate between ring[0].b and ring[1].b)
#pragma unroll
    for (int t = 0; t < AD; ++t) fetch_a(ring[t], 0u, t);
    for (int ch = 0; ch < chunks; ++ch) {
      const unsigned soff_chunk = (unsigned)ch * 54u * mp16;
      const unsigned soff_next = ch + 1 < chunks ? soff_chunk + 54u * mp16 : 0u;       // (as the patch: chunk 0 again, unused)
      __syncthreads();
      commit_x(16 * ch);
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
      fetch_b(ring[0], 0);
      const int i0n = ch + 1 < chunks ? 16 * (ch + 1) : 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        __builtin_amdgcn_sched_barrier(0);
        fetch_a(ring[(t + AD) % AR], t + AD < 9 ? soff_chunk : soff_next, (t + AD) % 9);
        __builtin_amdgcn_sched_barrier(0);
        if (t == 0) {                      // the next chunk's whole patch at once: nine taps to arrive in
#pragma unroll
          for (int kc = 0; kc < 16; ++kc) issue_x(i0n, kc);
        }
        if (t + 1 < 9) fetch_b(ring[(t + 1) & 1], t + 1);
        __builtin_amdgcn_sched_barrier(0);
        const Ops &oa = ring[t % AR], &ob = ring[t & 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) wflag |= ((oa.a[0][e] & 0x7f807f80u) + 0x00800080u) & 0x80008000u;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
          for (int g = 0; g < RNP; ++g) {
            f32x16& dst = q == 5 ? acc[g] : acc_lo[g];
            dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, oa.a[PA[q]]), ob.b[PB[q]][g], dst, 0, 0, 0);
          }
        __builtin_amdgcn_s_setprio(0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else
  for (int ch = 0; ch < chunks; ++ch) {
    const unsigned soff_chunk = (unsigned)ch * 54u * mp16;
    Ops ops[2];
    fetch_a(ops[0], soff_chunk, 0);        // in flight over the split
    __syncthreads();                       // every wave is done reading the previous chunk's patch
    commit_x(16 * ch);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    fetch_b(ops[0], 0);
    const int i0n = ch + 1 < chunks ? 16 * (ch + 1) : 0;       // (the last chunk loads chunk 0 again, unused: no branch)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < 9) {
        // in this order: the wait for tap t's weights then leaves this tap's and the previous tap's patch loads in flight
        fetch_a(ops[(t + 1) & 1], soff_chunk, t + 1);
        __builtin_amdgcn_sched_barrier(0);
        issue_x(i0n, 2 * t); issue_x(i0n, 2 * t + 1);          // the next chunk's patch, two channels per tap
        fetch_b(ops[(t + 1) & 1], t + 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      const Ops& o = ops[t & 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) wflag |= ((o.a[0][e] & 0x7f807f80u) + 0x00800080u) & 0x80008000u;
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int g = 0; g < RNP; ++g) {
          f32x16& dst = q == 5 ? acc[g] : acc_lo[g];
          dst = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, o.a[PA[q]]), o.b[PB[q]][g], dst, 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int g = 0; g < RNP; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = __fadd_rn(acc[g][r], acc_lo[g][r]);

  float* out_b = p.out + (long long)b * p.cout * p.oh * p.ow;
  const float alpha = p.alpha;
  // the epilogue on one accumulator value; a = bias[o] (C3_LRELU: fused_leaky_relu's order with scale 1) or slope[o]
  // (C3_PRELU: aten's prelu, weight * x on the negative side)
  auto epilogue = [&](float v, float a) -> float {
    if constexpr (EPI == C3_LRELU) {
      const float t = __fadd_rn(v, a);
      return t > 0.f ? t : t * alpha;
    } else if constexpr (EPI == C3_PRELU) {
      return v > 0.f ? v : a * v;
    } else {
      return v;
    }
  };
  const long long ost_o = p.out_nhwc ? 1 : (long long)p.oh * p.ow, ost_p = p.out_nhwc ? p.cout : 1;   // channel / position strides
  if (__syncthreads_or((xflag != xflag) | (wflag != 0u))) {
    // Inf / NaN among this block's operands: the tile again as fp32 products.  Thread = one position x CPT channels
    // (32 for the 64 x 128 tile).
    constexpr int CPT = BM * Tile::NPOS / 256;
    const int pp = tid & (Tile::NPOS - 1), oy = y0 + (pp >> Tile::TW_LOG2), ox = x0 + (pp & (TW - 1));
    if (oy >= p.oh || ox >= p.ow) return;
    for (int oo = 0; oo < CPT; ++oo) {
      const int o = o0 + (tid >> Tile::NPOS_LOG2) * CPT + oo;
      if (o >= p.cout) return;
      float s = 0.f;
      for (int i = 0; i < p.cin; ++i) {
        const long long slot0 = (long long)(i >> 4) * 54 * p.mp;
        const int hh = (i >> 3) & 1, j = i & 7;
        for (int t = 0; t < 9; ++t) {
          const int y = S * oy + t / 3 - 1, x = S * ox + t % 3 - 1;
          const long long at = NHWC_IN ? (long long)(y * p.w + x) * p.cin + i : (long long)i * hw + y * p.w + x;
          const float xin = (y >= 0 && y < p.h && x >= 0 && x < p.w) ? in_b[at] : 0.f;
          float wv = 0.f;
#pragma unroll
          for (int pc = 0; pc < 3; ++pc)     // hi + mid + lo is the fp32 weight again, exactly
            wv += bf16_to_f32(p.wt[((slot0 + (long long)(pc * 18 + t * 2 + hh) * p.mp + o) << 3) + j]);
          s = __builtin_fmaf(wv, xin, s);
        }
      }
      out_b[o * ost_o + ((long long)oy * p.ow + ox) * ost_p] = epilogue(s, (EPI != C3_NONE && p.aux) ? p.aux[o] : 0.f);
    }
    return;
  }

  // ---- store through the epilogue; NCHW: 32 lanes on 32 / TW rows of TW consecutive x; NHWC: a lane's four consecutive channels
  // (r & 3) as one 16-byte store, the two k-halves and four row groups of a position filling 128 consecutive bytes
  const int orow = o0 + wm * 32 + 4 * khalf;            // row r of the 32-row group adds (r&3) + 8*(r>>2)
  float aux_r[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    aux_r[r] = (EPI != C3_NONE && p.aux) ? p.aux[min(orow + (r & 3) + 8 * (r >> 2), p.cout - 1)] : 0.f;
#pragma unroll
  for (int g = 0; g < RNP; ++g) {
    const int py_ = y0 + (wn * RNP + g) * RPG + lr, px_ = x0 + lc;
    if (py_ >= p.oh || px_ >= p.ow) continue;
    float* dpos = out_b + ((long long)py_ * p.ow + px_) * ost_p;
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = epilogue(acc[g][r], aux_r[r]);
    if (p.out_nhwc && (p.cout & 3) == 0) {               // o and cout are multiples of 4: a quad is inside or outside
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = orow + 8 * j;
        if (o < p.cout) {
          f32x4 q4 = {v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
          *reinterpret_cast<f32x4*>(dpos + o) = q4;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = orow + (r & 3) + 8 * (r >> 2);
        if (o < p.cout) dpos[o * ost_o] = v[r];
      }
    }
  }
}

template <int S, bool NHWC_IN, int EPI>
__global__ __launch_bounds__(256, C3Tile<S>::BLOCKS_PER_CU) void conv3x3_mfma_bf16x3(const C3Params p) {
  c3_block<C3Tile<S>, S, NHWC_IN, EPI>(p);
}

// The narrow-tile members: stride 2, channels_last input, bias + LeakyReLU, for outputs at most 16 wide, where the
// 32-column tile above leaves MFMA position lanes empty (the pSp style heads' convolutions after the first, and the
// first one of the middle and coarse heads).  A position group is 2 output rows of 16 columns (TW = 16) or 4 rows of 8
// (TW = 8), one group per wave: TW = 16 is 64 channels x (4 rows x 16 columns), patch 9 x 33 slots (28 KB); TW = 8 is 64
// channels x (8 rows x 8 columns), patch 17 x 17 slots (28 KB).  At the heads' B = 8 the grid is one block per CU or
// fewer, so nothing covers a wave's waits but the wave itself: the weights come through a ring of nine taps (a whole
// chunk ahead) and the next chunk's patch is requested at once at tap 0.  64 x (4 x 16) was measured against 64 x
// (8 x 16) and 32 x (8 x 16) (profiles/psp_tail_x3.md).  Same staging, contraction, summation order and fallback: on
// finite operands the bits are those of conv3x3_mfma_bf16x3<2, true, C3_LRELU>.
template <int TW> struct TailTile { using type = C3Tile<2, TW, 64, 1, 9>; };

template <int TW>
__global__ __launch_bounds__(256, 2) void conv3x3_tail_x3(const C3Params p) {
  c3_block<typename TailTile<TW>::type, 2, true, C3_LRELU>(p);
}

template <class Tile>
int c3_launch_kernel(void (*kernel)(const C3Params), bool& opted_in, const C3Params& p, hipStream_t s) {
  opt_in_dynamic_lds(kernel, Tile::LDS, opted_in);
  const long long blocks = (long long)p.o_tiles * p.tiles_x * p.tiles_y * p.batch;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), Tile::LDS, s, p);
  return fmgan_check_launch();
}

template <int S, bool NHWC_IN, int EPI>
int c3_launch(const C3Params& p, hipStream_t s) {
  static bool opted_in = false;     // per instantiation
  return c3_launch_kernel<C3Tile<S>>(conv3x3_mfma_bf16x3<S, NHWC_IN, EPI>, opted_in, p, s);
}

template <int TW>
int tail_launch(const C3Params& p, hipStream_t s) {
  static bool opted_in = false;
  return c3_launch_kernel<typename TailTile<TW>::type>(conv3x3_tail_x3<TW>, opted_in, p, s);
}

// The tail's plan: the tile width (16 or 8) that serves the shape, or the status the launch returns.
int tail_plan(C3Params& p) {
  if (p.batch <= 0 || p.cin <= 0 || p.cout <= 0 || p.h <= 0 || p.w <= 0) return FMGAN_EINVAL;
  p.stride = 2; p.epi = C3_LRELU; p.in_nhwc = 1;
  const int ow = (p.w - 1) / 2 + 1;
  if (ow > 16 || ow <= 4) return FMGAN_EUNSUPPORTED;     // wider: conv3x3_mfma_bf16x3; narrower: launch-latency-bound, MIOpen's
  if (ow > 8) return c3_plan_tile<TailTile<16>::type>(p) ? 16 : FMGAN_EUNSUPPORTED;
  return c3_plan_tile<TailTile<8>::type>(p) ? 8 : FMGAN_EUNSUPPORTED;
}

template <int S, bool NHWC_IN>
int c3_launch_epi(const C3Params& p, hipStream_t s) {
  if (p.epi == C3_LRELU) return c3_launch<S, NHWC_IN, C3_LRELU>(p, s);
  if (p.epi == C3_PRELU) return c3_launch<S, NHWC_IN, C3_PRELU>(p, s);
  return c3_launch<S, NHWC_IN, C3_NONE>(p, s);
}

// The host side of fmgan_conv3x3_bf16x3_f32 and of fmgan_conv3x3s2_bf16x3_f32 (stride 2, NCHW in, bias + LeakyReLU).
int conv3x3_bf16x3(const float* in, const void* wt, const float* aux, float* out, int batch, int cin, int cout, int h, int w,
                   int stride, int in_nhwc, int out_nhwc, int epi, float alpha, hipStream_t s) {
  if (batch < 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || (stride != 1 && stride != 2)) return FMGAN_EINVAL;
  if ((in_nhwc != 0 && in_nhwc != 1) || (out_nhwc != 0 && out_nhwc != 1) || epi < C3_NONE || epi > C3_PRELU) return FMGAN_EINVAL;
  if (batch == 0) return FMGAN_OK;
  C3Params p{};
  p.in = in; p.wt = (const unsigned short*)wt; p.aux = aux; p.out = out;
  p.batch = batch; p.cin = cin; p.cout = cout; p.h = h; p.w = w; p.alpha = alpha;
  p.stride = stride; p.epi = epi; p.in_nhwc = in_nhwc; p.out_nhwc = out_nhwc;
  if (!c3_plan(p)) return FMGAN_EUNSUPPORTED;
  if (!in || !wt || !out || (epi == C3_PRELU && !aux)) return FMGAN_EINVAL;
  if (in_nhwc && ((uintptr_t)in & 15)) return FMGAN_EINVAL;                            // the 16-byte loads
  if (out_nhwc && (cout & 3) == 0 && ((uintptr_t)out & 15)) return FMGAN_EINVAL;       // the 16-byte stores
  if (stride == 1) return in_nhwc ? c3_launch_epi<1, true>(p, s) : c3_launch_epi<1, false>(p, s);
  return in_nhwc ? c3_launch_epi<2, true>(p, s) : c3_launch_epi<2, false>(p, s);
}

}  // namespace

// ---- pSp style heads: plain 3x3 / stride 2 / pad 1 conv + bias + LeakyReLU on the split-operand contraction
extern "C" int fmgan_conv3x3s2_bf16x3_supported(int batch, int cin, int cout, int h, int w) {
  return fmgan_conv3x3_bf16x3_supported(batch, cin, cout, h, w, 2, 0);
}

extern "C" int fmgan_conv3x3s2_bf16x3_f32(const float* in, const void* wt_split, const float* bias, float* out, int batch,
                                          int cin, int cout, int h, int w, float alpha, int out_nhwc, void* stream) {
  return conv3x3_bf16x3(in, wt_split, bias, out, batch, cin, cout, h, w, 2, 0, out_nhwc, C3_LRELU, alpha, (hipStream_t)stream);
}

// ---- the family: stride 1 or 2, NCHW or channels_last on either side, one of three epilogues (pSp encoder body)
extern "C" int fmgan_conv3x3_bf16x3_supported(int batch, int cin, int cout, int h, int w, int stride, int in_nhwc) {
  C3Params p{};
  p.batch = batch; p.cin = cin; p.cout = cout; p.h = h; p.w = w; p.stride = stride; p.in_nhwc = in_nhwc;
  return c3_plan(p) ? 1 : 0;
}

extern "C" int fmgan_conv3x3_bf16x3_f32(const float* in, const void* wt_split, const float* aux, float* out, int batch,
                                        int cin, int cout, int h, int w, int stride, int in_nhwc, int out_nhwc,
                                        int epilogue, float alpha, void* stream) {
  return conv3x3_bf16x3(in, wt_split, aux, out, batch, cin, cout, h, w, stride, in_nhwc, out_nhwc, epilogue, alpha,
                        (hipStream_t)stream);
}

// ---- pSp style heads, outputs 5 .. 16 wide: the narrow-tile members (stride 2, channels_last in, bias + LeakyReLU)
extern "C" int fmgan_conv3x3_tail_bf16x3_select(int batch, int cin, int cout, int h, int w) {
  C3Params p{};
  p.batch = batch; p.cin = cin; p.cout = cout; p.h = h; p.w = w;
  return tail_plan(p);
}

extern "C" int fmgan_conv3x3_tail_bf16x3_f32(const float* in, const void* wt_split, const float* bias, float* out, int batch,
                                             int cin, int cout, int h, int w, float alpha, int out_nhwc, void* stream) {
  if (out_nhwc != 0 && out_nhwc != 1) return FMGAN_EINVAL;
  C3Params p{};
  p.in = in; p.wt = (const unsigned short*)wt_split; p.aux = bias; p.out = out;
  p.batch = batch; p.cin = cin; p.cout = cout; p.h = h; p.w = w; p.alpha = alpha; p.out_nhwc = out_nhwc;
  const int tw = tail_plan(p);
  if (tw < 0) return tw;
  if (!in || !wt_split || !out) return FMGAN_EINVAL;
  if (((uintptr_t)in & 15) || (out_nhwc && (cout & 3) == 0 && ((uintptr_t)out & 15))) return FMGAN_EINVAL;   // 16-byte loads / stores
  return tw == 16 ? tail_launch<16>(p, (hipStream_t)stream) : tail_launch<8>(p, (hipStream_t)stream);
}
