// ModulatedConv2d / ToRGB for gfx950 (MI355X).
//
// Replaces the reference's per-sample weight materialisation + grouped conv
// (stylegan2.py:250-298: `weight = scale*W*style; weight *= demod; F.conv2d(..., groups=batch)` /
// `F.conv_transpose2d(..., stride=2, groups=batch)`) and ToRGB (stylegan2.py:389-404).
//
// Design.  The reference builds a [B*Cout, Cin, 3, 3] weight per call (302 MB at B=32, 512 ch) and
// runs B independent small GEMMs.  Here the modulation moves to the input and the demodulation to
// the epilogue, so all samples share ONE weight matrix and the whole batch is a single implicit GEMM
//     out[b,o,p] = demod[b,o] * sum_{i,tap} wt[i,tap,o] * (style[b,i] * in[b,i,p+tap])
// with M = Cout, N = B*H*W, K = Cin*9, contracted on v_mfma_f32_32x32x2_f32 (exact fp32; gfx950 has no
// reduced-precision f32 path and bf16 cannot hold the 1e-5 parity bar — SURVEY.md §7 "Hard parts").
//   * A operand (weights): wt[i][tap][o] staged to LDS as [kc][tap][o] — a 32-lane read is one bank row.
//   * B operand (pixels): a (TH+2)x(TW+2) halo patch per channel is staged once per 8-channel chunk,
//     multiplied by style[b,i] on the way in; the 9 taps are 9 constant LDS offsets from one base.
//   * 4 waves per block, 2-4 independent 32x32 accumulators per wave (64-cycle MFMA issue needs no
//     more), 2-3 blocks per CU so one block's staging overlaps another's MFMAs.
//   * Transposed (upsampling) conv = 4 output phases of the same contraction; a block owns one row
//     parity and both column parities so each lane stores the two adjacent columns as one 8-byte store.
//   * Tiny layers (4x4 .. 8x8) pack several samples into one pixel tile.
// Demodulation and the weight layouts: modconv_prep.hip; weight gradients: modconv_wgrad.hip; the stand-alone ToRGB: torgb.hip.
#include <type_traits>
#include "common.h"
#include <cstdio>
#include <cstdlib>

namespace {

// LDS-DMA: `buffer_load_dword(x4) ... lds` — 64 lanes x SIZE bytes land at lds + lane * SIZE (wave-uniform base), from
// rsrc base + voff (per lane, range-checked against the resource: out of range -> zeros) + soff (wave-uniform).
// (Kept in a helper with a device-pass guard: the host pass of hipcc silently drops the host stub of a template
// kernel whose body names this builtin directly.)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int SIZE, typename RSRC>
__device__ __forceinline__ void dma_to_lds(RSRC rsrc, float* lds, unsigned voff, unsigned soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(3))) void* lds_void_ptr;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_ptr)lds, SIZE, voff, soff, 0, 0);
#endif
}

// A pointer / word the compiler cannot prove wave-uniform (it came through a runtime-indexed segment table), declared
// uniform: buffer resources built from it stay in SGPRs instead of sending every buffer_load through a waterfall loop.
__device__ __forceinline__ const float* uniform_ptr(const float* q) {
  const unsigned long long v = (unsigned long long)q;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const float*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ unsigned uniform_u32(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }

// ------------------------------------------------------------------ MFMA conv
struct MCParams {
  const float* in; const float* wt; const float* style; const float* demod; float* out;
  int batch, cin, cout, h, w, oh, ow;
  long long out_plane_stride; int out_row_stride;   // elements; contiguous: oh*ow and ow
  // Position grid = up to 3 rectangular segments tiled independently but launched together (mode 1: the h x w
  // quad grid plus the last output row and the last output column; mode 0: one segment h x w).
  struct Seg {
    int m_off, n_off, gh, gw;        // sub-grid origin and size (positions)
    int th, nb, tw_log2;             // tile rows per sample, samples per tile, log2(tile width)
    int tiles_x, tiles_y, tiles_b;
    unsigned block_end;              // first logical block id after this segment
    int wide;                        // PIPE 1: the halo patch is staged in 16-byte pieces (see "wide patch" in the kernel)
  } seg[3];
  int nseg, o_tiles;
  int ksplit, cin_per_split;         // split-K over input channels (tiny layers); partials go to `ws`
  float* ws;
  const float* noise; const float* noise_weight; const float* bias;
  int noise_batch, fuse_act; float alpha, act_scale;
  // ToRGB fused into the epilogue (MODE 0, one output-channel tile, no split-K): the block holds every channel of
  // its pixels, so rgb[b,c,pix] = sum_o act[b,o,pix] * wmod[b,c,o] (+ bias + skip) is a reduction over
  // the accumulator rows; `out` may then be null (last layer: the activation has no other consumer).
  const float* rgb_wmod;   // [batch][3][cout] = rgb_scale * W[c,o] * rgb_style[b,o], rows >= rgb_c zero
  const float* rgb_bias; const float* rgb_skip; float* rgb_out;
  int rgb_c;
  // PIPE 1 (all staging by LDS-DMA): floats per LDS buffer = weights + patch region + style region, and the patch
  // region's size (both rounded to 64 floats so every DMA piece of 64 lanes x 4 B stays inside its region)
  int lds_buf_floats, lds_patch_floats;
  int lds_style_floats;              // PIPE 1: > 0 = the tile's whole style slice [cin_per_split] is staged once, behind bias/demod
  // experiments only (FMGAN_MC_DEBUG, tools/bench_conv_variants.py --debug): bit 0 = stage the first chunk only (ablation:
  // what the MFMA + operand-fetch loop alone reaches; results are wrong), bit 1 = no barriers in the K loop (wrong too),
  // bit 2 = PIPE 1: issue all DMA pieces of the next chunk up front instead of spreading them over the MFMA stages.
  int debug;
  // experiments only (FMGAN_MC_CLOCKPTR = device address of 16 x uint64): block 0 adds its shader-clock cycles
  // (s_memtime) and its constant-100-MHz ticks (s_memrealtime): their ratio is the clock the chip held during the kernel
  unsigned long long* dbg_clock;
  int exp_flags;     // experiments only (FMGAN_MC_FLAGS, read per call): bit 0 = set-up and epilogue at wave priority 3
};

#ifdef FMGAN_EXPERIMENTS
#define MC_DEBUG(p) ((p).debug)
#define MC_CLOCK(p) ((p).dbg_clock)
#define MC_FLAGS(p) ((p).exp_flags)
#else                                   // product build: the ablation branches fold away
#define MC_DEBUG(p) 0
#define MC_CLOCK(p) false
#define MC_FLAGS(p) 0
#endif

constexpr int MC_KC = 8;  // input channels per LDS chunk

// demod scale + optional StyledConv epilogue (stylegan2.py:371-373) — shared by the conv epilogue and the split-K finish
__device__ __forceinline__ float mc_epilogue(float v, const MCParams& p, float nw, int b, int o, int pix) {
  if (p.demod) v *= p.demod[(long long)b * p.cout + o];
  if (p.fuse_act) {
    const float n = p.noise ? p.noise[(long long)(p.noise_batch == 1 ? 0 : b) * p.oh * p.ow + pix] : 0.f;
    const float bv = p.bias ? p.bias[o] : 0.f;
    v = __fadd_rn(__fadd_rn(v, __fmul_rn(nw, n)), bv);
    v = (v > 0.f ? v : v * p.alpha) * p.act_scale;
  }
  return v;
}

// MODE 0: plain 3x3, one output pixel per position, 9 taps.
// MODE 2: stride-2 valid 3x3 (the reference's downsample branch, and the data-gradient of MODE 1):
//         out[y,x] = sum w[ky][kx] * in[2y+ky, 2x+kx]; same contraction as MODE 0 over a stride-2 patch.
// MODE 1: transposed stride-2 3x3. Position (m,n) owns the 2x2 output quad (2m+py, 2n+px); its four phases
//         use 4+2+2+1 = 9 taps of the same staged weights and only 4 distinct input offsets:
//         out[2m+py, 2n+px] += w[ky][kx] * in[m - ky/2, n - kx/2],  ky = py (mod 2), kx = px (mod 2).
// (A single-barrier variant — LDS double-buffered, the fill of chunk c+1 sliced between chunk c's MFMA stages — was
// built and measured: 95 vs 121 TFLOP/s on the 128x128 tile.  It halves the co-resident blocks per CU and puts the
// staging instructions of the only remaining wave per SIMD in front of its own MFMAs.  Not kept.
// Persistent tiles for the short-K layers (a block walks 2-8 tiles and loads the next tile's first chunk under the
// current tile's last chunk / epilogue) were also measured: 56-88 vs 68-97 TFLOP/s on the 512^2-1024^2 layers —
// holding the prefetched chunk across the epilogue spills 20-70 VGPRs, and the two co-resident blocks per SIMD
// already overlap one block's prologue/epilogue with the other's MFMAs.  Not kept.
// Two LDS images with ONE barrier per chunk, keeping two blocks per CU (possible for the 64- and 32-channel tiles and
// both transposed tiles: <= 39 KB per image): issue(c+1); MFMAs(c); commit(c+1 -> other image); barrier.  Measured
// slower on every layer it applies to (transposed 128^2..512^2: 860/850/940 vs 812/793/893 us; plain 1024^2: 1713 vs
// 1673 us).  Not kept.
// Interleaving the two 32-channel halves of each 64-channel group in the LDS weight image (so the RM = 2 tiles read
// both A operands of a tap with one ds_read_b64: 25-40 % fewer LDS read instructions, same loads and writes) changed
// nothing measurable (+-1 %): the count of A-operand reads is not what limits the MFMA rate.  Not kept.
// 16-channel chunks for the 64- and 32-channel tiles (twice the MFMAs per pair of barriers): with the same register
// budgets 28-94 VGPRs spill (1964 vs 1603 us on the 1024^2 layer); with budgets that fit (one block per CU less)
// 1820 vs 1603 us, 1550 vs 1400 us (512^2), transposed 1033 vs 890 us: co-resident blocks beat longer chunks.  Not kept.
// The 128 x 128 tile on 8 waves (512 threads, each wave 64 x 32, 4 waves per SIMD in a 128-register budget): 24 VGPRs
// spill and it ties with the 4-wave tile (123.6 vs 125.0 TFLOP/s at 64^2).  Not kept.)
// PIPE 0: register-prefetch staging (global -> VGPR one chunk ahead -> ds_write after a barrier; two barriers per chunk).
// PIPE 1: everything a chunk needs — weights (16-byte pieces), the halo patch and the style slice (4-byte pieces) — is
//         written into LDS by `buffer_load ... lds` (LDS-DMA: no VGPR destination, no ds_write, no commit phase), into
//         the buffer the PREVIOUS chunk is not reading; one barrier per chunk.  The style modulation moves from the
//         staging write to the operand fetch (x * s in a VALU op right before the MFMA: the same fp32 product, so both
//         pipelines give identical bits).  Patch slots outside the image rely on the buffer range check: their
//         voffset is parked out of range and the DMA writes zeros (tools/exp/dma_probe.hip).  Chunks that the range check
//         cannot serve (a partial last chunk, tensors of 4 GB and more, ragged Cout) are filled synchronously instead.
// Tile: one of the named tile types below (its name shows in the mangled symbol and in rocprofv3 output).
//   MODE           see above
//   RM x RNP       32 x 32 accumulators per wave: rows of 32 output channels x groups of 32 positions
//   WM x WN        waves of the block along output channels x positions (4 in all)
//   MINB           blocks per CU the register budget is set for (launch bounds: 512 / MINB registers per lane)
//   KC             input channels per LDS chunk
//   PIPE           see above
template <int MODE_, int RM_, int RNP_, int WM_, int WN_, int MINB_, int KC_, int PIPE_>
struct TileShape {
  static constexpr int MODE = MODE_, RM = RM_, RNP = RNP_, WM = WM_, WN = WN_, MINB = MINB_, KC = KC_, PIPE = PIPE_;
  static constexpr int BM = 32 * RM * WM, BN = 32 * RNP * WN;   // output channels x positions of a block
};
// Named <conv><BM>x<BN><pipeline>[Kc4][R<registers per lane>]: Reg = register prefetch, Dma = LDS-DMA; Kc4 = 4-channel
// chunks (8 otherwise); R... where two tiles differ in nothing but the register budget.
//                                         MODE  RM  RNP  WM  WN  MINB     KC  PIPE
struct Plain128x128Reg         : TileShape<   0,  2,   2,  2,  2,    2, MC_KC,    0> {};
struct Plain128x128DmaKc4      : TileShape<   0,  2,   2,  2,  2,    3,     4,    1> {};
struct Plain128x256DmaKc4      : TileShape<   0,  4,   2,  1,  4,    2,     4,    1> {};   // 0.75 LDS reads / MFMA
struct Plain64x128Reg          : TileShape<   0,  2,   1,  1,  4,    3, MC_KC,    0> {};
struct Plain64x128Dma          : TileShape<   0,  2,   1,  1,  4,    3,     8,    1> {};
struct Plain64x256DmaKc4       : TileShape<   0,  2,   2,  1,  4,    3,     4,    1> {};   // 3 blocks per CU
struct Plain32x128Reg          : TileShape<   0,  1,   1,  1,  4,    4, MC_KC,    0> {};
struct Plain32x128Dma          : TileShape<   0,  1,   1,  1,  4,    4,     8,    1> {};
struct Plain32x256DmaKc4R128   : TileShape<   0,  1,   2,  1,  4,    4,     4,    1> {};   // in a 128-register budget (4 blocks per CU, no spills)
struct Stride2x128x128Reg      : TileShape<   2,  2,   2,  2,  2,    2, MC_KC,    0> {};
struct Stride2x64x128Reg       : TileShape<   2,  2,   1,  1,  4,    2, MC_KC,    0> {};
struct Stride2x32x128Reg       : TileShape<   2,  1,   1,  1,  4,    2, MC_KC,    0> {};
struct Transposed64x128Reg     : TileShape<   1,  2,   1,  1,  4,    2, MC_KC,    0> {};
struct Transposed64x128Dma     : TileShape<   1,  2,   1,  1,  4,    2,     8,    1> {};
struct Transposed32x128Reg     : TileShape<   1,  1,   1,  1,  4,    3, MC_KC,    0> {};
struct Transposed32x128DmaR128 : TileShape<   1,  1,   1,  1,  4,    4,     8,    1> {};   // 4 blocks per CU instead of 3
#ifdef FMGAN_EXPERIMENTS   // tiles no default and no fall-back reaches: measured, kept for A/B runs (see mc_variant)
struct Plain32x256Dma          : TileShape<   0,  1,   2,  1,  4,    3,     8,    1> {};   // 3 blocks per CU
struct Plain32x256DmaKc4R96    : TileShape<   0,  1,   2,  1,  4,    5,     4,    1> {};   // 4-channel chunks: 5-6 blocks per CU
struct Transposed32x256Dma     : TileShape<   1,  1,   2,  1,  4,    2,     8,    1> {};   // 32 x 256 positions
struct Transposed32x128DmaR170 : TileShape<   1,  1,   1,  1,  4,    3,     8,    1> {};
#endif

template <class Tile, bool RGB>
__global__ __launch_bounds__(256, Tile::MINB) void modconv_mfma_f32(const MCParams p) {
  constexpr int MODE = Tile::MODE, RM = Tile::RM, RNP = Tile::RNP, WM = Tile::WM, WN = Tile::WN, KC = Tile::KC, PIPE = Tile::PIPE;
  static_assert(!RGB || MODE == 0, "the RGB epilogue belongs to the plain conv");
  static_assert(PIPE == 1 || KC == MC_KC, "the register pipeline is built for 8-channel chunks");
  constexpr int BM = Tile::BM;
  constexpr int NPH = MODE == 1 ? 4 : 1;   // output phases per position
  static_assert(WM * WN == 4, "4 waves per block");
  extern __shared__ float smem[];
  float* Ws = smem;                 // [KC][9][BM]
  float* Xs = smem + KC * 9 * BM;   // [nb][KC][PH][PWP]

  // wave index as an SGPR: LDS-DMA destinations (M0), piece guards and tile offsets derived from it stay scalar
  // (left in a VGPR, every `buffer_load ... lds` sat in a waterfall loop with v_readfirstlane)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int l31 = lane & 31, khalf = lane >> 5;
  unsigned long long clk0 = 0, rt0 = 0;
  if (MC_CLOCK(p)) { clk0 = __builtin_readcyclecounter(); rt0 = wall_clock64(); }
  if (MC_FLAGS(p) & 1) __builtin_amdgcn_s_setprio(3);

  unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
  int si = 0;
  while (si + 1 < p.nseg && lb >= p.seg[si].block_end) ++si;
  if (si > 0) lb -= p.seg[si - 1].block_end;
  // mode 1: taps (bit ky*3+kx) this block's segment needs — row strip: ky = 2, column strip: kx = 2, main grid: all
  const unsigned tapmask = (MODE == 1 && p.nseg == 3) ? (si == 0 ? 0x1C0u : (si == 1 ? 0x124u : 0x1FFu)) : 0x1FFu;
  const int seg_th = p.seg[si].th, seg_nb = p.seg[si].nb, tw_log2 = p.seg[si].tw_log2;
  const int seg_m_end = p.seg[si].m_off + p.seg[si].gh, seg_n_end = p.seg[si].n_off + p.seg[si].gw;
  constexpr int SP = MODE == 2 ? 2 : 1;          // input step per position
  constexpr int ORG = MODE == 2 ? 0 : 1;         // patch origin = SP * first position - ORG
  // Wide patch (PIPE 1, unit-step modes, 32-wide tiles of images whose rows are whole 16-byte groups; host decides): the
  // patch starts FOUR columns left of the tile instead of one and is TW + 8 wide, so every row is ten aligned 16-byte groups,
  // each either inside the image row or outside it as a whole — one `buffer_load_dwordx4 ... lds` lane moves what four
  // dword lanes moved.  The short-K layers issue ~3.5x fewer vector-memory instructions per chunk: measured with s_memtime
  // stamps (profiles/r03_modconv_block_phases.md) a wave of the 1024^2 layer held the matrix pipe 25 % of its K loop with 2.7
  // waves per SIMD in the loop — it sat in the issue of its DMA pieces, and each epilogue store took ~350 cycles to issue
  // behind them (vector memory is one in-order pipeline per CU).
  const bool wide = PIPE == 1 && SP == 1 && p.seg[si].wide != 0;
  const int XORG = wide ? 4 : ORG;               // patch column c holds image column SP * x0 + c - XORG
  const int TW = 1 << tw_log2, PWP = wide ? TW + 8 : SP * (TW - 1) + 3;
  const int o_tile = lb % p.o_tiles;
  unsigned pt = lb / p.o_tiles;
  const int tx_i = pt % p.seg[si].tiles_x; pt /= p.seg[si].tiles_x;
  const int ty_i = pt % p.seg[si].tiles_y;
  const int tb_i = pt / p.seg[si].tiles_y;
  const int ks = blockIdx.y;
  const int o0 = o_tile * BM, b0 = tb_i * seg_nb;
  const int x0 = p.seg[si].n_off + tx_i * TW, y0 = p.seg[si].m_off + ty_i * seg_th;   // first position of the tile
  const int PH = SP * (seg_th - 1) + 3;
  const int plane = PH * PWP;
  const int samp = KC * plane;

  // this lane's position in each of the wave's 32-position groups
  int pbase[RNP], pos_b[RNP], pos_y[RNP], pos_x[RNP];
#pragma unroll
  for (int g = 0; g < RNP; ++g) {
    const int pos = (wn * RNP + g) * 32 + l31;
    const int tx = pos & (TW - 1), r = pos >> tw_log2;
    const int ty = r % seg_th, nbi = r / seg_th;
    // (a thin segment's tile may hold fewer than BN positions — launch_tile shrinks it until its patch fits the main
    // segment's LDS image: the rows past nb * th read sample nb - 1's patch and are never stored)
    pbase[g] = min(nbi, seg_nb - 1) * samp + SP * ty * PWP + SP * tx + (XORG - ORG);
    pos_b[g] = nbi < seg_nb ? b0 + nbi : p.batch; pos_y[g] = y0 + ty; pos_x[g] = x0 + tx;
  }

  f32x16 acc[RM][RNP][NPH];
#pragma unroll
  for (int a = 0; a < RM; ++a)
#pragma unroll
    for (int b = 0; b < RNP; ++b)
#pragma unroll
      for (int c = 0; c < NPH; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][c][r] = 0.f;

  const bool wvec = (p.cout & 3) == 0;
  const int i_begin = ks * p.cin_per_split;
  const int i_end = min(p.cin, i_begin + p.cin_per_split);
  const int hw = p.h * p.w;

  // ---- staging plan, fixed for the whole K loop.
  // Patch: thread owns up to NU spatial slots (sample, row, col) of the halo patch and moves all KC channels of
  // each; weights: NWV float4 per thread.  Everything a chunk needs is loaded into registers one chunk AHEAD
  // (while the previous chunk is on the matrix pipe) and written to LDS after the barrier.
  constexpr int BNP = 32 * RNP * WN;
  constexpr int NU = ((SP * (BNP / 32 - 1) + 3) * (SP * 31 + 3) + 255) / 256;   // covers a full-width main tile
  constexpr int NWV = (KC * 9 * (BM / 4) + 255) / 256;
  const int spatial = seg_nb * plane;                              // patch slots per channel
  // element offsets are 32-bit, relative to the tile's first sample (host checks nb*cin*h*w < 2^31)
  const float* in_b0 = uniform_ptr(p.in + (long long)b0 * p.cin * hw);
  const float* style_b0 = uniform_ptr(p.style + (long long)b0 * p.cin);
  // PIPE 1, tiles of one sample: the tile's bias and demodulation values go to LDS now, one vector load per wave, and the
  // epilogue reads them back with ds_read_b128 — it used to issue 32 two-address vector loads per wave and row group
  // right when the block's stores want the (in-order, shared) vector-memory pipeline.  Visible to every wave after the
  // K loop's first barrier.
  // (The load is issued here and its value written to LDS after the first chunk's DMA pieces are out, so its latency hides
  // under the wait for that chunk.)
  const bool epi_lds = PIPE == 1 && seg_nb == 1 && p.ksplit == 1;
  float* Es = smem + 2 * p.lds_buf_floats;        // [2][BM]: bias, demod
  float epi_v = 0.f;
  if constexpr (PIPE == 1) {
    if (epi_lds && tid < 2 * BM) {
      const bool isd = tid >= BM;
      const int oc = min(o0 + (isd ? tid - BM : tid), p.cout - 1);
      epi_v = isd ? 1.f : 0.f;
      if (isd) { if (p.demod) epi_v = p.demod[(long long)min(b0, p.batch - 1) * p.cout + oc]; }
      else if (MODE == 0 && p.fuse_act && p.bias) epi_v = p.bias[oc];
    }
  }
  int gofs[NU], lofs[NU], sofs[NU]; bool inb[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int q = tid + 256 * u;
    const int c = q % PWP;
    int t = q / PWP;
    const int r = t % PH, nbi = t / PH;
    const int b = b0 + nbi, y = SP * y0 + r - ORG, x = SP * x0 + c - ORG;
    inb[u] = q < spatial && b < p.batch && y >= 0 && y < p.h && x >= 0 && x < p.w;
    gofs[u] = inb[u] ? (nbi * p.cin * p.h + y) * p.w + x : 0;
    sofs[u] = nbi * p.cin;
    lofs[u] = q < spatial ? nbi * samp + r * PWP + c : -1;
  }
  float xv[NU][KC];
  f32x4 wv[NWV];
  // Fast path: buffer loads.  The per-thread byte offsets are fixed for the whole K loop (voffset), the chunk only
  // moves a scalar (soffset), and the hardware range check returns 0 for patch slots that fall outside the image
  // (their voffset is parked past the end) — no per-load 64-bit address math, no branches.  A partial last chunk
  // (cin not a multiple of 8) takes the guarded path.
  // (An ablation showed the MFMA stages alone reach 140 TFLOP/s and the staging INSTRUCTIONS, not the bytes, are
  // what the co-resident block has to hide.)
  // The range check compares voffset (+4) with num_records and ignores soffset: a slot is "out of range" only through
  // its parked voffset 0xFFFFFFF0, so the buffers must be SHORTER than that (with num_records >= 0xFFFFFFF4 a parked
  // slot would pass the check and read base + 0xFFFFFFF0 + soffset).  Larger tensors take the guarded path.
  constexpr long long PARK = 0xFFFFFFF0LL;
  const bool fastw = wvec && o0 + BM <= p.cout && (long long)p.cin * 9 * p.cout * 4 < PARK;
  const bool fastx = (long long)min(seg_nb, p.batch - b0) * p.cin * hw * 4 < PARK;
  const unsigned w_bytes = uniform_u32((unsigned)((long long)p.cin * 9 * p.cout * 4));
  const unsigned x_bytes = uniform_u32((unsigned)((long long)min(seg_nb, p.batch - b0) * p.cin * hw * 4));
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wt), 0, w_bytes, 0x00020000);
  const auto rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in_b0), 0, x_bytes, 0x00020000);
  unsigned wofs[NWV], xofs[NU];
#pragma unroll
  for (int j = 0; j < NWV; ++j) {
    const int idx = tid + 256 * j;
    const int row = idx / (BM / 4), c4 = idx % (BM / 4);
    wofs[j] = idx < KC * 9 * (BM / 4) ? (unsigned)((row * p.cout + o0 + c4 * 4) * 4) : 0xFFFFFFF0u;
  }
#pragma unroll
  for (int u = 0; u < NU; ++u) xofs[u] = inb[u] ? (unsigned)gofs[u] * 4u : 0xFFFFFFF0u;
  auto issue = [&](int i0) {
    if (fastw && i0 + KC <= i_end) {
      const unsigned soff = (unsigned)(i0 * 9 * p.cout * 4);
#pragma unroll
      for (int j = 0; j < NWV; ++j) {
        const auto t = __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, wofs[j], soff, 0);
        wv[j] = __builtin_bit_cast(f32x4, t);
      }
    } else {
#pragma unroll
      for (int j = 0; j < NWV; ++j) {
        const int idx = tid + 256 * j;
        const int row = idx / (BM / 4), c4 = idx % (BM / 4);
        const int i = i0 + row / 9, o = o0 + c4 * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (idx < KC * 9 * (BM / 4) && i < i_end) {
          const float* src = p.wt + ((long long)i * 9 + row % 9) * p.cout + o;
          if (wvec && o + 3 < p.cout) {
            v = *reinterpret_cast<const f32x4*>(src);
          } else {
            if (o + 0 < p.cout) v.x = src[0];
            if (o + 1 < p.cout) v.y = src[1];
            if (o + 2 < p.cout) v.z = src[2];
            if (o + 3 < p.cout) v.w = src[3];
          }
        }
        wv[j] = v;
      }
    }
    if (fastx && i0 + KC <= i_end) {
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        const unsigned soff = (unsigned)((i0 + kc) * hw * 4);
#pragma unroll
        for (int u = 0; u < NU; ++u)
          xv[u][kc] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_x, xofs[u], soff, 0));
      }
    } else {
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          const int i = i0 + kc;
          xv[u][kc] = (inb[u] && i < i_end) ? in_b0[gofs[u] + i * hw] : 0.f;
        }
    }
  };
  auto commit = [&](int i0) {
#pragma unroll
    for (int j = 0; j < NWV; ++j) {
      const int idx = tid + 256 * j;
      if (idx < KC * 9 * (BM / 4)) *reinterpret_cast<f32x4*>(Ws + idx * 4) = wv[j];
    }
    // modulate on the way in: x[b,i] * style[b,i] (the style loads are L1 hits, issued ahead of the weight writes)
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (lofs[u] >= 0) {
        float sv[KC];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) sv[kc] = (inb[u] && i0 + kc < i_end) ? style_b0[sofs[u] + i0 + kc] : 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) Xs[lofs[u] + kc * plane] = xv[u][kc] * sv[kc];
      }
    // patches larger than a main tile's (sample-packed tiny layers, thin edge segments): synchronous remainder
    for (int q = tid + 256 * NU; q < spatial; q += 256) {
      const int c = q % PWP;
      int t = q / PWP;
      const int r = t % PH, nbi = t / PH;
      const int b = b0 + nbi, y = SP * y0 + r - ORG, x = SP * x0 + c - ORG;
      const bool ok = b < p.batch && y >= 0 && y < p.h && x >= 0 && x < p.w;
      for (int kc = 0; kc < KC; ++kc) {
        const int i = i0 + kc;
        float v = 0.f;
        if (ok && i < i_end) {
          const long long ch = (long long)b * p.cin + i;
          v = p.in[(ch * p.h + y) * p.w + x] * p.style[ch];
        }
        Xs[nbi * samp + kc * plane + r * PWP + c] = v;
      }
    }
  };

  // LDS -> registers, one pipeline stage = one row of taps (MODE 0: 3 taps x channel pair) or one channel pair
  // (MODE 1: its 9 taps share 4 input offsets).  Stage s+1 is fetched while stage s is on the matrix pipe.
  constexpr int NTA = MODE == 1 ? 9 : 3;     // A (weight) values per stage per 32-row tile
  constexpr int NTB = MODE == 1 ? 4 : 3;     // B (input) values per stage per position group
  constexpr int NSTAGE = (KC / 2) * (MODE == 1 ? 1 : 3);
  struct Ops { float a[NTA][RM]; float b[NTB][RNP]; float s[RNP]; };
  const float* Wc = Ws;            // LDS image the current chunk is read from (PIPE 1: toggles between two buffers)
  const float* Xc = Xs;
  const float* Sc = nullptr;       // PIPE 1: style slice [nb][KC] of the chunk
  int sbase[RNP];                  // PIPE 1: this lane's sample row in the style slice
#pragma unroll
  for (int g = 0; g < RNP; ++g) sbase[g] = (pbase[g] / samp) * KC;
  auto fetch = [&](Ops& o, int st) {
    const int kk = MODE == 1 ? st : st / 3, ky = MODE == 1 ? 0 : st % 3;
    const int kc = 2 * kk + khalf;
    const float* wrow = Wc + (kc * 9 + ky * 3) * BM + wm * 32 * RM + l31;
    const float* xrow = Xc + kc * plane;
#pragma unroll
    for (int t = 0; t < NTA; ++t)
#pragma unroll
      for (int m = 0; m < RM; ++m) o.a[t][m] = wrow[t * BM + m * 32];
    if constexpr (PIPE == 1) {
      if (MODE == 1 || ky == 0) {
#pragma unroll
        for (int g = 0; g < RNP; ++g) o.s[g] = Sc[sbase[g] + kc];
      }
    }
#pragma unroll
    for (int j = 0; j < NTB; ++j) {
      // MODE 0: offset (ky, kx = j); MODE 1: j -> (ro, co) = (1,1) (1,0) (0,1) (0,0)
      const int ro = MODE == 1 ? 1 - (j >> 1) : ky;
      const int co = MODE == 1 ? 1 - (j & 1) : j;
#pragma unroll
      for (int g = 0; g < RNP; ++g) o.b[j][g] = xrow[pbase[g] + ro * PWP + co];
    }
  };
  // PIPE 1: x * style[b, i] on the way to the matrix pipe (PIPE 0 did it on the way into LDS)
  auto modulate = [&](Ops& o) {
    if constexpr (PIPE == 1) {
#pragma unroll
      for (int j = 0; j < NTB; ++j)
#pragma unroll
        for (int g = 0; g < RNP; ++g) o.b[j][g] *= o.s[g];
    }
  };
  auto mma = [&](const Ops& o, auto all_taps) {
    if constexpr (MODE != 1) {
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int m = 0; m < RM; ++m)
#pragma unroll
          for (int g = 0; g < RNP; ++g)
            acc[m][g][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[t][m], o.b[t][g], acc[m][g][0], 0, 0, 0);
    } else {
      // (tap = ky*3+kx, input-offset index j, phase = py*2+px)
      constexpr int T[9][3] = {{0, 0, 0}, {2, 1, 0}, {6, 2, 0}, {8, 3, 0}, {1, 0, 1}, {7, 2, 1}, {3, 0, 2}, {5, 1, 2}, {4, 0, 3}};
      // The two thin segments (last output row: positions m = h; last output column: n = w) only ever see the taps
      // whose input lies inside the image — ky = 2 resp. kx = 2: every other product has a zero operand.  Their
      // blocks skip those MFMAs (a wave-uniform bit per tap: same sums, bit for bit) and finish three times sooner.
#pragma unroll
      for (int q = 0; q < 9; ++q)
        if (decltype(all_taps)::value || (tapmask & (1u << T[q][0])))
#pragma unroll
          for (int m = 0; m < RM; ++m)
#pragma unroll
            for (int g = 0; g < RNP; ++g)
              acc[m][g][T[q][2]] =
                  __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[T[q][0]][m], o.b[T[q][1]][g], acc[m][g][T[q][2]], 0, 0, 0);
    }
  };

  // ---- contract: operands of stage st+1 are fetched while stage st is on the matrix pipe.
  // (hipcc otherwise sinks every ds_read next to its MFMA and waits lgkmcnt(0) in front of each group of four:
  // the sched_barriers keep "issue all reads of stage st+1, then run stage st's MFMAs" as written.)
  // hook(st): extra issue work placed in front of stage st's MFMAs (PIPE 1: a slice of the next chunk's DMA pieces)
  // Two operand sets used alternately (NSTAGE is even).  The MFMA cluster of a stage runs at raised wave priority
  // (s_setprio): with three or more waves per SIMD the arbiter otherwise lets the other waves' LDS reads and address
  // VALU in between the matrix instructions — 1024^2 plain 1707 -> 1628 us, transposed 64^2 811 -> 782, the 17 layers
  // 11.87 -> 11.70 ms; little effect on the two-wave 128 x 256 tile.
  static_assert(NSTAGE % 2 == 0, "stages are processed in pairs");
  auto contract = [&](auto&& hook, auto all_taps) {
    Ops o0, o1;
    fetch(o0, 0);
#pragma unroll
    for (int st = 0; st < NSTAGE; st += 2) {
      __builtin_amdgcn_sched_barrier(0);
      hook(st);
      fetch(o1, st + 1);
      if constexpr (PIPE == 1 && MODE != 1) {
        // the style value of a channel pair is read with its first tap row and reused for the other two
        if ((st + 1) % 3 != 0) {
#pragma unroll
          for (int g = 0; g < RNP; ++g) o1.s[g] = o0.s[g];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      modulate(o0);
      __builtin_amdgcn_s_setprio(1);
      mma(o0, all_taps);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      hook(st + 1);
      if (st + 2 < NSTAGE) {
        fetch(o0, st + 2);
        if constexpr (PIPE == 1 && MODE != 1) {
          if ((st + 2) % 3 != 0) {
#pragma unroll
            for (int g = 0; g < RNP; ++g) o0.s[g] = o1.s[g];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      modulate(o1);
      __builtin_amdgcn_s_setprio(1);
      mma(o1, all_taps);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  unsigned long long clk1 = 0, clk2 = 0, clkw = 0, clke = 0, clkl = 0;
  if (MC_CLOCK(p)) clk1 = __builtin_readcyclecounter();
  if (MC_FLAGS(p) & 1) __builtin_amdgcn_s_setprio(0);
  if constexpr (PIPE == 0) {
    if (i_begin < i_end) issue(i_begin);
    for (int i0 = i_begin; i0 < i_end; i0 += KC) {
      const bool live = !(MC_DEBUG(p) & 1) || i0 == i_begin;
      if (!(MC_DEBUG(p) & 2)) __syncthreads();            // every wave is done reading the previous chunk
      if (live) commit(i0);
      if (!(MC_DEBUG(p) & 2)) __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
      if (live && i0 + KC < i_end) issue(i0 + KC);   // in flight during this chunk's MFMAs
      contract([](int) {}, std::false_type{});
    }
  } else {
    constexpr unsigned PARKED = 0xFFFFFFF0u;
    // floats of one weight image, rounded up to whole 16-byte DMA pieces (64 lanes x 16 B = 256 floats; the lanes past the
    // image are parked and write zeros into the padding)
    constexpr int WSZ = (KC * 9 * BM + 255) / 256 * 256;
    constexpr int WPIECES = WSZ / 256;
    constexpr int NWP = (WPIECES + 3) / 4;                  // per wave
    constexpr int NUP = ((KC * (SP * (BNP / 32 - 1) + 3) * (SP * 31 + 3) + 63) / 64 + 3) / 4;   // patch pieces per wave, main tile
    const int xs_total = seg_nb * samp;                     // patch floats
    const int x_piece_floats = wide ? 256 : 64;             // one DMA piece = 64 lanes x 16 or 4 bytes
    const int x_pieces = (xs_total + x_piece_floats - 1) / x_piece_floats;
    const int s_pieces = (seg_nb * KC + 63) >> 6;
    const int bstride = p.lds_buf_floats;
    const bool fastc = fastw && fastx;                      // DMA-servable tensors (chunk completeness checked per chunk)
    const unsigned s_bytes = (unsigned)(min(seg_nb, p.batch - b0) * p.cin * 4);
    const auto rsrc_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(style_b0), 0, s_bytes, 0x00020000);
    // patch element (linear LDS index) -> byte offset from in_b0 of channel i0, or PARKED
    auto x_voff = [&](int e) -> unsigned {
      if (e >= xs_total) return PARKED;
      const int nbi = e / samp, rem = e - nbi * samp;
      const int kc = rem / plane, q = rem - kc * plane;
      const int r = q / PWP, c = q - r * PWP;
      const int b = b0 + nbi, y = SP * y0 + r - ORG, x = SP * x0 + c - XORG;
      const bool ok = b < p.batch && y >= 0 && y < p.h && x >= 0 && x < p.w;
      return ok ? (unsigned)(((nbi * p.cin + kc) * p.h + y) * p.w + x) * 4u : PARKED;
    };
    // wide patch: 16-byte group g16 (four floats, linear LDS index 4 * g16) -> byte offset of its first float, or PARKED;
    // x is a multiple of 4 and so is p.w (host), so a group never straddles the end of an image row
    auto x_voff16 = [&](int g16) -> unsigned { return x_voff(4 * g16); };
    auto s_voff = [&](int e) -> unsigned {
      const int nbi = e / KC, kc = e - nbi * KC;
      return (nbi < seg_nb && b0 + nbi < p.batch) ? (unsigned)(nbi * p.cin + kc) * 4u : PARKED;
    };
    unsigned wvo[NWP], xvo[NUP];
#pragma unroll
    for (int j = 0; j < NWP; ++j) {
      const int idx = (4 * j + wave) * 64 + lane;           // float4 index in the image [KC*9][BM/4]
      const int row = idx / (BM / 4), c4 = idx % (BM / 4);
      wvo[j] = idx < KC * 9 * (BM / 4) ? (unsigned)((row * p.cout + o0 + c4 * 4) * 4) : PARKED;
    }
#pragma unroll
    for (int u = 0; u < NUP; ++u)
      xvo[u] = 4 * u + wave < x_pieces ? (wide ? x_voff16((4 * u + wave) * 64 + lane) : x_voff((4 * u + wave) * 64 + lane)) : PARKED;
    const unsigned svo = s_voff(wave * 64 + lane);          // first style piece of this wave (all of them when nb*KC <= 256)

    // This wave's DMA pieces of one chunk, numbered k = 0 .. NPC-1: weights, patch, then the style slice together with
    // whatever a larger-than-main-tile patch / a sample-packed style slice has left.
    constexpr int NPC = NWP + NUP + 1;
    constexpr int PER_STAGE = (NPC + NSTAGE - 1) / NSTAGE;
    auto dma_piece = [&](int k, int i0, int buf) {
      float* Wb = smem + buf * bstride;
      float* Xb = Wb + WSZ;
      const unsigned soff_x = (unsigned)(i0 * hw * 4);
      if (k < NWP) {
        if (4 * k + wave < WPIECES)
          dma_to_lds<16>(rsrc_w, Wb + (4 * k + wave) * 256, wvo[k < NWP ? k : 0], (unsigned)(i0 * 9 * p.cout * 4));
      } else if (k < NWP + NUP) {
        const int u = k - NWP;
        if (4 * u + wave < x_pieces) {
          if (wide) dma_to_lds<16>(rsrc_x, Xb + (4 * u + wave) * 256, xvo[(u >= 0 && u < NUP) ? u : 0], soff_x);
          else dma_to_lds<4>(rsrc_x, Xb + (4 * u + wave) * 64, xvo[(u >= 0 && u < NUP) ? u : 0], soff_x);
        }
      } else {
        float* Sb = Xb + p.lds_patch_floats;
        for (int pc = 4 * NUP + wave; pc < x_pieces; pc += 4) {     // patches larger than a main tile's
          if (wide) dma_to_lds<16>(rsrc_x, Xb + pc * 256, x_voff16(pc * 64 + lane), soff_x);
          else dma_to_lds<4>(rsrc_x, Xb + pc * 64, x_voff(pc * 64 + lane), soff_x);
        }
        if (wave < s_pieces)
          dma_to_lds<4>(rsrc_s, Sb + wave * 64, svo, (unsigned)(i0 * 4));
        for (int pc = 4 + wave; pc < s_pieces; pc += 4)
          dma_to_lds<4>(rsrc_s, Sb + pc * 64, s_voff(pc * 64 + lane), (unsigned)(i0 * 4));
      }
    };
    auto dma_ok = [&](int i0) { return fastc && i0 + KC <= i_end; };

    auto stage = [&](int i0, int buf) {
      float* Wb = smem + buf * bstride;
      float* Xb = Wb + WSZ;
      float* Sb = Xb + p.lds_patch_floats;
      if (dma_ok(i0)) {
#pragma unroll
        for (int k = 0; k < NPC; ++k) dma_piece(k, i0, buf);
      } else {
        // guarded synchronous fill (same images, zeros where the DMA's range check would have produced them)
        for (int idx = tid; idx < KC * 9 * (BM / 4); idx += 256) {
          const int row = idx / (BM / 4), c4 = idx % (BM / 4);
          const int i = i0 + row / 9, o = o0 + c4 * 4;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (i < i_end) {
            const float* src = p.wt + ((long long)i * 9 + row % 9) * p.cout + o;
            if (o + 0 < p.cout) v.x = src[0];
            if (o + 1 < p.cout) v.y = src[1];
            if (o + 2 < p.cout) v.z = src[2];
            if (o + 3 < p.cout) v.w = src[3];
          }
          *reinterpret_cast<f32x4*>(Wb + idx * 4) = v;
        }
        for (int e = tid; e < x_pieces * x_piece_floats; e += 256) {
          float v = 0.f;
          if (e < xs_total) {
            const int nbi = e / samp, rem = e - nbi * samp;
            const int kc = rem / plane, q = rem - kc * plane;
            const int r = q / PWP, c = q - r * PWP;
            const int b = b0 + nbi, y = SP * y0 + r - ORG, x = SP * x0 + c - XORG, i = i0 + kc;
            if (b < p.batch && y >= 0 && y < p.h && x >= 0 && x < p.w && i < i_end)
              v = p.in[(((long long)b * p.cin + i) * p.h + y) * p.w + x];
          }
          Xb[e] = v;
        }
        for (int e = tid; e < seg_nb * KC; e += 256) {
          const int nbi = e / KC, kc = e - nbi * KC;
          Sb[e] = (b0 + nbi < p.batch && i0 + kc < i_end) ? p.style[(long long)(b0 + nbi) * p.cin + i0 + kc] : 0.f;
        }
      }
    };

    // Lean K loop for the common case — every chunk complete and DMA-servable, the patch and the style slice within the
    // main tile's piece budget, all nine taps live, no debug switches: the general loop below re-tests all of that per
    // chunk and per stage (spread / dma_ok / debug bits, the larger-than-main-tile piece loops with their div/mod
    // address maths, one wave-uniform branch per tap in MODE 1), ~1300 scalar and vector instructions around the 60-72
    // MFMAs of a chunk on the small tiles.  Same DMA pieces, same MFMA order: identical bits.
    // (FMGAN_MC_DEBUG bit 3 forces the general loop: A/B measurements.  Unrolling the lean loop by two chunks, so that the
    // double buffer's index is a compile-time constant in each half, was measured too: no gain — 12.19 vs 12.10-12.13 ms over
    // the 17 layers — and 24-31 more spilled SGPRs; not kept.)
    const bool lean = fastc && MC_DEBUG(p) == 0 && i_begin < i_end && ((i_end - i_begin) % KC) == 0 && x_pieces <= 4 * NUP &&
                      s_pieces <= 4 && tapmask == 0x1FFu;
    const bool style_once = lean && seg_nb == 1 && p.lds_style_floats > 0;
    float* Ss = Es + 2 * BM;
    if (lean) {
      auto piece = [&](int k, int i0, int bufi) {
        float* Wb = smem + bufi * bstride;
        float* Xb = Wb + WSZ;
        if (k < NWP) {
          if (WPIECES % 4 == 0 || 4 * k + wave < WPIECES)
            dma_to_lds<16>(rsrc_w, Wb + (4 * k + wave) * 256, wvo[k < NWP ? k : 0], (unsigned)(i0 * 9 * p.cout * 4));
        } else if (k < NWP + NUP) {
          const int u = k - NWP;
          if (4 * u + wave < x_pieces) {
            if (wide) dma_to_lds<16>(rsrc_x, Xb + (4 * u + wave) * 256, xvo[(u >= 0 && u < NUP) ? u : 0], (unsigned)(i0 * hw * 4));
            else dma_to_lds<4>(rsrc_x, Xb + (4 * u + wave) * 64, xvo[(u >= 0 && u < NUP) ? u : 0], (unsigned)(i0 * hw * 4));
          }
        } else if (!style_once && wave < s_pieces) {
          dma_to_lds<4>(rsrc_s, Xb + p.lds_patch_floats + wave * 64, svo, (unsigned)(i0 * 4));
        }
      };
      // style slice of the whole K range, once (one DMA piece per wave and chunk less; the loads fly with the first chunk)
      float sty0 = 0.f, sty1 = 0.f;
      if (style_once) {
        const int n = i_end - i_begin;
        if (tid < n) sty0 = style_b0[i_begin + tid];
        if (tid + 256 < n) sty1 = style_b0[i_begin + tid + 256];
      }
#pragma unroll
      for (int k = 0; k < NPC; ++k) piece(k, i_begin, 0);
      if (epi_lds && tid < 2 * BM) Es[tid] = epi_v;
      if (style_once) {
        if (tid < p.lds_style_floats) Ss[tid] = sty0;
        if (tid + 256 < p.lds_style_floats) Ss[tid + 256] = sty1;
      }
      int bufl = 0;
      for (int i0 = i_begin; i0 < i_end; i0 += KC, bufl ^= 1) {
        const unsigned long long tw0 = MC_CLOCK(p) ? __builtin_readcyclecounter() : 0;
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (MC_CLOCK(p)) clkw += __builtin_readcyclecounter() - tw0;
        const int i1 = i0 + KC;
        const bool more = i1 < i_end;
        Wc = smem + bufl * bstride;
        Xc = Wc + WSZ;
        Sc = style_once ? Ss + (i0 - i_begin) : Xc + p.lds_patch_floats;
        contract([&](int st) {
          if (more) {
#pragma unroll
            for (int q = 0; q < PER_STAGE; ++q)
              if (st * PER_STAGE + q < NPC) piece(st * PER_STAGE + q, i1, bufl ^ 1);
          }
        }, std::true_type{});
      }
    }
    if (!lean && i_begin < i_end) {
      stage(i_begin, 0);
      if (epi_lds && tid < 2 * BM) Es[tid] = epi_v;
    }
    int buf = 0;
    for (int i0 = lean ? i_end : i_begin; i0 < i_end; i0 += KC, buf ^= 1) {
      // this wave's DMA pieces / LDS stores of chunk i0 have landed; after the barrier everyone's have, and every wave
      // has finished reading the other buffer (its ds_reads were retired before the MFMAs that consumed them)
      __builtin_amdgcn_s_waitcnt(0);
      if (!(MC_DEBUG(p) & 2)) __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      const int i1 = i0 + KC;
      const bool more = i1 < i_end && !(MC_DEBUG(p) & 1);
      // the next chunk's pieces: spread over this chunk's MFMA stages (each DMA issue then hides behind a matrix
      // instruction of the same wave), or all at once for a chunk the DMA cannot serve / with debug bit 2
      const bool spread = more && dma_ok(i1) && !(MC_DEBUG(p) & 4);
      if (more && !spread) stage(i1, buf ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      Wc = smem + buf * bstride;
      Xc = Wc + WSZ;
      Sc = Xc + p.lds_patch_floats;
      contract([&](int st) {
        if (spread) {
#pragma unroll
          for (int q = 0; q < PER_STAGE; ++q)
            if (st * PER_STAGE + q < NPC) dma_piece(st * PER_STAGE + q, i1, buf ^ 1);
        }
      }, std::false_type{});
    }
  }

  if (MC_CLOCK(p)) clk2 = __builtin_readcyclecounter();
  if (MC_FLAGS(p) & 1) __builtin_amdgcn_s_setprio(3);
  // ---- epilogue.  All loads first (bias, demod, noise: clamped indices, no branches — a load inside a divergent
  // `if` costs one full memory round trip per element, 64 of them in a row per thread), then arithmetic on the
  // accumulators in place, then predicated stores.
  const bool partial = p.ksplit > 1;
  const bool actf = MODE == 0 && p.fuse_act && !partial;
  const bool use_demod = p.demod != nullptr && !partial;
  const float nw = (actf && p.noise && p.noise_weight) ? p.noise_weight[0] : 0.f;
  float* dstbase = partial ? p.ws + (long long)ks * p.batch * p.cout * p.oh * p.ow : p.out;
  const long long dps = partial ? (long long)p.oh * p.ow : p.out_plane_stride;
  const int drs = partial ? p.ow : p.out_row_stride;
  const int orow = o0 + wm * 32 * RM + 4 * khalf;     // this lane's first output channel; row r adds (r&3) + 8*(r>>2)
  // per position group: validity, destination, noise term (loaded up front, clamped indices)
  bool vgs[RNP]; float nzs[RNP];
#pragma unroll
  for (int g = 0; g < RNP; ++g) {
    const int b = pos_b[g], bc = min(b, p.batch - 1);
    if constexpr (MODE != 1) {
      const int y = pos_y[g], x = pos_x[g];
      vgs[g] = b < p.batch && y < p.oh && x < p.ow;
      const int pix = vgs[g] ? y * p.ow + x : 0;
      nzs[g] = (actf && p.noise) ? __fmul_rn(nw, p.noise[(long long)(p.noise_batch == 1 ? 0 : bc) * p.oh * p.ow + pix]) : 0.f;
    } else {
      vgs[g] = b < p.batch && pos_y[g] < seg_m_end && pos_x[g] < seg_n_end;
      nzs[g] = 0.f;
    }
  }
  // destination of a position group's first channel (generic store path)
  auto dpos_of = [&](int g) -> float* {
    const int bc = min(pos_b[g], p.batch - 1);
    const int sc = MODE == 1 ? 2 : 1;
    return dstbase + (long long)bc * p.cout * dps + (long long)(vgs[g] ? sc * pos_y[g] : 0) * drs + (vgs[g] ? sc * pos_x[g] : 0);
  };
  // Buffer stores (every tile whose channels all exist and whose samples' output slabs fit 32-bit offsets — every layer of
  // the model): per-lane byte offset fixed per position group (parked for positions outside the grid: the range check
  // drops the store), channel / phase row as a scalar offset.  One SALU op + one store per value instead of a 64-bit
  // multiply-add chain and an exec-mask branch (the generic form below costs ~25 instructions per value).
  const long long slab = (long long)p.cout * dps * 4;                         // bytes of one sample's output
  bool bstore = dstbase != nullptr && o0 + BM <= p.cout && (long long)seg_nb * slab < 0xFFFFFFF0LL;
  if constexpr (MODE == 1) bstore = bstore && 2 * seg_m_end <= p.oh && 2 * seg_n_end <= p.ow;   // every quad complete
  unsigned vofs[RNP];
  const float* obase = dstbase ? uniform_ptr(dstbase + (long long)b0 * p.cout * dps) : nullptr;
  const auto rsrc_o = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(obase), 0,
      uniform_u32(bstore ? (unsigned)((long long)min(seg_nb, p.batch - b0) * slab) : 0u), 0x00020000);
#pragma unroll
  for (int g = 0; g < RNP; ++g) {
    const long long e = (long long)(pos_b[g] - b0) * p.cout * dps + (long long)(4 * khalf) * dps +
                        (long long)(MODE == 1 ? 2 * pos_y[g] : pos_y[g]) * drs + (MODE == 1 ? 2 * pos_x[g] : pos_x[g]);
    vofs[g] = (bstore && vgs[g]) ? (unsigned)(e * 4) : 0xFFFFFFF0u;
  }
  // activation constants pinned in SGPRs (left to the compiler they are re-read from the kernel arguments, with a wait,
  // for every value)
  unsigned alpha_bits = __float_as_uint(p.alpha), ascale_bits = __float_as_uint(p.act_scale);
  asm volatile("" : "+s"(alpha_bits), "+s"(ascale_bits));
  const float alpha = __uint_as_float(alpha_bits), ascale = __uint_as_float(ascale_bits);
  const unsigned dps4 = uniform_u32((unsigned)(dps * 4)), drs4 = uniform_u32((unsigned)drs * 4u);   // used by bstore only
  if (MC_CLOCK(p)) clke = __builtin_readcyclecounter();
  // One 32-channel row group at a time: its bias / demodulation values are loaded together (16 + 16 registers live
  // beside the accumulators instead of 32 * RM + 32 * RM: what lets the 128 x 128 tile fit three blocks per CU).
  auto rows = [&](auto act_c, auto bst_c) {
    constexpr bool ACT = decltype(act_c)::value, BST = decltype(bst_c)::value;
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      float bias_m[16], dm_m[16];
      if (epi_lds) {
        const float* eb = Es + (orow - o0) + m * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          bias_m[r] = ACT ? eb[(r & 3) + 8 * (r >> 2)] : 0.f;
          dm_m[r] = eb[BM + (r & 3) + 8 * (r >> 2)];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int oc = min(orow + m * 32 + (r & 3) + 8 * (r >> 2), p.cout - 1);
          bias_m[r] = (ACT && p.bias) ? p.bias[oc] : 0.f;
          dm_m[r] = 1.f;
        }
      }
      const unsigned so_m = (unsigned)(o0 + wm * 32 * RM + m * 32) * dps4;     // scalar: first channel of the row group
#pragma unroll
      for (int g = 0; g < RNP; ++g) {
        const int bc = min(pos_b[g], p.batch - 1);
        if (!epi_lds && use_demod && (g == 0 || seg_nb > 1)) {        // tiles of one sample (every large layer) load demod once
#pragma unroll
          for (int r = 0; r < 16; ++r)
            dm_m[r] = p.demod[(long long)bc * p.cout + min(orow + m * 32 + (r & 3) + 8 * (r >> 2), p.cout - 1)];
        }
        const bool vg = vgs[g];
        float* dpos = BST ? nullptr : dpos_of(g);
        if (MC_CLOCK(p) && m == 0 && g == 0) {          // every load of the epilogue has landed (stamps only)
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_waitcnt(0);
          clkl = __builtin_readcyclecounter();
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (MODE != 1) {
          const float nz = nzs[g];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int o = orow + m * 32 + (r & 3) + 8 * (r >> 2);
            float v = acc[m][g][0][r] * dm_m[r];
            if constexpr (ACT) {
              v = __fadd_rn(__fadd_rn(v, nz), bias_m[r]);
              v = (v > 0.f ? v : v * alpha) * ascale;
            }
            if constexpr (BST) {
              if constexpr (RGB) acc[m][g][0][r] = vg ? v : 0.f;
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc_o, vofs[g], so_m + (unsigned)((r & 3) + 8 * (r >> 2)) * dps4, 0);
            } else {
              if constexpr (RGB) acc[m][g][0][r] = (vg && o < p.cout) ? v : 0.f;
              if ((!RGB || dstbase) && vg && o < p.cout) dpos[(long long)o * dps] = v;
            }
          }
        } else {
          const int X = 2 * pos_x[g], Y0 = 2 * pos_y[g];
          const bool pair = X + 1 < p.ow;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int o = orow + m * 32 + (r & 3) + 8 * (r >> 2);
            if constexpr (BST) {
#pragma unroll
              for (int py = 0; py < 2; ++py) {
                u32x2 t;
                t.x = __float_as_uint(acc[m][g][py * 2][r] * dm_m[r]);
                t.y = __float_as_uint(acc[m][g][py * 2 + 1][r] * dm_m[r]);
                __builtin_amdgcn_raw_buffer_store_b64(t, rsrc_o, vofs[g], so_m + (unsigned)((r & 3) + 8 * (r >> 2)) * dps4 + (unsigned)py * drs4, 0);
              }
            } else {
              if (!(vg && o < p.cout)) continue;
              float* dst = dpos + (long long)o * dps;
#pragma unroll
              for (int py = 0; py < 2; ++py) {
                if (Y0 + py >= p.oh) continue;
                const float v0 = acc[m][g][py * 2][r] * dm_m[r], v1 = acc[m][g][py * 2 + 1][r] * dm_m[r];
                if (pair) {
                  f32x2_u t; t.x = v0; t.y = v1;
                  *reinterpret_cast<f32x2_u*>(dst + (long long)py * drs) = t;
                } else {
                  dst[(long long)py * drs] = v0;
                }
              }
            }
          }
        }
      }
    }
  };
  if (bstore) {
    if (actf) rows(std::true_type{}, std::true_type{}); else rows(std::false_type{}, std::true_type{});
  } else {
    if (actf) rows(std::true_type{}, std::false_type{}); else rows(std::false_type{}, std::false_type{});
  }
  if (MC_CLOCK(p) && tid == 0 && (blockIdx.x & 63) == 0) {
    const unsigned long long clk3 = __builtin_readcyclecounter();
    atomicAdd(p.dbg_clock, clk3 - clk0);
    atomicAdd(p.dbg_clock + 1, wall_clock64() - rt0);
    atomicAdd(p.dbg_clock + 2, clk1 - clk0);       // set-up (tile decode, staging plan)
    atomicAdd(p.dbg_clock + 3, clk2 - clk1);       // first chunk's wait + K loop
    atomicAdd(p.dbg_clock + 4, clk3 - clk2);       // epilogue up to the last store's issue
    atomicAdd(p.dbg_clock + 5, 1ULL);
    atomicAdd(p.dbg_clock + 8, clkl - clke);       // of the epilogue: waiting for bias / demod / noise
    __builtin_amdgcn_s_waitcnt(0);
    atomicAdd(p.dbg_clock + 9, __builtin_readcyclecounter() - clk3);   // after the last store's issue: until all are acknowledged
    atomicAdd(p.dbg_clock + 7, clke - clk2);       // of the epilogue: destinations, validity, noise loads issued
    atomicAdd(p.dbg_clock + 6, clkw);               // of the K loop: waiting for the chunk's DMA + barrier (lean loop)
  }
  if constexpr (RGB) {
    // second pass over the activated values (now in the accumulators): rgb = sum over rows of act * wmod, where
    // wmod[b,c,o] = rgb_scale * W[c,o] * rgb_style[b,o]; rows of one position live in both lane halves (khalf) and,
    // with WM = 2, in two waves: fixed-order reduction.
    float rs[RNP][3];
#pragma unroll
    for (int g = 0; g < RNP; ++g) rs[g][0] = rs[g][1] = rs[g][2] = 0.f;
    // (the host only fuses layers whose tiles hold one sample: b0 is the sample of every position of this block)
    const float* wmod = p.rgb_wmod + (long long)min(b0, p.batch - 1) * 3 * p.cout;
#pragma unroll
    for (int m = 0; m < RM; ++m) {
      float rw[3][16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int oc = min(orow + m * 32 + (r & 3) + 8 * (r >> 2), p.cout - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) rw[c][r] = wmod[c * p.cout + oc];
      }
#pragma unroll
      for (int g = 0; g < RNP; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) rs[g][c] = fmaf(acc[m][g][0][r], rw[c][r], rs[g][c]);
    }
#pragma unroll
    for (int g = 0; g < RNP; ++g)
#pragma unroll
      for (int c = 0; c < 3; ++c) rs[g][c] += __shfl_xor(rs[g][c], 32, 64);
    if constexpr (WM > 1) {
      static_assert(WM == 2, "two output-channel waves at most");
      __syncthreads();            // every wave is done with the last chunk's LDS operands
      float* red = smem + ((wn * RNP) * 3) * 32;
      if (wm == 1 && khalf == 0)
#pragma unroll
        for (int g = 0; g < RNP; ++g)
#pragma unroll
          for (int c = 0; c < 3; ++c) red[(g * 3 + c) * 32 + l31] = rs[g][c];
      __syncthreads();
      if (wm == 0 && khalf == 0)
#pragma unroll
        for (int g = 0; g < RNP; ++g)
#pragma unroll
          for (int c = 0; c < 3; ++c) rs[g][c] += red[(g * 3 + c) * 32 + l31];
    }
    if (wm == 0 && khalf == 0) {
#pragma unroll
      for (int g = 0; g < RNP; ++g) {
        const int b = pos_b[g], y = pos_y[g], x = pos_x[g];
        if (b >= p.batch || y >= p.oh || x >= p.ow) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c >= p.rgb_c) continue;
          const long long off = (((long long)b * p.rgb_c + c) * p.oh + y) * p.ow + x;
          float v = rs[g][c];
          if (p.rgb_bias) v = __fadd_rn(v, p.rgb_bias[c]);
          if (p.rgb_skip) v = __fadd_rn(v, p.rgb_skip[off]);
          p.rgb_out[off] = v;
        }
      }
    }
  }
}

// split-K finish: out = epilogue(sum_ks ws[ks])
__global__ __launch_bounds__(256) void modconv_splitk_finish_f32(const MCParams p) {
  const float nw = (p.fuse_act && p.noise && p.noise_weight) ? p.noise_weight[0] : 0.f;
  const int hw = p.oh * p.ow;
  const long long total = (long long)p.batch * p.cout * hw;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int ks = 0; ks < p.ksplit; ++ks) v += p.ws[ks * total + idx];
    const int pix = (int)(idx % hw);
    const long long bo = idx / hw;
    p.out[bo * p.out_plane_stride + (long long)(pix / p.ow) * p.out_row_stride + pix % p.ow] =
        mc_epilogue(v, p, nw, (int)(bo / p.cout), (int)(bo % p.cout), pix);
  }
}

// Tile width.  Thin column segments of small images use 1- or 2-wide tiles (fewer, fuller blocks: 220 vs 284 us on the
// 16^2 -> 32^2 layer); on large images the taller patch would overflow the prefetch slots and fall to the
// synchronous staging path (+15 %), so they keep 4-wide tiles.
inline int pick_tw_log2(int gw, int gh) {
  if (gh <= 32 && gw <= 2) return gw <= 1 ? 0 : 1;
  return gw <= 4 ? 2 : (gw <= 8 ? 3 : (gw <= 16 ? 4 : 5));
}

// experiments build: FMGAN_MC_WIDE=0 keeps the 4-byte patch pieces (A/B measurements); product: always on
inline bool mc_wide_patch() {
#ifdef FMGAN_EXPERIMENTS
  const char* e = getenv("FMGAN_MC_WIDE");
  return !(e && e[0] == '0');
#else
  return true;
#endif
}

// tile plan of one segment; returns its block count (without the o_tiles factor) and LDS floats for the patch
inline long long plan_segment(MCParams::Seg& sg, int batch, int BN) {
  sg.tw_log2 = pick_tw_log2(sg.gw, sg.gh);
  const int TW = 1 << sg.tw_log2;
  const int rows_total = BN / TW;
  int th = rows_total, nb = 1;
  if (sg.gh < rows_total) {
    th = 1;
    while (th < sg.gh) th <<= 1;
    nb = rows_total / th;
  }
  sg.th = th; sg.nb = nb;
  sg.tiles_x = (sg.gw + TW - 1) / TW;
  sg.tiles_y = (sg.gh + th - 1) / th;
  sg.tiles_b = (batch + nb - 1) / nb;
  return (long long)sg.tiles_x * sg.tiles_y * sg.tiles_b;
}

constexpr size_t MC_LDS_LIMIT = 64 * 1024;   // dynamic LDS a launch may ask for without a function attribute
constexpr size_t MC_LDS_MAX = 160 * 1024;    // LDS of a CU

// What a planning call (fmgan_modconv2d_select) gets back in place of a launch: the tile that would have run.
struct MCPick {
  int cfg; char variant; int bm, bn, ksplit;
};

// Returns FMGAN_OK, an error, or +1 when this variant cannot serve the shape (PIPE 1 with an LDS image over the limit):
// the caller then launches the register-pipeline variant.
// FUSES_RGB: the tile's kernel with the ToRGB epilogue is built too, for launches with p.rgb_out.
// plan_only: every decision of the launch, no HIP call — returns what the launch would return just before it launches.
template <class Tile, bool FUSES_RGB>
int launch_tile(MCParams& p, hipStream_t s, bool plan_only) {
  constexpr int MODE = Tile::MODE, MINB = Tile::MINB, KC = Tile::KC, PIPE = Tile::PIPE, BM = Tile::BM, BN = Tile::BN;
  static_assert(!FUSES_RGB || MODE == 0, "the RGB epilogue belongs to the plain conv");
  if constexpr (!FUSES_RGB) { if (p.rgb_out) return FMGAN_EUNSUPPORTED; }
  constexpr int SP = MODE == 2 ? 2 : 1;
  p.o_tiles = (p.cout + BM - 1) / BM;
  long long blocks = 0;
  size_t patch = 0, nbmax = 1;
  // LDS floats of a segment's halo patch (wide patch: rows of whole, aligned 16-byte groups — see the kernel)
  auto patch_floats = [&](const MCParams::Seg& sg) {
    size_t f = (size_t)sg.nb * KC * (SP * (sg.th - 1) + 3) * (sg.wide ? (1 << sg.tw_log2) + 8 : SP * ((1 << sg.tw_log2) - 1) + 3);
    return sg.wide ? (f + 255) / 256 * 256 : f;             // whole 64-lane x 16-byte pieces
  };
  long long seg_blocks[3] = {0, 0, 0};
  int main_seg = 0;
  for (int i = 0; i < p.nseg; ++i) {
    seg_blocks[i] = plan_segment(p.seg[i], p.batch, BN);
    if (seg_blocks[i] > seg_blocks[main_seg]) main_seg = i;
    p.seg[i].wide = PIPE == 1 && SP == 1 && p.seg[i].tw_log2 == 5 && (p.seg[i].n_off & 3) == 0 && (p.w & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(p.in) & 15) == 0 && mc_wide_patch();
  }
  // The LDS image is sized by the largest patch of the launch and decides how many blocks a CU holds.  The thin segments of
  // the transposed conv (one row / one column of quads) pack samples or rows into their tiles and used to need twice the
  // main segment's patch — one block per CU less for the whole layer.  They now take smaller tiles (fewer samples, then
  // fewer rows, per tile: part of the tile's positions stay empty) until their patch fits the main segment's.
  // (Only for launches of several rounds of blocks: there the thin segments are < 1 % of the blocks.  A small layer runs in
  // one round, and four times as many mostly-empty strip blocks with full-length K loops cost it 25 %: 8^2, 16^2 at B = 8.)
  const size_t main_patch = patch_floats(p.seg[main_seg]);
  const bool cap_strips = seg_blocks[main_seg] * p.o_tiles >= 4LL * FMGAN_NUM_CU;
  for (int i = 0; i < p.nseg; ++i) {
    MCParams::Seg& sg = p.seg[i];
    while (cap_strips && i != main_seg && patch_floats(sg) > main_patch && (sg.nb > 1 || sg.th > 1)) {
      if (sg.nb > 1) sg.nb >>= 1; else sg.th >>= 1;
      sg.tiles_y = (sg.gh + sg.th - 1) / sg.th;
      sg.tiles_b = (p.batch + sg.nb - 1) / sg.nb;
      seg_blocks[i] = (long long)sg.tiles_x * sg.tiles_y * sg.tiles_b;
    }
    blocks += seg_blocks[i] * p.o_tiles;
    if (blocks > 0x7fffffffLL) return FMGAN_EOVERFLOW;
    sg.block_end = (unsigned)blocks;
    // 32-bit in-tile element offsets: (samples of a tile that exist) x cin x h x w must fit.  (Slots of a tile's
    // samples beyond the batch are never addressed: their offsets are parked / their loads masked.)
    const int nb_live = sg.nb < p.batch ? sg.nb : p.batch;
    if ((long long)nb_live * p.cin * p.h * p.w >= (1LL << 31)) return FMGAN_EOVERFLOW;
    const size_t f = patch_floats(sg);
    if (f > patch) patch = f;
    if ((size_t)sg.nb > nbmax) nbmax = sg.nb;
  }
  size_t lds = sizeof(float) * ((size_t)KC * 9 * BM + patch);
  if constexpr (PIPE == 1) {
    if (p.cin_per_split % KC != 0) return 1;
    p.lds_patch_floats = (int)((patch + 63) / 64 * 64);
    p.lds_buf_floats = (KC * 9 * BM + 255) / 256 * 256 + p.lds_patch_floats + (int)((nbmax * KC + 63) / 64 * 64);
    // + this tile's bias and demodulation values + (tiles of one sample, <= 512 input channels) its style slice, staged once
    p.lds_style_floats = (nbmax == 1 && p.cin_per_split <= 512) ? p.cin_per_split : 0;
    lds = sizeof(float) * (2 * (size_t)p.lds_buf_floats + 2 * BM + p.lds_style_floats);
    if (lds > (MINB == 1 ? MC_LDS_MAX : MC_LDS_LIMIT)) return 1;
    if (lds > MC_LDS_LIMIT && !plan_only) {
      // one block per CU may use more than the 64 KB a launch gets by default (160 KB per CU on gfx950)
      static bool raised = false;
      if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&modconv_mfma_f32<Tile, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)MC_LDS_MAX) != hipSuccess) {
          (void)hipGetLastError();
          return 1;
        }
        raised = true;
      }
    }
  }
  if constexpr (FUSES_RGB) {
    if (p.rgb_out) {
      if (p.o_tiles != 1 || p.ksplit != 1) return FMGAN_EUNSUPPORTED;
      // The RGB epilogue reads ONE sample's wmod per block.  rgb_fusable() vouches for that on the 128-position planning
      // model; a 256-position tile packs two samples of a 4-row image (TW = 32; 8 rows at TW = 16, ...) into one tile
      // where the 128-position tile holds one: such a launch goes to the register tile instead.
      if (nbmax > 1) return PIPE == 1 ? 1 : FMGAN_EUNSUPPORTED;
      if (plan_only) return FMGAN_OK;
      hipLaunchKernelGGL((modconv_mfma_f32<Tile, true>), dim3((unsigned)blocks, 1), dim3(256), lds, s, p);
      return fmgan_check_launch();
    }
  }
  if (plan_only) return FMGAN_OK;
  hipLaunchKernelGGL((modconv_mfma_f32<Tile, false>), dim3((unsigned)blocks, p.ksplit), dim3(256), lds, s, p);
  return fmgan_check_launch();
}

// ---- the tile table: every tile a (mode, cfg) can run on, by variant letter.  'A' = register prefetch (serves every
// shape: the fall-back of the others), 'B'..'E' = LDS-DMA variants.  The FIRST entry of a (mode, cfg) is its default, the
// measured winner (profiles/r02_modconv_variants.md).  The product build holds the defaults and what launch_any can turn them
// into; the experiments build (make experiments: -DFMGAN_EXPERIMENTS, tools/exp/lib/libfmgan_hip_exp.so) adds the other
// measured tiles, the fused-ToRGB kernels of the tiles a fused launch only reaches through a variant switch, and alone reads
// FMGAN_MC_V<mode><cfg>=A..E, FMGAN_MC_DEBUG and FMGAN_MC_CLOCKPTR; the product library has no environment switch, no
// ablation code path and no kernel it cannot launch.
// measured on MI355X (profiles/r02_modconv_variants.md): plain conv, Cout >= 96: 128 x 256 tile by LDS-DMA (C);
// Cout >= 48: 64 x 256 in 4-channel chunks, three blocks per CU (C; 1470 -> 1390 us at 512^2 against 8-channel chunks
// at two blocks per CU, possible since the scalar wave index freed ~25 VGPRs); Cout < 48: 32 x 256, three blocks per CU
// (C: 1701 us at 1024^2; 32 x 128 by LDS-DMA 1809, register pipeline 1760-1790, 32 x 512 1873);
// transposed conv: LDS-DMA (B) for every width.
// Round 3 (profiles/r03_modconv_block_phases.md, r03_modconv_layers_ab.md), after the wide patch and the buffer-store
// epilogue: Cout < 48 plain: 32 x 256 in 4-channel chunks (24 KB of LDS): E = in a 128-register budget, 4 blocks per
// CU instead of 3, no spills (1446 -> 1361 us at 1024^2, with the fused ToRGB 1852 -> 1796-1800); D = in a 96-register
// budget, 5 blocks per CU, 55-90 spilled dwords: 1 % behind E (1377 / 1806-1826).  Transposed 32-channel tile in a
// 128-register budget (D: 4 blocks per CU instead of 3, 7 spilled dwords in the epilogue; 785 -> 757 us at 512^2).
struct TileEntry {
  int mode, cfg;           // cfg: pick_cfg's output-channel class, 0 = 128, 1 = 64, 2 = 32 channels per block
  char variant;
  int BM, BN;              // output channels x positions of the launched block
  bool fuses_rgb;          // takes launches with the ToRGB epilogue (p.rgb_out)
  int (*launch)(MCParams&, hipStream_t, bool plan_only);
};
template <class Tile, bool FUSES_RGB = false>
constexpr TileEntry tile_entry(int cfg, char variant) {
  return {Tile::MODE, cfg, variant, Tile::BM, Tile::BN, FUSES_RGB, &launch_tile<Tile, FUSES_RGB>};
}
#ifdef FMGAN_EXPERIMENTS
constexpr bool MC_EXP = true;
#else
constexpr bool MC_EXP = false;
#endif
constexpr TileEntry MC_TILES[] = {
    // plain conv.  (A fused-ToRGB launch on the 128- and 64-channel classes never takes 'C' and takes 'B' only when
    // FMGAN_MC_V0<cfg> asks for it: launch_any.)
    tile_entry<Plain128x256DmaKc4>(0, 'C'),
    tile_entry<Plain128x128DmaKc4, MC_EXP>(0, 'B'),
    tile_entry<Plain128x128Reg, true>(0, 'A'),
    tile_entry<Plain64x256DmaKc4>(1, 'C'),
    tile_entry<Plain64x128Dma, MC_EXP>(1, 'B'),
    tile_entry<Plain64x128Reg, true>(1, 'A'),
    tile_entry<Plain32x256DmaKc4R128, true>(2, 'E'),
    tile_entry<Plain32x128Dma, true>(2, 'B'),
    tile_entry<Plain32x128Reg, true>(2, 'A'),
#ifdef FMGAN_EXPERIMENTS
    tile_entry<Plain32x256Dma, true>(2, 'C'),
    tile_entry<Plain32x256DmaKc4R96, true>(2, 'D'),
#endif
    // transposed conv (pick_cfg has no 128-channel class for it)
    tile_entry<Transposed64x128Dma>(1, 'B'),
    tile_entry<Transposed64x128Reg>(1, 'A'),
    tile_entry<Transposed32x128DmaR128>(2, 'D'),
    tile_entry<Transposed32x128Reg>(2, 'A'),
#ifdef FMGAN_EXPERIMENTS
    tile_entry<Transposed32x256Dma>(1, 'C'),
    tile_entry<Transposed32x128DmaR170>(2, 'B'),
    tile_entry<Transposed32x256Dma>(2, 'C'),
#endif
    // stride-2 conv
    tile_entry<Stride2x128x128Reg>(0, 'A'),
    tile_entry<Stride2x64x128Reg>(1, 'A'),
    tile_entry<Stride2x32x128Reg>(2, 'A'),
};

// null: this (mode, cfg) has no tile for the letter
inline const TileEntry* find_tile(int mode, int cfg, char variant) {
  for (const TileEntry& e : MC_TILES)
    if (e.mode == mode && e.cfg == cfg && e.variant == variant) return &e;
  return nullptr;
}

inline char mc_variant(int mode, int cfg) {
  char v = 'A';
  for (const TileEntry& e : MC_TILES)
    if (e.mode == mode && e.cfg == cfg) { v = e.variant; break; }
#ifdef FMGAN_EXPERIMENTS
  // (read per call: the A/B tools sweep variants inside one process)
  char name[32];
  snprintf(name, sizeof(name), "FMGAN_MC_V%d%d", mode, cfg);
  const char* e = getenv(name);
  if (e && e[0] >= 'A' && e[0] <= 'E') v = e[0];
#endif
  return v;
}

// Tile configurations (output channels x positions per block; blocks per CU the register budget allows):
//   mode 0: 0 = 128 x 128 (2 per CU), 1 = 64 x 128 (3 per CU), 2 = 32 x 128 (4 per CU)
//   mode 2: 0 = 128 x 128, 1 = 64 x 128, 2 = 32 x 128
//   mode 1: 1 = 64 x 128 (2 per CU; 4 phases = 128 accumulator registers), 2 = 32 x 128 (3 per CU)
// For Cout < 96 larger position tiles (64 x 256, 32 x 512; mode 1: 32 x 256) were the first design: fewer weight
// re-reads per MFMA, but 245-256 VGPRs and only two blocks per CU.  On these short-K layers (4-16 chunks per block) more
// co-resident blocks hide the prologue/epilogue better: 1024^2 plain 1681 -> 1597 us, 1024^2 transposed 980 -> 894 us,
// 512^2 plain 1440 -> 1403 us (B=8).  The same trade for Cout >= 96 loses (64 x 128 x 3: 1283 vs 1233 us at 64^2), and
// 32 x 128 tiles for the transposed conv at Cout >= 48 are a wash (+-3 %, sign depends on batch), so those stay.
inline int pick_cfg(int mode, int cout, long long positions) {
  if (mode == 0) {
    if (positions <= 2048) return 2;          // tiny layers: many small tiles (+ split-K)
    return cout >= 96 ? 0 : (cout >= 48 ? 1 : 2);
  }
  if (mode == 2) return cout >= 96 ? 0 : (cout >= 48 ? 1 : 2);   // stride-2 patches are 4x larger: 128 positions only
  // transposed conv: the 32-channel tile (three blocks per CU) also serves the widest layers once they are large
  // enough (Cout 256-512 at 32^2-64^2, B=8: 518 -> 501 and 850 -> 808 us); a tie at Cout 64-128, slower below 4096 positions
  if (cout >= 192 && positions >= 4096) return 2;
  return cout >= 48 ? 1 : 2;
}

// The PLANNING MODEL of a cfg — what pick_ksplit, count_blocks and rgb_fusable reckon with: 128 positions per block for
// every cfg and 2 / 3 / 4 co-resident blocks per CU.  Not the launched tile (MC_TILES): the 256-position tiles and the
// transposed 32-channel default (4 blocks per CU, modelled as 3) differ from it.  Split-K factors and workspace sizes
// follow from these values, so they stay as they are when a tile changes.
inline void model_tile_dims(int mode, int cfg, int& BM, int& BN) {
  (void)mode;
  const int bm[3] = {128, 64, 32};
  BM = bm[cfg]; BN = 128;
}

inline int model_blocks_per_cu(int mode, int cfg) {
  if (mode == 1) return cfg == 2 ? 3 : 2;
  return cfg == 0 ? 2 : (cfg == 1 ? (mode == 0 ? 3 : 2) : 4);
}

// blocks a (BM x BN) tiling of this launch would have (all segments)
inline long long blocks_with(const MCParams& p, int BM, int BN) {
  long long blocks = 0;
  for (int i = 0; i < p.nseg; ++i) {
    MCParams::Seg sg = p.seg[i];
    blocks += plan_segment(sg, p.batch, BN);
  }
  return blocks * ((p.cout + BM - 1) / BM);
}

// pick: null = launch; otherwise plan only (no HIP call) and report the tile the launch would have run
inline int launch_any(int mode, int cfg, MCParams& p, hipStream_t s, MCPick* pick = nullptr) {
  char v = mc_variant(mode, cfg);
  // the large-tile variants need enough tiles to fill the chip twice over (2 blocks per CU); smaller launches keep
  // the 128-position tiles (and their split-K plan)
  // (mid-size launches — 16^2 .. 32^2 at B=8 — then take the LDS-DMA pipeline on the 128-position tile: 119 vs 126 us
  // and 380 vs 396 us; below ~1500 positions the register pipeline is as fast or faster)
  const TileEntry* e = nullptr;
  if (mode == 0 && v == 'C' && (e = find_tile(0, cfg, 'C')) != nullptr) {
    const bool small = p.ksplit > 1 || blocks_with(p, e->BM, e->BN) < 2LL * FMGAN_NUM_CU;
    if (cfg < 2 && (small || p.rgb_out)) v = (!p.rgb_out && (long long)p.batch * p.h * p.w >= 1536) ? 'B' : 'A';
    else if (cfg == 2 && small) v = 'B';
  }
  // ('D' and 'E' are tiles of the 32-channel class; the rule measures with their size whatever the cfg)
  if (mode == 0 && (v == 'D' || v == 'E') && (e = find_tile(0, 2, v)) != nullptr) {
    const bool small = p.ksplit > 1 || blocks_with(p, e->BM, e->BN) < 2LL * FMGAN_NUM_CU;
    if (small) v = 'B';
  }
  int st = 1;
  if (v != 'A' && (e = find_tile(mode, cfg, v)) != nullptr) st = e->launch(p, s, pick != nullptr);
  if (st == 1) {
    e = find_tile(mode, cfg, 'A');                      // the register pipeline serves what the LDS-DMA tile could not
    st = e ? e->launch(p, s, pick != nullptr) : FMGAN_EUNSUPPORTED;
  }
  if (pick && st == FMGAN_OK) *pick = {cfg, e->variant, e->BM, e->BN, p.ksplit};
  return st;
}

// Blocks of one launch (all segments), for a given tile configuration.
inline void out_dims(int mode, int h, int w, int& oh, int& ow) {
  if (mode == 1) { oh = 2 * h + 1; ow = 2 * w + 1; }
  else if (mode == 2) { oh = (h - 3) / 2 + 1; ow = (w - 3) / 2 + 1; }
  else { oh = h; ow = w; }
}

inline long long count_blocks(int mode, int cfg, int batch, int cout, int h, int w) {
  int BM, BN;
  model_tile_dims(mode, cfg, BM, BN);
  if (mode == 2) out_dims(2, h, w, h, w);   // positions = outputs
  MCParams::Seg sg[3] = {{0, 0, h, w}, {h, 0, 1, w + 1}, {0, w, h, 1}};   // any order: only the sum matters
  long long blocks = 0;
  for (int i = 0; i < (mode == 1 ? 3 : 1); ++i) blocks += plan_segment(sg[i], batch, BN);
  return blocks * ((cout + BM - 1) / BM);
}

// Split-K factor.  A launch runs in rounds of `slots` co-resident blocks; 608 equal blocks on 512 slots take two
// rounds, i.e. 1.7x their ideal time.  Splitting the input-channel loop ks ways makes the blocks ks times shorter
// (plus a fixed prologue/epilogue per block and a finish pass over ks partial slabs).  Pick the ks that minimises
// the modelled time; layers with many rounds keep ks = 1.
inline int pick_ksplit(int mode, int batch, int cin, int cout, int h, int w) {
  int poh, pow_;
  out_dims(mode == 2 ? 2 : 0, h, w, poh, pow_);   // position grid (mode 1: the input grid)
  const int cfg = pick_cfg(mode, cout, (long long)batch * poh * pow_);
  const long long blocks = count_blocks(mode, cfg, batch, cout, h, w);
  const int chunks = (cin + MC_KC - 1) / MC_KC;
  const int slots = FMGAN_NUM_CU * model_blocks_per_cu(mode, cfg);   // co-resident blocks (VGPR-limited)
  if (blocks >= 4LL * slots || chunks < 4) return 1;
  int BM, BN;
  model_tile_dims(mode, cfg, BM, BN);
  // time unit: one chunk of one block.  Finish pass: (2*ks + 1) * out_bytes at ~4 TB/s against ~5 us per full-size chunk
  const double mfma_per_chunk = (double)(BM / 32) * (BN / 32) * (mode == 1 ? 9 : 9) * (MC_KC / 2) / 4.0;  // per wave
  const double t_chunk_us = mfma_per_chunk * 64.0 / 2360.0 * 2.0;       // two blocks share each SIMD
  int ooh, oow;
  out_dims(mode, h, w, ooh, oow);
  const double out_mb = (double)batch * cout * ooh * (double)oow * 4e-6;
  int best = 1;
  double best_t = 1e30;
  for (int ks = 1; ks <= 16 && ks <= chunks / 2; ++ks) {
    const long long rounds = (blocks * ks + slots - 1) / slots;
    double t = (double)rounds * ((double)((chunks + ks - 1) / ks) + 2.0) * t_chunk_us;
    if (ks > 1) t += (2.0 * ks + 1.0) * out_mb / 4.0 + 3.0;   // MB / (4 MB per us) + launch
    if (t < best_t * 0.97) { best_t = t; best = ks; }
  }
  return best;
}

}  // namespace

extern "C" long long fmgan_modconv2d_workspace_bytes(int batch, int cin, int cout, int h, int w, int mode) {
  if (batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || mode < 0 || mode > 2) return 0;
  if (mode == 2 && (h < 3 || w < 3)) return 0;
  const int ks = pick_ksplit(mode, batch, cin, cout, h, w);
  if (ks <= 1) return 0;
  int oh, ow;
  out_dims(mode, h, w, oh, ow);
  return (long long)ks * batch * cout * oh * ow * (long long)sizeof(float);
}

namespace {
struct RgbArgs {
  const float* wmod; const float* bias; const float* skip; float* out; int c;
};

bool rgb_fusable(int batch, int cin, int cout, int h, int w) {
  const int cfg = pick_cfg(0, cout, (long long)batch * h * w);
  int BM, BN;
  model_tile_dims(0, cfg, BM, BN);
  (void)cin;
  MCParams::Seg sg{0, 0, h, w};
  plan_segment(sg, batch, BN);
  // one output-channel tile, tiles of a single sample; the fused launch runs without split-K
  return cout <= BM && sg.nb == 1;
}

int modconv2d_impl(const float* in, const float* wt, const float* style, const float* demod,
                   float* out, int batch, int cin, int cout, int h, int w, int mode,
                   const float* noise, const float* noise_weight, const float* bias, int noise_batch,
                   int fuse_act, float alpha, float act_scale, long long out_plane_stride,
                   int out_row_stride, void* workspace, long long workspace_bytes, void* stream, const RgbArgs* rgb,
                   MCPick* pick = nullptr) {
  if (batch < 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return FMGAN_EINVAL;
  if (mode < 0 || mode > 2) return FMGAN_EUNSUPPORTED;
  if (mode != 0 && fuse_act) return FMGAN_EUNSUPPORTED;  // the blur sits between conv and activation
  if (mode == 2 && (h < 3 || w < 3)) return FMGAN_EINVAL;
  if (rgb) {
    if (rgb->c < 1 || rgb->c > 3) return FMGAN_EUNSUPPORTED;
    if (!rgb_fusable(batch, cin, cout, h, w)) return FMGAN_EUNSUPPORTED;
  }
  if (batch == 0) return FMGAN_OK;
  if (!pick) {                                             // (a planning call has no tensors)
    if (!in || !wt || !style || (!out && !rgb)) return FMGAN_EINVAL;
    if (rgb && (!rgb->wmod || !rgb->out)) return FMGAN_EINVAL;
  }
  if (fuse_act && noise && noise_batch != 1 && noise_batch != batch) return FMGAN_EINVAL;
  MCParams p{};
#ifdef FMGAN_EXPERIMENTS
  {
    static int dbg = -1;
    if (dbg < 0) { const char* e = getenv("FMGAN_MC_DEBUG"); dbg = e ? atoi(e) : 0; }
    p.debug = dbg;
    static long long clk = -1;
    if (clk < 0) { const char* e = getenv("FMGAN_MC_CLOCKPTR"); clk = e ? atoll(e) : 0; }
    p.dbg_clock = (unsigned long long*)clk;
    { const char* e = getenv("FMGAN_MC_FLAGS"); p.exp_flags = e ? atoi(e) : 0; }
  }
#endif
  if (rgb) {
    p.rgb_wmod = rgb->wmod; p.rgb_bias = rgb->bias; p.rgb_skip = rgb->skip; p.rgb_out = rgb->out; p.rgb_c = rgb->c;
  }
  p.in = in; p.wt = wt; p.style = style; p.demod = demod; p.out = out;
  p.batch = batch; p.cin = cin; p.cout = cout; p.h = h; p.w = w;
  out_dims(mode, h, w, p.oh, p.ow);
  if (out_row_stride == 0) out_row_stride = p.ow;
  if (out_plane_stride == 0) out_plane_stride = (long long)p.oh * out_row_stride;
  if (out_row_stride < p.ow || out_plane_stride < (long long)p.oh * out_row_stride) return FMGAN_EINVAL;
  p.out_plane_stride = out_plane_stride; p.out_row_stride = out_row_stride;
  p.noise = noise; p.noise_weight = noise_weight; p.bias = bias;
  p.noise_batch = noise_batch; p.fuse_act = fuse_act; p.alpha = alpha; p.act_scale = act_scale;
  // index ranges the kernel relies on: pixel indices (y*ow + x, h*w) and per-chunk weight offsets are 32-bit ints,
  // whole-tensor offsets are 64-bit; per-tile input offsets (nb*cin*h*w) are checked per segment in launch_tile
  if ((long long)batch * cout * p.oh * p.ow > (1LL << 40)) return FMGAN_EOVERFLOW;
  if ((long long)p.oh * p.ow >= (1LL << 31) || (long long)h * w >= (1LL << 31)) return FMGAN_EOVERFLOW;
  if (cin > (1 << 20) || cout > (1 << 20)) return FMGAN_EOVERFLOW;
  hipStream_t s = (hipStream_t)stream;
  const int cfg = pick_cfg(mode, cout, (long long)batch * (mode == 2 ? p.oh * p.ow : h * w));
  // split-K only when the caller supplied the workspace fmgan_modconv2d_workspace_bytes() asks for
  p.ksplit = pick_ksplit(mode, batch, cin, cout, h, w);
  const long long need = (long long)p.ksplit * batch * cout * p.oh * p.ow * (long long)sizeof(float);
  if (p.ksplit > 1 && (!workspace || workspace_bytes < need)) p.ksplit = 1;
  if (rgb) p.ksplit = 1;   // the RGB reduction needs the finished sums in one block
  p.ws = (float*)workspace;
  const int chunks = (cin + MC_KC - 1) / MC_KC;
  p.cin_per_split = ((chunks + p.ksplit - 1) / p.ksplit) * MC_KC;
  // Main segment: the h x w grid.  Mode 1: quads (2m+py, 2n+px) of m < h, n < w cover Y < 2h, X < 2w; the last
  // output row (m = h) and column (n = w) are two thin segments of the same launch, so they run beside the
  // main tiles instead of serialising their own latency-bound K loops.
  // The thin segments come FIRST in block order: their blocks pack few useful outputs and must not be the tail.
  if (mode == 1) {
    p.seg[0] = {h, 0, 1, w + 1};
    p.seg[1] = {0, w, h, 1};
    p.seg[2] = {0, 0, h, w};
    p.nseg = 3;
  } else {
    p.seg[0] = {0, 0, p.oh, p.ow};      // mode 0: oh = h; mode 2: the output grid
    p.nseg = 1;
  }
  int st = launch_any(mode, cfg, p, s, pick);
  if (st != FMGAN_OK || pick) return st;
  if (p.ksplit > 1) {
    const long long total = (long long)batch * cout * p.oh * p.ow;
    long long blocks = (total + 255) / 256;
    if (blocks > FMGAN_NUM_CU * 16) blocks = FMGAN_NUM_CU * 16;
    hipLaunchKernelGGL(modconv_splitk_finish_f32, dim3((unsigned)blocks), dim3(256), 0, s, p);
    st = fmgan_check_launch();
  }
  return st;
}
}  // namespace

extern "C" int fmgan_modconv2d_f32(const float* in, const float* wt, const float* style, const float* demod,
                                   float* out, int batch, int cin, int cout, int h, int w, int mode,
                                   const float* noise, const float* noise_weight, const float* bias, int noise_batch,
                                   int fuse_act, float alpha, float act_scale, long long out_plane_stride,
                                   int out_row_stride, void* workspace, long long workspace_bytes, void* stream) {
  return modconv2d_impl(in, wt, style, demod, out, batch, cin, cout, h, w, mode, noise, noise_weight, bias, noise_batch,
                        fuse_act, alpha, act_scale, out_plane_stride, out_row_stride, workspace, workspace_bytes, stream,
                        nullptr);
}

extern "C" int fmgan_modconv2d_rgb_fusable(int batch, int cin, int cout, int h, int w) {
  if (batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return 0;
  return rgb_fusable(batch, cin, cout, h, w) ? 1 : 0;
}

extern "C" int fmgan_modconv2d_rgb_f32(const float* in, const float* wt, const float* style, const float* demod,
                                       float* out, int batch, int cin, int cout, int h, int w,
                                       const float* noise, const float* noise_weight, const float* bias,
                                       int noise_batch, int fuse_act, float alpha, float act_scale,
                                       const float* rgb_wmod, const float* rgb_bias,
                                       const float* rgb_skip, float* rgb_out, int rgb_channels, void* stream) {
  const RgbArgs rgb{rgb_wmod, rgb_bias, rgb_skip, rgb_out, rgb_channels};
  return modconv2d_impl(in, wt, style, demod, out, batch, cin, cout, h, w, 0, noise, noise_weight, bias, noise_batch,
                        fuse_act, alpha, act_scale, 0, 0, nullptr, 0, stream, &rgb);
}

// The planning half of fmgan_modconv2d_f32 / fmgan_modconv2d_rgb_f32 alone: the same modconv2d_impl -> launch_any ->
// launch_tile walk with plan_only set, so the rules are stated once.  The wide patch (and with it the LDS image a DMA tile
// is judged by) depends on the input's alignment: the plan assumes a 16-byte-aligned input, the larger image — a tile that
// takes the aligned tensor takes the misaligned one too.
extern "C" int fmgan_modconv2d_select(int batch, int cin, int cout, int h, int w, int mode, int rgb, int has_workspace,
                                      int* cfg, int* variant, int* bm, int* bn, int* ksplit) {
  alignas(16) static float aligned[4];
  MCPick pick{-1, 0, 0, 0, 0};
  const RgbArgs ra{aligned, nullptr, nullptr, aligned, 3};
  const int st = (rgb && mode != 0) ? FMGAN_EUNSUPPORTED :   // the fused entry point is the plain conv's
                 modconv2d_impl(aligned, nullptr, nullptr, nullptr, aligned, batch, cin, cout, h, w, mode,
                                nullptr, nullptr, nullptr, 1, rgb ? 1 : 0, 0.2f, 1.f, 0, 0,
                                has_workspace && !rgb ? aligned : nullptr, has_workspace && !rgb ? (1LL << 62) : 0,
                                nullptr, rgb ? &ra : nullptr, &pick);
  if (cfg) *cfg = pick.cfg;
  if (variant) *variant = pick.variant;
  if (bm) *bm = pick.bm;
  if (bn) *bn = pick.bn;
  if (ksplit) *ksplit = pick.ksplit;
  return st;
}

extern "C" int fmgan_modconv2d_tiles(int* out, int cap) {
  int n = 0;
  for (const TileEntry& e : MC_TILES) {
    if (out && n < cap) {
      int* o = out + 6 * n;
      o[0] = e.mode; o[1] = e.cfg; o[2] = e.variant; o[3] = e.BM; o[4] = e.BN; o[5] = e.fuses_rgb ? 1 : 0;
    }
    ++n;
  }
  return n;
}
