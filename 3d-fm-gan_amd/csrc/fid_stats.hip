// Running feature statistics of the FID (reference Evaluation/fid.py:126-127: np.mean / np.cov of all features on the
// host, in float64) for gfx950: first and second moments accumulated on the device, batch by batch, in float64.
//
//   feat  [b, d] f32 row-major (one batch of Inception features)
//   y     = (double)feat[r, c] - shift[c]                       shift fixed before the first update
//   sum   [d]     += sum_r y[r, c]
//   outer [d, d]  += sum_r y[r, i] * y[r, j]   for i <= j       elements below the diagonal are never touched
//
// The contraction is Y^T Y with K = the batch rows, on v_mfma_f64_16x16x4_f64.  A 16 x 16 tile (i0, j0) takes, per step of
// four rows r0 .. r0+3, lane l's A element y[r0 + (l >> 4), i0 + (l & 15)] and B element y[r0 + (l >> 4), j0 + (l & 15)]:
// both slabs come from the same feat rows, a lane's load is one float of 16 contiguous floats of a row, and a wave's load
// is four such 64-byte runs.  Rows beyond b contribute exact zeros (y = 0, not -shift).  Accumulator element reg of lane l
// is (row (l >> 4) + 4 * reg, column l & 15) of the tile: the lane reads outer there, adds, writes back: every element has
// one owner, no atomics, and an element's bits depend on b and the data alone (rows in order, four per instruction), not
// on the grid.
//
// Tiling: a block of four waves owns a 64 x 64 block tile (bi <= bj only: D = 2048 gives 528 blocks); wave w owns the 16
// rows i0 = 64 bi + 16 w and the four 16-column tiles of the block tile: one A and four B operands per step, 16
// accumulator doubles per lane.  Tiles past d (d % 64 != 0) and, in a diagonal block, tiles below the diagonal are not
// written (their MFMAs run on the wave's own columns, so that the loop has no branch).  A diagonal tile (i0 == j0) also carries the column sums: each lane adds its own A elements over the steps,
// the four row groups are added in order 0..3 through the wave, and lanes 0..15 add the total to sum[i0 + lane].
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FS_TILE = 16;                   // MFMA tile edge
constexpr int FS_WAVES = 4;                   // waves per block = 16-row strips per block tile
constexpr int FS_BLOCK = FS_TILE * FS_WAVES;  // block tile edge
constexpr int FS_THREADS = FMGAN_WAVE * FS_WAVES;
constexpr int FS_DEPTH = 4;                   // steps of four rows whose loads are in flight together

__global__ __launch_bounds__(FS_THREADS) void fid_stats_update_f32(const float* __restrict__ feat,
                                                                   const double* __restrict__ shift,
                                                                   double* __restrict__ sum, double* __restrict__ outer,
                                                                   int b, int d, int nb) {
  // linear block id -> (bi, bj), bi <= bj, rows of the upper triangle in order
  int bi = 0, rem = (int)blockIdx.x, len = nb;
  while (rem >= len) {
    rem -= len;
    --len;
    ++bi;
  }
  const int bj = bi + rem;
  const int wave = threadIdx.x / FMGAN_WAVE, lane = threadIdx.x % FMGAN_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int i0 = bi * FS_BLOCK + wave * FS_TILE;
  if (i0 >= d) return;
  const int jbase = bj * FS_BLOCK;
  // tile t of this wave is live when it is inside the matrix and not below the diagonal.  A dead tile runs on the
  // wave's own A columns (valid memory) and is never written: the loop body is straight-line code, so the loads of
  // several steps are in flight at once (a branch per tile made each step wait for its five loads in turn)
  bool live[FS_WAVES];
  int jc[FS_WAVES];
  double shb[FS_WAVES];
#pragma unroll
  for (int t = 0; t < FS_WAVES; ++t) {
    const int j0 = jbase + t * FS_TILE;
    live[t] = j0 < d && j0 >= i0;
    jc[t] = (live[t] ? j0 : i0) + col;
    shb[t] = shift[jc[t]];
  }
  const double sha = shift[i0 + col];
  f64x4 acc[FS_WAVES];
#pragma unroll
  for (int t = 0; t < FS_WAVES; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;
  // FS_DEPTH steps of four rows per trip: all their loads first, then their MFMAs in row order.  A step past b adds
  // exact zeros (acc + 0 * 0), so the bits are those of ceil(b / 4) steps.
  for (int r0 = 0; r0 < b; r0 += 4 * FS_DEPTH) {
    float fa[FS_DEPTH], fv[FS_DEPTH][FS_WAVES];
#pragma unroll
    for (int s = 0; s < FS_DEPTH; ++s) {
      const int r = r0 + 4 * s + grp;
      const float* row = feat + (long long)(r < b ? r : 0) * d;
      fa[s] = row[i0 + col];
#pragma unroll
      for (int t = 0; t < FS_WAVES; ++t) fv[s][t] = row[jc[t]];
    }
#pragma unroll
    for (int s = 0; s < FS_DEPTH; ++s) {
      const bool in = r0 + 4 * s + grp < b;
      const double a = in ? (double)fa[s] - sha : 0.0;
      colsum += a;
#pragma unroll
      for (int t = 0; t < FS_WAVES; ++t) {
        const double v = in ? (double)fv[s][t] - shb[t] : 0.0;
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, v, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < FS_WAVES; ++t) {
    if (!live[t]) continue;
    const int j0 = jbase + t * FS_TILE;
    const bool diag = j0 == i0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ti = grp + 4 * reg;
      if (!diag || ti <= col) {
        double* p = outer + (long long)(i0 + ti) * d + (j0 + col);
        *p = *p + acc[t][reg];
      }
    }
  }
  if (jbase <= i0 && i0 < jbase + FS_BLOCK) {      // this wave holds the diagonal tile of its 16 columns
    const double g1 = __shfl(colsum, col + 16), g2 = __shfl(colsum, col + 32), g3 = __shfl(colsum, col + 48);
    if (grp == 0) sum[i0 + col] = sum[i0 + col] + (((colsum + g1) + g2) + g3);
  }
}

constexpr int FF_TILE = 16;

__global__ __launch_bounds__(FF_TILE* FF_TILE) void fid_stats_finish_f64(const double* __restrict__ sum,
                                                                         const double* __restrict__ outer,
                                                                         const double* __restrict__ shift, double n,
                                                                         double* __restrict__ mean,
                                                                         double* __restrict__ cov, int d) {
  if (blockIdx.y > blockIdx.x) return;
  const int i = blockIdx.y * FF_TILE + threadIdx.y, j = blockIdx.x * FF_TILE + threadIdx.x;
  if (i >= d || j >= d || i > j) return;
  const double si = sum[i], sj = sum[j];
  const double prod = si * sj;
  const double c = (outer[(long long)i * d + j] - prod / n) / (n - 1.0);
  cov[(long long)i * d + j] = c;
  cov[(long long)j * d + i] = c;
  if (i == j) mean[i] = shift[i] + si / n;
}

// Index ranges: element offsets are long long; tile and block indices are ints, and the linear grid of
// nb * (nb + 1) / 2 blocks has to fit grid.x.
int fs_plan(int b, int d) {
  if (b <= 0 || d <= 0) return FMGAN_EINVAL;
  if (d % FS_TILE != 0) return FMGAN_EUNSUPPORTED;
  if (d > (1 << 21) || b > 0x7fffffff - 4) return FMGAN_EOVERFLOW;      // nb <= 2^15: nb * (nb + 1) / 2 < 2^31
  return 1;
}

}  // namespace

extern "C" int fmgan_fid_stats_select(int b, int d) { return fs_plan(b, d); }

extern "C" int fmgan_fid_stats_update_f32(const float* feat, const double* shift, double* sum, double* outer, int b,
                                          int d, void* stream) {
  if (!feat || !shift || !sum || !outer) return FMGAN_EINVAL;
  const int id = fs_plan(b, d);
  if (id <= 0) return id;
  const int nb = (d + FS_BLOCK - 1) / FS_BLOCK;
  const dim3 grid((unsigned)((long long)nb * (nb + 1) / 2)), block(FS_THREADS);
  hipLaunchKernelGGL(fid_stats_update_f32, grid, block, 0, (hipStream_t)stream, feat, shift, sum, outer, b, d, nb);
  return fmgan_check_launch();
}

extern "C" int fmgan_fid_stats_finish_f64(const double* sum, const double* outer, const double* shift, long long n,
                                          double* mean, double* cov, int d, void* stream) {
  if (!sum || !outer || !shift || !mean || !cov || d <= 0 || n < 2) return FMGAN_EINVAL;
  if (d > 65535 * FF_TILE) return FMGAN_EOVERFLOW;      // grid.y
  const int nt = (d + FF_TILE - 1) / FF_TILE;
  const dim3 grid(nt, nt), block(FF_TILE, FF_TILE);
  hipLaunchKernelGGL(fid_stats_finish_f64, grid, block, 0, (hipStream_t)stream, sum, outer, shift, (double)n, mean, cov,
                     d);
  return fmgan_check_launch();
}
