// K11: per-row quadratic forms and products in float64 of float32 rows (irbfn_rows_quad_f64, include/irbfn_hip.h) -- the pass over
// the rows behind the leverages and leave-one-out residuals of the closed-form output-layer fit (irbfn_amd/loo.py).  The
// reference has no counterpart.
//
//   q[n]    = sum_{j<m} ( sum_{k<=j} z[n][k] p[k][j] )^2          the first m columns of p: an upper triangle (the host passes T^T,
//                                                                  T = L^-1 diag(s), so q[n] = |T z_n|^2 is the leverage of row n)
//   v[n][o] = sum_{k<m} z[n][k] p[k][m + o],  o < nd               nd dense columns (the host passes [W; b]: the prediction)
//
// The product u = z p is rows x m x m / 2 and is never stored.  Arithmetic as K8 (syrk_f64.hip): z is converted float32 -> float64
// (exact), every product and sum runs on v_mfma_f64_16x16x4_f64 with that file's lane layout: lane l holds A[l & 15][l >> 4] =
// (double) z[r0 + (l & 15)][k0 + (l >> 4)], B[l >> 4][l & 15] = p[k0 + (l >> 4)][c0 + (l & 15)] and D[(l >> 4) + 4 reg][l & 15].
//
// Geometry: a block of 4 RT waves owns 64 RT whole rows (RT = kRqRowTiles = 2: eight waves on 128 rows, registers capped for four
// waves per SIMD -- 13 % faster than four waves on 64 rows at three per SIMD, profiles/loo_ab.txt) and walks the m + nd columns in
// tiles of 64; for a tile that lies inside the triangle the k chunks run up to the tile's end only (the tiles below the diagonal
// are skipped), for the tile that holds column m and the later ones up to m.  Wave w owns the 32 x 32 patch (w >> 1, w & 1) of the
// 64 RT x 64 tile of u as 2 x 2 accumulators.  Per chunk of kRqChunk = 32 values of k the block stages z [64 RT rows][32] as
// float (pitch 34: the 32 lanes of a half-wave read 16 rows x 2 k on 32 banks) and p [32][64] as double (pitch 80: the two k rows
// of a half-wave 32 banks apart) through LDS, the next chunk's global loads in flight while this one is multiplied.  An entry of p is loaded only where it is
// used: k < m, column < m + nd and, in the triangle, k <= column; everything else enters as a zero operand and is never read, so
// whatever the strict lower triangle holds reaches no output.  Rows past `rows` are zero operands too.
// After the last chunk of a tile a lane squares its accumulators of the columns < m onto eight running sums (one per row it
// holds) and stores those of the columns >= m to v.  At the end the sixteen lanes that share a row are added by a butterfly
// (xor 1, 2, 4, 8) and the two waves that share it through LDS (w & 1 = 0 first).
// Order of every sum: k ascending within an accumulator, the column tiles ascending, then that fixed tree; which lane holds which
// column depends on the column alone.  So a row's q and v depend on that row's values, m, nd and p only -- not on `rows`, on where
// the row sits in the call or on its neighbours: bit-identical across repeats and across any division of the rows over calls, and a
// non-finite row touches no other row.  No workspace, no atomics, one launch.
#include "common.h"

namespace irbfn {

constexpr int kRqRows = 64;            // rows of z per four waves
constexpr int kRqRowTiles = 2;         // the geometry the library runs: 64 kRqRowTiles rows and 4 kRqRowTiles waves per block,
constexpr int kRqMinWaves = 4;         // registers for four waves per SIMD (tools/ab_rows_quad.hip times the others; DESIGN section 4, "K11")
constexpr int kRqTile = 64;            // columns of p per tile
constexpr int kRqChunk = 32;           // values of k staged at a time
constexpr int kRqPitchZ = 34;          // floats per staged row of z
constexpr int kRqPitchP = 80;          // doubles per staged row of p
constexpr int kRqMaxM = 8192;          // the limit of irbfn_syrk_f64
constexpr int kRqMaxNd = 256;
constexpr long kRqMaxBlocks = 1 << 16; // row tiles beyond it are walked by a grid-stride loop

typedef double rq_d4_t __attribute__((ext_vector_type(4)));

// RT: the block owns 64 RT rows with 4 RT waves; MINW: waves per SIMD asked of the register allocator
template <int RT, int MINW>
__global__ __launch_bounds__(256 * RT, MINW) void rows_quad_f64_kernel(const float* __restrict__ z, long ldz, long rows, int m,
                                                                     const double* __restrict__ p, long ldp, int nd,
                                                                     double* __restrict__ q, double* __restrict__ v) {
  constexpr int PZ = kRqPitchZ, PP = kRqPitchP;
  constexpr int NT = 256 * RT, BR = kRqRows * RT;   // threads and rows of the block
  constexpr int NZ = BR * kRqChunk / NT;            // staged values of z per thread
  constexpr int NP = kRqChunk * kRqTile / NT;       // staged values of p per thread
  __shared__ float zs[BR * PZ];
  __shared__ double ps[kRqChunk * PP];
  __shared__ double qred[2 * BR];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int ncols = m + nd;
  const long ntiles = (rows + BR - 1) / BR;
  // staging: z -- thread t loads k = t % 32 of rows t / 32 + 8 RT i; p -- column t % 64 of the k rows t / 64 + 4 RT i
  const int zk = tid & (kRqChunk - 1), zr = tid / kRqChunk;
  const int pc = tid & (kRqTile - 1), pk = tid / kRqTile;
  const float* __restrict__ za = zs + (wr * 32 + (lane & 15)) * PZ + (lane >> 4);
  const double* __restrict__ pb = ps + (lane >> 4) * PP + wc * 32 + (lane & 15);

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long r0 = tile * BR;
    float rz[NZ];
    double rp[NP];
    auto fetch = [&](int c0, int k0) {
      const int k = k0 + zk;
#pragma unroll
      for (int i = 0; i < NZ; ++i) {
        const long n = r0 + zr + (NT / kRqChunk) * i;
        rz[i] = (n < rows && k < m) ? z[n * ldz + k] : 0.0f;
      }
      const int c = c0 + pc;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int kk = k0 + pk + (NT / kRqTile) * i;
        rp[i] = (kk < m && c < ncols && (c >= m || kk <= c)) ? p[(long)kk * ldp + c] : 0.0;
      }
    };
    auto stage = [&]() {
#pragma unroll
      for (int i = 0; i < NZ; ++i) zs[(zr + (NT / kRqChunk) * i) * PZ + zk] = rz[i];
#pragma unroll
      for (int i = 0; i < NP; ++i) ps[(pk + (NT / kRqTile) * i) * PP + pc] = rp[i];
    };

    rq_d4_t acc[2][2];
    double qs[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = rq_d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) qs[a][r] = 0.0;
    }

    int c0 = 0, k0 = 0;
    fetch(c0, k0);
    while (true) {
      const int kend = c0 + kRqTile <= m ? c0 + kRqTile : m;      // a tile inside the triangle ends at its own last column
      __syncthreads();                       // the previous chunk has been multiplied
      stage();
      __syncthreads();
      const bool last = k0 + kRqChunk >= kend;
      const int nc0 = last ? c0 + kRqTile : c0, nk0 = last ? 0 : k0 + kRqChunk;
      const bool more = nc0 < ncols;
      if (more) fetch(nc0, nk0);
#pragma unroll
      for (int k4 = 0; k4 < kRqChunk / 4; ++k4) {
        double av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          av[a] = (double)za[a * 16 * PZ + k4 * 4];
          bv[a] = pb[k4 * 4 * PP + a * 16];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
      if (last) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int c = c0 + wc * 32 + b * 16 + (lane & 15);
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const double u = acc[a][b][r];
              if (c < m) {
                qs[a][r] += u * u;
              } else if (c < ncols) {
                const long n = r0 + wr * 32 + a * 16 + (lane >> 4) + 4 * r;
                if (n < rows) v[n * nd + (c - m)] = u;
              }
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = rq_d4_t{0.0, 0.0, 0.0, 0.0};
      }
      if (!more) break;
      c0 = nc0;
      k0 = nk0;
    }

    // the sixteen lanes of a row, then its two waves
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double s = qs[a][r];
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) s += __shfl_xor(s, d, kWave);
        if ((lane & 15) == 0) qred[wc * BR + wr * 32 + a * 16 + (lane >> 4) + 4 * r] = s;
      }
    __syncthreads();
    if (tid < BR && r0 + tid < rows) q[r0 + tid] = qred[tid] + qred[BR + tid];
  }
}

// every geometry gives the same bits: which lane holds which column, and every order of a row's sums, does not depend on RT
template <int RT, int MINW>
static int launch_rows_quad(const float* z, int64_t ldz, int64_t rows, int m, const double* p, int64_t ldp, int nd, double* q,
                            double* v, hipStream_t s) {
  const int64_t ntiles = (rows + kRqRows * RT - 1) / (kRqRows * RT);
  const unsigned grid = (unsigned)(ntiles < kRqMaxBlocks ? ntiles : kRqMaxBlocks);
  return launch_kernel<rows_quad_f64_kernel<RT, MINW>>(dim3(grid), dim3(256 * RT), 0, s, z, (long)ldz, (long)rows, m, p, (long)ldp,
                                                       nd, q, v);
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int irbfn_rows_quad_f64(const float* z_dev, int64_t ldz, int64_t rows, int m, const double* p_dev, int64_t ldp, int nd,
                        double* q_dev, double* v_dev, void* stream) {
  if (m < 1 || m > kRqMaxM || nd < 0 || nd > kRqMaxNd || ldz < m || ldp < (int64_t)m + nd || rows < 0) return IRBFN_ERR_BAD_ARG;
  if (rows == 0) return IRBFN_OK;
  if (!z_dev || !p_dev || !q_dev || (nd > 0 && !v_dev)) return IRBFN_ERR_BAD_ARG;
  return launch_rows_quad<kRqRowTiles, kRqMinWaves>(z_dev, ldz, rows, m, p_dev, ldp, nd, q_dev, v_dev,
                                                    reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
