// K8: float64 Gram matrix of float32 rows (irbfn_syrk_f64, include/irbfn_hip.h) -- the normal equations of the closed-form
// output-layer fit (irbfn_amd/linear_fit.py).  The reference has no counterpart: it reaches its Dense weights by Adam alone.
//
//   g[i][j] (+)= sum_n z[n][i] z[n][j]            i, j < M, both triangles of the full row-major [M][M] matrix
//
// Why float64: RBF design matrices are ill-conditioned and the normal equations square the condition number; a float32 sum
// over 65 536 rows already loses 1e-5.  Every product here is float32 x float32, which is EXACT in float64 (24 + 24 < 53 bits),
// so the only rounding is that of the float64 additions: |g - exact| <= rows 2^-53 sum_n |z_ni z_nj| in any order.
//
// Arithmetic: v_mfma_f64_16x16x4_f64, D[16][16] += A[16][4] B[4][16] with A[i][k] = (double) z[n0 + k][I + i] and
// B[k][j] = (double) z[n0 + k][J + j], four rows of z per instruction.  Lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], one
// f64 each; it holds D[(l >> 4) + 4 reg][l & 15] in reg = 0 .. 3 (NOT the f32 forms' 4 (l >> 4) + reg).
//
// Geometry: G is cut into kSyTile x kSyTile = 64 x 64 tiles and only the pairs I >= J are computed; the rows into S slabs of L
// rows (syrk_plan).  One block of four waves per (pair, slab): wave w owns the 32 x 32 patch (w >> 1, w & 1) of the tile as 2 x 2
// accumulators (32 VGPRs) that stay in registers over the whole slab.  z is staged kSyChunk = 32 rows at a time through LDS as
// float (global -> registers while the previous chunk is multiplied -> LDS), so per four MFMAs a wave issues four ds_read_b32
// and four v_cvt_f64_f32: the conversion is VALU work that runs beside the matrix pipe (the instruction takes 64 cycles, and one
// wave per SIMD with one accumulator already issues it back to back: tools/ubench_mfma_f64.hip).  Rows past the slab or `rows`, and
// columns past M, enter as zero operands and are never read.  Each block stores its 64 x 64 partial to the workspace (written in
// full: nothing relies on a cleared workspace); syrk_reduce_kernel adds the S partials of an entry in slab order onto g (or over
// it) and writes entry (i, j), i < j, from the partials of (j, i): g is symmetric bit for bit, and bit-identical across repeats.
// S aims at kSyBlocksWant blocks, four rounds of the 1024 a card holds at once: with one round's worth the last, part-filled
// round costs 8 % at M = 4107; eight rounds gain nothing more and double the workspace ("K8", also for the
// 128 x 128 tile that was tried and lost).
#include "common.h"

namespace irbfn {

constexpr int kSyTile = 64;           // rows / columns of g per block
constexpr int kSyChunk = 32;          // rows of z staged in LDS at a time
constexpr int kSyPitch = 80;          // floats per staged row: the four k groups of a wave land 16 banks apart
constexpr int kSyMaxM = 8192;
constexpr int kSySlabRows = 256;      // no slab shorter than this (but the last)
#ifndef IRBFN_SY_BLOCKS_WANT          // A/B builds (profiles/linear_fit.txt)
#define IRBFN_SY_BLOCKS_WANT 4096
#endif
constexpr int kSyBlocksWant = IRBFN_SY_BLOCKS_WANT;   // (pair, slab) blocks aimed at: 16 per CU, 4 rounds of the 4 a CU holds
constexpr int kSyMaxSlabs = 256;

typedef double d4_t __attribute__((ext_vector_type(4)));

struct SyrkPlan {
  int T;          // tiles per side
  int64_t P;      // tile pairs I >= J
  int S;          // slabs
  int64_t L;      // rows per slab, a multiple of kSyChunk
};

static SyrkPlan syrk_plan(int64_t rows, int M) {
  SyrkPlan p;
  p.T = (M + kSyTile - 1) / kSyTile;
  p.P = (int64_t)p.T * (p.T + 1) / 2;
  int64_t want = (kSyBlocksWant + p.P - 1) / p.P;                     // fewer slabs for a large M: the workspace is P S 32 KiB
  const int64_t most = (rows + kSySlabRows - 1) / kSySlabRows;
  if (want > most) want = most;
  if (want > kSyMaxSlabs) want = kSyMaxSlabs;
  if (want < 1) want = 1;
  p.L = ((rows + want - 1) / want + kSyChunk - 1) / kSyChunk * kSyChunk;
  if (p.L < kSyChunk) p.L = kSyChunk;
  p.S = rows > 0 ? (int)((rows + p.L - 1) / p.L) : 0;
  return p;
}

static int64_t syrk_workspace_bytes(int64_t rows, int M) {
  const SyrkPlan p = syrk_plan(rows, M);
  return p.P * p.S * (int64_t)(kSyTile * kSyTile * sizeof(double));
}

// pair index of the tile (I, J), I >= J
__host__ __device__ inline long sy_pair(int I, int J) { return (long)I * (I + 1) / 2 + J; }

// two blocks per CU at the least: at most 256 VGPRs (the kernel takes 116: four blocks per CU)
__global__ __launch_bounds__(256, 2) void syrk_f64_kernel(const float* __restrict__ z, long ldz, long rows, int M, long L, int S,
                                                       double* __restrict__ ws) {
  constexpr int WT = kSyTile / 32;      // 16 x 16 accumulators per side of a wave's patch
  constexpr int TS = kSyTile, PITCH = kSyPitch;
  constexpr int RPP = 256 / TS;         // rows staged per pass of the block
  constexpr int NQ = kSyChunk / RPP;    // passes per chunk = staged values per thread and tile
  __shared__ float za[kSyChunk * PITCH], zb[kSyChunk * PITCH];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // blockIdx.x = pair, blockIdx.y = slab
  int I = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while (sy_pair(I + 1, 0) <= (long)blockIdx.x) ++I;
  while (sy_pair(I, 0) > (long)blockIdx.x) --I;
  const int J = (int)((long)blockIdx.x - sy_pair(I, 0));
  const bool diag = I == J;
  const long r0 = (long)blockIdx.y * L;
  const long r1 = r0 + L < rows ? r0 + L : rows;

  // staging: thread t loads column t % TS of rows t / TS + RPP q, q = 0 .. NQ - 1, of each tile (coalesced over the columns)
  const int sc = tid & (TS - 1), sr = tid / TS;
  const int ci = I * TS + sc, cj = J * TS + sc;
  const bool oki = ci < M, okj = cj < M && !diag;
  float ra[NQ], rb[NQ];
  auto fetch = [&](long n0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const long n = n0 + sr + RPP * q;
      const bool in = n < r1;
      ra[q] = (in && oki) ? z[n * ldz + ci] : 0.0f;
      rb[q] = (in && okj) ? z[n * ldz + cj] : 0.0f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      za[(sr + RPP * q) * PITCH + sc] = ra[q];
      if (!diag) zb[(sr + RPP * q) * PITCH + sc] = rb[q];
    }
  };

  d4_t acc[WT][WT];
#pragma unroll
  for (int a = 0; a < WT; ++a)
#pragma unroll
    for (int b = 0; b < WT; ++b) acc[a][b] = d4_t{0.0, 0.0, 0.0, 0.0};
  const int wr = wave >> 1, wc = wave & 1;
  const float* __restrict__ pa = za + (lane >> 4) * PITCH + wr * (16 * WT) + (lane & 15);
  const float* __restrict__ pb = (diag ? za : zb) + (lane >> 4) * PITCH + wc * (16 * WT) + (lane & 15);

  fetch(r0);
  for (long n0 = r0; n0 < r1; n0 += kSyChunk) {
    __syncthreads();                       // the previous chunk has been multiplied
    stage();
    __syncthreads();
    if (n0 + kSyChunk < r1) fetch(n0 + kSyChunk);
#pragma unroll
    for (int k4 = 0; k4 < kSyChunk / 4; ++k4) {
      double av[WT], bv[WT];
#pragma unroll
      for (int a = 0; a < WT; ++a) {
        av[a] = (double)pa[k4 * 4 * PITCH + 16 * a];
        bv[a] = (double)pb[k4 * 4 * PITCH + 16 * a];
      }
#pragma unroll
      for (int a = 0; a < WT; ++a)
#pragma unroll
        for (int b = 0; b < WT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
  }

  double* __restrict__ out = ws + ((long)blockIdx.x * S + blockIdx.y) * (TS * TS);
#pragma unroll
  for (int a = 0; a < WT; ++a)
#pragma unroll
    for (int b = 0; b < WT; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * (16 * WT) + a * 16 + (lane >> 4) + 4 * r, col = wc * (16 * WT) + b * 16 + (lane & 15);
        out[row * TS + col] = acc[a][b][r];
      }
}

// g[i][j] (+)= the S partials of entry (max, min) in slab order; one thread per entry of the full matrix
__global__ __launch_bounds__(256) void syrk_reduce_kernel(const double* __restrict__ ws, double* __restrict__ g, int M, int S,
                                                          int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= M) return;
  const int hi = i > j ? i : j, lo = i > j ? j : i;
  constexpr int TS = kSyTile;
  constexpr long tile = (long)TS * TS;
  const double* __restrict__ p = ws + sy_pair(hi / TS, lo / TS) * S * tile + (hi % TS) * TS + lo % TS;
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += p[k * tile];
  double* __restrict__ o = g + (long)i * M + j;
  *o = accumulate ? *o + s : s;
}

static int launch_syrk_f64(const float* z, int64_t ldz, int64_t rows, int M, double* g, int accumulate, void* ws, hipStream_t s) {
  const SyrkPlan p = syrk_plan(rows, M);
  if (p.S > 0) {
    const int rc = launch_kernel<syrk_f64_kernel>(dim3((unsigned)p.P, (unsigned)p.S), dim3(256), 0, s, z, (long)ldz, (long)rows, M,
                                                  (long)p.L, p.S, static_cast<double*>(ws));
    if (rc != IRBFN_OK) return rc;
  }
  return launch_kernel<syrk_reduce_kernel>(dim3((unsigned)((M + 255) / 256), (unsigned)M), dim3(256), 0, s,
                                           static_cast<const double*>(ws), g, M, p.S, accumulate);
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int64_t irbfn_syrk_f64_workspace_bytes(int64_t rows, int M) {
  if (rows < 0 || M < 1 || M > kSyMaxM) return IRBFN_ERR_BAD_ARG;
  return syrk_workspace_bytes(rows, M);
}

int irbfn_syrk_f64(const float* z_dev, int64_t ldz, int64_t rows, int M, double* g_dev, int accumulate, void* ws_dev,
                   int64_t ws_bytes, void* stream) {
  if (M < 1 || M > kSyMaxM || ldz < M || rows < 0 || !g_dev || (rows > 0 && !z_dev)) return IRBFN_ERR_BAD_ARG;
  if (rows == 0 && accumulate) return IRBFN_OK;
  const int64_t need = syrk_workspace_bytes(rows, M);
  if (need > 0 && (!ws_dev || (reinterpret_cast<uintptr_t>(ws_dev) & 7) != 0 || ws_bytes < need)) return IRBFN_ERR_BAD_ARG;
  return launch_syrk_f64(z_dev, ldz, rows, M, g_dev, accumulate, ws_dev, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
