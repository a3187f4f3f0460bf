// K10: orthogonal least squares forward selection on a Gram matrix (irbfn_ols_begin / irbfn_ols_steps, include/irbfn_hip.h).
//
// The reference places no centre by what it explains (it trains every leaf by Adam): parity is unpinned.  What is pinned is the
// arithmetic below against a float64 statement of it (tests/_ols_util.py: ols_ref).
//
// From G = Z^T Z, Z = [h | 1 | y] (NormalEquations), a Cholesky factorisation of A = H^T H + lambda I (+ the ones column) whose
// pivot is the column with the largest drop of the residual, sum_o c[i,o]^2 / d[i], instead of the largest diagonal.  State: d (the
// running diagonal), d0 (the first one), c (the running right-hand side), L (the factor, one row per step), and in the workspace the
// pivot record, the taken flags and the per-block best scores.
//
// A step is two launches, because it has two grid-wide dependencies and a block never waits for another block:
//   ols_step_kernel   64 rows per block, one row i per lane: col[i] = (A[i,j] - sum_{s<t} L[s][i] L[s][j]) / sqrt(d[j]) -> L[t][i];
//                     d[i] -= col^2, c[i,:] -= col ly; the new score of row i; the block's best (score, index)
//   ols_pivot_kernel  one block: count += 1; the best of the block partials (ties to the lowest index, NaN never wins) -> the pivot
//                     record: j, d[j], c[j,:] and the gathered factor column L[0..t)[j], contiguous
// The record is what makes the step race-free: the block that owns row j updates d[j] and c[j,:] while every other block needs
// their values from before the step; all of them read the record, which only the pivot kernel writes.  The pivot kernel also
// gathers L[.][j] (one 8-byte read per factor row, t cache lines) once, so that the step kernel's blocks stage t contiguous
// doubles in LDS instead of each walking t cache lines.
//
// Layout: L is step-major, L[s][i] with i contiguous and the row length npad = M + 1 rounded up to 64: a lane's reads along s
// are coalesced over the wave and L[s][j] is one LDS broadcast.  The sum over s is split over the block's kOlsWaves waves (wave w
// takes s = w, w + kOlsWaves, ...), each with kOlsAcc independent accumulators (a float64 FMA chain is latency-bound); they are
// folded in a fixed order -- the accumulators by halving, (0 + 2) + (1 + 3), then the waves in order -- so that a column's bits depend
// on nothing but the inputs.  A[i,j] is read as G[j][i] (G is symmetric bit for bit): coalesced.
//
// No atomics, no barrier between blocks, nothing read by the host: every output is bit-identical across repeats and across how
// the pivots are divided over calls of irbfn_ols_steps.
#include "common.h"

namespace irbfn {

constexpr int kOlsMaxG = 8192;        // M + 1 + O: the limit of irbfn_syrk_f64
constexpr int kOlsRows = 64;          // rows of a block of the step kernel: one per lane
#ifndef IRBFN_OLS_WAVES               // A/B builds (profiles/ols_ab.txt)
#define IRBFN_OLS_WAVES 16
#endif
#ifndef IRBFN_OLS_ACC
#define IRBFN_OLS_ACC 4
#endif
constexpr int kOlsWaves = IRBFN_OLS_WAVES;        // waves of such a block: the sum over s in kOlsWaves interleaved parts (16: a block of 1024)
constexpr int kOlsAcc = IRBFN_OLS_ACC;            // independent accumulators per lane (a power of two)
constexpr int kOlsChunk = 2048;       // factor-column values staged in LDS at a time (a multiple of kOlsWaves * kOlsAcc)
static_assert(kOlsChunk % (kOlsWaves * kOlsAcc) == 0 && (kOlsAcc & (kOlsAcc - 1)) == 0 && kOlsWaves <= 16, "geometry");
constexpr int kOlsMaxBlocks = kOlsMaxG / kOlsRows;      // 128 partial scores
constexpr int kOlsHeadBytes = 64;

struct OlsHead {                      // the pivot record's fixed part
  int j;                              // the column the next step takes
  int done;                           // 1: the pool is exhausted, every later step is a no-op
  double dj;                          // d[j] before that step
};

__host__ __device__ inline int ols_npad(int M) { return (M + 1 + kOlsRows - 1) & ~(kOlsRows - 1); }

// Workspace: head | cj double [O] | lj double [kmax + 1] | best score double [128] | best index int [128] | taken int [npad]
struct OlsWs {
  OlsHead* head;
  double* cj;
  double* lj;
  double* pscore;
  int* pidx;
  int* taken;
};
__host__ __device__ inline OlsWs ols_ws(void* ws, int O, int kmax) {
  OlsWs w;
  char* p = static_cast<char*>(ws);
  w.head = reinterpret_cast<OlsHead*>(p);
  w.cj = reinterpret_cast<double*>(p + kOlsHeadBytes);
  w.lj = w.cj + O;
  w.pscore = w.lj + kmax + 1;
  w.pidx = reinterpret_cast<int*>(w.pscore + kOlsMaxBlocks);
  w.taken = w.pidx + kOlsMaxBlocks;
  return w;
}
static int64_t ols_workspace_bytes(int M, int O, int kmax) {
  return (int64_t)kOlsHeadBytes + 8 * ((int64_t)O + kmax + 1 + kOlsMaxBlocks) + 4 * ((int64_t)kOlsMaxBlocks + ols_npad(M));
}

struct OlsArgs {
  const double* __restrict__ g;       // [Mg][Mg]
  double* __restrict__ l;             // [kmax + 1][npad]
  double* __restrict__ d;             // [2][npad]: d, d0
  double* __restrict__ c;             // [npad][O]
  int* __restrict__ sel;              // [kmax + 1]
  double* __restrict__ gain;          // [kmax + 1][O]
  int* __restrict__ count;            // [1]
  void* ws;
  double lam, tol;
  int M, O, n, npad, kmax, tmax;      // n: columns of A (M + 1 with the ones column); tmax: pivots at most (kmax + 1 with it)
};

// (score, index) of one row: sum_o c[i,o]^2 / d[i] where the row may still be taken, else (0, -1).  A NaN compares false everywhere.
__device__ __forceinline__ void ols_score(const OlsArgs& a, int i, bool live, double di, double d0i, const double* __restrict__ ci,
                                          double& s, int& idx) {
  s = 0.0;
  idx = -1;
  if (live && i < a.M && di > a.tol * d0i) {
    double q = 0.0;
    for (int o = 0; o < a.O; ++o) q += ci[o] * ci[o];
    const double v = q / di;
    if (v > 0.0) { s = v; idx = i; }
  }
}

// the better of two (score, index): the larger score, equal scores to the lower index; index -1 = none (its score is 0)
__device__ __forceinline__ void ols_better(double& s, int& i, double s2, int i2) {
  if (i2 >= 0 && (i < 0 || s2 > s || (s2 == s && i2 < i))) { s = s2; i = i2; }
}

__device__ __forceinline__ void ols_wave_best(double& s, int& i) {
#pragma unroll
  for (int h = kWave / 2; h > 0; h >>= 1) {
    const double s2 = __shfl_xor(s, h, kWave);
    const int i2 = __shfl_xor(i, h, kWave);
    ols_better(s, i, s2, i2);
  }
}

// d = d0 = diag(A), c = B, nothing taken, the first scores.  One wave per block of 64 rows.
__global__ __launch_bounds__(kOlsRows) void ols_init_kernel(const OlsArgs a) {
  const OlsWs w = ols_ws(a.ws, a.O, a.kmax);
  const int i = blockIdx.x * kOlsRows + threadIdx.x;
  const int Mg = a.M + 1 + a.O;
  const bool in = i < a.n;
  double di = 0.0;
  if (in) {
    di = a.g[(size_t)i * Mg + i] + (i < a.M ? a.lam : 0.0);
    a.d[i] = di;
    a.d[a.npad + i] = di;
    for (int o = 0; o < a.O; ++o) a.c[(size_t)i * a.O + o] = a.g[(size_t)i * Mg + a.M + 1 + o];
    w.taken[i] = 0;
  }
  double s;
  int idx;
  ols_score(a, i, in, di, di, a.c + (size_t)(in ? i : 0) * a.O, s, idx);
  ols_wave_best(s, idx);
  if (threadIdx.x == 0) { w.pscore[blockIdx.x] = s; w.pidx[blockIdx.x] = idx; }
  if (i == 0) { *a.count = 0; }
}

// One block.  first: the pivot of step 0 (the ones column where there is one); else what follows a step: count += 1, the next pivot.
__global__ __launch_bounds__(256) void ols_pivot_kernel(const OlsArgs a, int first, int bias, int nblocks) {
  __shared__ double sm_s[256 / kWave];
  __shared__ int sm_i[256 / kWave];
  __shared__ int sm_j;
  const OlsWs w = ols_ws(a.ws, a.O, a.kmax);
  const int tid = threadIdx.x;
  int t = *a.count;
  const int done = first ? 0 : w.head->done;
  __syncthreads();                                  // every thread has read count and the record before thread 0 writes them
  if (!first) {
    if (done || t >= a.tmax) return;                // the step before this launch was a no-op
    t += 1;
    if (tid == 0) *a.count = t;
    if (t >= a.tmax) return;                        // no further step will run: no pivot to choose
  }
  if (first && bias) {
    if (tid == 0) sm_j = a.d[a.M] > 0.0 ? a.M : -1;
  } else {
    double s = 0.0;
    int idx = -1;
    if (tid < nblocks) { s = w.pscore[tid]; idx = w.pidx[tid]; }      // nblocks <= 128
    ols_wave_best(s, idx);
    if ((tid & (kWave - 1)) == 0) { sm_s[tid >> 6] = s; sm_i[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < 256 / kWave; ++k) ols_better(s, idx, sm_s[k], sm_i[k]);
      sm_j = idx;
    }
  }
  __syncthreads();
  const int j = sm_j;
  if (tid == 0) {
    w.head->j = j;
    w.head->done = j < 0 ? 1 : 0;
    w.head->dj = j < 0 ? 0.0 : a.d[j];
  }
  if (j < 0) return;
  for (int o = tid; o < a.O; o += 256) w.cj[o] = a.c[(size_t)j * a.O + o];
  for (int s = tid; s < t; s += 256) w.lj[s] = a.l[(size_t)s * a.npad + j];
}

__global__ __launch_bounds__(kOlsRows* kOlsWaves) void ols_step_kernel(const OlsArgs a) {
  __shared__ double lj[kOlsChunk];
  __shared__ double fold[kOlsWaves][kOlsRows];
  const OlsWs w = ols_ws(a.ws, a.O, a.kmax);
  const int t = *a.count;
  if (w.head->done || t >= a.tmax) return;          // uniform over the grid
  const int j = w.head->j;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int i = blockIdx.x * kOlsRows + lane;
  const bool in = i < a.n;
  const double* __restrict__ lp = a.l + (in ? i : 0);

  double acc[kOlsAcc];
#pragma unroll
  for (int u = 0; u < kOlsAcc; ++u) acc[u] = 0.0;
  for (int s0 = 0; s0 < t; s0 += kOlsChunk) {
    const int ns = t - s0 < kOlsChunk ? t - s0 : kOlsChunk;
    __syncthreads();                                // the chunk before is done with
    for (int k = tid; k < ns; k += kOlsRows * kOlsWaves) lj[k] = w.lj[s0 + k];
    __syncthreads();
    if (in) {
      // wave w takes s = w, w + kOlsWaves, ...; accumulator u every kOlsAcc-th of those: kOlsChunk is a multiple of their product,
      // so the assignment of s to (wave, accumulator) does not depend on the chunking
      int k = wave;
      for (; k + (kOlsAcc - 1) * kOlsWaves < ns; k += kOlsAcc * kOlsWaves) {
        double v[kOlsAcc];
#pragma unroll
        for (int u = 0; u < kOlsAcc; ++u) v[u] = lp[(size_t)(s0 + k + u * kOlsWaves) * a.npad];
#pragma unroll
        for (int u = 0; u < kOlsAcc; ++u) acc[u] = fma(v[u], lj[k + u * kOlsWaves], acc[u]);
      }
#pragma unroll
      for (int u = 0; u < kOlsAcc; ++u) {
        const int ku = k + u * kOlsWaves;
        if (ku < ns) acc[u] = fma(lp[(size_t)(s0 + ku) * a.npad], lj[ku], acc[u]);
      }
    }
  }
#pragma unroll
  for (int h = kOlsAcc / 2; h > 0; h >>= 1) {
#pragma unroll
    for (int u = 0; u < h; ++u) acc[u] += acc[u + h];
  }
  fold[wave][lane] = acc[0];
  __syncthreads();
  if (wave != 0) return;

  const int Mg = a.M + 1 + a.O;
  const double dj = w.head->dj;
  const double sq = sqrt(dj);
  double s = 0.0;
  int idx = -1;
  if (in) {
    double dot = fold[0][lane];
#pragma unroll
    for (int k = 1; k < kOlsWaves; ++k) dot += fold[k][lane];
    const bool was = w.taken[i] != 0;
    double col = 0.0;
    if (i == j) col = sq;
    else if (!was) col = (a.g[(size_t)j * Mg + i] - dot) / sq;
    a.l[(size_t)t * a.npad + i] = col;
    double di = a.d[i];
    double* __restrict__ ci = a.c + (size_t)i * a.O;
    if (!was) {
      di -= col * col;
      a.d[i] = di;
      for (int o = 0; o < a.O; ++o) ci[o] -= col * (w.cj[o] / sq);
    }
    if (i == j) w.taken[i] = 1;
    ols_score(a, i, !was && i != j, di, a.d[a.npad + i], ci, s, idx);
  }
  ols_wave_best(s, idx);
  if (lane == 0) { w.pscore[blockIdx.x] = s; w.pidx[blockIdx.x] = idx; }
  if (blockIdx.x == 0) {
    if (lane == 0) a.sel[t] = j;
    for (int o = lane; o < a.O; o += kWave) {
      const double ly = w.cj[o] / sq;
      a.gain[(size_t)t * a.O + o] = ly * ly;
    }
  }
}

static int ols_check(const double* g, int M, int O, double tol, int kmax, const double* l, const double* d, const double* c,
                     const int32_t* sel, const double* gain, const int32_t* count, const void* ws, int64_t ws_bytes) {
  if (M < 1 || O < 1 || kmax < 1 || kmax > M || (int64_t)M + 1 + O > kOlsMaxG) return IRBFN_ERR_BAD_ARG;
  if (!(tol >= 0.0)) return IRBFN_ERR_BAD_ARG;     // a NaN fails the comparison
  if (!g || !l || !d || !c || !sel || !gain || !count || !ws) return IRBFN_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < ols_workspace_bytes(M, O, kmax)) return IRBFN_ERR_BAD_ARG;
  return IRBFN_OK;
}

static OlsArgs ols_args(const double* g, int M, int O, int fit_bias, double lam, double tol, int kmax, double* l, double* d, double* c,
                        int32_t* sel, double* gain, int32_t* count, void* ws) {
  OlsArgs a;
  a.g = g; a.l = l; a.d = d; a.c = c; a.sel = sel; a.gain = gain; a.count = count; a.ws = ws;
  a.lam = lam; a.tol = tol;
  a.M = M; a.O = O; a.n = fit_bias ? M + 1 : M; a.npad = ols_npad(M); a.kmax = kmax; a.tmax = kmax + (fit_bias ? 1 : 0);
  return a;
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int64_t irbfn_ols_workspace_bytes(int M, int O, int kmax) {
  if (M < 1 || O < 1 || kmax < 1 || kmax > M || (int64_t)M + 1 + O > kOlsMaxG) return IRBFN_ERR_BAD_ARG;
  return ols_workspace_bytes(M, O, kmax);
}

int irbfn_ols_begin(const double* g_dev, int M, int O, int fit_bias, double ridge_abs, double tol, int kmax, double* l_dev,
                    double* d_dev, double* c_dev, int32_t* sel_dev, double* gain_dev, int32_t* count_dev, void* ws_dev,
                    int64_t ws_bytes, void* stream) {
  const int rc = ols_check(g_dev, M, O, tol, kmax, l_dev, d_dev, c_dev, sel_dev, gain_dev, count_dev, ws_dev, ws_bytes);
  if (rc != IRBFN_OK) return rc;
  if (!(ridge_abs >= 0.0)) return IRBFN_ERR_BAD_ARG;
  const OlsArgs a = ols_args(g_dev, M, O, fit_bias, ridge_abs, tol, kmax, l_dev, d_dev, c_dev, sel_dev, gain_dev, count_dev, ws_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = a.npad / kOlsRows;
  const int r1 = launch_kernel<ols_init_kernel>(dim3(nb), dim3(kOlsRows), 0, s, a);
  if (r1 != IRBFN_OK) return r1;
  return launch_kernel<ols_pivot_kernel>(dim3(1), dim3(256), 0, s, a, 1, fit_bias ? 1 : 0, nb);
}

int irbfn_ols_steps(const double* g_dev, int M, int O, int fit_bias, double tol, int kmax, double* l_dev, double* d_dev,
                    double* c_dev, int32_t* sel_dev, double* gain_dev, int32_t* count_dev, void* ws_dev, int64_t ws_bytes, int steps,
                    void* stream) {
  const int rc = ols_check(g_dev, M, O, tol, kmax, l_dev, d_dev, c_dev, sel_dev, gain_dev, count_dev, ws_dev, ws_bytes);
  if (rc != IRBFN_OK) return rc;
  if (steps < 0) return IRBFN_ERR_BAD_ARG;
  const OlsArgs a = ols_args(g_dev, M, O, fit_bias, 0.0, tol, kmax, l_dev, d_dev, c_dev, sel_dev, gain_dev, count_dev, ws_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nb = a.npad / kOlsRows;
  for (int k = 0; k < steps; ++k) {
    const int r1 = launch_kernel<ols_step_kernel>(dim3(nb), dim3(kOlsRows * kOlsWaves), 0, s, a);
    if (r1 != IRBFN_OK) return r1;
    const int r2 = launch_kernel<ols_pivot_kernel>(dim3(1), dim3(256), 0, s, a, 0, 0, nb);
    if (r2 != IRBFN_OK) return r2;
  }
  return IRBFN_OK;
}

}  // extern "C"
