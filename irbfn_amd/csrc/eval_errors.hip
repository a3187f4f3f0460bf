// K6: roll-out error statistics of a whole table, on device (irbfn_eval_rollout_errors, include/irbfn_hip.h).
//
// What scripts/eval_irbfn_dnmpc.py:92-167 does on the host for one table: roll the label controls and the predicted
// controls out side by side from the same initial state and report how far the two end states are apart.  One thread per
// table row; the two roll-outs are roll_init / roll_step of rollout_step.h (no model is restated here), the loop over the
// T steps is rolled (no adjoint, so nothing is parked per step), the next step's four controls are fetched while the
// current step computes.  A row gives M = S + 2 float32 metrics:
//   [0, S)  |p_i - a_i|                    final-state error per component (plain difference, no angle wrapping)
//   S       hypotf(p_0 - a_0, p_1 - a_1)   position error (x, y; Frenet: s, e_y)
//   S + 1   mean_j |y_pred_j - y_j|        over the 2T controls (summed in float64, rounded once)
// and the kernel keeps, per metric, n / sum / sum_sq / max (float64), the lowest row that attains the maximum and a
// histogram of 512 bins, eight per octave: bin = clamp((float_bits(e) >> 20) - 696, 0, 511), i.e. the exponent and the top
// three mantissa bits: bin 0 = [0, 2^-40 * 9/8), bin 511 = everything finite from 2^23 * 15/8 up (eval_bin).  A value that
// is not finite enters none of them (the caller gets their number as rows - n).
//
// Deterministic, bit-identical across repeats: per-thread float64 accumulators -> a fixed tree (lanes of a wave by
// shuffles, then the block's four waves in order) -> per-block partials in the workspace -> block 0 of eval_final_kernel
// adds them IN BLOCK ORDER onto the running values.  The histogram is int32 [M][512] in LDS (20 KiB at M = 10) and leaves
// the block as a plain copy into the workspace; the other blocks of eval_final_kernel add the per-block copies bin by bin
// onto the int64 histogram (one writer per bin; integer sums do not depend on order).  First version: every block added
// its non-zero bins to the int64 histogram with 64-bit atomics -- device-scope atomics are resolved behind the per-XCD L2s,
// and ~125 000 of them (313 blocks, B = 80 000) cost ~10 us per metric; with a one-thread-per-quantity final kernel that
// fetched one partial per loop trip the call took 146 - 175 us (profiles/evaluate.txt).
#include "common.h"
#include "rollout_step.h"

namespace irbfn {

constexpr int kEvalBins = 512;
constexpr int kEvalBinBias = 696;        // (127 - 40) << 3: float_bits(2^-40) >> 20
constexpr int kEvalMaxT = 64;
constexpr int kEvalMaxM = 10;            // Frenet: S = 8
constexpr long kEvalNoRow = 0x7fffffffffffffffL;   // "no row yet" of a partial: loses every tie

// The workspace: five per-block partial tables [kSeedBlocksMax][M] of 8-byte entries, then the per-block histogram copies
// [kSeedBlocksMax][M][512] int32.
struct EvalWs {
  double* sum;
  double* sq;
  double* mx;
  long* n;
  long* arg;
  int* hist;
};

__host__ __device__ inline EvalWs eval_ws(void* ws, int M) {
  const size_t tab = (size_t)kSeedBlocksMax * M;
  double* d = static_cast<double*>(ws);
  return EvalWs{d, d + tab, d + 2 * tab, reinterpret_cast<long*>(d + 3 * tab), reinterpret_cast<long*>(d + 4 * tab),
                reinterpret_cast<int*>(d + 5 * tab)};
}

struct EvalArgs {
  const float* __restrict__ state0;   // [B][S0]
  const float* __restrict__ yp;       // [B][2T]
  const float* __restrict__ y;        // [B][2T]
  float* __restrict__ err;            // [B][M] or null
  void* ws;
  long B, row0;
  int T;
  DynParams dp;
};

__device__ __forceinline__ int eval_bin(float e) {
  const int k = (int)(__float_as_uint(e) >> 20) - kEvalBinBias;
  return k < 0 ? 0 : (k > kEvalBins - 1 ? kEvalBins - 1 : k);
}

// (value, row) pairs order by the larger value, then the lower row
__device__ __forceinline__ bool eval_beats(double vb, long rb, double va, long ra) { return vb > va || (vb == va && rb < ra); }

template <int MODE>
__global__ __launch_bounds__(256) void eval_errors_kernel(const EvalArgs a) {
  constexpr int S = ModeTraits<MODE>::S, S0 = ModeTraits<MODE>::S0, M = S + 2;
  constexpr int NW = 256 / kWave;
  static_assert(M <= kEvalMaxM, "workspace and LDS are sized for M <= 10");
  __shared__ int hist[M * kEvalBins];
  __shared__ double sm_sum[NW][M], sm_sq[NW][M], sm_mx[NW][M];
  __shared__ long sm_arg[NW][M];
  __shared__ int sm_n[NW][M];
  const int tid = threadIdx.x;
  for (int i = tid; i < M * kEvalBins; i += 256) hist[i] = 0;
  __syncthreads();

  const int T = a.T;
  const double inv_2t = 1.0 / (double)(2 * T);
  double sum[M], sq[M], mx[M];
  long arg[M];
  int n[M];
#pragma unroll
  for (int m = 0; m < M; ++m) { sum[m] = 0.0; sq[m] = 0.0; mx[m] = -INFINITY; arg[m] = kEvalNoRow; n[m] = 0; }

  for (long b = (long)blockIdx.x * 256 + tid; b < a.B; b += (long)gridDim.x * 256) {
    const float* yr = a.y + b * 2 * T;
    const float* pr = a.yp + b * 2 * T;
    float sa[S], sp[S];
    roll_init<MODE>(a.state0 + b * S0, sa);
#pragma unroll
    for (int i = 0; i < S; ++i) sp[i] = sa[i];
    double dsum = 0.0;
    float ya = yr[0], ys = yr[T], pa = pr[0], ps = pr[T];
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const float ya0 = ya, ys0 = ys, pa0 = pa, ps0 = ps;
      const int tn = t + 1 < T ? t + 1 : t;                 // the last step fetches its own controls again: in bounds
      ya = yr[tn]; ys = yr[T + tn]; pa = pr[tn]; ps = pr[T + tn];
      roll_step<MODE>(sa, ya0, ys0, a.dp);
      roll_step<MODE>(sp, pa0, ps0, a.dp);
      dsum += (double)fabsf(pa0 - ya0) + (double)fabsf(ps0 - ys0);
    }
    float e[M];
#pragma unroll
    for (int i = 0; i < S; ++i) e[i] = fabsf(sp[i] - sa[i]);
    e[S] = hypotf(sp[0] - sa[0], sp[1] - sa[1]);
    e[S + 1] = (float)(dsum * inv_2t);
    if (a.err) {
#pragma unroll
      for (int m = 0; m < M; ++m) a.err[b * M + m] = e[m];
    }
    const long row = a.row0 + b;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if ((__float_as_uint(e[m]) & 0x7f800000u) != 0x7f800000u) {      // finite (e >= 0 or NaN by construction)
        const double d = (double)e[m];
        n[m] += 1;
        sum[m] += d;
        sq[m] += d * d;
        if (d > mx[m]) { mx[m] = d; arg[m] = row; }                    // rows ascend per thread: the first one stays
        atomicAdd(&hist[m * kEvalBins + eval_bin(e[m])], 1);
      }
    }
  }

  // fixed tree: the 64 lanes of a wave by shuffles (no barrier), then the block's waves in order
  const int lane = tid & (kWave - 1), wave = tid >> 6;
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int h = kWave / 2; h > 0; h >>= 1) {
      sum[m] += __shfl_down(sum[m], h, kWave);
      sq[m] += __shfl_down(sq[m], h, kWave);
      n[m] += __shfl_down(n[m], h, kWave);
      const double vb = __shfl_down(mx[m], h, kWave);
      const long rb = __shfl_down(arg[m], h, kWave);
      if (eval_beats(vb, rb, mx[m], arg[m])) { mx[m] = vb; arg[m] = rb; }
    }
    if (lane == 0) { sm_sum[wave][m] = sum[m]; sm_sq[wave][m] = sq[m]; sm_mx[wave][m] = mx[m]; sm_arg[wave][m] = arg[m]; sm_n[wave][m] = n[m]; }
  }
  __syncthreads();
  const EvalWs w = eval_ws(a.ws, M);
  if (tid < M) {
    double t1 = sm_sum[0][tid], t2 = sm_sq[0][tid], v = sm_mx[0][tid];
    long r = sm_arg[0][tid], c = sm_n[0][tid];
    for (int k = 1; k < NW; ++k) {
      t1 += sm_sum[k][tid]; t2 += sm_sq[k][tid]; c += sm_n[k][tid];
      if (eval_beats(sm_mx[k][tid], sm_arg[k][tid], v, r)) { v = sm_mx[k][tid]; r = sm_arg[k][tid]; }
    }
    const size_t o = (size_t)blockIdx.x * M + tid;
    w.sum[o] = t1; w.sq[o] = t2; w.mx[o] = v; w.n[o] = c; w.arg[o] = r;
  }
  // the block's histogram: a plain copy (the LDS atomics above are behind the barrier)
  int* ph = w.hist + (size_t)blockIdx.x * (M * kEvalBins);
  for (int i = tid; i < M * kEvalBins; i += 256) ph[i] = hist[i];
}

constexpr int kEvalChunk = 64;     // block partials staged per pass of the final kernel's block 0
constexpr int kEvalHistBins = 32;  // histogram bins per block of the final kernel (512 is a multiple)

// Block 0: thread (q, m) = (tid / 16, tid % 16), q < 4, m < M, adds the nb block partials of one quantity of metric m onto the
// running value IN BLOCK ORDER: q = 0: n, 1: sum, 2: sum_sq, 3: max with its row.  The partials come through LDS in passes of
// kEvalChunk blocks, fetched by all 256 threads (one partial per loop trip from global memory made the serial chain a chain
// of memory round trips).  Blocks 1 ..: 32 bins of one metric each, the nb per-block histogram copies added onto hist.
// reset: start from the empty statistics (n = sum = sum_sq = 0, max = -inf, argmax = -1, empty histogram) instead of the caller's.
__global__ __launch_bounds__(256) void eval_final_kernel(void* ws, int nb, int M, int reset, double* __restrict__ stats,
                                                         long* __restrict__ argmax, long* __restrict__ hist) {
  const EvalWs w = eval_ws(ws, M);
  const int tid = threadIdx.x;
  if (blockIdx.x > 0) {
    // kEvalHistBins bins x 8 slices of the block partials per block: many short load chains instead of a few long ones
    __shared__ long part[256 / kEvalHistBins][kEvalHistBins];
    const int bl = tid & (kEvalHistBins - 1), slice = tid / kEvalHistBins;
    const int i = (blockIdx.x - 1) * kEvalHistBins + bl;
    const int* p = w.hist + i;
    const size_t stride = (size_t)M * kEvalBins;
    long c = 0;
#pragma unroll 16
    for (int k = slice; k < nb; k += 256 / kEvalHistBins) c += p[k * stride];
    part[slice][bl] = c;
    __syncthreads();
    if (slice == 0) {
      long t = reset ? 0 : hist[i];
      for (int k = 0; k < 256 / kEvalHistBins; ++k) t += part[k][bl];
      hist[i] = t;
    }
    return;
  }
  __shared__ double l_sum[kEvalChunk * kEvalMaxM], l_sq[kEvalChunk * kEvalMaxM], l_mx[kEvalChunk * kEvalMaxM];
  __shared__ long l_n[kEvalChunk * kEvalMaxM], l_arg[kEvalChunk * kEvalMaxM];
  const int q = tid >> 4, m = tid & 15;
  const bool mine = q < 4 && m < M;
  double acc = 0.0, v = -INFINITY;
  long cnt = 0, r = -1;
  if (mine && !reset) {
    if (q == 0) cnt = (long)stats[m * 4 + 0];
    else if (q < 3) acc = stats[m * 4 + q];
    else { v = stats[m * 4 + 3]; r = argmax[m]; }
  }
  for (int c0 = 0; c0 < nb; c0 += kEvalChunk) {
    const int cn = nb - c0 < kEvalChunk ? nb - c0 : kEvalChunk;
    const size_t off = (size_t)c0 * M;
    __syncthreads();
    for (int i = tid; i < cn * M; i += 256) {
      l_sum[i] = w.sum[off + i]; l_sq[i] = w.sq[off + i]; l_mx[i] = w.mx[off + i]; l_n[i] = w.n[off + i]; l_arg[i] = w.arg[off + i];
    }
    __syncthreads();
    if (mine) {
      if (q == 0) {
        for (int i = 0; i < cn; ++i) cnt += l_n[i * M + m];
      } else if (q < 3) {
        const double* p = q == 1 ? l_sum : l_sq;
#pragma unroll 8
        for (int i = 0; i < cn; ++i) acc += p[i * M + m];
      } else {
        for (int i = 0; i < cn; ++i)
          if (eval_beats(l_mx[i * M + m], l_arg[i * M + m], v, r)) { v = l_mx[i * M + m]; r = l_arg[i * M + m]; }
      }
    }
  }
  if (mine) {
    if (q == 0) stats[m * 4 + 0] = (double)cnt;
    else if (q < 3) stats[m * 4 + q] = acc;
    else { stats[m * 4 + 3] = v; argmax[m] = r; }
  }
}

int eval_num_metrics(int mode) {
  const ModeDims d = mode_dims(mode);
  return d.S < 0 ? IRBFN_ERR_BAD_ARG : (d.NU == 0 ? IRBFN_ERR_UNSUPPORTED : d.S + 2);
}

int64_t eval_workspace_bytes(int mode) {
  const int M = eval_num_metrics(mode);
  return M < 0 ? (int64_t)M : (int64_t)kSeedBlocksMax * M * (5 * 8 + kEvalBins * 4);
}

template <int MODE>
static void launch_eval_mode(const EvalArgs& a, int nb, hipStream_t s) {
  hipLaunchKernelGGL(eval_errors_kernel<MODE>, dim3(nb), dim3(256), 0, s, a);
}

int launch_eval_errors(int mode, const float* state0, const float* y_pred, const float* y, const DynParams& dp, int64_t B, int T,
                       int64_t row0, int accumulate, float* err, double* stats, int64_t* argmax, int64_t* hist, void* ws,
                       hipStream_t s) {
  const int M = eval_num_metrics(mode);
  if (M < 0) return M;
  if (T > kEvalMaxT) return IRBFN_ERR_UNSUPPORTED;
  if (B == 0 && accumulate) return IRBFN_OK;
  int nb = 0;
  if (B > 0) {
    const int64_t blocks = (B + 255) / 256;
    nb = blocks > kSeedBlocksMax ? kSeedBlocksMax : (int)blocks;
    EvalArgs a;
    a.state0 = state0; a.yp = y_pred; a.y = y; a.err = err;
    a.ws = ws;
    a.B = (long)B; a.row0 = (long)row0; a.T = T; a.dp = dp;
    switch (mode) {
      case IRBFN_ROLLOUT_ST_SELECT: launch_eval_mode<IRBFN_ROLLOUT_ST_SELECT>(a, nb, s); break;
      case IRBFN_ROLLOUT_ST_KS: launch_eval_mode<IRBFN_ROLLOUT_ST_KS>(a, nb, s); break;
      case IRBFN_ROLLOUT_FULLINT: launch_eval_mode<IRBFN_ROLLOUT_FULLINT>(a, nb, s); break;
      default: launch_eval_mode<IRBFN_ROLLOUT_FRENET_LS>(a, nb, s); break;
    }
    IRBFN_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(eval_final_kernel, dim3(1 + M * kEvalBins / kEvalHistBins), dim3(256), 0, s, ws, nb, M, accumulate ? 0 : 1, stats,
                     reinterpret_cast<long*>(argmax), reinterpret_cast<long*>(hist));
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

}  // namespace irbfn
