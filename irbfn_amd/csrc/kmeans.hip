// K7: one Lloyd iteration of k-means on a table (irbfn_kmeans_step, include/irbfn_hip.h).
//
// The reference derives the centres of its fixed-centre nets and the cluster labels of train_step_fullint_withcluster in
// notebooks that are not part of its snapshot (VERDICT missing #3): parity with its clustering is
// unpinned.  What is pinned is the arithmetic below, against a float64 statement of it (tests/_kmeans_util.py).
//
// Three launches behind one memset of the accumulators:
//   kmeans_colmax_kernel   per column the largest |x| over the finite rows, one partial per block (a max has no order)
//   kmeans_assign_kernel   one pass over the rows: nearest centre, label, d2, the scatter-add, the step statistics
//   kmeans_update_kernel   sums -> new centres, counts, the largest shift^2; block 0 adds the partial statistics
//
// Assignment: two rows per lane (their D values in registers), the centres staged kTile at a time in LDS and read as
// broadcasts (every lane of a wave reads the same address), d2 = the float32 chain fmaf(t, t, d2) with t = x - c over
// d = 0 .. D-1 -- the direct difference of lut_nearest_kernel, no Gram expansion -- and a running (best d2, best k) per row
// with a strict <: centres ascend, so ties stay with the lowest k, a NaN or Inf d2 never wins, and a row that nothing beat
// INFINITY for (a non-finite component, or every d2 overflowing) gets label -1, d2 NaN and enters nothing.
//
// Accumulation: N rows into K (D + 1) cells, exact and order-free.  Column d lives on a fixed-point grid: with
// max |x[:, d]| < 2^e and N < 2^L a row adds q = rint(x * 2^(S - e)), S = 62 - L, to a 64-bit integer cell, so no sum
// leaves int64 whatever the order, and a count adds 1.  |q * 2^(e - S) - x| <= 2^(e - S - 1) <= 2^-S max|x|, and the mean of
// rows inherits that bound: 2^-39 of the column's largest magnitude at N = 2^22, 2^-30 at N = 2^31 (the float32 rounding
// of the result is 2^-24).  Where K (D + 1) <= kLdsCells the cells are first summed per block in LDS (ds_add_u64) and
// each block adds its non-zero cells to the workspace once; above that the rows add to the workspace directly
// (global_atomic_add_x2).  Float atomics would be order-dependent; per-block float64 slabs are K (D + 1) x 8 bytes per
// block, 360 KB at K = 5000, D = 8 -- neither an LDS nor, times a thousand blocks, a workspace size.
//
// Statistics: per-thread (float64 inertia, finite rows, moved rows) -> shuffles over the wave -> the block's four waves in
// order -> one partial per block -> block 0 of the update kernel adds them in a fixed tree (thread t takes partials t, t + 256,
// ... in order, then halving steps through LDS): bit-identical across repeats.  The largest shift^2 is an integer max of
// float64 bits (non-negative doubles order as their bits).
#include "common.h"

namespace irbfn {

constexpr int kKmMaxD = 16;
constexpr int kKmMaxK = 65536;
constexpr int kKmTile = 256;          // centres staged in LDS per pass
#ifndef IRBFN_KM_ROWS                 // A/B builds (profiles/kmeans.txt)
#define IRBFN_KM_ROWS 2
#endif
#ifndef IRBFN_KM_LDS_CELLS
#define IRBFN_KM_LDS_CELLS 4608
#endif
constexpr int kKmRows = IRBFN_KM_ROWS;            // rows per lane
constexpr int kKmBlocksMax = 1024;    // blocks of the assignment pass = partial statistics in the workspace
constexpr int kKmLdsCells = IRBFN_KM_LDS_CELLS;   // K (D + 1) up to here: the block's sums in LDS (36 KiB); K = 500, D = 8 is 4500
constexpr int kKmHeadBytes = 64;      // colmax bits [16]
constexpr int kKmColBlocks = 512;     // blocks of the column-maximum pass = partial maxima in the workspace

struct KmPartial {
  double inertia;
  long finite, moved;
};

// Workspace: colmax bits [16] | cells int64 [K][D + 1] | partials [kKmBlocksMax] | colmax partials [kKmColBlocks][16]
__host__ __device__ inline unsigned* km_colmax(void* ws) { return static_cast<unsigned*>(ws); }
__host__ __device__ inline long* km_cells(void* ws) { return reinterpret_cast<long*>(static_cast<char*>(ws) + kKmHeadBytes); }
__host__ __device__ inline KmPartial* km_partials(void* ws, int K, int D) {
  return reinterpret_cast<KmPartial*>(static_cast<char*>(ws) + kKmHeadBytes + (size_t)K * (D + 1) * sizeof(long));
}

__host__ __device__ inline unsigned* km_colpart(void* ws, int K, int D) {
  return reinterpret_cast<unsigned*>(km_partials(ws, K, D) + kKmBlocksMax);
}

int64_t kmeans_workspace_bytes(int64_t N, int K, int D) {
  (void)N;
  return (int64_t)kKmHeadBytes + (int64_t)K * (D + 1) * 8 + (int64_t)kKmBlocksMax * (int64_t)sizeof(KmPartial) +
         (int64_t)kKmColBlocks * kKmMaxD * 4;
}

__device__ __forceinline__ bool km_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// 2^p as a double, -1022 <= p <= 1023
__device__ __forceinline__ double km_pow2(int p) { return __longlong_as_double((long)(1023 + p) << 52); }
// e with |v| < 2^e for the float whose magnitude bits are `bits` (a subnormal counts as the smallest normal exponent)
__device__ __forceinline__ int km_exp(unsigned bits) {
  const int E = (int)(bits >> 23);
  return (E < 1 ? 1 : E) - 126;
}

template <int D>
__device__ __forceinline__ bool km_load_row(const float* __restrict__ x, long n, bool vec, float (&r)[D]) {
  const float* p = x + n * D;
  if constexpr (D % 4 == 0) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < D / 4; ++j) {
        const float4 v = reinterpret_cast<const float4*>(p)[j];
        r[4 * j] = v.x; r[4 * j + 1] = v.y; r[4 * j + 2] = v.z; r[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) r[d] = p[d];
    }
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) r[d] = p[d];
  }
  bool fin = true;
#pragma unroll
  for (int d = 0; d < D; ++d) fin = fin && km_finite(r[d]);
  return fin;
}

template <int D>
__global__ __launch_bounds__(256) void kmeans_colmax_kernel(const float* __restrict__ x, long N, int vec, unsigned* __restrict__ colpart) {
  __shared__ unsigned sm[256 / kWave][D];
  unsigned m[D];
#pragma unroll
  for (int d = 0; d < D; ++d) m[d] = 0u;
  for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long)gridDim.x * 256) {
    float r[D];
    if (km_load_row<D>(x, n, vec != 0, r)) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const unsigned b = __float_as_uint(r[d]) & 0x7fffffffu;
        m[d] = b > m[d] ? b : m[d];
      }
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
#pragma unroll
    for (int h = kWave / 2; h > 0; h >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)m[d], h, kWave);
      m[d] = o > m[d] ? o : m[d];
    }
    if ((threadIdx.x & (kWave - 1)) == 0) sm[threadIdx.x >> 6][d] = m[d];
  }
  __syncthreads();
  if (threadIdx.x < D) {
    unsigned v = sm[0][threadIdx.x];
    for (int w = 1; w < 256 / kWave; ++w) v = sm[w][threadIdx.x] > v ? sm[w][threadIdx.x] : v;
    colpart[blockIdx.x * kKmMaxD + threadIdx.x] = v;
  }
}

struct KmArgs {
  const float* __restrict__ x;        // [N][D]
  const float* __restrict__ c;        // [K][D]
  int* __restrict__ labels;           // [N] in/out
  float* __restrict__ d2;             // [N] or null
  double* __restrict__ stats;         // [4]: this kernel clears [3]
  void* ws;
  long N;
  int K, S;                           // S: bits of the fixed-point grid below 2^e
  int ncol;                           // blocks of the column-maximum pass (0: none ran)
  int vec, sums, counts, lds;         // 16-byte row loads; add the row sums; add the counts; cells in LDS first
};

template <int D>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const KmArgs a) {
  __shared__ __attribute__((aligned(16))) float ct[kKmTile * D];
  __shared__ long cells[kKmLdsCells];
  __shared__ double sm_in[256 / kWave];
  __shared__ long sm_fin[256 / kWave], sm_mov[256 / kWave];
  __shared__ unsigned sm_col[16][kKmMaxD];
  const int tid = threadIdx.x;
  const int K = a.K;
  const int ncell = K * (D + 1);
  long* __restrict__ gcells = km_cells(a.ws);
  if (a.lds) {
    for (int i = tid; i < ncell; i += 256) cells[i] = 0;
  }
  if (blockIdx.x == 0 && tid == 0) a.stats[3] = 0.0;
  // the column maxima from the partials of the pass before: 16 slices x 16 columns, then the slices in order
  {
    const unsigned* part = km_colpart(a.ws, K, D);
    const int d = tid & (kKmMaxD - 1), slice = tid >> 4;
    unsigned v = 0u;
    if (d < D)
      for (int i = slice; i < a.ncol; i += 16) { const unsigned o = part[i * kKmMaxD + d]; v = o > v ? o : v; }
    sm_col[slice][d] = v;
    __syncthreads();
    if (tid < kKmMaxD) {
      for (int i = 1; i < 16; ++i) v = sm_col[i][tid] > v ? sm_col[i][tid] : v;
      sm_col[0][tid] = v;
      if (blockIdx.x == 0) km_colmax(a.ws)[tid] = v;          // for the update kernel
    }
    __syncthreads();
  }
  double scale[D];
#pragma unroll
  for (int d = 0; d < D; ++d) scale[d] = km_pow2(a.S - km_exp(sm_col[0][d]));
  double inertia = 0.0;
  long fin = 0, mov = 0;

  constexpr long kSpan = 256 * kKmRows;
  for (long base = (long)blockIdx.x * kSpan; base < a.N; base += (long)gridDim.x * kSpan) {
    float r[kKmRows][D];
    long row[kKmRows];
    bool live[kKmRows];
    float best[kKmRows];
    int bk[kKmRows];
#pragma unroll
    for (int j = 0; j < kKmRows; ++j) {
      row[j] = base + j * 256 + tid;
      live[j] = row[j] < a.N;
      km_load_row<D>(a.x, live[j] ? row[j] : a.N - 1, a.vec != 0, r[j]);     // a lane past the end repeats the last row
      best[j] = INFINITY;
      bk[j] = -1;
    }
    for (int k0 = 0; k0 < K; k0 += kKmTile) {
      const int tk = K - k0 < kKmTile ? K - k0 : kKmTile;
      __syncthreads();                                                       // the previous tile (and the cleared cells) are done with
      for (int i = tid; i < tk * D; i += 256) ct[i] = a.c[(size_t)k0 * D + i];
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < tk; ++kk) {
        float cv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) cv[d] = ct[kk * D + d];
#pragma unroll
        for (int j = 0; j < kKmRows; ++j) {
          float d2 = 0.0f;
#pragma unroll
          for (int d = 0; d < D; ++d) { const float t = r[j][d] - cv[d]; d2 = __builtin_fmaf(t, t, d2); }
          if (d2 < best[j]) { best[j] = d2; bk[j] = k0 + kk; }               // centres ascend: strict < keeps the lowest k
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kKmRows; ++j) {
      if (!live[j]) continue;
      const int lab = bk[j];
      const int old = a.labels[row[j]];
      a.labels[row[j]] = lab;
      if (a.d2) a.d2[row[j]] = lab < 0 ? NAN : best[j];
      if (lab < 0) continue;
      fin += 1;
      mov += old != lab ? 1 : 0;
      inertia += (double)best[j];
      if (a.counts) {
        long* cell = (a.lds ? cells : gcells) + (size_t)lab * (D + 1);
        if (a.sums) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
            const long q = __double2ll_rn((double)r[j][d] * scale[d]);
            if (q != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cell + d), (unsigned long long)q);
          }
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(cell + D), 1ull);
      }
    }
  }

  // the block's sums: one add per non-zero cell (integer sums do not depend on the order)
  if (a.lds && a.counts) {
    __syncthreads();
    for (int i = tid; i < ncell; i += 256) {
      const long v = cells[i];
      if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(gcells + i), (unsigned long long)v);
    }
  }
  // statistics: the lanes of a wave by shuffles, then the block's waves in order
#pragma unroll
  for (int h = kWave / 2; h > 0; h >>= 1) {
    inertia += __shfl_down(inertia, h, kWave);
    fin += __shfl_down(fin, h, kWave);
    mov += __shfl_down(mov, h, kWave);
  }
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  if (lane == 0) { sm_in[wave] = inertia; sm_fin[wave] = fin; sm_mov[wave] = mov; }
  __syncthreads();
  if (tid == 0) {
    KmPartial p{sm_in[0], sm_fin[0], sm_mov[0]};
    for (int w = 1; w < 256 / kWave; ++w) { p.inertia += sm_in[w]; p.finite += sm_fin[w]; p.moved += sm_mov[w]; }
    km_partials(a.ws, K, D)[blockIdx.x] = p;
  }
}

// One thread per centre: cells -> new centre (an empty cluster keeps the old one bit for bit), count, shift^2.  Block 0 also
// adds the nb partial statistics in a fixed tree.
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ c, float* __restrict__ newc, long* __restrict__ counts,
                                                            double* __restrict__ stats, void* ws, int K, int D, int S, int nb) {
#pragma clang fp contract(off)      // the two-sum below must stay as written
  const long* __restrict__ cells = km_cells(ws);
  const int k = blockIdx.x * 256 + threadIdx.x;
  double shift = 0.0, comp = 0.0;     // shift^2 as a compensated sum: the D additions cost one rounding, not D
  if (k < K && (newc || counts)) {
    const long cnt = cells[(size_t)k * (D + 1) + D];
    if (counts) counts[k] = cnt;
    if (newc) {
      const unsigned* cm = km_colmax(ws);
      for (int d = 0; d < D; ++d) {
        const float o = c[(size_t)k * D + d];
        float v = o;
        if (cnt > 0) v = (float)((double)cells[(size_t)k * (D + 1) + d] * km_pow2(km_exp(cm[d]) - S) / (double)cnt);
        newc[(size_t)k * D + d] = v;
        const double t = cnt > 0 ? (double)v - (double)o : 0.0;           // an unchanged (possibly non-finite) centre has not moved
        const double p = t * t, pe = fma(t, t, -p);
        const double y = shift + p, bb = y - shift;
        comp += ((shift - (y - bb)) + (p - bb)) + pe;
        shift = y;
      }
    }
  }
  shift += comp;
  if (newc) {
    unsigned long long b = (unsigned long long)__double_as_longlong(shift);     // shift >= 0 or NaN: NaN bits order above every number
#pragma unroll
    for (int h = kWave / 2; h > 0; h >>= 1) {
      const unsigned long long o = (unsigned long long)__shfl_xor((long long)b, h, kWave);
      b = o > b ? o : b;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && b != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(stats + 3), b);
  }
  if (blockIdx.x == 0) {
    __shared__ double t_in[256];
    __shared__ long t_fin[256], t_mov[256];
    const KmPartial* p = km_partials(ws, K, D);
    const int t = threadIdx.x;
    KmPartial v{0.0, 0, 0};
    for (int i = t; i < nb; i += 256) { v.inertia += p[i].inertia; v.finite += p[i].finite; v.moved += p[i].moved; }
    t_in[t] = v.inertia; t_fin[t] = v.finite; t_mov[t] = v.moved;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (t < h) { t_in[t] += t_in[t + h]; t_fin[t] += t_fin[t + h]; t_mov[t] += t_mov[t + h]; }
      __syncthreads();
    }
    if (t == 0) { stats[0] = (double)t_fin[0]; stats[1] = t_in[0]; stats[2] = (double)t_mov[0]; }
  }
}

static int launch_kmeans_step(const float* x, const float* c, int32_t* labels, float* d2, float* newc, int64_t* counts, double* stats,
                       int64_t N, int K, int D, void* ws, hipStream_t s) {
  KmArgs a;
  a.x = x; a.c = c; a.labels = labels; a.d2 = d2; a.stats = stats; a.ws = ws;
  a.N = (long)N; a.K = K;
  int L = 1;
  while (L < 62 && (N >> L) != 0) ++L;                       // N < 2^L
  a.S = 62 - L;
  a.vec = (D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0;
  a.sums = newc ? 1 : 0;
  a.counts = (newc || counts) ? 1 : 0;
  a.lds = K * (D + 1) <= kKmLdsCells ? 1 : 0;
  IRBFN_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)kKmHeadBytes + (size_t)K * (D + 1) * 8, s));
  const int64_t span = 256 * kKmRows;
  const int64_t want = (N + span - 1) / span;
  const int nb = want > kKmBlocksMax ? kKmBlocksMax : (int)want;
  const int64_t wantc = (N + 255) / 256;
  const int nbc = !a.sums ? 0 : (wantc > kKmColBlocks ? kKmColBlocks : (int)wantc);
  a.ncol = nbc;
  const int rc = dispatch<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(D, [&](auto d) {
    if (nbc > 0) {
      const int rcc = launch_kernel<kmeans_colmax_kernel<d()>>(dim3(nbc), dim3(256), 0, s, x, (long)N, a.vec, km_colpart(ws, K, d()));
      if (rcc != IRBFN_OK) return rcc;
    }
    return launch_kernel<kmeans_assign_kernel<d()>>(dim3(nb), dim3(256), 0, s, a);
  });
  if (rc != IRBFN_OK) return rc;
  hipLaunchKernelGGL(kmeans_update_kernel, dim3((K + 255) / 256), dim3(256), 0, s, c, newc, reinterpret_cast<long*>(counts), stats,
                     ws, K, D, a.S, nb);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int64_t irbfn_kmeans_workspace_bytes(int64_t N, int K, int D) {
  if (N < 0 || K < 1 || D < 1) return IRBFN_ERR_BAD_ARG;
  if (K > kKmMaxK || D > kKmMaxD) return IRBFN_ERR_UNSUPPORTED;
  return kmeans_workspace_bytes(N, K, D);
}

int irbfn_kmeans_step(const float* x_dev, const float* centers_dev, int32_t* labels_dev, float* d2_dev, float* new_centers_dev,
                      int64_t* counts_dev, double* stats_dev, int64_t N, int K, int D, void* workspace_dev,
                      int64_t workspace_bytes, void* stream) {
  if (K < 1 || D < 1 || N < 0) return IRBFN_ERR_BAD_ARG;
  if (N > 0 && (!x_dev || !centers_dev || !labels_dev || !stats_dev)) return IRBFN_ERR_BAD_ARG;
  if (K > kKmMaxK || D > kKmMaxD) return IRBFN_ERR_UNSUPPORTED;
  if (N == 0) return IRBFN_OK;
  if (!workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 7) != 0 ||
      workspace_bytes < kmeans_workspace_bytes(N, K, D))
    return IRBFN_ERR_BAD_ARG;
  return launch_kmeans_step(x_dev, centers_dev, labels_dev, d2_dev, new_centers_dev, counts_dev, stats_dev, N, K, D, workspace_dev,
                            reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
