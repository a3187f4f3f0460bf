// K9: the p nearest centres of every row (irbfn_knn_d2, include/irbfn_hip.h; irbfn_amd/widths.py).
//
// The reference leaves the widths of its RBF layers to Adam from log_sig = 0 and has no width rule: parity is unpinned.  What is
// pinned is the arithmetic below, against a float64 statement of it (tests/_widths_util.py).
//
// knn_part_kernel: kmeans_assign_kernel's loop (kmeans.hip) with a list in place of the running minimum.  Two rows per lane
// (their D values in registers), the centres staged kKnnTile at a time in LDS and read as broadcasts, d2 = the float32 chain
// fmaf(t, t, d2) with t = q - c over d = 0 .. D-1 -- bit for bit the chain of irbfn_kmeans_step.  Every row keeps the P smallest
// keys seen so far, P = p rounded up to a power of two, sorted, in registers:
//   key = (bits(d2) << 32) | k.  A sum of squares is +0 or positive, and non-negative floats order as their bits, so keys order as
//   the pair (d2, k): equal d2 goes to the lower k, and the order is total.  An empty slot holds kKnnEmpty = (bits(+Inf) << 32); a
//   candidate enters only if key < the list's worst key, which a NaN (bits above +Inf's, either sign) or an Inf d2 never is.  So
//   non-finite centres and rows with a non-finite component need no test of their own: they leave empty slots.
//   The list is indexed by unrolled compile-time indices only (a runtime index would put it in scratch).  A candidate is first
//   held against the high word of the worst key (one 32-bit compare); after the first tiles almost none pass.
// The centres are cut into nseg segments of whole tiles, grid = (row blocks, nseg).  With one segment the lists are the result
// and are written as d2 / idx.  With more, every (row block, segment) writes its lists to the workspace, [segment][slot][row] so
// that lanes write and read consecutive words, and knn_merge_kernel (one row per lane) inserts the nseg P keys of a row into
// one list in the same way.  The P smallest keys of a union are among the P smallest of its parts and the order is total: the
// result does not depend on the cut.  No atomics; the workspace is written before it is read.
#include "common.h"

namespace irbfn {

constexpr int kKnnMaxD = 16;
constexpr int kKnnMaxK = 65536;
constexpr int kKnnMaxP = 16;
constexpr int kKnnTile = 128;             // centres staged in LDS per pass; a segment is a whole number of them
constexpr int kKnnRows = 2;               // rows per lane
constexpr int kKnnSpan = 256 * kKnnRows;  // rows per block and grid-stride trip
constexpr int kKnnBlocks = 1024;          // split = 0: segments until row blocks x segments reaches this
constexpr int kKnnGridMax = 2048;         // blocks of the list pass; more rows are taken by the grid-stride loop
constexpr unsigned long long kKnnEmpty = 0x7f800000ull << 32;

inline int knn_tiles(int K) { return (K + kKnnTile - 1) / kKnnTile; }
inline int knn_list(int p) { return p <= 1 ? 1 : p <= 2 ? 2 : p <= 4 ? 4 : p <= 8 ? 8 : 16; }

// the segments a call cuts the centres into
inline int knn_segments(int64_t N, int K, int split) {
  const int tiles = knn_tiles(K);
  int64_t want = split;
  if (split == 0) {
    const int64_t rb = (N + kKnnSpan - 1) / kKnnSpan;
    want = rb >= kKnnBlocks ? 1 : kKnnBlocks / (rb < 1 ? 1 : rb);
  }
  const int nseg = want > tiles ? tiles : (int)want;
  const int tps = (tiles + nseg - 1) / nseg;          // tiles per segment
  return (tiles + tps - 1) / tps;                     // no empty segment
}

// lists (of P keys) the workspace holds: none with one segment; split = 0 is bounded by a form that grows with N and K.
// The exact need of split = 0, knn_segments(N, K, 0) * N, falls where a longer table gets fewer segments (4096 rows in 64
// segments, 4097 in 61) and is 0 from 2^19 rows on; the size must not shrink as N grows, so from there on the call asks for
// 2^19 lists it does not touch (4 MiB at P = 1, 64 MiB at P = 16).  A caller who minds passes split = 1, which needs 8 bytes.
inline int64_t knn_workspace_lists(int64_t N, int K, int split) {
  const int64_t tiles = knn_tiles(K);
  if (tiles < 2) return 0;
  if (split == 0) {
    const int64_t cap = (int64_t)kKnnBlocks * kKnnSpan;
    return tiles * N < cap ? tiles * N : cap;
  }
  const int64_t seg = split > tiles ? tiles : split;
  return seg < 2 ? 0 : seg * N;
}

int64_t knn_workspace_bytes(int64_t N, int K, int p, int split) {
  const int64_t bytes = knn_workspace_lists(N, K, split) * knn_list(p) * 8;
  return bytes < 8 ? 8 : bytes;
}

template <int P>
__device__ __forceinline__ void knn_clear(unsigned long long (&list)[P]) {
#pragma unroll
  for (int j = 0; j < P; ++j) list[j] = kKnnEmpty;
}

// key < list[P - 1]: the sorted list takes the key and drops its worst
template <int P>
__device__ __forceinline__ void knn_insert(unsigned long long (&list)[P], unsigned long long key) {
#pragma unroll
  for (int j = P - 1; j > 0; --j) {
    const unsigned long long below = list[j - 1];
    list[j] = key < below ? below : (key < list[j] ? key : list[j]);
  }
  list[0] = key < list[0] ? key : list[0];
}

template <int P>
__device__ __forceinline__ void knn_emit(const unsigned long long (&list)[P], long n, int p, float* __restrict__ d2, int* __restrict__ idx) {
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (j < p) {
      const bool none = list[j] >= kKnnEmpty;
      d2[n * p + j] = none ? NAN : __uint_as_float((unsigned)(list[j] >> 32));
      if (idx) idx[n * p + j] = none ? -1 : (int)(unsigned)list[j];
    }
  }
}

// km_load_row of kmeans.hip without its finite flag.  Not shared: routing K7 through a common loader changes the instruction
// stream of kmeans_colmax_kernel<4, 8, 12, 16> (tools/isa_diff.py), and K7 stays as it was measured.
template <int D>
__device__ __forceinline__ void knn_load_row(const float* __restrict__ x, long n, bool vec, float (&r)[D]) {
  const float* p = x + n * D;
  if constexpr (D % 4 == 0) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < D / 4; ++j) {
        const float4 v = reinterpret_cast<const float4*>(p)[j];
        r[4 * j] = v.x; r[4 * j + 1] = v.y; r[4 * j + 2] = v.z; r[4 * j + 3] = v.w;
      }
      return;
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) r[d] = p[d];
}

struct KnnArgs {
  const float* __restrict__ q;        // [N][D]
  const float* __restrict__ c;        // [K][D]
  float* __restrict__ d2;             // [N][p]
  int* __restrict__ idx;              // [N][p] or null
  unsigned long long* __restrict__ ws;   // [nseg][P][N] with nseg > 1
  long N, self0;
  int K, p, nseg, tps, vec;           // tps: tiles per segment
};

template <int D, int P>
__global__ __launch_bounds__(256) void knn_part_kernel(const KnnArgs a) {
  __shared__ __attribute__((aligned(16))) float ct[kKnnTile * D];
  const int tid = threadIdx.x;
  const int seg = blockIdx.y;
  const int kbeg = seg * a.tps * kKnnTile;
  const int kend = a.K - kbeg < a.tps * kKnnTile ? a.K : kbeg + a.tps * kKnnTile;
  for (long base = (long)blockIdx.x * kKnnSpan; base < a.N; base += (long)gridDim.x * kKnnSpan) {
    float r[kKnnRows][D];
    long row[kKnnRows];
    int self[kKnnRows];
    unsigned long long list[kKnnRows][P];
#pragma unroll
    for (int j = 0; j < kKnnRows; ++j) {
      row[j] = base + j * 256 + tid;
      const long src = row[j] < a.N ? row[j] : a.N - 1;                     // a lane past the end repeats the last row
      knn_load_row<D>(a.q, src, a.vec != 0, r[j]);
      const long sk = a.self0 + src;
      self[j] = (a.self0 >= 0 && sk < (long)a.K) ? (int)sk : -1;
      knn_clear<P>(list[j]);
    }
    for (int k0 = kbeg; k0 < kend; k0 += kKnnTile) {
      const int tk = kend - k0 < kKnnTile ? kend - k0 : kKnnTile;
      __syncthreads();                                                      // the previous tile is done with
      for (int i = tid; i < tk * D; i += 256) ct[i] = a.c[(size_t)k0 * D + i];
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < tk; ++kk) {
        float cv[D];
#pragma unroll
        for (int d = 0; d < D; ++d) cv[d] = ct[kk * D + d];
#pragma unroll
        for (int j = 0; j < kKnnRows; ++j) {
          float d2 = 0.0f;
#pragma unroll
          for (int d = 0; d < D; ++d) { const float t = r[j][d] - cv[d]; d2 = __builtin_fmaf(t, t, d2); }
          const unsigned bits = __float_as_uint(d2);
          if (bits <= (unsigned)(list[j][P - 1] >> 32)) {
            const int k = k0 + kk;
            const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned)k;
            if (key < list[j][P - 1] && k != self[j]) knn_insert<P>(list[j], key);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kKnnRows; ++j) {
      if (row[j] >= a.N) continue;
      if (a.nseg == 1) {
        knn_emit<P>(list[j], row[j], a.p, a.d2, a.idx);
      } else {
#pragma unroll
        for (int s = 0; s < P; ++s) a.ws[((size_t)seg * P + s) * (size_t)a.N + (size_t)row[j]] = list[j][s];
      }
    }
  }
}

template <int P>
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long* __restrict__ ws, long N, int nseg, int p,
                                                        float* __restrict__ d2, int* __restrict__ idx) {
  for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long)gridDim.x * 256) {
    unsigned long long list[P];
    knn_clear<P>(list);
    for (int seg = 0; seg < nseg; ++seg) {
#pragma unroll
      for (int s = 0; s < P; ++s) {
        const unsigned long long key = ws[((size_t)seg * P + s) * (size_t)N + (size_t)n];
        if (key < list[P - 1]) knn_insert<P>(list, key);
      }
    }
    knn_emit<P>(list, n, p, d2, idx);
  }
}

static int launch_knn(const float* q, const float* c, int64_t N, int K, int D, int p, int64_t self0, int split, float* d2, int32_t* idx,
                      void* ws, hipStream_t s) {
  KnnArgs a;
  a.q = q; a.c = c; a.d2 = d2; a.idx = idx;
  a.ws = static_cast<unsigned long long*>(ws);
  a.N = (long)N; a.self0 = self0 >= K ? -1 : (long)self0; a.K = K; a.p = p;      // self0 + n >= K for every row: nothing to exclude
  a.nseg = knn_segments(N, K, split);
  a.tps = (knn_tiles(K) + a.nseg - 1) / a.nseg;
  a.vec = (D % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) ? 1 : 0;
  const int64_t rb = (N + kKnnSpan - 1) / kKnnSpan;
  const int64_t room = kKnnGridMax / a.nseg < 1 ? 1 : kKnnGridMax / a.nseg;
  const int gx = (int)(rb < room ? rb : room);
  const int P = knn_list(p);
  int rc = dispatch<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(D, [&](auto d) {
    return dispatch<1, 2, 4, 8, 16>(P, [&](auto pp) {
      return launch_kernel<knn_part_kernel<d(), pp()>>(dim3(gx, a.nseg), dim3(256), 0, s, a);
    });
  });
  if (rc != IRBFN_OK || a.nseg == 1) return rc;
  const int64_t mrows = (N + 255) / 256;
  const unsigned mb = (unsigned)(mrows < kKnnGridMax ? mrows : kKnnGridMax);       // more rows: the grid-stride loop
  return dispatch<1, 2, 4, 8, 16>(P, [&](auto pp) {
    return launch_kernel<knn_merge_kernel<pp()>>(dim3(mb), dim3(256), 0, s, (const unsigned long long*)a.ws, (long)N, a.nseg, p, d2, idx);
  });
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int64_t irbfn_knn_workspace_bytes(int64_t N, int K, int D, int p, int split) {
  if (N < 0 || K < 1 || D < 1 || p < 1 || split < 0) return IRBFN_ERR_BAD_ARG;
  if (K > kKnnMaxK || D > kKnnMaxD || p > kKnnMaxP) return IRBFN_ERR_UNSUPPORTED;
  return knn_workspace_bytes(N, K, p, split);
}

int irbfn_knn_d2(const float* q_dev, const float* c_dev, int64_t N, int K, int D, int p, int64_t self0, int split, float* d2_dev,
                 int32_t* idx_dev, void* ws_dev, int64_t ws_bytes, void* stream) {
  if (K < 1 || D < 1 || p < 1 || N < 0 || self0 < -1 || split < 0) return IRBFN_ERR_BAD_ARG;
  if (N > 0 && (!q_dev || !c_dev || !d2_dev || !ws_dev || (reinterpret_cast<uintptr_t>(ws_dev) & 7) != 0)) return IRBFN_ERR_BAD_ARG;
  if (K > kKnnMaxK || D > kKnnMaxD || p > kKnnMaxP) return IRBFN_ERR_UNSUPPORTED;
  if (N == 0) return IRBFN_OK;
  if (ws_bytes < knn_workspace_bytes(N, K, p, split)) return IRBFN_ERR_BAD_ARG;      // a size exists for supported shapes only
  return launch_knn(q_dev, c_dev, N, K, D, p, self0, split, d2_dev, idx_dev, ws_dev, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
