// Batched planner front / back end: what surrounds pred_step in the reference planners.
//   * query construction + mirror trick of IRBFNPlanner.plan (src/irbfn_mpc/irbfn_planner.py:181-208) and
//     IRBFNFrenetPlanner.plan (:456-492), one lane per (pose, goal) pair, float64 like the NumPy host
//     code it replaces, float32 out (jnp.array(...) under the default x64-off config);
//   * the sign flip of the steer-velocity controls of mirrored rows (:203-204, :487-488);
//   * the explicit-MPC table look-ups the learned network is benchmarked against:
//     per-axis searchsorted grid lookup (src/irbfn_mpc/explicit_planner.py:165-175) and the exact nearest
//     neighbour (scipy KDTree.query at :383; brute force here -- HBM-bound streaming of the table).
#include <math.h>
#include <string.h>

#include "common.h"
#include "planner_geom.h"

namespace irbfn {

__global__ __launch_bounds__(256) void plan_queries_cartesian_kernel(const double* __restrict__ pose,
                                                                     const double* __restrict__ goal,
                                                                     float* __restrict__ x_out,
                                                                     float* __restrict__ state0_out,
                                                                     int* __restrict__ mirror_out, long B) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double p[7], g[4];
  float xo[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) p[i] = pose[b * 7 + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) g[i] = goal[b * 4 + i];
  const bool m = cartesian_query(p, g, xo);
#pragma unroll
  for (int i = 0; i < 7; ++i) x_out[b * 7 + i] = xo[i];
  if (state0_out) {
#pragma unroll
    for (int i = 0; i < 7; ++i) state0_out[b * 7 + i] = (float)p[i];
  }
  mirror_out[b] = m ? 1 : 0;
}

__global__ __launch_bounds__(256) void plan_queries_frenet_kernel(const double* __restrict__ fr,
                                                                  const double* __restrict__ vx_goal,
                                                                  float* __restrict__ x_out,
                                                                  float* __restrict__ state0_out,
                                                                  int* __restrict__ mirror_out, long B) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double p[8];
  float xo[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = fr[b * 8 + i];
  const bool m = frenet_query(p, vx_goal[b], xo);
#pragma unroll
  for (int i = 0; i < 8; ++i) x_out[b * 8 + i] = xo[i];
  if (state0_out) {
#pragma unroll
    for (int i = 0; i < 8; ++i) state0_out[b * 8 + i] = (float)p[i];
  }
  mirror_out[b] = m ? 1 : 0;
}

__global__ __launch_bounds__(256) void unmirror_kernel(float* __restrict__ controls, const int* __restrict__ mirror,
                                                       long B, int O, int sv0) {
  const int w = O - sv0;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * w) return;
  const long b = i / w;
  const int o = sv0 + (int)(i - b * w);
  if (mirror[b] != 0) controls[b * O + o] = -controls[b * O + o];
}

int launch_unmirror(float* controls, const int* mirror, int64_t B, int O, int sv0, hipStream_t s) {
  const long n = (long)B * (O - sv0);
  if (n <= 0) return IRBFN_OK;
  hipLaunchKernelGGL(unmirror_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, controls, mirror, (long)B, O,
                     sv0);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

// ---- grid look-up: idx_d = min(shape_d - 1, searchsorted(keys_d, x_d, side="right"))   explicit_planner.py:165-172
constexpr int kLutMaxD = 16;
struct LutGrid {
  int off[kLutMaxD + 1];     // keys of axis d are keys[off[d] .. off[d+1])
  int shape[kLutMaxD];       // table shape per axis (row-major, last axis fastest)
};

__global__ __launch_bounds__(256) void lut_grid_lookup_kernel(const double* __restrict__ keys, const LutGrid g,
                                                              const float* __restrict__ table,
                                                              const double* __restrict__ x, long* __restrict__ idx_out,
                                                              float* __restrict__ out, long B, int D, int OW) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  long flat = 0;
  for (int d = 0; d < D; ++d) {
    const double v = x[b * D + d];
    int lo = g.off[d], hi = g.off[d + 1];         // first index with keys[i] > v  (side="right")
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] <= v) lo = mid + 1;           // NaN compares false -> lo stays: searchsorted sorts NaN last
      else hi = mid;
    }
    int i = lo - g.off[d];
    if (v != v) i = g.off[d + 1] - g.off[d];      // NaN -> len(keys), as numpy
    if (i > g.shape[d] - 1) i = g.shape[d] - 1;
    flat = flat * g.shape[d] + i;
  }
  idx_out[b] = flat;
  if (out) {
    const float* row = table + flat * OW;
    for (int o = 0; o < OW; ++o) out[b * OW + o] = row[o];
  }
}

// ---- exact nearest neighbour: argmin_n ||inputs[n] - x_b||  (ties -> lowest n; no finite distance -> idx -1, NaN)
// One lane per table row, grid-stride; the QT queries of a tile are wave-uniform (scalar loads); per-block
// (d2, n) minima go to a [B][nblocks] slab, a second kernel takes the fixed-order minimum: deterministic.
template <int D, int QT>
__global__ __launch_bounds__(256) void lut_nearest_kernel(const float* __restrict__ inputs, const float* __restrict__ x,
                                                          float* __restrict__ part_d, long* __restrict__ part_i, long N,
                                                          long B, int nblocks) {
  __shared__ float sd[4][QT];
  __shared__ long si[4][QT];
  const long q0 = (long)blockIdx.y * QT;
  float best[QT];
  long bidx[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) { best[q] = INFINITY; bidx[q] = 0x7fffffffffffffffL; }
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
    float r[D];
#pragma unroll
    for (int d = 0; d < D; ++d) r[d] = inputs[n * D + d];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const long qb = q0 + q < B ? q0 + q : B - 1;
      float d2 = 0.0f;
#pragma unroll
      for (int d = 0; d < D; ++d) { const float t = r[d] - x[qb * D + d]; d2 = __builtin_fmaf(t, t, d2); }
      if (d2 < best[q]) { best[q] = d2; bidx[q] = n; }     // rows ascend per lane: strict < keeps the lowest n
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    float bd = best[q];
    long bi = bidx[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float od = __shfl_xor(bd, off);
      const long oi = __shfl_xor(bi, off);
      if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) { sd[wave][q] = bd; si[wave][q] = bi; }
  }
  __syncthreads();
  if (threadIdx.x < QT && q0 + threadIdx.x < B) {
    const int q = threadIdx.x;
    float bd = sd[0][q];
    long bi = si[0][q];
    for (int w = 1; w < 4; ++w)
      if (sd[w][q] < bd || (sd[w][q] == bd && si[w][q] < bi)) { bd = sd[w][q]; bi = si[w][q]; }
    part_d[(q0 + q) * nblocks + blockIdx.x] = bd;
    part_i[(q0 + q) * nblocks + blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(64) void lut_nearest_final_kernel(const float* __restrict__ part_d,
                                                               const long* __restrict__ part_i, int nblocks,
                                                               const float* __restrict__ table, long* __restrict__ idx_out,
                                                               float* __restrict__ dist_out, float* __restrict__ out,
                                                               int OW) {
  const long b = blockIdx.x;
  const int lane = threadIdx.x;
  float bd = INFINITY;
  long bi = 0x7fffffffffffffffL;
  for (int k = lane; k < nblocks; k += 64) {
    const float d = part_d[b * nblocks + k];
    const long i = part_i[b * nblocks + k];
    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float od = __shfl_xor(bd, off);
    const long oi = __shfl_xor(bi, off);
    if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
  }
  const bool none = bi == 0x7fffffffffffffffL;   // no row compared below infinity (NaN / Inf query, or an overflowing d2)
  if (lane == 0) {
    idx_out[b] = none ? -1L : bi;
    if (dist_out) dist_out[b] = none ? NAN : sqrtf(bd);
  }
  if (out && table)
    for (int o = lane; o < OW; o += 64) out[b * OW + o] = none ? NAN : table[bi * OW + o];
}

}  // namespace irbfn

using namespace irbfn;

// ---- way-point geometry of the pure-pursuit front end (src/irbfn_mpc/planner_utils.py:109-240) -----------------
// The reference runs nearest_point / intersect_point once per planner tick under numba; here they are batched over B
// query points against ONE piecewise-linear trajectory, one wave per point.  The arithmetic types
// follow the reference line by line: float32 segment vectors / squared lengths / dot products, float64 everything
// else in nearest_point (:125-141); float32 trajectory, +1e-6f end points, float32 t in intersect_point (:160-170),
// with the point kept in float64 as the callers pass it.  numba's typing of the mixed expressions cannot be
// checked here (numba is not importable): parity unpinned, tested against the NumPy statement of the same lines.
struct WayArgs {
  const double* __restrict__ pts;    // [B][2]
  const double* __restrict__ traj;   // [N][2]
  long B;
  int N;
};

// One WAVE per point: the lanes take the segments lane, lane + 64, ... and the wave picks the smallest distance (the
// smallest segment index among equal distances: np.argmin's first minimum).  A segment whose distance is NaN (a repeated
// way-point: t = 0/0; a NaN way-point) is skipped, where np.argmin returns the first NaN: a deliberate departure, stated in the
// oracle as nearest_point(skip_nan=True).  (One thread per point walking all N
// segments with a float64 divide and square root each took 200 us at ANY batch size -- the planner calls this with one
// point per tick.)
__global__ __launch_bounds__(256) void nearest_point_kernel(const WayArgs a, double* __restrict__ proj,
                                                            double* __restrict__ dist, double* __restrict__ tt,
                                                            int* __restrict__ seg) {
#pragma clang fp contract(off)                   // every product of the reference's lines is rounded before its sum
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                          // the whole wave
  const double* __restrict__ wp = a.traj;
  const double px = a.pts[2 * b], py = a.pts[2 * b + 1];
  double best = INFINITY, bt = 0.0, bx = 0.0, by = 0.0;
  int bi = 0x7fffffff;
  for (int i = lane; i + 1 < a.N; i += 64) {
    double d, t, qx, qy;
    segment_distance<2>(wp, i, px, py, d, t, qx, qy);
    if (d < best) { best = d; bt = t; bx = qx; by = qy; bi = i; }                        // first minimum of this lane's segments
  }
  double gbest = best;
  int gbi = bi;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(gbest, off);
    const int oi = __shfl_xor(gbi, off);
    if (od < gbest || (od == gbest && oi < gbi)) { gbest = od; gbi = oi; }
  }
  if (gbi == 0x7fffffff) {                       // no segment compared below infinity (all NaN): the scalar loop's defaults
    if (lane == 0) { proj[2 * b] = 0.0; proj[2 * b + 1] = 0.0; dist[b] = INFINITY; tt[b] = 0.0; seg[b] = 0; }
  } else if (bi == gbi) {
    proj[2 * b] = bx; proj[2 * b + 1] = by;
    dist[b] = best; tt[b] = bt; seg[b] = bi;
  }
}

// One wave per point: the search order of the reference (segments start_i .. N - 2, then, with wrap, -1 .. start_i - 1) is
// walked 64 segments at a time; the first round with a hit ends the search and its lowest lane is the first intersection.
__global__ __launch_bounds__(256) void intersect_point_kernel(const WayArgs a, const double* __restrict__ t0, float radius,
                                                              int wrap, float* __restrict__ first_p, int* __restrict__ first_i,
                                                              float* __restrict__ first_t, int* __restrict__ found) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                          // the whole wave
  const double* __restrict__ wp = a.traj;
  const double px = a.pts[2 * b], py = a.pts[2 * b + 1];
  const double ts = t0 ? t0[b] : 0.0;
  const HitOrder order(ts, a.N, wrap);
  float t = NAN, qx = NAN, qy = NAN;                                                     // (None, None, None)
  int fi = 0, hit = 0;
  for (int base = 0; base < order.total(); base += 64) {
    int i;
    const bool h = order.probe<2>(wp, a.N, base + lane, px, py, radius, i, t, qx, qy);
    const unsigned long long m = __ballot(h);
    if (m != 0ull) {
      const int src = __ffsll((long long)m) - 1;                                         // the first hit in search order
      t = __shfl(t, src); qx = __shfl(qx, src); qy = __shfl(qy, src); fi = __shfl(i, src);
      hit = 1;
      break;
    }
    t = NAN; qx = NAN; qy = NAN;
  }
  if (lane == 0) {
    found[b] = hit;
    first_i[b] = fi;
    first_t[b] = t;
    first_p[2 * b] = qx;
    first_p[2 * b + 1] = qy;
  }
}

extern "C" {

int irbfn_plan_queries_cartesian(const double* pose_dev, const double* goal_dev, float* x_dev, float* state0_dev,
                                 int32_t* mirror_dev, int64_t B, void* stream) {
  if (B < 0) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!pose_dev || !goal_dev || !x_dev || !mirror_dev) return IRBFN_ERR_BAD_ARG;
  hipLaunchKernelGGL(plan_queries_cartesian_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), pose_dev, goal_dev, x_dev, state0_dev, mirror_dev, (long)B);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

int irbfn_plan_queries_frenet(const double* frenet_dev, const double* vx_goal_dev, float* x_dev, float* state0_dev,
                              int32_t* mirror_dev, int64_t B, void* stream) {
  if (B < 0) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!frenet_dev || !vx_goal_dev || !x_dev || !mirror_dev) return IRBFN_ERR_BAD_ARG;
  hipLaunchKernelGGL(plan_queries_frenet_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), frenet_dev, vx_goal_dev, x_dev, state0_dev, mirror_dev,
                     (long)B);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

int irbfn_lut_grid_lookup(const double* keys_dev, const int32_t* key_offsets_host, const int32_t* shape_host,
                          const float* table_dev, const double* x_dev, int64_t* idx_dev, float* out_dev, int64_t B,
                          int D, int OW, void* stream) {
  if (B < 0 || D < 1 || D > kLutMaxD || OW < 0) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!keys_dev || !key_offsets_host || !shape_host || !x_dev || !idx_dev || (out_dev && !table_dev))
    return IRBFN_ERR_BAD_ARG;
  LutGrid g;
  memset(&g, 0, sizeof(g));
  for (int d = 0; d <= D; ++d) g.off[d] = key_offsets_host[d];
  for (int d = 0; d < D; ++d) {
    g.shape[d] = shape_host[d];
    if (g.shape[d] < 1 || g.off[d + 1] < g.off[d]) return IRBFN_ERR_BAD_ARG;
  }
  hipLaunchKernelGGL(lut_grid_lookup_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), keys_dev, g, table_dev, x_dev,
                     reinterpret_cast<long*>(idx_dev), out_dev, (long)B, D, OW);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

int64_t irbfn_lut_nearest_workspace_bytes(int64_t N, int64_t B) {
  if (N < 0 || B < 0) return -1;
  const int nblocks = 2048;
  return (int64_t)B * nblocks * (int64_t)(sizeof(float) + sizeof(long));
}

int irbfn_lut_nearest(const float* inputs_dev, const float* table_dev, const float* x_dev, int64_t* idx_dev,
                      float* dist_dev, float* out_dev, int64_t N, int64_t B, int D, int OW, void* ws_dev,
                      int64_t ws_bytes, void* stream) {
  if (N < 1 || B < 0 || OW < 0) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!inputs_dev || !x_dev || !idx_dev || !ws_dev || (out_dev && !table_dev)) return IRBFN_ERR_BAD_ARG;
  // the scan puts ceil(B / 8) query tiles on gridDim.y and the final kernel B blocks on gridDim.x: the device's limits
  int dev = 0, max_y = 0, max_x = 0;
  IRBFN_HIP_CHECK(hipGetDevice(&dev));
  IRBFN_HIP_CHECK(hipDeviceGetAttribute(&max_y, hipDeviceAttributeMaxGridDimY, dev));   // hipDeviceProp_t::maxGridSize[1]
  IRBFN_HIP_CHECK(hipDeviceGetAttribute(&max_x, hipDeviceAttributeMaxGridDimX, dev));
  if ((B + 7) / 8 > (int64_t)max_y || B > (int64_t)max_x) return IRBFN_ERR_BAD_ARG;
  if (ws_bytes < irbfn_lut_nearest_workspace_bytes(N, B)) return IRBFN_ERR_BAD_ARG;
  const int cap = 2048;
  long want = (N + 255) / 256;
  const int nblocks = (int)(want < cap ? want : cap);
  float* pd = reinterpret_cast<float*>(ws_dev);
  long* pi = reinterpret_cast<long*>(reinterpret_cast<char*>(ws_dev) + (size_t)B * cap * sizeof(float));
  // 8-byte alignment of the index slab: B * cap * 4 is a multiple of 8 because cap is even
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  constexpr int QT = 8;
  const int rc = dispatch<3, 4, 7, 8>(D, [&](auto d) {
    return launch_kernel<lut_nearest_kernel<d(), QT>>(dim3((unsigned)nblocks, (unsigned)((B + QT - 1) / QT)), dim3(256), 0, s, inputs_dev,
                                                     x_dev, pd, pi, (long)N, (long)B, nblocks);
  });
  if (rc != IRBFN_OK) return rc;
  hipLaunchKernelGGL(lut_nearest_final_kernel, dim3((unsigned)B), dim3(64), 0, s, pd, pi, nblocks, table_dev,
                     reinterpret_cast<long*>(idx_dev), dist_dev, out_dev, OW);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}


/* planner_utils.py:109-146 and :149-233, batched over B query points against one trajectory (see the kernels). */
int irbfn_nearest_point(const double* points_dev, const double* trajectory_dev, double* proj_dev, double* dist_dev,
                        double* t_dev, int32_t* seg_dev, int64_t B, int N, void* stream) {
  if (B < 0 || N < 2) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!points_dev || !trajectory_dev || !proj_dev || !dist_dev || !t_dev || !seg_dev) return IRBFN_ERR_BAD_ARG;
  WayArgs a{points_dev, trajectory_dev, (long)B, N};
  hipLaunchKernelGGL(nearest_point_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     a, proj_dev, dist_dev, t_dev, seg_dev);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

int irbfn_intersect_point(const double* points_dev, const double* trajectory_dev, const double* t_start_dev, float radius,
                          int wrap, float* first_p_dev, int32_t* first_i_dev, float* first_t_dev, int32_t* found_dev,
                          int64_t B, int N, void* stream) {
  if (B < 0 || N < 2) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!points_dev || !trajectory_dev || !first_p_dev || !first_i_dev || !first_t_dev || !found_dev) return IRBFN_ERR_BAD_ARG;
  WayArgs a{points_dev, trajectory_dev, (long)B, N};
  hipLaunchKernelGGL(intersect_point_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     a, t_start_dev, radius, wrap, first_p_dev, first_i_dev, first_t_dev, found_dev);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

}  // extern "C"
