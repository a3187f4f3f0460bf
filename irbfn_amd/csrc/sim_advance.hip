// Closed-loop simulation, the part of a planning tick that is not the net (include/irbfn_hip.h: irbfn_sim_advance): plant
// step(s) -> way-point search in a window around the car's last segment -> statistics -> look-ahead goal -> next query.
// Composed from the stand-alone entry points this is six launches and several gathers per tick, and the full-track search
// (B x N segment distances with a float64 divide and square root each) costs more than the net it feeds.
//
// G lanes per car (64 / G cars per wave); the library runs G = kSimLanes = 16 (8 and 64 lose: tools/ab_sim_lanes.hip,
// profiles/closed_loop_ab.txt).  The lanes of a group share the segments of the window and of the intersection
// search; everything else (plant, statistics, query) is a few hundred instructions that every lane of the group evaluates on
// the same values -- in lockstep that costs what one lane costs, and no value has to be handed from the first lane to the
// others -- and the group's first lane stores.  A group's lanes never diverge from each other: every branch and loop bound
// below is a function of the car alone, so the shuffles and ballots inside them always find their partner lanes active.
#include <math.h>

#include "common.h"
#include "planner_geom.h"
#include "rollout_step.h"

namespace irbfn {

constexpr int kSimRecord = 7;    // doubles per car: ticks, sum_d2, max_d, sum_dv, progress, s_last, fail_tick
enum SimRec : int { SR_TICKS = 0, SR_SUM_D2, SR_MAX_D, SR_SUM_DV, SR_PROGRESS, SR_S_LAST, SR_FAIL_TICK };

struct SimArgs {
  irbfn_sim_track tr;
  const float* __restrict__ controls;   // [B][2T] or null
  const float* __restrict__ dyn_dev;    // [B][13] or null
  DynParams dp;                         // the shared row (dyn_dev null)
  int T, n_sub, tick;
  float* __restrict__ state;
  int* __restrict__ seg;
  int* __restrict__ status;
  double* __restrict__ record;
  float* __restrict__ x;
  int* __restrict__ mirror;
  double* __restrict__ goal;            // optional
  double* __restrict__ dist;            // optional
  double* __restrict__ tt;              // optional
  long B;
};

// The window of step 2 as positions 0 .. count - 1; seg(ord) visits each segment of the window once.
struct SimWindow {
  int first, count, M;
  bool wrap;
  __device__ __forceinline__ SimWindow(const irbfn_sim_track& tr, int last) {
    M = tr.N - 1;                                          // segments of the polyline
    wrap = tr.wrap != 0;
    const int s = last < 0 ? 0 : (last > M - 1 ? M - 1 : last);
    const long w = (long)tr.win_back + (long)tr.win_fwd + 1;
    if (tr.win_back < 0 || (wrap && w >= (long)M)) {       // every segment
      first = 0;
      count = M;
      wrap = false;
    } else if (wrap) {
      first = (int)((((long)s - tr.win_back) % M + M) % M);
      count = (int)w;
    } else {
      const long lo = (long)s - tr.win_back < 0 ? 0 : (long)s - tr.win_back;
      const long hi = (long)s + tr.win_fwd > M - 1 ? M - 1 : (long)s + tr.win_fwd;
      first = (int)lo;
      count = (int)(hi - lo + 1);
    }
  }
  __device__ __forceinline__ int seg(int ord) const {
    const int i = first + ord;
    return wrap && i >= M ? i - M : i;
  }
};

template <int G, bool SELECT>
__global__ __launch_bounds__(256) void sim_advance_kernel(const SimArgs a) {
#pragma clang fp contract(off)                   // the statistics and every shared body: each product rounded before its sum
  constexpr int CPB = 256 / G;                   // cars per block
  const int gl = threadIdx.x & (G - 1);          // lane of the group
  const long b = (long)blockIdx.x * CPB + threadIdx.x / G;
  if (b >= a.B) return;                          // the whole group
  if (a.status[b] != IRBFN_SIM_OK) return;       // frozen: nothing read, nothing written
  const bool lead = gl == 0;
  const int N = a.tr.N;
  const double* __restrict__ wp = a.tr.waypoints_dev;

  float s[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) s[i] = a.state[b * 7 + i];

  // ---- 1. plant
  if (a.controls) {
    DynParams dp = a.dp;
    if (a.dyn_dev) {
#pragma unroll
      for (int i = 0; i < 13; ++i) dp.p[i] = a.dyn_dev[b * 13 + i];
    }
    dp.p[8] = dp.p[8] / (float)a.n_sub;          // n_sub = 1: the same bits
    const float ua = a.controls[b * 2 * a.T], us = a.controls[b * 2 * a.T + a.T];
#pragma unroll 1
    for (int k = 0; k < a.n_sub; ++k) st_step<SELECT>(s, ua, us, dp);
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) finite = finite && (fabsf(s[i]) < INFINITY);
    if (lead) {
#pragma unroll
      for (int i = 0; i < 7; ++i) a.state[b * 7 + i] = s[i];
    }
    if (!finite) {
      if (lead) {
        a.status[b] = IRBFN_SIM_NONFINITE;
        a.record[b * kSimRecord + SR_FAIL_TICK] = (double)a.tick;
      }
      return;
    }
  }

  // ---- 2. nearest segment of the window: the (distance, index) order of nearest_point_kernel, within the lane too (a window
  // across the seam does not visit its segments in index order)
  const double px = (double)s[0], py = (double)s[1];
  const SimWindow win(a.tr, a.seg[b]);
  double best = INFINITY, bt = 0.0;
  int bi = 0x7fffffff;
  for (int ord = gl; ord < win.count; ord += G) {
    const int i = win.seg(ord);
    double d, t, qx, qy;
    segment_distance<4>(wp, i, px, py, d, t, qx, qy);
    if (d < best || (d == best && d < INFINITY && i < bi)) { best = d; bt = t; bi = i; }   // an infinite distance is never taken
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const double od = __shfl_xor(best, off);
    const double ot = __shfl_xor(bt, off);
    const int oi = __shfl_xor(bi, off);
    if (od < best || (od == best && oi < bi)) { best = od; bt = ot; bi = oi; }
  }
  if (bi == 0x7fffffff) { best = INFINITY; bt = 0.0; bi = 0; }   // nothing comparable: the scalar loop's defaults
  const double d = best, t = bt;
  const int i = bi;

  // ---- 3. statistics
  double* __restrict__ rec = a.record + b * kSimRecord;
  const double ticks0 = rec[SR_TICKS];
  const double sum_d2 = rec[SR_SUM_D2] + d * d;
  const double max0 = rec[SR_MAX_D];
  const double max_d = d > max0 ? d : max0;      // max(max_d, d) as Python's: a NaN never replaces
  const double dv = (double)s[3] - wp[4 * i + 3];
  const double sum_dv = rec[SR_SUM_DV] + fabs(dv);
  const double sarc = a.tr.cum_dev[i] + t * a.tr.len_dev[i];
  double progress = rec[SR_PROGRESS];
  if (ticks0 != 0.0) {
    double e = sarc - rec[SR_S_LAST];
    if (a.tr.wrap) {
      const double half = a.tr.length / 2.0;
      if (e > half) e = e - a.tr.length;
      else if (e <= -half) e = e + a.tr.length;
    }
    progress = progress + e;
  }
  if (lead) {
    rec[SR_TICKS] = ticks0 + 1.0;
    rec[SR_SUM_D2] = sum_d2;
    rec[SR_MAX_D] = max_d;
    rec[SR_SUM_DV] = sum_dv;
    rec[SR_PROGRESS] = progress;
    rec[SR_S_LAST] = sarc;
  }

  // ---- 4. off track
  int stop = IRBFN_SIM_OK;
  if (a.tr.half_width > 0.0 && d > a.tr.half_width) stop = IRBFN_SIM_OFF_TRACK;

  // ---- 5. goal
  int gi = i;
  if (stop == IRBFN_SIM_OK) {
    if (d < a.tr.lookahead) {
      const HitOrder order((double)i + t, N, a.tr.wrap);
      const float radius = (float)a.tr.lookahead;
      const int g0 = (threadIdx.x & 63) & ~(G - 1);              // the group's first lane in the wave
      const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull) << g0;
      bool hit = false;
      for (int base = 0; base < order.total(); base += G) {
        int si;
        float ht, hx, hy;
        const bool h = order.probe<4>(wp, N, base + gl, px, py, radius, si, ht, hx, hy);
        const unsigned long long m = __ballot(h) & gmask;
        if (m != 0ull) {
          gi = __shfl(si, __ffsll((long long)m) - 1);            // the first hit in search order
          hit = true;
          break;
        }
      }
      if (hit) gi = (gi + N) % N;
      else stop = IRBFN_SIM_LOST;
    } else if (!(d < a.tr.max_reacquire)) {
      stop = IRBFN_SIM_LOST;
    }
  }
  if (stop != IRBFN_SIM_OK) {
    if (lead) {
      a.status[b] = stop;
      rec[SR_FAIL_TICK] = (double)a.tick;
    }
    return;
  }

  // ---- 6. query
  double pose[7], g[4];
  float xo[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) pose[k] = (double)s[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = wp[4 * gi + k];
  const bool m = cartesian_query(pose, g, xo);
  if (lead) {
#pragma unroll
    for (int k = 0; k < 7; ++k) a.x[b * 7 + k] = xo[k];
    a.mirror[b] = m ? 1 : 0;
    a.seg[b] = i;
    if (a.goal) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a.goal[b * 4 + k] = g[k];
    }
    if (a.dist) a.dist[b] = d;
    if (a.tt) a.tt[b] = t;
  }
}

constexpr int kSimLanes = 16;

template <int G>
static int launch_sim(const SimArgs& a, bool select, hipStream_t s) {
  const dim3 grid((unsigned)((a.B + 256 / G - 1) / (256 / G)));
  if (select) return launch_kernel<sim_advance_kernel<G, true>>(grid, dim3(256), 0, s, a);
  return launch_kernel<sim_advance_kernel<G, false>>(grid, dim3(256), 0, s, a);
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int irbfn_sim_record_doubles(void) { return kSimRecord; }

int irbfn_sim_advance(const irbfn_sim_track* track, int mode, int tick, const float* controls_dev, int T,
                      const float* dyn_params_host, const float* dyn_params_dev, int n_sub, float* state_dev, int32_t* seg_dev,
                      int32_t* status_dev, double* record_dev, float* x_dev, int32_t* mirror_dev, double* goal_dev,
                      double* dist_dev, double* t_dev, int64_t B, void* stream) {
  if (!track || B < 0 || track->N < 2 || n_sub < 1) return IRBFN_ERR_BAD_ARG;
  if (track->win_back < -1 || track->win_fwd < -1 || ((track->win_back == -1) != (track->win_fwd == -1)))
    return IRBFN_ERR_BAD_ARG;
  if (mode != IRBFN_ROLLOUT_ST_SELECT && mode != IRBFN_ROLLOUT_ST_KS) return IRBFN_ERR_BAD_ARG;
  if (controls_dev && T < 1) return IRBFN_ERR_BAD_ARG;
  if (!(track->lookahead >= 0.0) || !(track->max_reacquire >= 0.0) || track->half_width != track->half_width)
    return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!track->waypoints_dev || !track->cum_dev || !track->len_dev || !state_dev || !seg_dev || !status_dev || !record_dev ||
      !x_dev || !mirror_dev)
    return IRBFN_ERR_BAD_ARG;
  if (controls_dev && !dyn_params_host && !dyn_params_dev) return IRBFN_ERR_BAD_ARG;
  SimArgs a;
  a.tr = *track;
  a.controls = controls_dev;
  a.dyn_dev = dyn_params_dev;
  for (int i = 0; i < 13; ++i) a.dp.p[i] = dyn_params_host ? dyn_params_host[i] : 0.0f;
  a.T = T;
  a.n_sub = n_sub;
  a.tick = tick;
  a.state = state_dev;
  a.seg = seg_dev;
  a.status = status_dev;
  a.record = record_dev;
  a.x = x_dev;
  a.mirror = mirror_dev;
  a.goal = goal_dev;
  a.dist = dist_dev;
  a.tt = t_dev;
  a.B = (long)B;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return launch_sim<kSimLanes>(a, mode == IRBFN_ROLLOUT_ST_SELECT, s);
}

}  // extern "C"
