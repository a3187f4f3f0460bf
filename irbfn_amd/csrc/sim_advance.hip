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
//
// The kernel has three forms (SimForm).  SIM_CARTESIAN is the tick of irbfn_sim_advance.  SIM_FRENET (K14,
// irbfn_sim_advance_frenet) is the same tick with step 6 replaced: the Frenet pose of the car on the polyline, then the
// 8-input query of the Frenet planner.  SIM_POSE (irbfn_cartesian_to_frenet) is the search and the pose alone: no status, no
// plant, no record, no goal.  The three share every line they have in common, so the fused Frenet tick repeats the other two
// entry points bit for bit.
#include <math.h>

#include "common.h"
#include "planner_geom.h"
#include "rollout_step.h"

namespace irbfn {

constexpr int kSimRecord = 7;    // doubles per car: ticks, sum_d2, max_d, sum_dv, progress, s_last, fail_tick
enum SimRec : int { SR_TICKS = 0, SR_SUM_D2, SR_MAX_D, SR_SUM_DV, SR_PROGRESS, SR_S_LAST, SR_FAIL_TICK };

enum SimForm : int { SIM_CARTESIAN = 0, SIM_FRENET, SIM_POSE };

struct SimArgs {
  irbfn_sim_track tr;
  const double* __restrict__ curv;      // [N] way-point curvatures (SIM_FRENET, SIM_POSE)
  const float* __restrict__ controls;   // [B][2T] or null
  const float* __restrict__ dyn_dev;    // [B][13] or null
  DynParams dp;                         // the shared row (dyn_dev null)
  int T, n_sub, tick;
  float* __restrict__ state;
  int* __restrict__ seg;
  int* __restrict__ status;
  double* __restrict__ record;
  float* __restrict__ x;                // [B][7], SIM_FRENET: [B][8]
  int* __restrict__ mirror;
  double* __restrict__ frenet;          // [B][8]: optional in SIM_FRENET, the result of SIM_POSE
  int* __restrict__ seg_out;            // SIM_POSE (which leaves seg as it is), optional
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

template <int G, bool SELECT, int FORM>
__global__ __launch_bounds__(256) void sim_advance_kernel(const SimArgs a) {
#pragma clang fp contract(off)                   // the statistics and every shared body: each product rounded before its sum
  constexpr int CPB = 256 / G;                   // cars per block
  const int gl = threadIdx.x & (G - 1);          // lane of the group
  const long b = (long)blockIdx.x * CPB + threadIdx.x / G;
  if (b >= a.B) return;                          // the whole group
  if constexpr (FORM != SIM_POSE) {
    if (a.status[b] != IRBFN_SIM_OK) return;     // frozen: nothing read, nothing written
  }
  const bool lead = gl == 0;
  const int N = a.tr.N;
  const double* __restrict__ wp = a.tr.waypoints_dev;

  float s[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) s[i] = a.state[b * 7 + i];

  // ---- 1. plant
  if (FORM != SIM_POSE && a.controls) {
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
  const SimWindow win(a.tr, a.seg ? a.seg[b] : 0);   // (no seg: SIM_POSE over every segment, the host set the window to -1)
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
  const double sarc = a.tr.cum_dev[i] + t * a.tr.len_dev[i];

  if constexpr (FORM == SIM_POSE) {
    double fr[8];
    frenet_pose(wp, a.curv, i, t, d, sarc, s, fr);
    if (lead) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a.frenet[b * 8 + k] = fr[k];
      if (a.seg_out) a.seg_out[b] = i;
      if (a.dist) a.dist[b] = d;
      if (a.tt) a.tt[b] = t;
    }
    return;
  }

  // ---- 3. statistics
  double* __restrict__ rec = a.record + b * kSimRecord;
  const double ticks0 = rec[SR_TICKS];
  const double sum_d2 = rec[SR_SUM_D2] + d * d;
  const double max0 = rec[SR_MAX_D];
  const double max_d = d > max0 ? d : max0;      // max(max_d, d) as Python's: a NaN never replaces
  const double dv = (double)s[3] - wp[4 * i + 3];
  const double sum_dv = rec[SR_SUM_DV] + fabs(dv);
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
  constexpr int XW = FORM == SIM_FRENET ? 8 : 7;
  double g[4];
  float xo[XW];
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = wp[4 * gi + k];
  bool m;
  if constexpr (FORM == SIM_FRENET) {
    double fr[8];
    frenet_pose(wp, a.curv, i, t, d, sarc, s, fr);
    m = frenet_query(fr, g[3], xo);
    if (lead && a.frenet) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a.frenet[b * 8 + k] = fr[k];
    }
  } else {
    double pose[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) pose[k] = (double)s[k];
    m = cartesian_query(pose, g, xo);
  }
  if (lead) {
#pragma unroll
    for (int k = 0; k < XW; ++k) a.x[b * XW + k] = xo[k];
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

template <int G, int FORM>
static int launch_sim(const SimArgs& a, bool select, hipStream_t s) {
  const dim3 grid((unsigned)((a.B + 256 / G - 1) / (256 / G)));
  if constexpr (FORM != SIM_POSE) {              // (SIM_POSE has no plant: one instance)
    if (select) return launch_kernel<sim_advance_kernel<G, true, FORM>>(grid, dim3(256), 0, s, a);
  }
  return launch_kernel<sim_advance_kernel<G, false, FORM>>(grid, dim3(256), 0, s, a);
}

// what every entry point asks of a track before any HIP call
static bool track_ok(const irbfn_sim_track* track) {
  if (!track || track->N < 2) return false;
  if (track->win_back < -1 || track->win_fwd < -1 || ((track->win_back == -1) != (track->win_fwd == -1))) return false;
  if (!(track->lookahead >= 0.0) || !(track->max_reacquire >= 0.0) || track->half_width != track->half_width) return false;
  return true;
}

// irbfn_sim_advance (frenet = false: no curvature, x [B,7]) and irbfn_sim_advance_frenet
static int sim_advance(bool frenet, const irbfn_sim_track* track, const double* curv_dev, int mode, int tick,
                       const float* controls_dev, int T, const float* dyn_params_host, const float* dyn_params_dev, int n_sub,
                       float* state_dev, int32_t* seg_dev, int32_t* status_dev, double* record_dev, float* x_dev,
                       int32_t* mirror_dev, double* frenet_dev, double* goal_dev, double* dist_dev, double* t_dev, int64_t B,
                       void* stream) {
  if (B < 0 || n_sub < 1 || !track_ok(track)) return IRBFN_ERR_BAD_ARG;
  if (mode != IRBFN_ROLLOUT_ST_SELECT && mode != IRBFN_ROLLOUT_ST_KS) return IRBFN_ERR_BAD_ARG;
  if (controls_dev && T < 1) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!track->waypoints_dev || !track->cum_dev || !track->len_dev || !state_dev || !seg_dev || !status_dev || !record_dev ||
      !x_dev || !mirror_dev || (frenet && !curv_dev))
    return IRBFN_ERR_BAD_ARG;
  if (controls_dev && !dyn_params_host && !dyn_params_dev) return IRBFN_ERR_BAD_ARG;
  SimArgs a;
  a.tr = *track;
  a.curv = curv_dev;
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
  a.frenet = frenet_dev;
  a.seg_out = nullptr;
  a.goal = goal_dev;
  a.dist = dist_dev;
  a.tt = t_dev;
  a.B = (long)B;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool select = mode == IRBFN_ROLLOUT_ST_SELECT;
  return frenet ? launch_sim<kSimLanes, SIM_FRENET>(a, select, s) : launch_sim<kSimLanes, SIM_CARTESIAN>(a, select, s);
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int irbfn_sim_record_doubles(void) { return kSimRecord; }

int irbfn_sim_advance(const irbfn_sim_track* track, int mode, int tick, const float* controls_dev, int T,
                      const float* dyn_params_host, const float* dyn_params_dev, int n_sub, float* state_dev, int32_t* seg_dev,
                      int32_t* status_dev, double* record_dev, float* x_dev, int32_t* mirror_dev, double* goal_dev,
                      double* dist_dev, double* t_dev, int64_t B, void* stream) {
  return sim_advance(false, track, nullptr, mode, tick, controls_dev, T, dyn_params_host, dyn_params_dev, n_sub, state_dev,
                     seg_dev, status_dev, record_dev, x_dev, mirror_dev, nullptr, goal_dev, dist_dev, t_dev, B, stream);
}

int irbfn_sim_advance_frenet(const irbfn_sim_track* track, const double* curv_dev, int mode, int tick,
                             const float* controls_dev, int T, const float* dyn_params_host, const float* dyn_params_dev,
                             int n_sub, float* state_dev, int32_t* seg_dev, int32_t* status_dev, double* record_dev,
                             float* x_dev, int32_t* mirror_dev, double* frenet_dev, double* goal_dev, double* dist_dev,
                             double* t_dev, int64_t B, void* stream) {
  return sim_advance(true, track, curv_dev, mode, tick, controls_dev, T, dyn_params_host, dyn_params_dev, n_sub, state_dev,
                     seg_dev, status_dev, record_dev, x_dev, mirror_dev, frenet_dev, goal_dev, dist_dev, t_dev, B, stream);
}

int irbfn_cartesian_to_frenet(const irbfn_sim_track* track, const double* curv_dev, const float* state_dev,
                              const int32_t* seg_dev, double* frenet_dev, int32_t* seg_out_dev, double* dist_dev,
                              double* t_dev, int64_t B, void* stream) {
  if (B < 0 || !track_ok(track)) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!track->waypoints_dev || !track->cum_dev || !track->len_dev || !curv_dev || !state_dev || !frenet_dev)
    return IRBFN_ERR_BAD_ARG;
  SimArgs a = {};
  a.tr = *track;
  if (!seg_dev) a.tr.win_back = a.tr.win_fwd = -1;           // every segment
  a.curv = curv_dev;
  a.state = const_cast<float*>(state_dev);                   // SIM_POSE only reads the state and the segments
  a.seg = const_cast<int32_t*>(seg_dev);
  a.frenet = frenet_dev;
  a.seg_out = seg_out_dev;
  a.dist = dist_dev;
  a.tt = t_dev;
  a.n_sub = 1;
  a.B = (long)B;
  return launch_sim<kSimLanes, SIM_POSE>(a, false, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
