// Per-pair / per-segment bodies of the planner front end, shared by its batched kernels (planner_front.hip) and the
// closed-loop tick (sim_advance.hip): one statement of each, so that the fused tick repeats the stand-alone kernels bit
// for bit.  LD: doubles per way-point row of the array a kernel walks ([N,2] trajectories, [N,4] race lines).
#pragma once

#include <math.h>

#include "common.h"

namespace irbfn {

// Python's float modulo: result has the sign of the divisor (b > 0 here)
__device__ __forceinline__ double py_mod(double a, double b) {
  double r = fmod(a, b);
  if (r == 0.0) return copysign(0.0, b);          // fmod keeps the sign of a: -0.0 % pi is +0.0 in Python and NumPy
  if ((r < 0.0) != (b < 0.0)) r += b;
  return r;
}

// Query and mirror flag of IRBFNPlanner.plan (src/irbfn_mpc/irbfn_planner.py:181-201) for one (pose, goal) pair.
// p: [x, y, delta, v, theta, angv, beta] (:240); g: ref_point [x, y, theta, v] (:170-171); xo: [v, x_g, y_g, t_g, v_g, beta, angv]
__device__ __forceinline__ bool cartesian_query(const double (&p)[7], const double (&g)[4], float (&xo)[7]) {
#pragma clang fp contract(off)                   // NumPy rounds each product: a fused s*dx + c*dy flips the sign of an exact 0
  const double x = p[0], y = p[1], v = p[3], theta = p[4], angv = p[5], beta = p[6];
  const double c = cos(-theta), s = sin(-theta); // rot = [[c, -s], [s, c]]               (:181-183)
  const double dx = g[0] - x, dy = g[1] - y;
  const double gl0 = c * dx + (-s) * dy;         // np.dot(rot, d): products then one add, no FMA
  const double gl1 = s * dx + c * dy;
  const double gt = g[2] - theta;
  const bool m = gl1 < 0.0;                      // goal_needs_mirror                     (:188)
  const double pi = 3.141592653589793;
  xo[0] = (float)v;                              // (:189-201)
  xo[1] = (float)gl0;
  xo[2] = (float)(m ? -gl1 : gl1);
  xo[3] = (float)(m ? py_mod(-gt, pi) : py_mod(gt, pi));
  xo[4] = (float)g[3];
  xo[5] = (float)beta;
  xo[6] = (float)angv;
  return m;
}

// Query and mirror flag of IRBFNFrenetPlanner.plan (src/irbfn_mpc/irbfn_planner.py:456-478) for one (Frenet pose, goal speed)
// pair.  p: [s, ey, delta, vx, vy, wz, epsi, curv] (:491-502); xo: [ey, delta, vx, vy, vx_goal, wz, epsi, curv]
__device__ __forceinline__ bool frenet_query(const double (&p)[8], double vx_goal, float (&xo)[8]) {
  const bool m = p[1] < -0.05;                   // goal_needs_mirror = ey < -0.05           (:457)
  xo[0] = (float)(m ? -p[1] : p[1]);             // (:459-478)
  xo[1] = (float)p[2];
  xo[2] = (float)p[3];
  xo[3] = (float)(m ? -p[4] : p[4]);
  xo[4] = (float)vx_goal;
  xo[5] = (float)(m ? -p[5] : p[5]);
  xo[6] = (float)(m ? -p[6] : p[6]);
  xo[7] = (float)p[7];
  return m;
}

// e - 2 pi rint(e / 2 pi): the angle e brought into [-pi, pi]
__device__ __forceinline__ double wrap_angle(double e) {
#pragma clang fp contract(off)
  const double two_pi = 6.283185307179586;
  return e - two_pi * rint(e / two_pi);
}

// Frenet pose of a car on a race line wp [N,4] with way-point curvatures curv [N] (include/irbfn_hip.h:
// irbfn_cartesian_to_frenet): st = [x, y, delta, v, psi, psi_dot, beta]; i, t, d: the nearest segment, its parameter and the
// distance as segment_distance<4> found them; sarc = cum[i] + t * len[i].  fr: [s, ey, delta, vx, vy, wz, epsi, curv].
// Way-point i + 1 exists: the polyline's segments end at N - 2.
__device__ __forceinline__ void frenet_pose(const double* __restrict__ wp, const double* __restrict__ curv, int i, double t,
                                            double d, double sarc, const float (&st)[7], double (&fr)[8]) {
#pragma clang fp contract(off)                   // the float64 statement rounds each product before its sum
  const double x0 = wp[4 * i], y0 = wp[4 * i + 1], th0 = wp[4 * i + 2];
  const double dx = wp[4 * (i + 1)] - x0, dy = wp[4 * (i + 1) + 1] - y0;
  const double c = dx * ((double)st[1] - y0) - dy * ((double)st[0] - x0);   // > 0: the car is left of the segment
  const double th = th0 + t * wrap_angle(wp[4 * (i + 1) + 2] - th0);
  const double k0 = curv[i];
  const double v = (double)st[3], beta = (double)st[6];
  fr[0] = sarc;
  fr[1] = c >= 0.0 ? d : -d;
  fr[2] = (double)st[2];
  fr[3] = v * cos(beta);
  fr[4] = v * sin(beta);
  fr[5] = (double)st[5];
  fr[6] = wrap_angle((double)st[4] - th);
  fr[7] = k0 + t * (curv[i + 1] - k0);
}

// nearest_point (src/irbfn_mpc/planner_utils.py:125-138) for segment i of a polyline: the distance d of (px, py) to the
// segment, the parameter t in [0, 1] of the closest point and that point.  d is NaN for a repeated or NaN way-point.
template <int LD>
__device__ __forceinline__ void segment_distance(const double* __restrict__ wp, int i, double px, double py, double& d,
                                                 double& t, double& qx, double& qy) {
#pragma clang fp contract(off)                   // every product of the reference's lines is rounded before its sum
  const double x0 = wp[LD * i], y0 = wp[LD * i + 1];
  const float dx = (float)(wp[LD * (i + 1)] - x0), dy = (float)(wp[LD * (i + 1) + 1] - y0);   // diffs.astype(float32) :125
  const float l2 = dx * dx + dy * dy;                                                  // :126
  const float lx = (float)(px - x0), ly = (float)(py - y0);                            // :129
  const float dot = lx * dx + ly * dy;                                                 // np.dot of two float32 pairs :130
  t = (double)dot / (double)l2;                                                        // :131
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);                                             // :132-133 (nan stays)
  qx = x0 + t * (double)dx;                                                            // :134
  qy = y0 + t * (double)dy;
  const double ex = px - qx, ey = py - qy;
  d = sqrt(ex * ex + ey * ey);                                                         // :137-138
}

template <int LD = 2>
__device__ __forceinline__ bool circle_hit(const double* wp, int N, int i, double px, double py, float radius,
                                           bool first, float start_t, float& t_out, float& qx, float& qy) {
#pragma clang fp contract(off)
  const int i0 = ((i % N) + N) % N, i1 = (((i + 1) % N) + N) % N;
  const float sx = (float)wp[LD * i0], sy = (float)wp[LD * i0 + 1];                       // trajectory.astype(float32) :160
  const float ex = (float)wp[LD * i1] + 1e-6f, ey = (float)wp[LD * i1 + 1] + 1e-6f;       // :163
  const float vx = ex - sx, vy = ey - sy;
  const float av = vx * vx + vy * vy;                                                    // :166
  const double bq = 2.0 * ((double)vx * ((double)sx - px) + (double)vy * ((double)sy - py));   // :167
  const double cq = (double)(sx * sx + sy * sy) + (px * px + py * py) - 2.0 * ((double)sx * px + (double)sy * py) -
                    (double)radius * (double)radius;                                     // :168-173
  double disc = bq * bq - 4.0 * (double)av * cq;                                         // :174
  if (disc < 0.0 || disc != disc) return false;
  disc = sqrt(disc);
  const double t1 = (-bq - disc) / (2.0 * (double)av), t2 = (-bq + disc) / (2.0 * (double)av);   // :182-183
  double t;
  if (first) {                                                                           // :184-193
    if (t1 >= 0.0 && t1 <= 1.0 && t1 >= (double)start_t) t = t1;
    else if (t2 >= 0.0 && t2 <= 1.0 && t2 >= (double)start_t) t = t2;
    else return false;
  } else {                                                                               // :194-203
    if (t1 >= 0.0 && t1 <= 1.0) t = t1;
    else if (t2 >= 0.0 && t2 <= 1.0) t = t2;
    else return false;
  }
  t_out = (float)t;
  qx = (float)((double)sx + t * (double)vx);
  qy = (float)((double)sy + t * (double)vy);
  return true;
}

// The search order of intersect_point (:155-156, :176, :205-231) from t_start = ts: segments start_i .. N - 2, then, with
// wrap, -1 .. start_i - 1.  seg(ord) is the segment at position ord < total(); only position 0 of the forward part is `first`.
struct HitOrder {
  int start_i, nfwd, nwrap;
  float start_t;
  __device__ __forceinline__ HitOrder(double ts, int N, int wrap) {
    start_i = (int)ts;                                                                   // :155
    start_t = (float)fmod(ts, 1.0);                                                      // :156
    nfwd = N - 1 - start_i > 0 ? N - 1 - start_i : 0;                                    // i = start_i .. N - 2
    nwrap = wrap ? (start_i + 1 > 0 ? start_i + 1 : 0) : 0;                              // i = -1 .. start_i - 1
  }
  __device__ __forceinline__ int total() const { return nfwd + nwrap; }
  // one position of the order on one lane: hit or not; i = the segment
  template <int LD>
  __device__ __forceinline__ bool probe(const double* wp, int N, int ord, double px, double py, float radius, int& i, float& t,
                                        float& qx, float& qy) const {
    i = 0;
    if (ord < nfwd) {
      i = start_i + ord;
      return circle_hit<LD>(wp, N, i, px, py, radius, ord == 0, start_t, t, qx, qy);
    }
    if (ord < nfwd + nwrap) {
      i = ord - nfwd - 1;
      return circle_hit<LD>(wp, N, i, px, py, radius, false, 0.0f, t, qx, qy);
    }
    return false;
  }
};

}  // namespace irbfn
