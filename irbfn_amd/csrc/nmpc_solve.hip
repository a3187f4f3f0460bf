// K13 / K15: batched NMPC solver (include/irbfn_hip.h: irbfn_nmpc_solve, irbfn_nmpc_solve_frenet; DESIGN.md "K13", "K15").  For
// every row a bounded least-squares problem in 2T <= 16 unknowns through the project's own roll-out step (single-track, or the
// Frenet low-speed model), solved by a projected Levenberg-Marquardt.
//
// One problem per lane, and everything the iteration touches lives in that lane's registers: u, u+, the sensitivities
// S_t = d s_t / d u (NS x 2T, advanced step by step with the forward form of the roll-out adjoints, rollout_adjoint.h), the
// packed upper triangle of H = J^T J, and g = J^T r.  Every array is indexed by compile-time constants: the T and 2T loops are
// fully unrolled (a runtime-indexed array would go to scratch), only the iteration loop is rolled.  A lane that is done keeps
// its u and idles; a wave leaves the loop when all its lanes are done.  No atomics, no workspace, no lane reads another's
// values: a row's result depends on that row alone.
//
// The weights enter as q e^2, never as sqrt(q): H = sum q s s^T and g = sum q e s need no square root.
#include <math.h>

#include "common.h"
#include "rollout_adjoint.h"

namespace irbfn {

struct NmpcArgs {
  const float* __restrict__ state0;    // [B][NmpcModel::SW]
  const float* __restrict__ goal;      // [B][4]
  const float* __restrict__ u0;        // [B][2T] or null
  const float* __restrict__ dyn_dev;   // [B][13] or null
  DynParams dp;                        // the shared row (dyn_dev null)
  irbfn_nmpc_options opt;
  float* __restrict__ u;               // [B][2T]
  float* __restrict__ cost;            // [B][2]
  int* __restrict__ info;              // [B][2]
  float* __restrict__ grad;            // [B][2T] or null
  long B;
};

constexpr float kNmpcTie = 0.5f;       // slope of the clips of delta and V on a bound (jnp.clip's, as the roll-out VJPs)

// What the solver has to know about a model beside its step and StepJac: SW, the width of a state row; kHeading, the state
// component behind the heading residual (the residuals are the state components {0, 1, kHeading, 3}, whose tangents are the
// rows {0, 1, 4, 3} of S in every model); kFrame, whether a step may start only where 1 - ey curv > 0.
template <int MODE>
struct NmpcModel {                     // ST_KS, ST_SELECT: [x, y, delta, v, psi, psi_dot, beta]
  static constexpr int SW = 7, kHeading = 4;
  static constexpr bool kFrame = false;
};
template <>
struct NmpcModel<IRBFN_ROLLOUT_FRENET_LS> {   // [s, ey, delta, vx, vy, wz, epsi, curv]: the frame ends at the centre of curvature
  static constexpr int SW = 8, kHeading = 6;
  static constexpr bool kFrame = true;
};

// index of (i, j), i <= j, in the packed upper triangle of an N x N matrix
__host__ __device__ constexpr int tri(int i, int j, int N) { return i * N - (i * (i - 1)) / 2 + (j - i); }

// wrap(e) = e - 2 pi rint(e / 2 pi), 2 pi as a float pair; |e| < pi comes back as it is
__device__ __forceinline__ float wrap_angle(float e) {
  const float k = rintf(e * 0.159154943091895336f);
  return __builtin_fmaf(-k, -1.7484556000744883e-07f, __builtin_fmaf(-k, 6.2831854820251465f, e));
}

// One pass over the horizon at u: the cost, and with LIN the gradient g [2T] and the packed Gauss-Newton matrix H as well.
// The cost arithmetic is the same instruction sequence with and without LIN (contraction off), so both give the same bits.
// A model with a frame (NmpcModel::kFrame): a roll-out that starts any step from 1 - ey curv <= 0 costs +inf.
template <int MODE, int T, bool LIN>
__device__ __forceinline__ float nmpc_pass(const float (&u)[2 * T], const float (&s0)[NmpcModel<MODE>::SW], const float (&gl)[4],
                                           const DynParams& dp, const irbfn_nmpc_options& w, float (&g)[2 * T],
                                           float (&H)[T * (2 * T + 1)]) {
#pragma clang fp contract(off)
  using M = NmpcModel<MODE>;
  constexpr int N = 2 * T, NS = StepJac<MODE>::NS;
  constexpr int kComp[4] = {0, 1, 4, 3};           // the row of S behind residual x, y, heading, speed (s, ey, epsi, vx)
  float s[M::SW];
#pragma unroll
  for (int i = 0; i < M::SW; ++i) s[i] = s0[i];
  bool inside = true;
  float S[LIN ? NS * N : 1];                       // S[i * N + j] = d s_i / d u_j
  if constexpr (LIN) {
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < T * (2 * T + 1); ++k) H[k] = 0.0f;
  }
  float c = 0.0f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if constexpr (LIN) {
      StepJac<MODE> J;
      jvp_coeffs<MODE>(s, u[t], kNmpcTie, dp, J);
      // the controls of earlier steps: a_j, sv_j, j < t
#pragma unroll
      for (int j = 0; j < T; ++j) {
        if (j >= t) continue;
        float da[NS], ds[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) { da[i] = S[i * N + j]; ds[i] = S[i * N + T + j]; }
        jvp_carry<MODE>(J, da);
        jvp_carry<MODE>(J, ds);
#pragma unroll
        for (int i = 0; i < NS; ++i) { S[i * N + j] = da[i]; S[i * N + T + j] = ds[i]; }
      }
      float da[NS], ds[NS];
      jvp_fresh<MODE>(J, dp.p[8], da, ds);
#pragma unroll
      for (int i = 0; i < NS; ++i) { S[i * N + t] = da[i]; S[i * N + T + t] = ds[i]; }
    }
    if constexpr (M::kFrame) inside = inside && (1.0f - s[1] * s[7] > 0.0f);
    roll_step<MODE>(s, u[t], u[T + t], dp);
    float e[4];
    e[0] = s[0] - gl[0];
    e[1] = s[1] - gl[1];
    e[2] = wrap_angle(s[M::kHeading] - gl[2]);
    e[3] = s[3] - gl[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float wk = t == T - 1 ? w.qf[k] : w.q[k];
      c = c + wk * (e[k] * e[k]);
      if constexpr (LIN) {
        // the columns that reach the residual components of s_{t+1} -- (x, y, psi, v), or (s, ey, epsi, vx) in the Frenet model:
        // a_0..a_t and sv_0..sv_{t-1} (sv_t has only moved delta)
        const int L = 2 * t + 1;
        float row[N], wrow[N];
#pragma unroll
        for (int l = 0; l < N; ++l) {
          if (l >= L) continue;
          const int j = l <= t ? l : T + (l - t - 1);
          row[l] = S[kComp[k] * N + j];
          wrow[l] = wk * row[l];
          g[j] = __builtin_fmaf(wrow[l], e[k], g[j]);
        }
#pragma unroll
        for (int l = 0; l < N; ++l) {
#pragma unroll
          for (int n = 0; n < N; ++n) {
            if (l >= L || n < l || n >= L) continue;
            const int i = l <= t ? l : T + (l - t - 1), j = n <= t ? n : T + (n - t - 1);
            H[tri(i, j, N)] = __builtin_fmaf(wrow[l], row[n], H[tri(i, j, N)]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    c = c + w.r[0] * (u[t] * u[t]);
    c = c + w.r[1] * (u[T + t] * u[T + t]);
    if constexpr (LIN) {
      g[t] = __builtin_fmaf(w.r[0], u[t], g[t]);
      g[T + t] = __builtin_fmaf(w.r[1], u[T + t], g[T + t]);
      H[tri(t, t, N)] += w.r[0];
      H[tri(T + t, T + t, N)] += w.r[1];
    }
  }
#pragma unroll
  for (int t = 0; t < T - 1; ++t) {
    const float da = u[t + 1] - u[t], ds = u[T + t + 1] - u[T + t];
    c = c + w.rd[0] * (da * da);
    c = c + w.rd[1] * (ds * ds);
    if constexpr (LIN) {
      const float ga = w.rd[0] * da, gs = w.rd[1] * ds;
      g[t] -= ga; g[t + 1] += ga;
      g[T + t] -= gs; g[T + t + 1] += gs;
      H[tri(t, t, N)] += w.rd[0]; H[tri(t + 1, t + 1, N)] += w.rd[0]; H[tri(t, t + 1, N)] -= w.rd[0];
      H[tri(T + t, T + t, N)] += w.rd[1]; H[tri(T + t + 1, T + t + 1, N)] += w.rd[1]; H[tri(T + t, T + t + 1, N)] -= w.rd[1];
    }
  }
  if constexpr (M::kFrame) return inside ? 0.5f * c : INFINITY;
  return 0.5f * c;
}

// d <- the damped step: (H + diag(lambda H_jj + eps max H_jj)) d = -g on the free variables, 0 on the fixed ones.  H is
// overwritten by its factor U (H = U^T U, upper), g by d.
template <int N>
__device__ __forceinline__ void nmpc_step(float (&H)[N * (N + 1) / 2], float (&g)[N], const bool (&fixed)[N], float lambda, float eps) {
  float top = 0.0f;
#pragma unroll
  for (int j = 0; j < N; ++j) top = fmaxf(top, H[tri(j, j, N)]);
  const float floor_ = eps * top;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (j < i) continue;
      float v = H[tri(i, j, N)];
      if (i == j) v = fixed[i] ? 1.0f : v + (lambda * v + floor_);
      else v = (fixed[i] || fixed[j]) ? 0.0f : v;
      H[tri(i, j, N)] = v;
    }
    g[i] = fixed[i] ? 0.0f : -g[i];
  }
  float rinv[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float piv = H[tri(k, k, N)];
    rinv[k] = piv > 0.0f ? __builtin_amdgcn_rsqf(piv) : 0.0f;     // a pivot <= 0 (or nan): no step in this variable
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (j > k) H[tri(k, j, N)] *= rinv[k];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        if (i > k && j >= i) H[tri(i, j, N)] = __builtin_fmaf(-H[tri(k, i, N)], H[tri(k, j, N)], H[tri(i, j, N)]);
      }
    }
  }
  // U^T y = -g, then U d = y
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float v = g[i];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (k < i) v = __builtin_fmaf(-H[tri(k, i, N)], g[k], v);
    }
    g[i] = v * rinv[i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    float v = g[i];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (k > i) v = __builtin_fmaf(-H[tri(i, k, N)], g[k], v);
    }
    g[i] = v * rinv[i];
  }
}

template <int MODE, int T>
__global__ __launch_bounds__(64) void nmpc_solve_kernel(const NmpcArgs a) {
  constexpr int N = 2 * T;
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  const bool live = b < a.B;
  const long row = live ? b : a.B - 1;             // a lane past the end solves the last row again and stores nothing
  DynParams dp = a.dp;
  if (a.dyn_dev) {
#pragma unroll
    for (int i = 0; i < 13; ++i) dp.p[i] = a.dyn_dev[row * 13 + i];
  }
  constexpr int SW = NmpcModel<MODE>::SW;
  float s0[SW], gl[4], u[N], g[N], H[T * (2 * T + 1)];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 13; ++i) finite = finite && (fabsf(dp.p[i]) < INFINITY);
#pragma unroll
  for (int i = 0; i < SW; ++i) { s0[i] = a.state0[row * SW + i]; finite = finite && (fabsf(s0[i]) < INFINITY); }
#pragma unroll
  for (int i = 0; i < 4; ++i) { gl[i] = a.goal[row * 4 + i]; finite = finite && (fabsf(gl[i]) < INFINITY); }
  const float hi_a = dp.p[10], hi_s = dp.p[9];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float v = a.u0 ? a.u0[row * N + j] : 0.0f;
    finite = finite && (fabsf(v) < INFINITY);
    const float hi = j < T ? hi_a : hi_s;
    u[j] = clipf(v, -hi, hi);
  }
  const irbfn_nmpc_options& w = a.opt;
  float lambda = w.lambda0, c0 = 0.0f, c = 0.0f;
  int status = IRBFN_NMPC_MAX_ITER, iters = 0;
  bool done = false;
#pragma unroll 1
  for (int it = 0;; ++it) {
    const float cl = nmpc_pass<MODE, T, true>(u, s0, gl, dp, w, g, H);
    if (it == 0) {
      c0 = cl;
      c = cl;
      if (!finite || !(fabsf(cl) < INFINITY)) {
        status = IRBFN_NMPC_NONFINITE;
        done = true;
        c0 = NAN;
        c = NAN;
      } else if (cl == 0.0f) {
        status = IRBFN_NMPC_CONVERGED;
        done = true;
      }
    }
    if (it >= w.max_iter) done = true;
    if (__all(done)) break;
    if (!done) {
      bool fixed[N];
      float d[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float hi = j < T ? hi_a : hi_s;
        fixed[j] = (u[j] <= -hi && g[j] > 0.0f) || (u[j] >= hi && g[j] < 0.0f);
        d[j] = g[j];
      }
      nmpc_step<N>(H, d, fixed, lambda, w.eps);
      float up[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float hi = j < T ? hi_a : hi_s;
        up[j] = clipf(u[j] + d[j], -hi, hi);
      }
      const float cp = nmpc_pass<MODE, T, false>(up, s0, gl, dp, w, d, H);
      ++iters;
      const bool near = fabsf(c - cp) <= w.tol * c;       // the cost moved by no more than tol c, either way
      if (cp < c) {
#pragma unroll
        for (int j = 0; j < N; ++j) u[j] = up[j];
        c = cp;
        lambda = fmaxf(lambda / 10.0f, w.lambda_min);
        if (near || cp == 0.0f) { status = IRBFN_NMPC_CONVERGED; done = true; }
      } else if (near) {
        status = IRBFN_NMPC_CONVERGED;
        done = true;
      } else {
        lambda = fminf(10.0f * lambda, w.lambda_max);
        if (lambda >= w.lambda_max) { status = IRBFN_NMPC_STALLED; done = true; }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < N; ++j) a.u[b * N + j] = u[j];
  a.cost[b * 2] = c0;
  a.cost[b * 2 + 1] = c;
  a.info[b * 2] = status;
  a.info[b * 2 + 1] = iters;
  if (a.grad) {
#pragma unroll
    for (int j = 0; j < N; ++j) a.grad[b * N + j] = g[j];
  }
}

template <int MODE>
static int launch_nmpc(int T, const NmpcArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.B + 63) / 64));
  switch (T) {
#define IRBFN_NMPC_T(TT) case TT: return launch_kernel<nmpc_solve_kernel<MODE, TT>>(grid, dim3(64), 0, s, a)
    IRBFN_NMPC_T(1); IRBFN_NMPC_T(2); IRBFN_NMPC_T(3); IRBFN_NMPC_T(4);
    IRBFN_NMPC_T(5); IRBFN_NMPC_T(6); IRBFN_NMPC_T(7); IRBFN_NMPC_T(8);
#undef IRBFN_NMPC_T
    default: return IRBFN_ERR_UNSUPPORTED;
  }
}

static bool weight_ok(float v) { return v >= 0.0f && v < INFINITY; }

}  // namespace irbfn

using namespace irbfn;

// the checks both entry points share, decided before any HIP call: IRBFN_OK with *launch set when there is work to do
static int nmpc_check(int T, const float* state0_dev, const float* goal_dev, const float* dyn_params_host, const float* dyn_params_dev,
                      const irbfn_nmpc_options* opt, const float* u_dev, const float* cost_dev, const int32_t* info_dev, int64_t B,
                      bool* launch) {
  *launch = false;
  if (B < 0 || !opt) return IRBFN_ERR_BAD_ARG;
  for (int k = 0; k < 4; ++k)
    if (!weight_ok(opt->q[k]) || !weight_ok(opt->qf[k])) return IRBFN_ERR_BAD_ARG;
  for (int k = 0; k < 2; ++k)
    if (!weight_ok(opt->r[k]) || !weight_ok(opt->rd[k])) return IRBFN_ERR_BAD_ARG;
  if (!weight_ok(opt->lambda0) || !weight_ok(opt->lambda_min) || !weight_ok(opt->lambda_max) || !weight_ok(opt->tol) ||
      !weight_ok(opt->eps) || opt->lambda_min > opt->lambda_max || opt->max_iter < 0)
    return IRBFN_ERR_BAD_ARG;
  if (T < 1 || T > 8) return IRBFN_ERR_UNSUPPORTED;
  if (B == 0) return IRBFN_OK;
  if (!state0_dev || !goal_dev || !u_dev || !cost_dev || !info_dev || (!dyn_params_host && !dyn_params_dev))
    return IRBFN_ERR_BAD_ARG;
  *launch = true;
  return IRBFN_OK;
}

static NmpcArgs nmpc_args(const float* state0_dev, const float* goal_dev, const float* u0_dev, const float* dyn_params_host,
                          const float* dyn_params_dev, const irbfn_nmpc_options* opt, float* u_dev, float* cost_dev,
                          int32_t* info_dev, float* grad_dev, int64_t B) {
  NmpcArgs a;
  a.state0 = state0_dev;
  a.goal = goal_dev;
  a.u0 = u0_dev;
  a.dyn_dev = dyn_params_dev;
  for (int i = 0; i < 13; ++i) a.dp.p[i] = dyn_params_host ? dyn_params_host[i] : 0.0f;
  a.opt = *opt;
  a.u = u_dev;
  a.cost = cost_dev;
  a.info = info_dev;
  a.grad = grad_dev;
  a.B = (long)B;
  return a;
}

extern "C" int irbfn_nmpc_solve(int mode, int T, const float* state0_dev, const float* goal_dev, const float* u0_dev,
                                const float* dyn_params_host, const float* dyn_params_dev, const irbfn_nmpc_options* opt,
                                float* u_dev, float* cost_dev, int32_t* info_dev, float* grad_dev, int64_t B, void* stream) {
  if (B < 0 || !opt) return IRBFN_ERR_BAD_ARG;
  if (mode != IRBFN_ROLLOUT_ST_SELECT && mode != IRBFN_ROLLOUT_ST_KS) return IRBFN_ERR_BAD_ARG;
  bool launch;
  const int st = nmpc_check(T, state0_dev, goal_dev, dyn_params_host, dyn_params_dev, opt, u_dev, cost_dev, info_dev, B, &launch);
  if (!launch) return st;
  const NmpcArgs a = nmpc_args(state0_dev, goal_dev, u0_dev, dyn_params_host, dyn_params_dev, opt, u_dev, cost_dev, info_dev,
                               grad_dev, B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (mode == IRBFN_ROLLOUT_ST_SELECT) return launch_nmpc<IRBFN_ROLLOUT_ST_SELECT>(T, a, s);
  return launch_nmpc<IRBFN_ROLLOUT_ST_KS>(T, a, s);
}

extern "C" int irbfn_nmpc_solve_frenet(int T, const float* state0_dev, const float* goal_dev, const float* u0_dev,
                                       const float* dyn_params_host, const float* dyn_params_dev, const irbfn_nmpc_options* opt,
                                       float* u_dev, float* cost_dev, int32_t* info_dev, float* grad_dev, int64_t B, void* stream) {
  bool launch;
  const int st = nmpc_check(T, state0_dev, goal_dev, dyn_params_host, dyn_params_dev, opt, u_dev, cost_dev, info_dev, B, &launch);
  if (!launch) return st;
  const NmpcArgs a = nmpc_args(state0_dev, goal_dev, u0_dev, dyn_params_host, dyn_params_dev, opt, u_dev, cost_dev, info_dev,
                               grad_dev, B);
  return launch_nmpc<IRBFN_ROLLOUT_FRENET_LS>(T, a, reinterpret_cast<hipStream_t>(stream));
}
