// Hand-derived one-step adjoints of the roll-out models (reverse-mode of rollout_step.h), shared by the roll-out VJP
// kernels (rollout_vjp.hip) and the loss-seed kernels of the training steps (train_step.hip).  The NumPy statement
// of the same adjoints is oracle/hand_vjp.py (checked against torch.autograd of the restatement to 1e-12).
// clip() gradient: 1 strictly inside, 0 strictly outside, `tie` on a bound (jnp.clip is minimum(maximum(.)), whose
// tie rule is 1/2).
// clipgrad, vjp_park and vjp_back_step<ST_KS / FULLINT / FRENET_LS> take their scalar type S as a template parameter (float
// by default; S = double with TrigF64 and DynParams64: the float64 training steps).
// ST_SELECT (float only, like its forward): the adjoint of the branch each step TOOK, the mask V > 3 a constant -- see
// vjp_back_step<ST_SELECT>.  Its NumPy statement is tests/_st_select_util.py: vjp_st_select.
#pragma once

#include "rollout_step.h"

namespace irbfn {

template <typename S>
__device__ __forceinline__ S clipgrad(S v, S lo, S hi, S tie) {
  return (v > lo && v < hi) ? S(1.0) : ((v == lo || v == hi) ? tie : S(0.0));
}

template <int MODE, typename S>
__device__ __forceinline__ void vjp_park(const S* s, S* p) {
  if constexpr (MODE == IRBFN_ROLLOUT_FRENET_LS) { p[0] = s[1]; p[1] = s[2]; p[2] = s[3]; p[3] = s[6]; }
  else if constexpr (MODE == IRBFN_ROLLOUT_ST_SELECT) { p[0] = s[2]; p[1] = s[3]; p[2] = s[4]; p[3] = s[5]; p[4] = s[6]; }
  else { p[0] = s[2]; p[1] = s[3]; p[2] = s[4]; }
}

// one reverse step: lam already holds the seeds of this step's output state; returns d/d(a_t), d/d(sv_t)
// Trig: how the step gets sin / cos of the heading and tan of the steering angle (rollout_step.h: TrigDirect, or the lane pair
// of rollout_pair.h -- same values bit for bit)
template <int MODE, typename Trig = TrigDirect, typename S = float>
__device__ __forceinline__ void vjp_back_step(const S* p, S a_in, S sv_in, S* lam, S cur, S tie,
                                              const typename DynOf<S>::type& dp, S& ga, S& gsv, const Trig trig = Trig()) {
  if constexpr (MODE == IRBFN_ROLLOUT_ST_KS) {
    const S lf = dp.p[3], lr = dp.p[4], dt = dp.p[8], sv_max = dp.p[9], a_max = dp.p[10], s_max = dp.p[11], v_max = dp.p[12];
    const S Lw = lr + lf;
    const S d_raw = p[0], v_raw = p[1], psi = p[2];
    const S DELTA = clipf(d_raw, -s_max, s_max), V = clipf(v_raw, -v_max, v_max);
    const S md = clipgrad(d_raw, -s_max, s_max, tie), mv = clipgrad(v_raw, -v_max, v_max, tie);
    const S ma = clipgrad(a_in, -a_max, a_max, tie), ms = clipgrad(sv_in, -sv_max, sv_max, tie);
    S cp, sp, td;
    trig.sincos_tan(psi, DELTA, s_max < 4194304.0f, sp, cp, td);
    ga = ma * dt * lam[3];
    gsv = ms * dt * lam[2];
    const S l2 = lam[2] + md * lam[4] * (V / Lw) * (S(1.0) + td * td) * dt;
    const S l3 = lam[3] + mv * dt * (lam[0] * cp + lam[1] * sp + lam[4] * td / Lw);
    const S l4 = lam[4] + dt * V * (-lam[0] * sp + lam[1] * cp);
    lam[2] = l2; lam[3] = l3; lam[4] = l4;
  } else if constexpr (MODE == IRBFN_ROLLOUT_ST_SELECT) {
    // x' = x + select(V > 3, f, f_ks) dt with the mask held constant: a step taken on the dynamic branch goes back through f
    // (dynamics.py:49-76), one taken on the kinematic branch through f_ks with ST_KS's expressions above, V = 3 is kinematic as
    // in the forward.  Branch-free like st_step<true>: ONE sincos of the selected angle, both sets of coefficients as
    // straight-line code, then selects.  At V = 0 the dynamic quantities (psi_dot / V, mu / (V L)) are inf / nan on a lane
    // that never took that branch: they are dropped by the selects, never multiplied by 0.  No reference counterpart (its
    // jax.grad through lax.select is NaN at V = 0); pinned by torch.autograd of a float64 restatement.
    static_assert(std::is_same<S, float>::value, "the select model runs in float32 only");
    const S g = S(9.81);
    const S mu = dp.p[0], m = dp.p[1], I = dp.p[2], lf = dp.p[3], lr = dp.p[4], C_Sf = dp.p[5], C_Sr = dp.p[6], h = dp.p[7],
            dt = dp.p[8], sv_max = dp.p[9], a_max = dp.p[10], s_max = dp.p[11], v_max = dp.p[12];
    const S Lw = lr + lf;
    const S d_raw = p[0], v_raw = p[1], psi = p[2], pd = p[3], beta = p[4];
    const S DELTA = clipf(d_raw, -s_max, s_max), V = clipf(v_raw, -v_max, v_max);
    const S A = clipf(a_in, -a_max, a_max);
    const S md = clipgrad(d_raw, -s_max, s_max, tie), mv = clipgrad(v_raw, -v_max, v_max, tie);
    const S ma = clipgrad(a_in, -a_max, a_max, tie), ms = clipgrad(sv_in, -sv_max, sv_max, tie);
    const bool dyn = V > S(3.0);
    S cp, sp, td;
    trig.sincos_tan(dyn ? psi + beta : psi, DELTA, s_max < 4194304.0f, sp, cp, td);
    // kinematic lanes: ST_KS
    const S gak = ma * dt * lam[3];
    const S l2k = lam[2] + md * lam[4] * (V / Lw) * (S(1.0) + td * td) * dt;
    const S l3k = lam[3] + mv * dt * (lam[0] * cp + lam[1] * sp + lam[4] * td / Lw);
    const S head = dt * V * (-lam[0] * sp + lam[1] * cp);      // the cotangent both f0 and f1 put on their angle
    // dynamic lanes
    const S glr = g * lr - A * h, glf = g * lf + A * h;
    const S E = C_Sf * glr, F = C_Sr * glf;
    const S P = lf * E, Q = lr * F, R = lf * lf * E + lr * lr * F, M = F * lr - E * lf;
    const S rV = S(1.0) / V, pv = pd * rV;
    const S c5 = (mu * m) / (I * Lw), c6 = (mu * rV) / Lw;
    const S U = E * DELTA - (F + E) * beta + M * pv;
    const S Ea = -C_Sf * h, Fa = C_Sr * h;                      // dE/dA, dF/dA
    const S f5A = c5 * (lf * Ea * DELTA + (lr * Fa - lf * Ea) * beta - (lf * lf * Ea + lr * lr * Fa) * pv);
    const S f6A = c6 * (Ea * DELTA - (Fa + Ea) * beta + (Fa * lr - Ea * lf) * pv);
    const S f5V = c5 * R * pv * rV, f6V = -c6 * (U + M * pv) * rV;
    const S f5W = -c5 * R * rV, f6W = c6 * M * rV - S(1.0);     // d/d psi_dot
    const S gad = ma * dt * (lam[3] + lam[5] * f5A + lam[6] * f6A);
    const S l2d = lam[2] + md * dt * (lam[5] * (c5 * P) + lam[6] * (c6 * E));
    const S l3d = lam[3] + mv * dt * (lam[0] * cp + lam[1] * sp + lam[5] * f5V + lam[6] * f6V);
    const S l5d = lam[5] + dt * (lam[4] + lam[5] * f5W + lam[6] * f6W);
    const S l6d = lam[6] + head + dt * (lam[5] * (c5 * (Q - P)) - lam[6] * (c6 * (F + E)));
    ga = dyn ? gad : gak;
    gsv = ms * dt * lam[2];
    const S l4 = lam[4] + head;
    lam[2] = dyn ? l2d : l2k; lam[3] = dyn ? l3d : l3k; lam[4] = l4;
    lam[5] = dyn ? l5d : lam[5]; lam[6] = dyn ? l6d : lam[6];
  } else if constexpr (MODE == IRBFN_ROLLOUT_FULLINT) {
    const S DT = S(0.1), WB = S(0.33), VMAX = S(7.0), VMIN = S(0.0), SMAX = S(0.4189);
    const S d0 = p[0], v0 = p[1], psi = p[2];
    const S dpre = d0 + sv_in * DT, vpre = v0 + a_in * DT;
    const S d1 = clipf(dpre, -SMAX, SMAX), v1 = clipf(vpre, VMIN, VMAX);
    const S md = clipgrad(dpre, -SMAX, SMAX, tie), mv = clipgrad(vpre, VMIN, VMAX, tie);
    S cp, sp, td;
    trig.sincos_tan(psi, d1, true, sp, cp, td);
    const S Ld = lam[2] + lam[4] * (v1 / WB) * (S(1.0) + td * td) * DT;       // cotangent on delta'
    const S Lv = lam[3] + lam[4] * td * DT / WB;                              // cotangent on v'
    ga = mv * Lv * DT;
    gsv = md * Ld * DT;
    const S l2 = md * Ld;
    const S l3 = mv * Lv + DT * (lam[0] * cp + lam[1] * sp);
    const S l4 = lam[4] + DT * v0 * (-lam[0] * sp + lam[1] * cp);
    lam[2] = l2; lam[3] = l3; lam[4] = l4;
  } else {
    const S LF = dp.p[3], LR = dp.p[4], dt = dp.p[8], sv_max = dp.p[9], a_max = dp.p[10], s_max = dp.p[11];
    const S Lw = LR + LF;
    const S ey = p[0], d_raw = p[1], vx = p[2], epsi = p[3];
    const S dc = clipf(d_raw, -s_max, s_max);
    const S md = clipgrad(d_raw, -s_max, s_max, tie);
    const S ma = clipgrad(a_in, -a_max, a_max, tie), ms = clipgrad(sv_in, -sv_max, sv_max, tie);
    S ce, se, td;
    trig.sincos_tan(epsi, dc, s_max < 4194304.0f, se, ce, td);
    const S den = S(1.0) - ey * cur;
    const S d0 = vx * ce / den;
    const S A = lam[0] * dt - lam[6] * dt * cur;          // total cotangent on d0
    ga = ma * dt * lam[3];
    gsv = ms * dt * lam[2];
    const S l1 = lam[1] + A * (vx * ce * cur / (den * den));
    const S l2 = lam[2] + md * lam[6] * dt * vx * (S(1.0) + td * td) / Lw;
    const S l3 = lam[3] + A * ce / den + lam[1] * dt * se + lam[6] * dt * td / Lw;
    const S l6 = lam[6] + A * (-vx * se / den) + lam[1] * dt * vx * ce;
    const S l7 = lam[7] + A * (vx * ce * ey / (den * den)) - lam[6] * dt * d0;
    lam[1] = l1; lam[2] = l2; lam[3] = l3; lam[6] = l6; lam[7] = l7;
  }
}

// The same one-step Jacobians in forward (JVP) form, for the two single-track modes and the Frenet one (nmpc_solve.hip advances
// the sensitivities S_t = d s_t / d u with them).  jvp_coeffs evaluates, from the state a step STARTS from, the dt-scaled entries
// of F_x = d s' / d s and of d s' / d a that are neither 0 nor 1 -- the coefficient expressions of vjp_back_step above, entry for
// entry; jvp_carry applies them to one tangent, jvp_fresh gives the tangents of this step's own two controls.  The controls are
// taken to lie inside their box (slope 1: the solver keeps them there by projection); the clips of delta and V have
// clipgrad's slope.  ST_KS never moves psi_dot and beta: its tangents have NS = 5 components [x, y, delta, v, psi]; ST_SELECT
// carries all 7 and holds the mask V > 3 constant, a coefficient of the branch not taken being 0 by select (never by a product
// with 0: at V = 0 the dynamic ones are inf / nan).  The NumPy statement is tests/_nmpc_util.py: step_jacobian.
// FRENET_LS never moves vy, wz and curv: its tangents have NS = 5 components [s, ey, delta, vx, epsi] (state components 0, 1, 2,
// 3, 6); vx has no clip in this model.  The NumPy statement is tests/_nmpc_frenet_util.py: step_jacobian.
template <int MODE>
struct StepJac;
template <>
struct StepJac<IRBFN_ROLLOUT_FRENET_LS> {
  static constexpr int NS = 5;
  float s1, s3, s4;        // row s': d / d ey, vx, epsi
  float y3, y4;            // row ey': d / d vx, epsi
  float e1, e2, e3, e4;    // row epsi': d / d ey, delta, vx, epsi (e4 on top of the diagonal 1)
};
template <>
struct StepJac<IRBFN_ROLLOUT_ST_KS> {
  static constexpr int NS = 5;
  float x3, x4, y3, y4, p2, p3;
};
template <>
struct StepJac<IRBFN_ROLLOUT_ST_SELECT> {
  static constexpr int NS = 7;
  float x3, x4, x6, y3, y4, y6, p2, p3, p5;   // rows x', y', psi'
  float w2, w3, w5, w6, wa;                   // row psi_dot' (wa: d / d a)
  float b2, b3, b5, b6, ba;                   // row beta'
};

template <int MODE, typename Trig = TrigDirect>
__device__ __forceinline__ void jvp_coeffs(const float* s, float a_in, float tie, const DynParams& dp, StepJac<MODE>& J,
                                           const Trig trig = Trig()) {
  static_assert(MODE == IRBFN_ROLLOUT_ST_KS || MODE == IRBFN_ROLLOUT_ST_SELECT || MODE == IRBFN_ROLLOUT_FRENET_LS,
                "single-track and Frenet modes only");
  const float lf = dp.p[3], lr = dp.p[4], dt = dp.p[8], s_max = dp.p[11], v_max = dp.p[12];
  const float Lw = lr + lf;
  if constexpr (MODE == IRBFN_ROLLOUT_FRENET_LS) {
    // s = [s, ey, delta, vx, vy, wz, epsi, curv]; with A = dt lam_s - dt curv lam_epsi the total cotangent on d0 = vx ce / den
    // in vjp_back_step<FRENET_LS>, row epsi' holds -curv times row s' beside its own tan term
    const float ey = s[1], d_raw = s[2], vx = s[3], epsi = s[6], cur = s[7];
    const float dc = clipf(d_raw, -s_max, s_max);
    const float md = clipgrad(d_raw, -s_max, s_max, tie);
    float ce, se, td;
    trig.sincos_tan(epsi, dc, s_max < 4194304.0f, se, ce, td);
    const float den = 1.0f - ey * cur;
    J.s1 = dt * (vx * ce * cur / (den * den));
    J.s3 = dt * (ce / den);
    J.s4 = dt * (-vx * se / den);
    J.y3 = dt * se;
    J.y4 = dt * vx * ce;
    J.e1 = -(cur * J.s1);
    J.e2 = md * dt * vx * (1.0f + td * td) / Lw;
    J.e3 = dt * td / Lw - cur * J.s3;
    J.e4 = -(cur * J.s4);
  } else {
    const float d_raw = s[2], v_raw = s[3], psi = s[4];
    const float DELTA = clipf(d_raw, -s_max, s_max), V = clipf(v_raw, -v_max, v_max);
    const float md = clipgrad(d_raw, -s_max, s_max, tie), mv = clipgrad(v_raw, -v_max, v_max, tie);
    float cp, sp, td;
    if constexpr (MODE == IRBFN_ROLLOUT_ST_KS) {
      trig.sincos_tan(psi, DELTA, s_max < 4194304.0f, sp, cp, td);
      J.x3 = mv * dt * cp;
      J.x4 = -(dt * V * sp);
      J.y3 = mv * dt * sp;
      J.y4 = dt * V * cp;
      J.p2 = md * (V / Lw) * (1.0f + td * td) * dt;
      J.p3 = mv * dt * (td / Lw);
    } else {
      const float g = 9.81f;
      const float mu = dp.p[0], m = dp.p[1], I = dp.p[2], C_Sf = dp.p[5], C_Sr = dp.p[6], h = dp.p[7], a_max = dp.p[10];
      const float pd = s[5], beta = s[6];
      const float A = clipf(a_in, -a_max, a_max);
      const bool dyn = V > 3.0f;
      trig.sincos_tan(dyn ? psi + beta : psi, DELTA, s_max < 4194304.0f, sp, cp, td);
      const float head_x = -(dt * V * sp), head_y = dt * V * cp;   // what f0 and f1 put on their angle
      const float glr = g * lr - A * h, glf = g * lf + A * h;
      const float E = C_Sf * glr, F = C_Sr * glf;
      const float P = lf * E, Q = lr * F, R = lf * lf * E + lr * lr * F, M = F * lr - E * lf;
      const float rV = 1.0f / V, pv = pd * rV;
      const float c5 = (mu * m) / (I * Lw), c6 = (mu * rV) / Lw;
      const float U = E * DELTA - (F + E) * beta + M * pv;
      const float Ea = -C_Sf * h, Fa = C_Sr * h;
      const float f5A = c5 * (lf * Ea * DELTA + (lr * Fa - lf * Ea) * beta - (lf * lf * Ea + lr * lr * Fa) * pv);
      const float f6A = c6 * (Ea * DELTA - (Fa + Ea) * beta + (Fa * lr - Ea * lf) * pv);
      const float f5V = c5 * R * pv * rV, f6V = -c6 * (U + M * pv) * rV;
      const float f5W = -c5 * R * rV, f6W = c6 * M * rV - 1.0f;
      J.x3 = mv * dt * cp;
      J.x4 = head_x;
      J.x6 = dyn ? head_x : 0.0f;
      J.y3 = mv * dt * sp;
      J.y4 = head_y;
      J.y6 = dyn ? head_y : 0.0f;
      J.p2 = dyn ? 0.0f : md * (V / Lw) * (1.0f + td * td) * dt;
      J.p3 = dyn ? 0.0f : mv * dt * (td / Lw);
      J.p5 = dyn ? dt : 0.0f;
      J.w2 = dyn ? md * dt * (c5 * P) : 0.0f;
      J.w3 = dyn ? mv * dt * f5V : 0.0f;
      J.w5 = dyn ? dt * f5W : 0.0f;
      J.w6 = dyn ? dt * (c5 * (Q - P)) : 0.0f;
      J.wa = dyn ? dt * f5A : 0.0f;
      J.b2 = dyn ? md * dt * (c6 * E) : 0.0f;
      J.b3 = dyn ? mv * dt * f6V : 0.0f;
      J.b5 = dyn ? dt * f6W : 0.0f;
      J.b6 = dyn ? -(dt * (c6 * (F + E))) : 0.0f;
      J.ba = dyn ? dt * f6A : 0.0f;
    }
  }
}

// d <- F_x d: the tangent of an earlier control through this step
template <int MODE>
__device__ __forceinline__ void jvp_carry(const StepJac<MODE>& J, float* d) {
  if constexpr (MODE == IRBFN_ROLLOUT_ST_KS) {
    const float n0 = d[0] + (J.x3 * d[3] + J.x4 * d[4]);
    const float n1 = d[1] + (J.y3 * d[3] + J.y4 * d[4]);
    const float n4 = d[4] + (J.p2 * d[2] + J.p3 * d[3]);
    d[0] = n0; d[1] = n1; d[4] = n4;
  } else if constexpr (MODE == IRBFN_ROLLOUT_FRENET_LS) {
    const float n0 = d[0] + (J.s1 * d[1] + J.s3 * d[3] + J.s4 * d[4]);
    const float n1 = d[1] + (J.y3 * d[3] + J.y4 * d[4]);
    const float n4 = d[4] + (J.e1 * d[1] + J.e2 * d[2] + J.e3 * d[3] + J.e4 * d[4]);
    d[0] = n0; d[1] = n1; d[4] = n4;
  } else {
    const float n0 = d[0] + (J.x3 * d[3] + J.x4 * d[4] + J.x6 * d[6]);
    const float n1 = d[1] + (J.y3 * d[3] + J.y4 * d[4] + J.y6 * d[6]);
    const float n4 = d[4] + (J.p2 * d[2] + J.p3 * d[3] + J.p5 * d[5]);
    const float n5 = d[5] + (J.w2 * d[2] + J.w3 * d[3] + J.w5 * d[5] + J.w6 * d[6]);
    const float n6 = d[6] + (J.b2 * d[2] + J.b3 * d[3] + J.b5 * d[5] + J.b6 * d[6]);
    d[0] = n0; d[1] = n1; d[4] = n4; d[5] = n5; d[6] = n6;
  }
}

// the tangents d s' / d a_t and d s' / d sv_t of the step's own controls
template <int MODE>
__device__ __forceinline__ void jvp_fresh(const StepJac<MODE>& J, float dt, float* da, float* dsv) {
#pragma unroll
  for (int i = 0; i < StepJac<MODE>::NS; ++i) { da[i] = 0.0f; dsv[i] = 0.0f; }
  da[3] = dt;
  dsv[2] = dt;
  if constexpr (MODE == IRBFN_ROLLOUT_ST_SELECT) { da[5] = J.wa; da[6] = J.ba; }
}

// cotangent of an input row's first S0 columns (roll_init) from the cotangent `lam` of the initial state
template <int MODE>
__device__ __forceinline__ void roll_init_grad(const float* row, const float* lam, float tie, float (&g)[ModeTraits<MODE>::S0]) {
  if constexpr (MODE == IRBFN_ROLLOUT_FULLINT) {
    g[0] = clipgrad(row[0], 0.0f, 7.0f, tie) * lam[3];
  } else {
#pragma unroll
    for (int i = 0; i < ModeTraits<MODE>::S0; ++i) g[i] = lam[i];
  }
}

}  // namespace irbfn
