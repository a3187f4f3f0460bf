// Hand-derived one-step adjoints of the roll-out models (reverse-mode of rollout_step.h), shared by the roll-out VJP
// kernels (rollout_vjp.hip) and the loss-seed kernels of the training steps (train_step.hip).  The NumPy statement
// of the same adjoints is oracle/hand_vjp.py (checked against torch.autograd of the restatement to 1e-12).
// clip() gradient: 1 strictly inside, 0 strictly outside, `tie` on a bound (jnp.clip is minimum(maximum(.)), whose
// tie rule is 1/2).
// clipgrad, vjp_park and vjp_back_step<ST_KS / FULLINT / FRENET_LS> take their scalar type S as a template parameter (float
// by default; S = double with TrigF64 and DynParams64: the float64 training steps).
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
