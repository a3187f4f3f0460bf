// Training-step pieces that sit between the forward (K1) and the parameter VJP (K2), and after it:
// the loss compositions of the reference's train steps (they define the VJP seeds) and the optimiser
// chain, all on device so that a step needs no host round trip (the reference pulls the loss with
// jax.device_get every step, scripts/train_nmpc.py:477-479).
//
//   seeds_oneint  : loss_fn of train_step_oneint  (scripts/train_nmpc.py:268-295)
//   seeds_fullint : loss_fn of train_step_fullint (scripts/train_nmpc.py:306-390)
//   seeds_frenet_fullint : loss_fn of the Frenet train_step_fullint (scripts/train_nmpc_frenet.py:394-421)
//   seeds_st_fullint : a full-integration loss through integrate_st_mult / the kinematic scan (this project's own)
//   adam_clip     : optax.chain(clip_by_global_norm(max_norm), adam(lr)) + apply_gradients
//                   (scripts/train_nmpc.py:231-233, :299)
// All reductions are two-stage with a fixed order (deterministic).
//
// Every kernel and launcher is a template over the scalar S.  S = double is a net trained under the reference's --use_float64
// (scripts/train_nmpc.py:41-42): the one-step maps and adjoints of rollout_step.h / rollout_adjoint.h with DynParams64 and
// ocml's double trigonometry (TrigOf<S>).  Only seeds_fullint has one form per type, see there.
#include <string.h>

#include "common.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"

namespace irbfn {

template <typename S> struct TrigOf { using type = TrigDirect; };
template <> struct TrigOf<double> { using type = TrigF64; };

template <typename S>
__device__ __forceinline__ S sgn(S d) { return d > S(0) ? S(1) : (d < S(0) ? S(-1) : S(0)); }   // d|.| = sign

// ---- train_step_oneint ----------------------------------------------------------------------------
// x[B,D>=7] = [v_c, x_g, y_g, t_g, v_g, beta, angv]; y_pred, y [B,O>=2] = (accel, steer-vel) in cols 0,1.
// initial_state = [0,0,0, x[:,0], 0, x[:,6], x[:,5]]                       (train_nmpc.py:260-266)
// loss = mean(0.5 (y_pred - y)^2) + mean(0.5 (s_pred - s_act)[:, [0,1,3,4]]^2)   (:286-292)
// gy = d loss / d y_pred (through dynamic_st_onestep_aux, dynamics.py:103-187).
template <typename S>
__global__ __launch_bounds__(256) void seeds_oneint_kernel(const S* __restrict__ x, const S* __restrict__ yp,
                                                           const S* __restrict__ y, S* __restrict__ gy,
                                                           S* __restrict__ loss_part, long B, int D, int O,
                                                           typename DynOf<S>::type dp, S tie) {
  using Trig = typename TrigOf<S>::type;
  __shared__ S sm[256];
  S lsum = S(0);
  const S inv_y = S(1) / ((S)B * (S)O), inv_s = S(1) / ((S)B * S(4));
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long)gridDim.x * 256) {
    const S* xb = x + b * D;
    S sp[7] = {S(0), S(0), S(0), xb[0], S(0), xb[6], xb[5]};
    S sa[7] = {S(0), S(0), S(0), xb[0], S(0), xb[6], xb[5]};
    S pk[ModeTraits<IRBFN_ROLLOUT_ST_KS>::NP];
    vjp_park<IRBFN_ROLLOUT_ST_KS>(sp, pk);
    const S ap = yp[b * O + 0], svp = yp[b * O + 1];
    st_step<false, Trig>(sp, ap, svp, dp);                       // predicted_integrated_states  (:276)
    st_step<false, Trig>(sa, y[b * O + 0], y[b * O + 1], dp);    // actual_integrated_states     (:275)
    S lam[7] = {0, 0, 0, 0, 0, 0, 0};
    const int idx[4] = {0, 1, 3, 4};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const S d = sp[idx[k]] - sa[idx[k]];
      lsum += S(0.5) * d * d * inv_s;
      lam[idx[k]] = d * inv_s;
    }
    for (int o = 0; o < O; ++o) {
      const S d = yp[b * O + o] - y[b * O + o];
      lsum += S(0.5) * d * d * inv_y;
      gy[b * O + o] = d * inv_y;
    }
    // adjoint of the kinematic step w.r.t. its controls (oracle/hand_vjp.py: vjp_st_ks, T = 1)
    S ga, gsv;
    vjp_back_step<IRBFN_ROLLOUT_ST_KS, Trig>(pk, ap, svp, lam, S(0), tie, dp, ga, gsv);
    gy[b * O + 0] += ga;
    gy[b * O + 1] += gsv;
  }
  const S tot = block_sum_256(lsum, sm);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = tot;
}

// ---- train_step_fullint ----------------------------------------------------------------------------
// loss = mean|y_pred[:, [0,T]] - y[:, [0,T]]| + mean|final_pred - final_actual|      (train_nmpc.py:386-390;
// the middle term |first_pred - first_pred| is identically 0).  O = 2T.
// TS: the horizon as a compile-time constant (the reference's T = 5: every label / prediction access a register with a static index
// instead of a 16-way select chain), 0 = run-time T <= TMAX
template <int TMAX, int TS = 0>
__global__ __launch_bounds__(256) void seeds_fullint_kernel(const float* __restrict__ x, const float* __restrict__ yp,
                                                            const float* __restrict__ y, float* __restrict__ gy,
                                                            float* __restrict__ loss_part, long B, int D, int Targ,
                                                            float tie) {
  __shared__ float sm[256];
  const int T = TS ? TS : Targ;
  const int O = 2 * T;
  const float DT = 0.1f, WB = 0.33f, VMAX = 7.0f, VMIN = 0.0f, SMAX = 0.4189f;
  const float inv_y = 1.0f / ((float)B * 2.0f), inv_s = 1.0f / ((float)B * 5.0f);
  float lsum = 0.0f;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long)gridDim.x * 256) {
    const float v0 = clipf(x[b * D + 0], VMIN, VMAX);       // :319
    // the row's label and prediction in registers up front (short horizons: the reference's T = 5): the roll-outs below
    // then run without a load in their dependency chain (one load per step: 30 serial round trips per row before)
    constexpr bool REGS = TMAX <= 8;
    float yr[REGS ? 2 * TMAX : 1], pr[REGS ? 2 * TMAX : 1], gr[REGS ? 2 * TMAX : 1];
    if constexpr (REGS) {
#pragma unroll
      for (int o = 0; o < 2 * TMAX; ++o) {
        yr[o] = o < O ? y[b * O + o] : 0.0f;
        pr[o] = o < O ? yp[b * O + o] : 0.0f;
        gr[o] = 0.0f;
      }
    }
    auto lab = [&](int t, int half) -> float {             // control `t` of the label: a_t (half = 0) / sv_t (half = 1)
      if constexpr (REGS && TS != 0) {
        return yr[half * TS + t];                          // t and half are loop constants after unrolling
      } else if constexpr (REGS) {
        float v = 0.0f;
#pragma unroll
        for (int o = 0; o < 2 * TMAX; ++o) v = (o == half * T + t) ? yr[o] : v;
        return v;
      } else {
        return y[b * O + half * T + t];
      }
    };
    auto prd = [&](int t, int half) -> float {
      if constexpr (REGS && TS != 0) {
        return pr[half * TS + t];
      } else if constexpr (REGS) {
        float v = 0.0f;
#pragma unroll
        for (int o = 0; o < 2 * TMAX; ++o) v = (o == half * T + t) ? pr[o] : v;
        return v;
      } else {
        return yp[b * O + half * T + t];
      }
    };
    float sa[5] = {0.0f, 0.0f, 0.0f, v0, 0.0f};
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
      if (t < T) fullint_step(sa, lab(t, 0), lab(t, 1));     // :329-347
    float sp[5] = {0.0f, 0.0f, 0.0f, v0, 0.0f};
    float pd[TMAX], pv[TMAX], pp[TMAX];                       // delta, v, yaw before step t
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t < T) {
        pd[t] = sp[2]; pv[t] = sp[3]; pp[t] = sp[4];
        fullint_step(sp, prd(t, 0), prd(t, 1));               // :356-374
      }
    }
    float lam[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float d = sp[i] - sa[i];
      lsum += fabsf(d) * inv_s;
      lam[i] = sgn(d) * inv_s;    // d|.| = sign
    }
    if constexpr (!REGS)
      for (int o = 0; o < O; ++o) gy[b * O + o] = 0.0f;
    auto put = [&](int o_idx, float v) {
      if constexpr (REGS) {
#pragma unroll
        for (int o = 0; o < 2 * TMAX; ++o) gr[o] = (o == o_idx) ? v : gr[o];
      } else {
        gy[b * O + o_idx] = v;
      }
    };
    // reverse sweep (oracle/hand_vjp.py: vjp_fullint): vjp_back_step<FULLINT> written out.  Calling it here changed which
    // multiply-adds the compiler contracts, and with them the last bits of the T = 5 gradients.
#pragma unroll
    for (int t = TMAX - 1; t >= 0; --t) {
      if (t < T) {
        const float a = prd(t, 0), dv = prd(t, 1);
        const float dpre = pd[t] + dv * DT, vpre = pv[t] + a * DT;
        const float d1 = clipf(dpre, -SMAX, SMAX), v1 = clipf(vpre, VMIN, VMAX);
        const float md = clipgrad(dpre, -SMAX, SMAX, tie), mv = clipgrad(vpre, VMIN, VMAX, tie);
        float sn, cs;
        sincos_fast(pp[t], sn, cs);
        const float td = tan_fast(d1);
        const float Ld = lam[2] + lam[4] * (v1 / WB) * (1.0f + td * td) * DT;
        const float Lv = lam[3] + lam[4] * td * DT / WB;
        put(t, mv * Lv * DT);
        put(T + t, md * Ld * DT);
        const float l2 = md * Ld;
        const float l3 = mv * Lv + DT * (lam[0] * cs + lam[1] * sn);
        const float l4 = lam[4] + DT * pv[t] * (-lam[0] * sn + lam[1] * cs);
        lam[2] = l2; lam[3] = l3; lam[4] = l4;
      }
    }
    const int cols[2] = {0, T};                               // y_predictions[:, [0, 5]]  (:387)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float d = prd(0, k) - lab(0, k);                  // column k * T
      lsum += fabsf(d) * inv_y;
      const float sg = sgn(d) * inv_y;
      if constexpr (REGS) {
#pragma unroll
        for (int o = 0; o < 2 * TMAX; ++o) gr[o] += (o == cols[k]) ? sg : 0.0f;
      } else {
        gy[b * O + cols[k]] += sg;
      }
    }
    if constexpr (REGS) {
#pragma unroll
      for (int o = 0; o < 2 * TMAX; ++o)
        if (o < O) gy[b * O + o] = gr[o];
    }
  }
  const float tot = block_sum_256(lsum, sm);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = tot;
}

// The same loss in float64: vjp_park / fullint_step / vjp_back_step<FULLINT> in a plain loop over T <= TMAX.  The float32
// form above is a different algorithm (register-resident rows, static indices, a written-out reverse sweep whose contraction
// the T = 5 gradients depend on), so the two stay side by side.
template <int TMAX>
__global__ __launch_bounds__(256) void seeds_fullint_f64_kernel(const double* __restrict__ x, const double* __restrict__ yp,
                                                                const double* __restrict__ y, double* __restrict__ gy,
                                                                double* __restrict__ loss_part, long B, int D, int T,
                                                                double tie) {
  __shared__ double sm[256];
  const int O = 2 * T;
  const DynParams64 dp = {};                                 // the inline bicycle has its own constants (:307-311)
  const double inv_y = 1.0 / ((double)B * 2.0), inv_s = 1.0 / ((double)B * 5.0);
  double lsum = 0.0;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long)gridDim.x * 256) {
    const double* yr = y + b * O;
    const double* pr = yp + b * O;
    double* gr = gy + b * O;
    const double v0 = clipf(x[b * D + 0], 0.0, 7.0);       // :319
    double sa[5] = {0.0, 0.0, 0.0, v0, 0.0};
    for (int t = 0; t < T; ++t) fullint_step<TrigF64>(sa, yr[t], yr[T + t]);       // :329-347
    double sp[5] = {0.0, 0.0, 0.0, v0, 0.0};
    double pk[TMAX][ModeTraits<IRBFN_ROLLOUT_FULLINT>::NP];
    for (int t = 0; t < T; ++t) {
      vjp_park<IRBFN_ROLLOUT_FULLINT>(sp, pk[t]);
      fullint_step<TrigF64>(sp, pr[t], pr[T + t]);                                 // :356-374
    }
    double lam[5];
    for (int i = 0; i < 5; ++i) {
      const double d = sp[i] - sa[i];
      lsum += fabs(d) * inv_s;
      lam[i] = sgn(d) * inv_s;
    }
    for (int t = T - 1; t >= 0; --t) {
      double ga, gsv;
      vjp_back_step<IRBFN_ROLLOUT_FULLINT, TrigF64>(pk[t], pr[t], pr[T + t], lam, 0.0, tie, dp, ga, gsv);
      gr[t] = ga;
      gr[T + t] = gsv;
    }
    for (int k = 0; k < 2; ++k) {                            // y_predictions[:, [0, T]]  (:387)
      const double d = pr[k * T] - yr[k * T];
      lsum += fabs(d) * inv_y;
      gr[k * T] += sgn(d) * inv_y;
    }
  }
  const double tot = block_sum_256(lsum, sm);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = tot;
}

// ---- the multi-step losses: every state of a T-step roll-out against the label's roll-out --------------------------------
// loss = mean|y_pred - y| + mean|roll([init, y_pred])[:, :, comps] - roll([init, y])[:, :, comps]| over all T states; gy = d loss /
// d y_pred through the roll-out's adjoint (rollout_adjoint.h).  O = 2T.  What a mode adds to ModeTraits (rollout_step.h) for it:
// the initial state from a query row, the NSEED seeded state components comp(0 .. NSEED), the curvature vjp_back_step takes,
// the step, and whether a float64 form exists.
template <int MODE>
struct SeedTraits;
// Frenet train_step_fullint (scripts/train_nmpc_frenet.py:394-421): x[B,8] = [ey, delta, vx_car, vy_car, vx_goal, wz, epsi, curv];
// initial_state = x[:, [0,0,1,2,3,5,6,7]] (:398); integrate_frenet_mult (:402-412; all 8 components; the adjoint of
// dynamics.py:190-290, low-speed RHS)
template <>
struct SeedTraits<IRBFN_ROLLOUT_FRENET_LS> {
  static constexpr int NSEED = 8;
  static constexpr bool F64 = true;
  __device__ static constexpr int comp(int k) { return k; }
  template <typename S>
  __device__ static void init(const S* xb, S (&s)[8]) {
    const S s0[8] = {xb[0], xb[0], xb[1], xb[2], xb[3], xb[5], xb[6], xb[7]};
    for (int i = 0; i < 8; ++i) s[i] = s0[i];
  }
  template <typename S>
  __device__ static S cur(const S (&s)[8]) { return s[7]; }
  template <typename Trig, typename S>
  __device__ static void step(S (&s)[8], S a, S sv, const typename DynOf<S>::type& dp) { frenet_step<Trig>(s, a, sv, dp); }
};
// single-track full integration (no reference counterpart; include/irbfn_hip.h: irbfn_train_seeds_st_fullint): x[B,D>=7] and the
// initial state as seeds_oneint; SELECT: integrate_st_mult's model (select(V > 3, dynamic, kinematic), the planner's roll-out) with
// the adjoint of the branch each step took, else the kinematic model alone; components [0,1,3,4].  float32 only.
template <bool SELECT>
struct SeedTraitsSt {
  static constexpr int NSEED = 4;
  static constexpr bool F64 = false;
  __device__ static constexpr int comp(int k) { return k < 2 ? k : k + 1; }
  template <typename S>
  __device__ static void init(const S* xb, S (&s)[7]) {
    const S s0[7] = {S(0), S(0), S(0), xb[0], S(0), xb[6], xb[5]};
    for (int i = 0; i < 7; ++i) s[i] = s0[i];
  }
  template <typename S>
  __device__ static S cur(const S (&)[7]) { return S(0); }
  template <typename Trig, typename S>
  __device__ static void step(S (&s)[7], S a, S sv, const typename DynOf<S>::type& dp) { st_step<SELECT, Trig>(s, a, sv, dp); }
};
template <> struct SeedTraits<IRBFN_ROLLOUT_ST_SELECT> : SeedTraitsSt<true> {};
template <> struct SeedTraits<IRBFN_ROLLOUT_ST_KS> : SeedTraitsSt<false> {};

// The loop shape follows S.  float: both sweeps unrolled to TMAX under a t < T guard, so park / seed stay in registers.
// double: rolled loops over T (ROLLED); unrolled, the Frenet kernel grows from 1768 to 6719 instructions at TMAX = 5 (22 364 at 16).
template <int MODE, int TMAX, typename S>
__global__ __launch_bounds__(256) void seeds_multistep_kernel(const S* __restrict__ x, const S* __restrict__ yp,
                                                              const S* __restrict__ y, S* __restrict__ gy,
                                                              S* __restrict__ loss_part, long B, int D, int T,
                                                              typename DynOf<S>::type dp, S tie) {
  using Trig = typename TrigOf<S>::type;
  using M = SeedTraits<MODE>;
  constexpr bool ROLLED = std::is_same<S, double>::value;
  static_assert(M::F64 || !ROLLED, "this mode has no float64 form");
  constexpr int UNROLL = ROLLED ? 1 : TMAX, NS = ModeTraits<MODE>::S, NSEED = M::NSEED;
  __shared__ S sm[256];
  const int O = 2 * T, TN = ROLLED ? T : TMAX;                                // trip count of the two sweeps
  const S inv_y = S(1) / ((S)B * (S)O), inv_s = S(1) / ((S)B * (S)T * S(NSEED));
  S lsum = S(0);
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long)gridDim.x * 256) {
    S sa[NS], sp[NS];
    M::init(x + b * D, sa);
    M::init(x + b * D, sp);
    const S cur = M::cur(sp);
    S park[TMAX][ModeTraits<MODE>::NP], seed[TMAX][NSEED];
#pragma unroll UNROLL
    for (int t = 0; t < TN; ++t) {
      if (ROLLED || t < T) {
        M::template step<Trig>(sa, y[b * O + t], y[b * O + T + t], dp);       // the label's states
        vjp_park<MODE>(sp, park[t]);
        M::template step<Trig>(sp, yp[b * O + t], yp[b * O + T + t], dp);     // the prediction's
#pragma unroll
        for (int k = 0; k < NSEED; ++k) {
          const S d = sp[M::comp(k)] - sa[M::comp(k)];
          lsum += fabs(d) * inv_s;
          seed[t][k] = sgn(d) * inv_s;
        }
      }
    }
    S lam[NS] = {};
#pragma unroll UNROLL
    for (int t = TN - 1; t >= 0; --t) {
      if (ROLLED || t < T) {
#pragma unroll
        for (int k = 0; k < NSEED; ++k) lam[M::comp(k)] += seed[t][k];
        S ga, gsv;
        vjp_back_step<MODE, Trig>(park[t], yp[b * O + t], yp[b * O + T + t], lam, cur, tie, dp, ga, gsv);
        gy[b * O + t] = ga;
        gy[b * O + T + t] = gsv;
      }
    }
    for (int o = 0; o < O; ++o) {                             // pred_loss = |y_pred - y|.mean()
      const S d = yp[b * O + o] - y[b * O + o];
      lsum += fabs(d) * inv_y;
      gy[b * O + o] += sgn(d) * inv_y;
    }
  }
  const S tot = block_sum_256(lsum, sm);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = tot;
}

template <typename S>
__global__ __launch_bounds__(256) void final_sum_kernel(const S* __restrict__ part, int n, S* __restrict__ out) {
  __shared__ S sm[256];
  S v = S(0);
  for (int i = threadIdx.x; i < n; i += 256) v += part[i];
  const S tot = block_sum_256(v, sm);
  if (threadIdx.x == 0) out[0] = tot;
}

// ---- optimiser: clip_by_global_norm + adam ----------------------------------------------------------
// Also hands the incremented step count to adam_clip_kernel through the int at the start of part[kRedBlocks] (the buffer
// holds kSeedBlocksMax scalars): every block of the Adam kernel reads THAT word, its thread (0, 0) stores it back to
// step[0] -- no block reads step[0] there, so no separate "bump" launch is needed.
template <typename S>
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const S* __restrict__ g, long n, S* __restrict__ part,
                                                             const int* __restrict__ step) {
  __shared__ S sm[256];
  if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int*>(part + kRedBlocks)[0] = step[0] + 1;
  S v = S(0);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) v += g[i] * g[i];
  const S tot = block_sum_256(v, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// optax.clip_by_global_norm: g <- g if ||g|| < max_norm else g / ||g|| * max_norm.
// optax.adam (scale_by_adam, eps_root = 0): m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ;
//   update = -lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) ; t is the incremented count.
template <typename S>
__global__ __launch_bounds__(256) void adam_clip_kernel(S* __restrict__ p, const S* __restrict__ g,
                                                        S* __restrict__ m, S* __restrict__ v, long n,
                                                        int* __restrict__ step, const S* __restrict__ part,
                                                        S lr, S b1, S b2, S eps, S max_norm) {
  __shared__ S sm[256];
  const S sq = block_sum_256(threadIdx.x < kRedBlocks ? part[threadIdx.x] : S(0), sm);   // same in every block
  const S gn = sqrt(sq);
  const S scale = (max_norm > S(0) && !(gn < max_norm)) ? max_norm / gn : S(1);
  const int t = reinterpret_cast<const int*>(part + kRedBlocks)[0];   // step[0] + 1, written by sqnorm_partial_kernel
  if (blockIdx.x == 0 && threadIdx.x == 0) step[0] = t;
  const S c1 = S(1) - pow(b1, (S)t), c2 = S(1) - pow(b2, (S)t);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const S gi = g[i] * scale;
    const S mi = b1 * m[i] + (S(1) - b1) * gi;
    const S vi = b2 * v[i] + (S(1) - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr * (mi / c1) / (sqrt(vi / c2) + eps);
  }
}

// ---- launchers: one per step, S = float / double (the argument rules and status codes of both entry points) -----------------

// blocks of the loss / seed kernels: one row per thread (a second pass over the rows doubled the kernel: 18 -> 9 us at the
// reference's batch of 80000), grid-stride beyond kSeedBlocksMax * 256 rows
static int seed_blocks(int64_t B) {
  const int64_t nb = (B + 255) / 256;
  return nb < 1 ? 1 : (nb > kSeedBlocksMax ? kSeedBlocksMax : (int)nb);
}

// the shared tail of the three seed launchers: the launch status of the seed kernel, then the loss from its partials
template <typename S>
static int finish_loss(S* partials_dev, S* loss_dev, int64_t B, hipStream_t s) {
  IRBFN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(final_sum_kernel<S>, dim3(1), dim3(256), 0, s, partials_dev, seed_blocks(B), loss_dev);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

template <typename S>
static int train_seeds_oneint(const S* x_dev, const S* y_pred_dev, const S* y_dev, const S* dyn_params_host, S clip_tie,
                              S* gy_dev, S* loss_dev, S* partials_dev, int64_t B, int D, int O, void* stream) {
  if (B < 0 || D < 7 || O < 2 || !dyn_params_host) return IRBFN_ERR_BAD_ARG;
  if (B > 0 && (!x_dev || !y_pred_dev || !y_dev || !gy_dev)) return IRBFN_ERR_BAD_ARG;
  if (!loss_dev || !partials_dev) return IRBFN_ERR_BAD_ARG;
  typename DynOf<S>::type dp;
  memcpy(dp.p, dyn_params_host, sizeof(dp.p));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(seeds_oneint_kernel<S>, dim3(seed_blocks(B)), dim3(256), 0, s, x_dev, y_pred_dev, y_dev, gy_dev,
                     partials_dev, (long)B, D, O, dp, clip_tie);
  return finish_loss(partials_dev, loss_dev, B, s);
}

template <typename S>
static int train_seeds_fullint(const S* x_dev, const S* y_pred_dev, const S* y_dev, S clip_tie, S* gy_dev, S* loss_dev,
                               S* partials_dev, int64_t B, int D, int T, void* stream) {
  if (B < 0 || D < 1 || T < 1) return IRBFN_ERR_BAD_ARG;
  if (T > 64) return IRBFN_ERR_UNSUPPORTED;
  if (B > 0 && (!x_dev || !y_pred_dev || !y_dev || !gy_dev)) return IRBFN_ERR_BAD_ARG;
  if (!loss_dev || !partials_dev) return IRBFN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(seed_blocks(B)), block(256);
#define IRBFN_SEEDS_FULLINT(KERNEL) \
  hipLaunchKernelGGL(KERNEL, grid, block, 0, s, x_dev, y_pred_dev, y_dev, gy_dev, partials_dev, (long)B, D, T, clip_tie)
  if constexpr (std::is_same<S, float>::value) {
    if (T == 5) IRBFN_SEEDS_FULLINT((seeds_fullint_kernel<8, 5>));    // the reference's horizon (train_nmpc.py:306-374)
    else if (T <= 8) IRBFN_SEEDS_FULLINT((seeds_fullint_kernel<8>));
    else IRBFN_SEEDS_FULLINT((seeds_fullint_kernel<64>));
  } else {
    if (T <= 8) IRBFN_SEEDS_FULLINT((seeds_fullint_f64_kernel<8>));
    else IRBFN_SEEDS_FULLINT((seeds_fullint_f64_kernel<64>));
  }
#undef IRBFN_SEEDS_FULLINT
  return finish_loss(partials_dev, loss_dev, B, s);
}

// the instances unroll to 5 steps (the reference's horizon) or to 16
template <int MODE, typename S>
static int train_seeds_multistep(const S* x_dev, const S* y_pred_dev, const S* y_dev, const S* dyn_params_host, S clip_tie,
                                 S* gy_dev, S* loss_dev, S* partials_dev, int64_t B, int D, int T, void* stream) {
  if (B < 0 || D < ModeTraits<MODE>::S0 || T < 1 || T > 16 || !dyn_params_host) return IRBFN_ERR_BAD_ARG;
  if (B > 0 && (!x_dev || !y_pred_dev || !y_dev || !gy_dev)) return IRBFN_ERR_BAD_ARG;
  if (!loss_dev || !partials_dev) return IRBFN_ERR_BAD_ARG;
  typename DynOf<S>::type dp;
  memcpy(dp.p, dyn_params_host, sizeof(dp.p));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto kernel = T <= 5 ? seeds_multistep_kernel<MODE, 5, S> : seeds_multistep_kernel<MODE, 16, S>;
  hipLaunchKernelGGL(kernel, dim3(seed_blocks(B)), dim3(256), 0, s, x_dev, y_pred_dev, y_dev, gy_dev, partials_dev, (long)B, D, T, dp,
                     clip_tie);
  return finish_loss(partials_dev, loss_dev, B, s);
}

template <typename S>
static int adam_clip_step(S* params_dev, const S* grads_dev, S* m_dev, S* v_dev, int64_t n, int* step_dev, S lr, S beta1,
                          S beta2, S eps, S max_grad_norm, S* partials_dev, void* stream) {
  if (n < 0 || !step_dev || !partials_dev) return IRBFN_ERR_BAD_ARG;
  if (n > 0 && (!params_dev || !grads_dev || !m_dev || !v_dev)) return IRBFN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sqnorm_partial_kernel<S>, dim3(kRedBlocks), dim3(256), 0, s, grads_dev, (long)n, partials_dev, step_dev);
  IRBFN_HIP_CHECK(hipGetLastError());
  long blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_clip_kernel<S>, dim3((unsigned)blocks), dim3(256), 0, s, params_dev, grads_dev, m_dev, v_dev,
                     (long)n, step_dev, partials_dev, lr, beta1, beta2, eps, max_grad_norm);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int irbfn_train_loss_partials(void) { return kSeedBlocksMax; }

int irbfn_train_seeds_oneint(const float* x_dev, const float* y_pred_dev, const float* y_dev,
                             const float* dyn_params_host, float clip_tie, float* gy_dev, float* loss_dev,
                             float* partials_dev, int64_t B, int D, int O, void* stream) {
  return train_seeds_oneint(x_dev, y_pred_dev, y_dev, dyn_params_host, clip_tie, gy_dev, loss_dev, partials_dev, B, D, O, stream);
}

int irbfn_train_seeds_fullint(const float* x_dev, const float* y_pred_dev, const float* y_dev, float clip_tie,
                              float* gy_dev, float* loss_dev, float* partials_dev, int64_t B, int D, int T,
                              void* stream) {
  return train_seeds_fullint(x_dev, y_pred_dev, y_dev, clip_tie, gy_dev, loss_dev, partials_dev, B, D, T, stream);
}

int irbfn_train_seeds_frenet_fullint(const float* x_dev, const float* y_pred_dev, const float* y_dev,
                                     const float* dyn_params_host, float clip_tie, float* gy_dev, float* loss_dev,
                                     float* partials_dev, int64_t B, int D, int T, void* stream) {
  return train_seeds_multistep<IRBFN_ROLLOUT_FRENET_LS>(x_dev, y_pred_dev, y_dev, dyn_params_host, clip_tie, gy_dev, loss_dev,
                                                        partials_dev, B, D, T, stream);
}

int irbfn_train_seeds_st_fullint(int mode, const float* x_dev, const float* y_pred_dev, const float* y_dev,
                                 const float* dyn_params_host, float clip_tie, float* gy_dev, float* loss_dev,
                                 float* partials_dev, int64_t B, int D, int T, void* stream) {
  if (mode == IRBFN_ROLLOUT_ST_SELECT)
    return train_seeds_multistep<IRBFN_ROLLOUT_ST_SELECT>(x_dev, y_pred_dev, y_dev, dyn_params_host, clip_tie, gy_dev, loss_dev,
                                                          partials_dev, B, D, T, stream);
  if (mode == IRBFN_ROLLOUT_ST_KS)
    return train_seeds_multistep<IRBFN_ROLLOUT_ST_KS>(x_dev, y_pred_dev, y_dev, dyn_params_host, clip_tie, gy_dev, loss_dev,
                                                      partials_dev, B, D, T, stream);
  return IRBFN_ERR_BAD_ARG;
}

int irbfn_adam_clip_step(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, int64_t n,
                         int* step_dev, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                         float* partials_dev, void* stream) {
  return adam_clip_step(params_dev, grads_dev, m_dev, v_dev, n, step_dev, lr, beta1, beta2, eps, max_grad_norm, partials_dev,
                        stream);
}

int irbfn_train_seeds_oneint_f64(const double* x_dev, const double* y_pred_dev, const double* y_dev,
                                 const double* dyn_params_host, double clip_tie, double* gy_dev, double* loss_dev,
                                 double* partials_dev, int64_t B, int D, int O, void* stream) {
  return train_seeds_oneint(x_dev, y_pred_dev, y_dev, dyn_params_host, clip_tie, gy_dev, loss_dev, partials_dev, B, D, O, stream);
}

int irbfn_train_seeds_fullint_f64(const double* x_dev, const double* y_pred_dev, const double* y_dev, double clip_tie,
                                  double* gy_dev, double* loss_dev, double* partials_dev, int64_t B, int D, int T,
                                  void* stream) {
  return train_seeds_fullint(x_dev, y_pred_dev, y_dev, clip_tie, gy_dev, loss_dev, partials_dev, B, D, T, stream);
}

int irbfn_train_seeds_frenet_fullint_f64(const double* x_dev, const double* y_pred_dev, const double* y_dev,
                                         const double* dyn_params_host, double clip_tie, double* gy_dev, double* loss_dev,
                                         double* partials_dev, int64_t B, int D, int T, void* stream) {
  return train_seeds_multistep<IRBFN_ROLLOUT_FRENET_LS>(x_dev, y_pred_dev, y_dev, dyn_params_host, clip_tie, gy_dev, loss_dev,
                                                        partials_dev, B, D, T, stream);
}

int irbfn_adam_clip_step_f64(double* params_dev, const double* grads_dev, double* m_dev, double* v_dev, int64_t n,
                             int* step_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm,
                             double* partials_dev, void* stream) {
  return adam_clip_step(params_dev, grads_dev, m_dev, v_dev, n, step_dev, lr, beta1, beta2, eps, max_grad_norm, partials_dev,
                        stream);
}

}  // extern "C"
