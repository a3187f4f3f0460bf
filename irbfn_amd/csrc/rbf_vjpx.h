// K5 / K5m: VJP of WCRBFNet.apply with respect to the QUERY x (replaces jax.grad(lambda x: apply(params, x)); nothing in the
// reference takes it).  Notation of SURVEY App. A: u = d^2 = r^2 exp(-2 log_sig), phi = f(u), hbar = gout W^T [B,K], gamma [B,R]:
//
//   gx[b,:] = 2 sum_{r,k} hbar[b,k] gamma[b,r] f'(u_brk) sigma_rk^-2 (x_b - c_rk)          (RBF term)
//           +   sum_r     q[b,r] d gamma[b,r] / d x_b,    q[b,r] = sum_k hbar[b,k] phi[b,r,k]   (gate term)
//
// The x-VJP is query-stationary: no reduction over the batch, no workspace, no atomics.  It has the shape of the forward (K1,
// rbf_forward.h), not of the parameter VJP (K2): one lane owns one query -- x, the cotangent row gout[b,:] and the D running
// sums live in VGPRs -- and the NW waves of a workgroup share 64 queries and split the N = R K centres.  The packed centre
// records of the forward (centre, folded width scale, weight row; pack_all.hip) are wave-uniform and stream through the scalar
// cache as in K1.  Per (query, centre) pair: the D differences (kept), r^2, one transcendental, hbar as OP FMAs against the
// record's weight row, then D FMAs of s (x - c).  The sums run over the kept differences, never over x sum(s) - sum(s c).
//
// Gate term: d gamma_r / d x_d = gamma_r delta_d [tanh(delta_d (hi - x_d)) - tanh(delta_d (x_d - lo))] for d < nsplit
// (model.py:74-93).  With a = (tanh(z1) + 1) / 2 and b = (tanh(z2) + 1) / 2 the bracket is 2 ((1 - a) - (1 - b)); 1 - a is
// evaluated as e / (1 + e), e = exp(-2 z1), for z1 >= 0 (no cancellation deep inside a region) and as 1 - a for z1 < 0 (a <= 1/2;
// e may be inf there), so it is bounded by 1 and a region whose gamma is 0 contributes exactly 0, never 0 * inf.
// THE ZERO OF THE GATE IS FLOAT64'S HERE (z < -53/2 ln 2 = -18.37, where a float64 tanh is exactly -1), not the forward's float32
// zero (z < -9.01, rbf_forward.h): the forward drops factors below 1.5e-8 of a region's own output, but in the gradient such a
// region still carries gamma_B dlog_B q_B = 1.5e-8 * 2 delta * q_B, the counterpart of its neighbour's -(1 - b_A) 2 delta q_A, and
// the two cancel to 2 delta 1.5e-8 (q_B - q_A).  Dropping one of them (or both) leaves an error of 2 delta 1.5e-8 |q| that is not
// small against the RBF term of a wide basis: measured 1.7e-5 of the sum of absolute terms on the gaussian_wider case of
// tests/test_gpu_vjpx.py with the float32 zero, 6 times the tests' bound (profiles/vjp_x_parity.txt).  Regions further than
// 18.37 / delta outside their bounds are still skipped by a whole wave, as in K1.
// A wave folds gamma_r dlog_rd q_r into its D sums as soon as its share of region r's centres is done (q is linear in the
// centres, so the waves' shares add up): nothing of size R stays in registers, R = 500 costs what R = 1 costs.
// With caller-provided region weights (ClusterWCRBFNet) the kernel returns the RBF term and, on request, dgamma[b,r] = q[b,r];
// the waves then split whole regions, so that one wave owns all of q[b,r].
//
// A query exactly ON a centre: the pair's RBF term is 0, the limit or a convention (basis_value_slope_finite, rbf_basis.h).
#pragma once

#include "rbf_forward.h"

namespace irbfn {

struct VjpxArgs {
  const float* __restrict__ x;          // [B][Dreal]
  const float* __restrict__ g;          // [B][O]   cotangent of the output
  const float* __restrict__ rec;        // [N][S]   the forward's packed records
  const float* __restrict__ gamma_ext;  // [B][R]   caller-provided region weights (no gate term), or null
  float* __restrict__ gx;               // [B][Dreal]
  float* __restrict__ dgamma;           // [B][R]   q[b,r] (gamma_ext only), or null
  GateTables gate;
  long B;
  int Dreal, O, N, K, R, S, basis;
  int region_split;                     // waves split whole regions (dgamma): one wave owns q[b,r]
};

// the x-VJP's kernel and geometry (plan_vjp_x, rbf_vjpx.hip)
enum VjpxKind : int { VX_NONE = 0, VX_K5 = 1, VX_K5M = 2 };
struct VjpxPlan {
  int kind = VX_NONE;
  int status = IRBFN_ERR_UNSUPPORTED;
  int nw = 0;                           // waves per workgroup
  size_t lds = 0;
  long grid = 0;
  int block = 0;
};

// 2 f'(u) sigma^-2 = kVjpxScale<BC> * (phi-dependent factor) * sc, with sc the record's folded scale (rbf_forward.h):
//   BC_GAUSS: f' = -a phi, sc = -a log2(e) sigma^-2   ->  2 ln 2 * phi * sc
//   BC_IQ:    f' = -phi^2                              -> -2 * phi^2 * sc
//   BC_IMQ:   f' = -phi^3 / 2                          -> -1 * phi^3 * sc
//   generic:  basis_value_slope_finite (rbf_basis.h)   ->  2 * f' * sc
template <int BC>
__host__ __device__ constexpr float vjpx_scale() {
  return BC == BC_GAUSS ? 1.3862943611198906f : (BC == BC_IQ ? -2.0f : (BC == BC_IMQ ? -1.0f : 2.0f));
}

// phi and the phi-dependent factor of f' for the fast classes, from the transcendental's result
template <int BC>
__device__ __forceinline__ float vjpx_fast_factor(float phi) {
  if constexpr (BC == BC_GAUSS) return phi;
  else if constexpr (BC == BC_IQ) return phi * phi;
  else return phi * phi * phi;
}

// one factor pair of the gate and its logarithmic derivative: *fac = a b with float64's zero (header comment),
// returns d log(a b) / d x = 2 delta ((1 - a) - (1 - b)).  NaN propagates (every comparison is false).
constexpr float kGateSatZ64 = 18.368f;           // 53/2 ln 2
__device__ __forceinline__ float gate_factor_dlog(float xv, float lo, float hi, float delta, float* fac) {
  const float z1 = delta * (xv - lo), z2 = delta * (hi - xv);
  const float e1 = fast_exp2(-2.0f * kLog2e<float> * z1), e2 = fast_exp2(-2.0f * kLog2e<float> * z2);
  const float a = fast_rcp(1.0f + e1), b = fast_rcp(1.0f + e2);
  const float fa = z1 < -kGateSatZ64 ? 0.0f : a, fb = z2 < -kGateSatZ64 ? 0.0f : b;
  const float na = z1 < 0.0f ? 1.0f - a : e1 * a, nb = z2 < 0.0f ? 1.0f - b : e2 * b;
  *fac = fa * fb;
  return 2.0f * delta * (na - nb);
}

// per-D instantiations (rbf_vjpx_kernels.hip)
int launch_vjpx_d3(const VjpxArgs&, int OP, int bc, int nw, size_t lds, hipStream_t);
int launch_vjpx_d4(const VjpxArgs&, int OP, int bc, int nw, size_t lds, hipStream_t);
int launch_vjpx_d7(const VjpxArgs&, int OP, int bc, int nw, size_t lds, hipStream_t);
int launch_vjpx_d8(const VjpxArgs&, int OP, int bc, int nw, size_t lds, hipStream_t);
// K5m (rbf_vjpx_mfma.hip): K1m's records (one region, fast basis class, d = 2..8, O <= 128)
bool vjpxm_eligible(const irbfn_net* net);
bool vjpxm_preferred(const irbfn_net* net, int64_t B, bool ext);
int vjpxm_width(const irbfn_net* net);
VjpxPlan plan_vjpx_mfma(const irbfn_net* net, int64_t B);
int launch_vjpx_mfma(irbfn_net* net, const VjpxPlan& p, const float* x, const float* gout, float* gx, int64_t B, hipStream_t s);

}  // namespace irbfn
