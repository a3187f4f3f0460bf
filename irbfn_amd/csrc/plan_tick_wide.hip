// The planning tick of BASELINE config 4 in ONE launch: fused RBF forward with wide outputs (O = 2T = 100 control
// knots, rbf_forward_f16_wide.h) -> the block's 32-query x 100-control tiles stay in LDS -> its slice-0 waves integrate
// the trajectories (K3p core, rollout_pair.h) and write the states as whole 128-byte lines.  Replaces the
// forward + sign flip + roll-out launches of launch_forward_rollout (src/irbfn_mpc/irbfn_planner.py:203-210) where
// the instance exists (d = 7, 96 < O <= 112, single-track modes); same bits as the separate launches (the forward's
// arithmetic and geometry, the step functions and the flush are shared code).
// Compiled with the roll-out's flags (the 50-knot register arrays need the full unroll).
#include "rbf_forward_gram_wide.h"

namespace irbfn {

template <int DC, int BC, int NT, int MODE>
__global__ __launch_bounds__(512) void rbf_tick_f16mfma_wide(const F16Args a, const F16Roll r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  wide_pipe_body<DC, BC, NT, MODE>(a, r, lds);
}

// the same tick on K1g's wide body (rbf_forward_gram_wide.h): the distances on the matrix cores as well
template <int DC, int BC, int NT, int MODE>
__global__ __launch_bounds__(512) void rbf_tick_f16gram_wide(const GramArgs a, const F16Roll r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  wide_gram_body<DC, BC, NT, MODE>(a, r, lds);
}

// is the one-launch tick compiled for this net / horizon / mode?
bool tick_wide_compiled(const irbfn_net* net, int mode, int T) {
  if (mode != IRBFN_ROLLOUT_ST_SELECT && mode != IRBFN_ROLLOUT_ST_KS) return false;
  return net->DC == 7 && net->O == 2 * T && T <= kTickTch && (net->O + 15) / 16 == 7;
}

// LDS floats of the trajectories' output tile, per query group
static size_t tick_out_floats() {
  constexpr int S = 7;
  return (kPairRows * pair_pitch(S, pair_ts(S)) + 3) & ~3;
}

size_t gram_wide_tick_lds_bytes(const irbfn_net* net, int SW, int QG) {
  const size_t lds = gram_wide_lds_bytes(net, SW, QG, (size_t)QG * 32 * (net->O | 1));
  const size_t out = (size_t)QG * tick_out_floats() * sizeof(float);
  return lds > out ? lds : out;
}

size_t f16_wide_tick_lds_bytes(const irbfn_net* net, int SW, int QG) {
  const size_t ring = (size_t)SW * kWideRing * f16_chunk_bytes(net->DC, 7);
  const size_t red = ((size_t)SW * QG * 2 * 4 * 64 + (size_t)QG * 32 + (size_t)QG * 32 * (net->O | 1)) * sizeof(float);
  const size_t out = (size_t)QG * tick_out_floats() * sizeof(float);
  size_t lds = ring > red ? ring : red;
  return lds > out ? lds : out;
}

int launch_tick_wide(irbfn_net* net, const LaunchPlan& p, const float* x, const int* mirror, const float* state0,
                     const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s) {
  F16Roll r;
  r.state0 = state0; r.states = states; r.mirror = mirror; r.T = T; r.dp = dp;
  r.wlds = (int)tick_out_floats();
  const bool ks = p.mode == IRBFN_ROLLOUT_ST_KS;
  const dim3 grid(p.grid), block(p.block);
  if (p.kind == LK_TICK_K1G_WIDE) {                // K1g's wide body: the distances on the matrix cores as well
    GramArgs a;
    gram_fill_args(net, x, controls, B, p.S, p.QG, &a);
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
      return ks ? launch_kernel<rbf_tick_f16gram_wide<7, bc(), 7, IRBFN_ROLLOUT_ST_KS>>(grid, block, p.lds, s, a, r)
                : launch_kernel<rbf_tick_f16gram_wide<7, bc(), 7, IRBFN_ROLLOUT_ST_SELECT>>(grid, block, p.lds, s, a, r);
    });
  }
  F16Args a;
  a.x = x; a.img = net->f16_img; a.oscale = net->f16_oscale; a.bias = net->bias; a.out = controls; a.gate = net->gate();
  a.B = (long)B; a.Dreal = net->D; a.O = net->O; a.nchunks = (net->N + kF16Chunk - 1) / kF16Chunk; a.S = p.S; a.QG = p.QG;
  return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
    return ks ? launch_kernel<rbf_tick_f16mfma_wide<7, bc(), 7, IRBFN_ROLLOUT_ST_KS>>(grid, block, p.lds, s, a, r)
              : launch_kernel<rbf_tick_f16mfma_wide<7, bc(), 7, IRBFN_ROLLOUT_ST_SELECT>>(grid, block, p.lds, s, a, r);
  });
}

}  // namespace irbfn
