// K1g for nets evaluated with caller-provided region weights gamma[B][R] (ClusterWCRBFNet; irbfn_net_forward_gamma,
// irbfn_plan_tick_gamma with IRBFN_OPT_FWD_GAMMA_KERNEL = IRBFN_FWDG_K1G): K1g's chunk loop (rbf_forward_gram_body.h) over the
// R regions of the net, each padded to cpr = ceil(K / 32) whole chunks, gamma[b][region of the chunk] multiplied onto the chunk's
// basis values.  out = sum_r gamma_br sum_k phi_brk W_ko + bias (src/irbfn_mpc/model.py:393-412); the epilogue's gate is 1.
// The images are K1g's and K1h's in the padded chunk order (pack_all.hip); they exist only for a net that selected this kernel.
#ifdef IRBFN_GRAM_STAMPS
#undef IRBFN_GRAM_STAMPS                 // the diagnosis stamps belong to rbf_forward_gram.hip
#endif
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "rbf_forward_gram_body.h"

namespace irbfn {

template <int DC, int BC>
__global__ __launch_bounds__(1024, IRBFN_GRAM_WAVES) void rbf_fwd_f16gram_gamma(const GramArgs ga, const GramGamma gm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  gram_body<DC, BC, false, true>(ga, F16Roll{}, -1, lds, gm);
}

// the planning tick in one launch (forward + sign flip + roll-out; irbfn_planner.py:203-212)
template <int DC, int BC>
__global__ __launch_bounds__(1024, IRBFN_GRAM_WAVES) void rbf_tick_f16gram_gamma(const GramArgs ga, const GramGamma gm, const F16Roll rl,
                                                                                 const int mode) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  gram_body<DC, BC, true, true>(ga, rl, mode, lds, gm);
}

// ---- host side -------------------------------------------------------------------------------------------
int gram_gamma_cpr(const irbfn_net* net) { return (net->K + kF16Chunk - 1) / kF16Chunk; }

bool gram_gamma_eligible(const irbfn_net* net) {
  return net->bclass != BC_GENERIC && net->O <= 16 && (net->DC == 3 || net->DC == 4 || net->DC == 7 || net->DC == 8);
}

bool gram_gamma_wanted(const irbfn_net* net) {
  return net->opt[IRBFN_OPT_FWD_GAMMA_KERNEL] == IRBFN_FWDG_K1G || net->opt[IRBFN_OPT_VJP_KERNEL] == IRBFN_VJP_K2G_GAMMA;
}

// A net of one region has K1g's images already, and its chunk order is the padded one.  A net of several regions gets them
// here, when it selects the kernel (this forward, or rbf_vjp_f16gram_gamma, which also takes K2g's ring of hand-over words); the
// next irbfn_net_set_params fills them.
int gram_gamma_select(irbfn_net* net) {
  if (!gram_gamma_eligible(net) || net->R == 1) return IRBFN_OK;                        // not eligible: refused at the call
  if (!net->vjp_flags) {
    void* f = nullptr;
    hipError_t e = hipMalloc(&f, 64 * sizeof(int));
    if (e == hipSuccess) e = hipMemset(f, 0, 64 * sizeof(int));
    if (e != hipSuccess) {
      g_last_hip_error = (int)e;
      if (f) (void)hipFree(f);
      return IRBFN_ERR_HIP;
    }
    net->vjp_flags = static_cast<int*>(f);
  }
  if (net->gram_img) return IRBFN_OK;
  const size_t nchunks = (size_t)net->R * gram_gamma_cpr(net);
  void* bufs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t bytes[5] = {nchunks * f16_chunk_bytes(net->DC, 1), 128 * sizeof(float), nchunks * gram_chunk_stride(1), sizeof(GramHdr),
                           pack_partials_bytes(net)};
  for (int i = 0; i < 5; ++i) {
    const hipError_t e = hipMalloc(&bufs[i], bytes[i]);
    if (e != hipSuccess) {
      g_last_hip_error = (int)e;
      for (int j = 0; j < i; ++j) (void)hipFree(bufs[j]);
      return IRBFN_ERR_HIP;
    }
  }
  net->f16_img = static_cast<unsigned char*>(bufs[0]);
  net->f16_oscale = static_cast<float*>(bufs[1]);
  net->gram_img = static_cast<unsigned char*>(bufs[2]);
  net->gram_hdr = bufs[3];
  net->pack_part = static_cast<float*>(bufs[4]);
  net->gamma_packed = 0;
  return IRBFN_OK;
}

static void gamma_fill_args(const irbfn_net* net, const float* x, const float* gamma, float* out, int64_t B, int S, int QG, GramArgs* a,
                            GramGamma* gm) {
  gram_fill_args(net, x, out, B, S, QG, a);
  gm->gamma = gamma; gm->R = net->R; gm->cpr = gram_gamma_cpr(net);
  a->f.nchunks = gm->R * gm->cpr;
  a->nsteps = gram_nsteps(a->f.nchunks, S);
}

int launch_forward_gram_gamma(irbfn_net* net, const LaunchPlan& p, const float* x, const float* gamma, float* out, int64_t B,
                              hipStream_t s) {
  GramArgs a;
  GramGamma gm;
  gamma_fill_args(net, x, gamma, out, B, p.S, p.QG, &a, &gm);
  return dispatch<3, 4, 7, 8>(net->DC, [&](auto dc) {
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
      return launch_kernel<rbf_fwd_f16gram_gamma<dc(), bc()>>(dim3(p.grid), dim3(p.block), p.lds, s, a, gm);
    });
  });
}

// The one-launch planning tick (rbf_tick_f16gram_gamma): d = 7 or 8, as tick_narrow_compiled says
int launch_tick_gram_gamma(irbfn_net* net, const LaunchPlan& p, const float* x, const float* gamma, const int* mirror,
                           const float* state0, const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s) {
  GramArgs a;
  GramGamma gm;
  gamma_fill_args(net, x, gamma, controls, B, p.S, p.QG, &a, &gm);
  F16Roll rl;
  rl.state0 = state0; rl.states = states; rl.mirror = mirror; rl.T = T; rl.wlds = 0; rl.dp = dp;
  return dispatch<7, 8>(net->DC, [&](auto dc) {
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
      return launch_kernel<rbf_tick_f16gram_gamma<dc(), bc()>>(dim3(p.grid), dim3(p.block), p.lds, s, a, gm, rl, p.mode);
    });
  });
}

}  // namespace irbfn
