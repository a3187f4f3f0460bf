/* irbfn_hip.h -- C ABI of libirbfn_hip.so: the MI355X (gfx950) implementation of the IRBFN hot path.
 *
 * Each entry point names the reference interface (hzheng40/irbfn @ 2024_10_08, path:line) it replaces.
 * Conventions
 *   - every function returns an int status: 0 = IRBFN_OK, negative = irbfn_status below; nothing
 *     throws or aborts across the ABI; irbfn_strerror() turns a status into text.
 *   - `_dev` pointers are device (HBM) pointers owned by the caller; `_host` pointers are host memory
 *     that is copied during the call.  The library never frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work of a call is
 *     enqueued on that stream; the call does not synchronise (no hipMalloc/hipFree/sync on the
 *     launch path, so calls can be captured into a hipGraph once a descriptor exists).
 *   - all floating point data is IEEE binary32, row-major, densely packed.
 *   - NaN/Inf inputs propagate as IEEE arithmetic dictates (no clamping), like the reference.
 */
#ifndef IRBFN_HIP_H_
#define IRBFN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRBFN_ABI_VERSION 1

typedef enum irbfn_status {
  IRBFN_OK = 0,
  IRBFN_ERR_BAD_ARG = -1,       /* NULL pointer, negative size, unknown enum */
  IRBFN_ERR_UNSUPPORTED = -2,   /* shape outside the compiled kernel set (see irbfn_net_create) */
  IRBFN_ERR_HIP = -3,           /* a HIP runtime call failed; irbfn_last_hip_error() has the code */
  IRBFN_ERR_NO_PARAMS = -4,     /* forward/vjp called before irbfn_net_set_params */
  IRBFN_ERR_NO_DEVICE = -5      /* no gfx950 device visible */
} irbfn_status;

/* Radial basis functions of flax_rbf (deprecated/f1tenth_gym/examples/flax_rbf/flax_rbf/flax_rbf.py:34-111),
 * selected in the reference by `basis_func: <name>` in the YAML model card (irbfn_planner.py:72). */
typedef enum irbfn_basis {
  IRBFN_GAUSSIAN = 0,             /* exp(-d^2)            flax_rbf.py:35-37 */
  IRBFN_GAUSSIAN_WIDE = 1,        /* exp(-0.1 d^2)        :40-42 */
  IRBFN_GAUSSIAN_WIDER = 2,       /* exp(-0.01 d^2)       :45-47 */
  IRBFN_INVERSE_QUADRATIC = 3,    /* 1/(1+d^2)            :50-52 */
  IRBFN_LINEAR = 4,               /* d                    :55-57 */
  IRBFN_QUADRATIC = 5,            /* d^2                  :61-63 */
  IRBFN_MULTIQUADRIC = 6,         /* sqrt(1+d^2)          :67-69 */
  IRBFN_INVERSE_MULTIQUADRIC = 7, /* 1/sqrt(1+d^2)        :73-75 */
  IRBFN_SPLINE = 8,               /* d^2 log(d+1)         :79-81 */
  IRBFN_POISSON_ONE = 9,          /* (d-1) exp(-d)        :85-87 */
  IRBFN_POISSON_TWO = 10,         /* ((d-2)/2) d exp(-d)  :91-97 */
  IRBFN_MATERN32 = 11,            /* :101-103 */
  IRBFN_MATERN52 = 12             /* :107-111 */
} irbfn_basis;

/* Roll-out models (one lane per trajectory). */
typedef enum irbfn_rollout_mode {
  IRBFN_ROLLOUT_ST_SELECT = 0, /* integrate_st_mult: scan of dynamic_st_onestep, select(V>3, f, f_ks)
                                  src/irbfn_mpc/dynamics.py:9-100.        state 7, x0u[B,7+2T] -> [B,T,7] */
  IRBFN_ROLLOUT_ST_KS = 1,     /* scan of the kinematic one-step map dynamic_st_onestep_aux
                                  src/irbfn_mpc/dynamics.py:103-187 (T=1 is that function itself).
                                                                          state 7, x0u[B,7+2T] -> [B,T,7] */
  IRBFN_ROLLOUT_FULLINT = 2,   /* inline kinematic bicycle of train_step_fullint
                                  scripts/train_nmpc.py:306-374.          state 5, x0u[B,1+2T]=[v0,u] -> [B,T,5] */
  IRBFN_ROLLOUT_FRENET_LS = 3, /* integrate_frenet_mult (low-speed RHS)
                                  src/irbfn_mpc/dynamics.py:190-290.      state 8, x0u[B,8+2T] -> [B,T,8] */
  IRBFN_ROLLOUT_SPIRAL = 4     /* integrate_path_mult: cubic-spiral path, T = number of samples N
                                  src/irbfn_mpc/planner_utils.py:8-77.    state 6, x0u[B,5]=(k0..k3,s) -> [B,N,6] */
} irbfn_rollout_mode;

/* ---------------------------------------------------------------------------------------------
 * Network descriptor.  Replaces the Flax module object `WCRBFNet(**cfg)` (src/irbfn_mpc/model.py:98-167)
 * plus the bound parameter pytree.  The static part is the YAML model card
 * (scripts/train_nmpc.py:431-450): in_features D, out_features O, num_kernels K, num_regions R,
 * basis_func, lower_bounds / upper_bounds / delta / dimension_ranges of the smooth region gate
 * `_region_activation` (model.py:42-95).
 *
 *   lo_tab_host, hi_tab_host : [nsplit][max_ranges] -- row d holds lower_bounds[d][:] / upper_bounds[d][:]
 *                              (ragged rows padded with anything; padding is never indexed)
 *   delta_host               : [nsplit]
 *   dim_ranges_host          : [n_ranges][nsplit] ints; regions r >= n_ranges have gamma = 0 (model.py:70)
 *   nsplit = len(activation_idx) (model.py:128); the gate reads x[:, d] for d < nsplit (model.py:74-81).
 *
 * Compiled kernel set: D in 1..8; any O >= 1 (O is padded internally to a compiled width);
 * R*K >= 1; nsplit <= 8.  Outside it: IRBFN_ERR_UNSUPPORTED.
 * The descriptor owns device buffers for the packed centre records, the gate tables and a small
 * scratch area of the small-batch latency kernel; calls that use the same descriptor must be ordered
 * on one stream (or serialised by the caller) -- use one descriptor per concurrent stream.
 */
typedef struct irbfn_net irbfn_net;

int irbfn_net_create(irbfn_net** out_net, int D, int R, int K, int O, int basis, int nsplit,
                     int max_ranges, const float* lo_tab_host, const float* hi_tab_host,
                     const float* delta_host, const int* dim_ranges_host, int n_ranges);
int irbfn_net_destroy(irbfn_net* net);

/* Binds the parameter pytree {"rbf_list": {"centers"[R,K,D], "log_sigs"[R,K]},
 * "linear": {"kernel"[K,O], "bias"[O]}} (checkpoint layout).  Device pointers; the
 * data is re-packed on `stream` into the descriptor's own images (two launches, pack_all.hip), so the
 * caller may overwrite its arrays afterwards.  Call again after every optimiser step.  For nets the
 * matrix-core kernels K1g / K2g can take (one region, d <= 8, fast basis) the call ends with ONE small
 * synchronous read-back on `stream` (64 bytes: do the bound parameters fit K1g's expansion?) -- the
 * kernel choice of later forwards is a property of the parameters; every other net returns without
 * synchronising. */
int irbfn_net_set_params(irbfn_net* net, const float* centers_dev, const float* log_sigs_dev,
                         const float* kernel_dev, const float* bias_dev, void* stream);

/* Per-descriptor options: kernel selection and launch geometry.  The defaults are what the library ships
 * with; everything else exists for A/B measurements and for the reduced-precision report of BASELINE config 5.
 * Nothing on the launch path reads the process environment.  value 0 of a geometry option = automatic.
 * Numbers missing below belong to retired options: irbfn_net_set_option / irbfn_net_get_option answer
 * IRBFN_ERR_BAD_ARG for them. */
typedef enum irbfn_option {
  IRBFN_OPT_FWD_KERNEL = 0,    /* irbfn_fwd_kernel below; default IRBFN_FWD_AUTO */
  IRBFN_OPT_FWD_F16_TERMS = 2, /* MFMA operands of K1h.  3 (default): (hi, lo) f16 pairs, float32-grade result;
                                  1: plain f16 operands (~1e-4 relative), 2: plain bf16 operands (~4e-3; O <= 16 only)
                                  -- the two reduced-precision variants BASELINE config 5 asks to report */
  IRBFN_OPT_FWD_F16_S = 7,     /* K1h / K1g: centre slices per query group */
  IRBFN_OPT_FWD_F16_QG = 8,    /* K1h / K1g: query groups of 32 per workgroup */
  IRBFN_OPT_VJP_KERNEL = 9,    /* irbfn_vjp_kernel below; default IRBFN_VJP_AUTO */
  IRBFN_OPT_TICK_FUSED = 13,   /* planning tick on the matrix-core kernels: 1 (default) one launch where the instance exists (wide: d = 7,
                                  O = 2T in (96, 112], single-track modes; narrow: O = 2T <= 16, d = 7 single-track / inline bicycle,
                                  d = 8 Frenet), 0: forward + sign flip + roll-out launches */
  IRBFN_OPT_GRAM_STICKY = 14,  /* K1g / K2g: 0 (default) every irbfn_net_set_params reads the pack's verdict back (one small synchronous copy);
                                  1: only the first one does and later calls keep its verdict -- for training loops, which re-bind every step.
                                  The kernels test the device-side verdict themselves and fall back to the VALU distances / to K2h, so a stale
                                  host verdict costs speed, never correctness */
  IRBFN_OPT_VJPX_KERNEL = 16,  /* irbfn_vjpx_kernel below; default IRBFN_VJPX_AUTO (15 is a retired number) */
  IRBFN_OPT_FWD_GAMMA_KERNEL = 17, /* irbfn_fwd_gamma_kernel below: the kernel of irbfn_net_forward_gamma / irbfn_plan_tick_gamma; default
                                      IRBFN_FWDG_AUTO.  Selecting IRBFN_FWDG_K1G allocates the kernel's images on a net of several regions;
                                      the next irbfn_net_set_params fills them (until then the two calls answer IRBFN_ERR_NO_PARAMS) */
  IRBFN_OPT_COUNT = 18
} irbfn_option;
typedef enum irbfn_fwd_kernel {
  IRBFN_FWD_AUTO = 0, /* B <= 64: K1s; sparse multi-region gate: K1r; one region + fast basis: K1g (d <= 8, parameters inside its budget; O <= 16:
                         B >= 12288; 16 < O <= 128: d = 7 or 8, B >= 2048, >= 256 centres) else K1h (O <= 128); O > 16: K1m; otherwise K1 */
  IRBFN_FWD_K1 = 1,   /* rbf_fwd_qlane: all-float32 VALU kernel (any net) */
  IRBFN_FWD_K1M = 2,  /* rbf_fwd_mfma: Phi x W on the f32-input matrix cores */
  IRBFN_FWD_K1H = 3,  /* rbf_fwd_f16mfma[_wide]: Phi x W on the f16 matrix cores, hi/lo operand pairs */
  IRBFN_FWD_K1R = 4,  /* rbf_fwd_sparse: several regions, every query visits only the regions whose gamma != 0 */
  IRBFN_FWD_K1G = 5   /* rbf_fwd_f16gram[_wide]: one region, d <= 8 (O <= 16) / d = 7 or 8 (16 < O <= 128): the squared distances as an exactly-cancelling Gram expansion
                         on the f16 matrix cores in front of K1h's Phi x W; IRBFN_ERR_UNSUPPORTED when the bound parameters
                         do not fit the expansion (widths of 1e-3 of the centres' spread, non-finite values) */
} irbfn_fwd_kernel;
typedef enum irbfn_fwd_gamma_kernel {
  IRBFN_FWDG_AUTO = 0, /* the gated K1 (rbf_fwd_qlane, GATED = 1); never selects K1g */
  IRBFN_FWDG_K1 = 1,   /* the same, forced */
  IRBFN_FWDG_K1G = 2   /* rbf_fwd_f16gram_gamma / rbf_tick_f16gram_gamma: K1g's chunk loop over the R regions, each padded to whole chunks of 32
                          centres, gamma[b][region] multiplied onto the basis values in front of their f16 hi/lo split.  Gaussian family /
                          inverse quadratic / inverse multiquadric, d <= 8, O <= 16, any R, K, B; one-launch tick for d = 7 / 8 as
                          IRBFN_OPT_TICK_FUSED describes.  Every finite gamma with |gamma| <= 1 (what irbfn_cluster_gate and irbfn_net_gate
                          produce; larger values leave the f16 range of the split); a product |gamma| phi below 2^-28 is flushed towards 0,
                          which is 2^-38 of a full term.  A NaN in a gamma row gives NaN in that output row only.  IRBFN_ERR_UNSUPPORTED at the
                          call for a net outside these shapes or parameters outside K1g's expansion; nothing else is launched in its place */
} irbfn_fwd_gamma_kernel;
typedef enum irbfn_vjp_kernel { IRBFN_VJP_AUTO = 0, IRBFN_VJP_K2 = 1, IRBFN_VJP_K2H = 2, IRBFN_VJP_K2R = 3, IRBFN_VJP_K2G = 4,
                                IRBFN_VJP_K2M = 5, IRBFN_VJP_K2G_GAMMA = 6 } irbfn_vjp_kernel;
/* K2: all-float32 VALU; K2H: hbar and dW on the f16 matrix cores; K2R: region-sparse pair lists; K2G: the squared distances (K1g's
 * expansion) and the centre gradients on the matrix cores as well -- automatic in front of K2H from 8192 queries and 2.5e7
 * (query, centre) pairs where K1g's expansion fits;
 * K2M: hbar and dW on the f32 matrix cores (full f32 operands), one region, gaussian / inverse quadratic / inverse multiquadric,
 * padded d in {3, 4, 7, 8}, 16 < O <= 128 -- forced only, IRBFN_VJP_AUTO never selects it.
 * IRBFN_VJP_K2H is a preference: on a net K2H cannot take (several regions, O > 16, a d-dependent basis), below 2048 queries and
 * with caller-provided region weights the call runs K2 with status IRBFN_OK.  IRBFN_VJP_K2G, IRBFN_VJP_K2R and IRBFN_VJP_K2M are
 * forces: where the kernel cannot take the net or the batch, the call that would launch it answers IRBFN_ERR_UNSUPPORTED and
 * irbfn_net_vjp_kernel_supported answers 0.  (Every option but IRBFN_VJP_K2 and IRBFN_VJP_K2M reaches K2H first, so
 * IRBFN_VJP_K2R refuses only where K2H does not take the call; irbfn_net_vjp_gamma does not look at IRBFN_VJP_K2R.)
 * K2G_GAMMA (rbf_vjp_f16gram_gamma): K2G's loop for irbfn_net_vjp_gamma -- over the R regions of the net, each padded to whole chunks
 * of 32 centres (the images of IRBFN_FWDG_K1G), gamma[b][region] multiplied onto the basis values per pair; slabs in the padded order,
 * fixed-order reduce, no atomics.  A force, and only irbfn_net_vjp_gamma takes it: irbfn_net_vjp and irbfn_net_vjp_frozen answer
 * IRBFN_ERR_UNSUPPORTED under it; irbfn_net_vjp_kernel_supported, which speaks of irbfn_net_vjp, does not know the value (< 0).  Gaussian family / inverse quadratic / inverse multiquadric,
 * padded d in {3, 4, 7, 8}, O <= 16, any R, K, B >= 1, every finite gamma with |gamma| <= 1; a net outside these shapes or parameters
 * outside K1g's expansion: IRBFN_ERR_UNSUPPORTED, nothing is launched in its place.  A call with a query outside K1g's box is done by
 * the gated K2 behind it and returns K2's bits.  d gamma comes from the float32 kernel of every other path.  Selecting it allocates
 * the images on a net of several regions; the next irbfn_net_set_params fills them (until then: IRBFN_ERR_NO_PARAMS).
 * The workspace size does not depend on the option (it grows for a net that holds the padded images). */
typedef enum irbfn_vjpx_kernel { IRBFN_VJPX_AUTO = 0, IRBFN_VJPX_K5 = 1, IRBFN_VJPX_K5M = 2 } irbfn_vjpx_kernel;
/* Kernels of irbfn_net_vjp_x.  K5 (rbf_vjpx_qlane): all-float32 VALU, every net the forward's K1 takes.  K5M (rbf_vjpx_mfma):
 * hbar = gout W^T on the f32 matrix cores (full f32 operands); one region, gaussian family / inverse quadratic / inverse
 * multiquadric, d = 2..8, O <= 128, the net's own gate (not irbfn_net_vjp_x_gamma); IRBFN_VJPX_AUTO selects it for O > 16,
 * where it was measured ahead of K5 (profiles/vjp_x.txt), otherwise K5.  A forced K5M on a net it does not take answers
 * IRBFN_ERR_UNSUPPORTED at the call. */
int irbfn_net_set_option(irbfn_net* net, int option, int value);
int irbfn_net_get_option(const irbfn_net* net, int option, int* value_out);

/* Forward: replaces `WCRBFNet.apply(params, x)` (model.py:169-198; called as
 * `state.apply_fn(state.params, x)` in pred_step, src/irbfn_mpc/irbfn_planner.py:29-32).
 * x_dev[B,D] -> out_dev[B,O].  B = 0 is a no-op. */
int irbfn_net_forward(irbfn_net* net, const float* x_dev, float* out_dev, int64_t B, void* stream);

/* Region gate alone: `_region_activation` (model.py:42-95).  x_dev[B,D] -> gamma_dev[B,R]. */
int irbfn_net_gate(irbfn_net* net, const float* x_dev, float* gamma_dev, int64_t B, void* stream);

/* Bytes of scratch irbfn_net_vjp needs for batch B (caller allocates; may be reused across calls). */
int64_t irbfn_net_vjp_workspace_bytes(const irbfn_net* net, int64_t B);

/* Parameter VJP: replaces `jax.value_and_grad(loss_fn)(state.params)` restricted to the network
 * (scripts/train_nmpc.py:297-298, scripts/train_nmpc_frenet.py:388-389,416-417).
 * Cotangent gout_dev[B,O] -> g_centers[R,K,D], g_log_sigs[R,K], g_kernel[K,O], g_bias[O]
 * (overwritten, not accumulated).  The gradient w.r.t. x is irbfn_net_vjp_x below.  Deterministic (no float atomics). */
int irbfn_net_vjp(irbfn_net* net, const float* x_dev, const float* gout_dev, float* g_centers_dev,
                  float* g_log_sigs_dev, float* g_kernel_dev, float* g_bias_dev, int64_t B,
                  void* workspace_dev, int64_t workspace_bytes, void* stream);

/* irbfn_net_vjp for the layer classes with frozen leaves (the reference's fixed-centre and fixed-width RBF layers,
 * src/irbfn_mpc/model.py:131-140): a NULL g_centers_dev / g_log_sigs_dev is a frozen leaf, neither computed nor
 * written.  Centres NULL runs K2g's no-centres instance, both NULL its Dense-only instance (named
 * "rbf_vjp_f16gram/no_centres<...>" / "rbf_vjp_f16gram/linear<...>" by irbfn_net_last_launch); live centres with
 * NULL widths take the full computation and skip the write.  Every other VJP kernel computes what irbfn_net_vjp
 * computes and writes the live leaves only.  g_kernel_dev and g_bias_dev must be non-NULL; B = 0 zeroes the live
 * leaves.  irbfn_net_vjp_workspace_bytes(net, B) is a sufficient workspace. */
int irbfn_net_vjp_frozen(irbfn_net* net, const float* x_dev, const float* gout_dev, float* g_centers_dev,
                         float* g_log_sigs_dev, float* g_kernel_dev, float* g_bias_dev, int64_t B,
                         void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Query VJP: `jax.vjp(lambda x: WCRBFNet.apply(params, x), x)[1](gout)` -- nothing in the reference takes this gradient
 * (its losses differentiate the parameters only); it is what the sensitivity d u / d state of the predicted controls,
 * gradient-based refinement of a query through net + roll-out (irbfn_rollout_vjp returns the gradient of the whole input row)
 * and composition under an autodiff framework need.  Cotangent gout_dev[B,O] -> gx_dev[B,D] (overwritten), RBF term and the
 * term through the smooth region gate (model.py:42-95).  No workspace, deterministic, B = 0 is a no-op; rows are independent
 * (NaN / Inf in one query or cotangent row stay in that row).  A query exactly on a centre: that pair contributes 0 -- the
 * limit for every basis but linear / poisson_one / poisson_two, whose derivative in d^2 diverges there (jax.grad: NaN).
 * Kernel: IRBFN_OPT_VJPX_KERNEL. */
int irbfn_net_vjp_x(irbfn_net* net, const float* x_dev, const float* gout_dev, float* gx_dev, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Roll-outs.  Replace integrate_st_mult (dynamics.py:94-100), dynamic_st_onestep_aux (:103-187),
 * integrate_frenet_mult (:284-290), the inline bicycle of train_step_fullint
 * (scripts/train_nmpc.py:329-374) and integrate_path_mult (planner_utils.py:62-77).
 * Control layout is the reference's column-major pairs u = [a_0..a_{T-1}, sv_0..sv_{T-1}]
 * (dynamics.py:98: reshape(5, 2, order="F")); T is a run-time parameter (the reference hard-codes
 * T = 5 and N = 9).  dyn_params_host[13] = [mu, m, I, lf, lr, C_Sf, C_Sr, h, dt, sv_max, a_max,
 * s_max, v_max] (dynamics.py:24-36); ignored (may be NULL) for FULLINT and SPIRAL.
 */
int irbfn_rollout_state_dim(int mode);              /* 7, 7, 5, 8, 6 */
int irbfn_rollout_input_dim(int mode, int T);       /* columns of x0u */
int irbfn_rollout_forward(int mode, const float* x0u_dev, const float* dyn_params_host,
                          float* states_dev, int64_t B, int T, void* stream);

/* VJP of the roll-out w.r.t. its input row: gstates_dev[B,T,S] -> g_x0u_dev[B, input_dim].
 * Replaces JAX's transpose of the scans under value_and_grad (scripts/train_nmpc.py:275-276,
 * :356-374; scripts/train_nmpc_frenet.py:408-409; deprecated/train_newlut.py:194-199).
 * clip() passes gradient 1 strictly inside its bounds, 0 strictly outside and `clip_tie` (0, 0.5 or
 * 1) exactly on a bound.  ST_SELECT returns IRBFN_ERR_UNSUPPORTED: the reference never
 * differentiates integrate_st_mult, and jax.grad through its lax.select is NaN at V = 0.  This project's
 * own adjoint of that mode, under the convention stated there, is irbfn_rollout_vjp_select. */
int irbfn_rollout_vjp(int mode, const float* x0u_dev, const float* dyn_params_host,
                      const float* gstates_dev, float* g_x0u_dev, int64_t B, int T, float clip_tie,
                      void* stream);

/* VJP of the ST_SELECT roll-out (integrate_st_mult, dynamics.py:94-100): gstates_dev[B,T,7] -> g_x0u_dev[B, 7+2T].  No
 * reference counterpart.  Convention: one step is x' = x + select(V > 3, f, f_ks) dt with V the clipped speed, and the adjoint
 * holds the mask V > 3 constant -- a step taken on the dynamic branch back-propagates through f (dynamics.py:49-76), a step
 * taken on the kinematic branch through f_ks (:78-88), V = 3 exactly is kinematic as in the forward; the derivative of the
 * branch a step did not take is never evaluated, so a kinematic step at V = 0 gives finite gradients.  Clips as in
 * irbfn_rollout_vjp (clip_tie).  float32 only, like the forward.  T = 0 zeroes g_x0u_dev, B = 0 is a no-op, T > 120 returns
 * IRBFN_ERR_UNSUPPORTED; deterministic, rows are independent. */
int irbfn_rollout_vjp_select(const float* x0u_dev, const float* dyn_params_host, const float* gstates_dev, float* g_x0u_dev,
                             int64_t B, int T, float clip_tie, void* stream);

/* Fused planning tick: net forward + roll-out in one launch, the predicted controls never leave
 * the chip.  Batched form of IRBFNPlanner.plan's `pred_step` -> `hstack` -> `integrate_st_mult`
 * (src/irbfn_mpc/irbfn_planner.py:205-212).  x_dev[B,D] queries, state0_dev[B,S] initial states,
 * requires O = 2T.  controls_dev may be NULL (then only states are written). */
int irbfn_net_forward_rollout(irbfn_net* net, int mode, const float* x_dev, const float* state0_dev,
                              const float* dyn_params_host, float* controls_dev, float* states_dev,
                              int64_t B, int T, void* stream);
/* 1 if irbfn_net_forward_rollout / irbfn_plan_tick with a states output run forward -> roll-out through the caller's
 * controls buffer for this net, mode, batch and horizon (wide outputs need it, narrow ones on the matrix-core kernel are
 * faster with it), 0 if the tick is one launch and controls_dev may be NULL, < 0 on a bad argument. */
int irbfn_net_tick_needs_controls(irbfn_net* net, int mode, int64_t B, int T);
/* 1 if irbfn_net_vjp with IRBFN_OPT_VJP_KERNEL = `kernel` (irbfn_vjp_kernel) runs for this net and batch, 0 if it would answer
 * IRBFN_ERR_UNSUPPORTED, < 0 on a bad argument.  Lets a caller ask before it forces a kernel; changes nothing. */
int irbfn_net_vjp_kernel_supported(irbfn_net* net, int kernel, int64_t B);

/* ---------------------------------------------------------------------------------------------
 * Training-step pieces: the loss compositions that define the VJP seeds, and the
 * optimiser chain, on device -- a step needs no host round trip (the reference pulls the loss with
 * jax.device_get every step, scripts/train_nmpc.py:477-479).  Caller-allocated buffers only.
 *
 * irbfn_train_seeds_oneint: loss_fn of train_step_oneint (scripts/train_nmpc.py:268-295):
 *   loss = mean(l2(y_pred, y)) + mean(l2(onestep(x_pred_u)[:, [0,1,3,4]], onestep(x_u)[:, [0,1,3,4]])),
 *   initial state [0,0,0, x[:,0], 0, x[:,6], x[:,5]] (:260-266), one step = dynamic_st_onestep_aux.
 *   Writes gy = d loss / d y_pred [B,O] and the scalar loss (device).  D >= 7, O >= 2.
 * irbfn_train_seeds_fullint: loss_fn of train_step_fullint (scripts/train_nmpc.py:306-390):
 *   loss = mean|y_pred[:, [0,T]] - y[:, [0,T]]| + mean|final_pred - final_actual| (T-step inline bicycle), O = 2T.
 * partials_dev: scratch of irbfn_train_loss_partials() floats.
 * B = 0 (every seed call): IRBFN_OK, *loss_dev = 0, gy_dev untouched; the row pointers may be NULL.
 * irbfn_adam_clip_step: optax.chain(clip_by_global_norm(max_grad_norm), adam(lr)) + apply_gradients
 *   (scripts/train_nmpc.py:231-233, :299) on flat float32 buffers of n elements; step_dev is the
 *   device-resident update count (incremented by the call).  max_grad_norm <= 0 disables clipping.
 */
int irbfn_train_loss_partials(void);
int irbfn_train_seeds_oneint(const float* x_dev, const float* y_pred_dev, const float* y_dev,
                             const float* dyn_params_host, float clip_tie, float* gy_dev, float* loss_dev,
                             float* partials_dev, int64_t B, int D, int O, void* stream);
int irbfn_train_seeds_fullint(const float* x_dev, const float* y_pred_dev, const float* y_dev, float clip_tie,
                              float* gy_dev, float* loss_dev, float* partials_dev, int64_t B, int D, int T,
                              void* stream);
/* irbfn_train_seeds_frenet_fullint: loss_fn of the Frenet train_step_fullint (scripts/train_nmpc_frenet.py:394-421):
 *   x [B,8] = [ey, delta, vx_car, vy_car, vx_goal, wz, epsi, curv], initial_state = x[:, [0,0,1,2,3,5,6,7]] (:398),
 *   loss = mean|y_pred - y| + mean|integrate_frenet_mult([init, y_pred]) - integrate_frenet_mult([init, y])|, O = 2T,
 *   T <= 16 (the reference: 5).  Writes gy = d loss / d y_pred [B,2T] and the scalar loss. */
int irbfn_train_seeds_frenet_fullint(const float* x_dev, const float* y_pred_dev, const float* y_dev,
                                     const float* dyn_params_host, float clip_tie, float* gy_dev, float* loss_dev,
                                     float* partials_dev, int64_t B, int D, int T, void* stream);
/* irbfn_train_seeds_st_fullint: a full-integration loss through the single-track roll-out, mode = IRBFN_ROLLOUT_ST_SELECT (the
 *   planner's model, differentiated as irbfn_rollout_vjp_select does) or IRBFN_ROLLOUT_ST_KS.  No reference counterpart: L1 as
 *   in its two full-integration losses, the state components of its one-step loss.
 *   x [B, D >= 7] as for irbfn_train_seeds_oneint, initial state [0,0,0, x[:,0], 0, x[:,6], x[:,5]]; O = 2T, T <= 16;
 *   loss = mean|y_pred - y| + mean|S_pred[:, :, [0,1,3,4]] - S_act[:, :, [0,1,3,4]]| with S_pred, S_act the T-step roll-outs of
 *   the predicted and of the label controls (the second mean over B * T * 4 entries).  Writes gy [B,2T] and the scalar loss. */
int irbfn_train_seeds_st_fullint(int mode, const float* x_dev, const float* y_pred_dev, const float* y_dev,
                                 const float* dyn_params_host, float clip_tie, float* gy_dev, float* loss_dev,
                                 float* partials_dev, int64_t B, int D, int T, void* stream);
int irbfn_adam_clip_step(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, int64_t n,
                         int* step_dev, float lr, float beta1, float beta2, float eps, float max_grad_norm,
                         float* partials_dev, void* stream);
/* float64 twins of four of the calls above (the select model is float32 only: irbfn_train_seeds_st_fullint has none),
 * for a net trained under --use_float64 (scripts/train_nmpc.py:41-42: jax_enable_x64):
 * double buffers and double dynamics parameters, the same argument rules and status codes.  partials_dev holds
 * irbfn_train_loss_partials() doubles.
 * irbfn_train_seeds_oneint_f64: loss_fn of train_step_oneint in float64 (scripts/train_nmpc.py:268-295).
 * irbfn_train_seeds_fullint_f64: loss_fn of train_step_fullint in float64 (scripts/train_nmpc.py:306-390).
 * irbfn_train_seeds_frenet_fullint_f64: loss_fn of the Frenet train_step_fullint in float64 (scripts/train_nmpc_frenet.py:394-421).
 * irbfn_adam_clip_step_f64: optax.chain(clip_by_global_norm(max_grad_norm), adam(lr)) + apply_gradients in float64
 *   (scripts/train_nmpc.py:231-233, :299). */
int irbfn_train_seeds_oneint_f64(const double* x_dev, const double* y_pred_dev, const double* y_dev,
                                 const double* dyn_params_host, double clip_tie, double* gy_dev, double* loss_dev,
                                 double* partials_dev, int64_t B, int D, int O, void* stream);
int irbfn_train_seeds_fullint_f64(const double* x_dev, const double* y_pred_dev, const double* y_dev, double clip_tie,
                                  double* gy_dev, double* loss_dev, double* partials_dev, int64_t B, int D, int T,
                                  void* stream);
int irbfn_train_seeds_frenet_fullint_f64(const double* x_dev, const double* y_pred_dev, const double* y_dev,
                                         const double* dyn_params_host, double clip_tie, double* gy_dev, double* loss_dev,
                                         double* partials_dev, int64_t B, int D, int T, void* stream);
int irbfn_adam_clip_step_f64(double* params_dev, const double* grads_dev, double* m_dev, double* v_dev, int64_t n,
                             int* step_dev, double lr, double beta1, double beta2, double eps, double max_grad_norm,
                             double* partials_dev, void* stream);

/* ---- Evaluating a net on a table: roll-out error statistics on device ---------------------------------------
 * What scripts/eval_irbfn_dnmpc.py:92-167 does on the host (roll the label controls and the predicted controls out side by side,
 * :95-159, and report position / heading / velocity errors, :162-167; deprecated/evaluate.py:265-283 likewise for trajectory end
 * points).  The METRIC DEFINITIONS below are this project's own: those lines of the reference are not in the snapshot this
 * library was written from, so parity with its numbers is unpinned.
 * Per row b < B both control sets y_dev[b], y_pred_dev[b] ([a_0..a_{T-1}, sv_0..sv_{T-1}]) are rolled out for T steps from
 * state0_dev[b] (the row layout of irbfn_plan_tick: [B,7] single-track, [B,1] = v0 inline bicycle, [B,8] Frenet) to the final
 * states a (label) and p (prediction); the row's M = S + 2 float32 metrics are
 *   m < S : |p_m - a_m|                    (plain difference, no angle wrapping, as the training losses take it)
 *   S     : hypotf(p_0 - a_0, p_1 - a_1)   position error (Cartesian x, y; Frenet: s, e_y)
 *   S + 1 : mean_j |y_pred[b,j] - y[b,j]|  over the 2T controls.
 * Modes ST_SELECT, ST_KS, FULLINT, FRENET_LS (S = 7, 7, 5, 8), any 1 <= T <= 64; SPIRAL has no controls.
 * Statistics per metric, merged across calls (accumulate != 0 adds this call's rows to what the buffers hold; 0 resets first):
 *   stats_dev  [M][4] double : n (rows whose value is finite), sum, sum_sq, max; a value that is not finite enters none of
 *                              them and no bin (the caller gets their number as rows - n); max is -inf while n = 0
 *   argmax_dev [M] int64     : row0 + b of the LOWEST row that attains max; -1 while n = 0
 *   hist_dev   [M][512] int64: bin = clamp((float_bits(e) >> 20) - 696, 0, 511): exponent and three mantissa bits, eight bins per
 *                              octave.  edge(k) = 2^(-40 + k / 8) * (1 + (k mod 8) / 8) (integer k / 8); bin 0 = [0, edge(1)), bin k =
 *                              [edge(k), edge(k + 1)), bin 511 = everything finite from edge(511) up.  Consecutive edges differ by a
 *                              factor <= 9/8: a quantile read off the histogram is bracketed by its bin's edges.
 *                              1.0 -> 320, 1.125 -> 321, <= 2^-40 -> 0, >= 2^24 -> 511.
 * err_dev [B][M] (optional, NULL skips the stores): the per-row metrics.  Deterministic, bit-identical across repeats.
 * workspace_dev: irbfn_eval_workspace_bytes(mode) bytes, 8-byte aligned.  dyn_params_host: NULL for FULLINT.
 * B = 0: IRBFN_OK; reset outputs under accumulate = 0, untouched outputs otherwise.  IRBFN_ERR_BAD_ARG: unknown mode, B < 0,
 * T < 1, a NULL stats / argmax / hist / workspace, a NULL row pointer with B > 0, missing dynamics parameters, a workspace too
 * small.  IRBFN_ERR_UNSUPPORTED: T > 64, a mode without controls. */
int irbfn_eval_num_metrics(int mode);            /* S + 2; < 0 for a mode without controls or an unknown one */
int64_t irbfn_eval_workspace_bytes(int mode);    /* < 0 where irbfn_eval_num_metrics is */
int irbfn_eval_rollout_errors(int mode, const float* state0_dev, const float* y_pred_dev, const float* y_dev,
                              const float* dyn_params_host, int64_t B, int T, int64_t row0, int accumulate,
                              float* err_dev /* or NULL */, double* stats_dev, int64_t* argmax_dev, int64_t* hist_dev,
                              void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ---- Batched planner front / back end ------------------------------------------------------
 * Query construction + mirror trick of IRBFNPlanner.plan (src/irbfn_mpc/irbfn_planner.py:181-201):
 * pose [B,7] = [x, y, delta, v, theta, angv, beta] (:240), goal [B,4] = ref_point [x, y, theta, v] (:170-171),
 * float64 like the NumPy host code; -> x [B,7] = [v, x_g, y_g, t_g, v_g, beta, angv] float32, mirror [B]
 * (goal_local[1] < 0), optional state0 [B,7] = float32(pose). */
int irbfn_plan_queries_cartesian(const double* pose_dev, const double* goal_dev, float* x_dev, float* state0_dev,
                                 int32_t* mirror_dev, int64_t B, void* stream);
/* IRBFNFrenetPlanner.plan (irbfn_planner.py:456-502): frenet [B,8] = [s, ey, delta, vx, vy, wz, epsi, curv],
 * vx_goal [B] -> x [B,8] = [+-ey, delta, vx, +-vy, vx_goal, +-wz, +-epsi, curv], mirror = ey < -0.05,
 * optional state0 [B,8] = float32(frenet). */
int irbfn_plan_queries_frenet(const double* frenet_dev, const double* vx_goal_dev, float* x_dev, float* state0_dev,
                              int32_t* mirror_dev, int64_t B, void* stream);
/* One planning tick: pred_step -> negate the steer-velocity controls [T, 2T) of mirrored rows
 * (irbfn_planner.py:203-204, :487-488) -> roll-out from state0 (:205-212).  mirror_dev may be NULL (then
 * identical to irbfn_net_forward_rollout); states_dev may be NULL (controls only; state0/dyn unused). */
int irbfn_plan_tick(irbfn_net* net, int mode, const float* x_dev, const int32_t* mirror_dev, const float* state0_dev,
                    const float* dyn_params_host, float* controls_dev, float* states_dev, int64_t B, int T,
                    void* stream);
/* Explicit-MPC table look-up, grid form (src/irbfn_mpc/explicit_planner.py:165-175): per axis
 * idx_d = min(shape_d - 1, searchsorted(keys_d, x_d, side="right")); keys_dev = the D sorted key arrays
 * concatenated (float64), key_offsets_host[D+1], shape_host[D]; table_dev [prod(shape), OW] float32 (may
 * be NULL with out_dev NULL).  -> flat row index idx_dev [B] and, if out_dev, the gathered rows [B,OW]. */
int irbfn_lut_grid_lookup(const double* keys_dev, const int32_t* key_offsets_host, const int32_t* shape_host,
                          const float* table_dev, const double* x_dev, int64_t* idx_dev, float* out_dev, int64_t B,
                          int D, int OW, void* stream);
/* Explicit-MPC table look-up, nearest-neighbour form (scipy KDTree.query at explicit_planner.py:383):
 * idx = argmin_n ||inputs[n] - x_b||_2 over inputs_dev [N,D] (float32; ties -> lowest n), dist_dev [B]
 * (optional), out_dev [B,OW] = table_dev[idx] (optional).  D in {3,4,7,8}.  A query with no finite float32 distance to
 * any row (a NaN or Inf component) gets idx = -1, dist = NaN and a NaN row of out_dev.  IRBFN_ERR_BAD_ARG, before the
 * workspace is touched, when ceil(B / 8) exceeds the device's maxGridSize[1] (or B its maxGridSize[0]). */
int64_t irbfn_lut_nearest_workspace_bytes(int64_t N, int64_t B);
int irbfn_lut_nearest(const float* inputs_dev, const float* table_dev, const float* x_dev, int64_t* idx_dev,
                      float* dist_dev, float* out_dev, int64_t N, int64_t B, int D, int OW, void* ws_dev,
                      int64_t ws_bytes, void* stream);

/* Way-point geometry of the planners' pure-pursuit front end, batched over B query points against ONE piecewise-linear
 * trajectory [N,2] (float64 device arrays as the NumPy callers hold them; one wave per point):
 * irbfn_nearest_point = nearest_point (src/irbfn_mpc/planner_utils.py:109-146): projection [B,2], distance, t in [0,1]
 *   and segment index of the closest point (first minimum, as np.argmin; but a segment whose distance is NaN -- a repeated
 *   or NaN way-point -- is skipped where np.argmin returns the first NaN; nothing left: (0, 0), inf, 0, segment 0);
 * irbfn_intersect_point = intersect_point (:149-233): first point one `radius` away along the trajectory from
 *   t_start (= i + t, may be NULL = 0; must not be NaN: the conversion to the start index is undefined), with
 *   wrap-around; found[b] = 0 where the reference returns (None, None, None) (then first_p / first_t are NaN); first_i
 *   may be -1 (the closing segment, :206). */
int irbfn_nearest_point(const double* points_dev, const double* trajectory_dev, double* proj_dev, double* dist_dev,
                        double* t_dev, int32_t* seg_dev, int64_t B, int N, void* stream);
int irbfn_intersect_point(const double* points_dev, const double* trajectory_dev, const double* t_start_dev, float radius,
                          int wrap, float* first_p_dev, int32_t* first_i_dev, float* first_t_dev, int32_t* found_dev,
                          int64_t B, int N, void* stream);

/* ClusterWCRBFNet (src/irbfn_mpc/model.py:341-414): the region weights are a learned softmax gate instead of the
 * tanh indicator.  irbfn_cluster_gate: logits = x Wc + bc [B,R] (second output of the reference module) and
 * gamma = softmax(logits) [B,R]; wc [D,R], bc [R] device pointers.  irbfn_net_forward_gamma: the fused
 * sum_r gamma[b,r] phi[b,r,k] -> Dense forward (model.py:405-412) with caller-provided gamma_dev [B,R], on a
 * descriptor created with R regions (its own gate tables are ignored). */
int irbfn_cluster_gate(const float* x_dev, const float* wc_dev, const float* bc_dev, float* logits_dev, float* gamma_dev,
                       int64_t B, int D, int R, void* stream);
int irbfn_net_forward_gamma(irbfn_net* net, const float* x_dev, const float* gamma_dev, float* out_dev, int64_t B,
                            void* stream);

/* irbfn_plan_tick with caller-provided region weights gamma_dev [B,R]: the planning tick (pred_step -> sign flip of the
 * mirrored rows -> roll-out, src/irbfn_mpc/irbfn_planner.py:203-212, :487-488) of a ClusterWCRBFNet (model.py:393-412) behind
 * irbfn_cluster_gate.  One launch of the fused kernel with the roll-out in its epilogue (fast bases, T * S <= 64; controls_dev
 * may then be NULL); otherwise irbfn_net_forward_gamma -> flip -> split-row roll-out through controls_dev (NULL there:
 * IRBFN_ERR_BAD_ARG).  mirror_dev / states_dev may be NULL as for irbfn_plan_tick. */
int irbfn_plan_tick_gamma(irbfn_net* net, int mode, const float* x_dev, const float* gamma_dev,
                          const int32_t* mirror_dev, const float* state0_dev, const float* dyn_params_host,
                          float* controls_dev, float* states_dev, int64_t B, int T, void* stream);

/* VJP of ClusterWCRBFNet (the reference trains it: scripts/train_nmpc_frenet.py:424-453).
 * irbfn_net_vjp_gamma: irbfn_net_vjp with caller-provided region weights gamma_dev [B,R] (the softmax gate) instead of
 *   the tanh tables, plus -- if dgamma_dev is not NULL -- the cotangent of those weights,
 *   dgamma[b,r] = sum_k (gout W^T)[b,k] phi[b,r,k]   (O <= 16).
 * irbfn_cluster_gate_vjp: softmax + Dense backward of the gate (model.py:402-404): dlogits = gamma * (dgamma -
 *   <gamma, dgamma>) [+ glogits_dev, the direct cotangent of the logits; may be NULL] -> g_wc [D,R], g_bc [R];
 *   dlogits_dev [B,R] is scratch / output; workspace_dev: irbfn_cluster_gate_vjp_workspace_bytes(D, R) bytes (per-block
 *   partial sums, added in block order: deterministic).  Supported: 1 <= D <= 16 (as irbfn_cluster_gate) and any R >= 1
 *   with (D + 1) * R < 2^31; R is otherwise limited by memory only (the workspace is 256 (D + 1) R floats, 4.6 MB at
 *   D = 8, R = 500).  Outside it: IRBFN_ERR_UNSUPPORTED.
 * irbfn_softmax_xent: optax.softmax_cross_entropy(logits, labels).mean() (train_nmpc_frenet.py:431) -> loss (added to
 *   *loss_dev if accumulate != 0) and glogits = d loss / d logits; partials_dev: irbfn_train_loss_partials() floats. */
int irbfn_net_vjp_gamma(irbfn_net* net, const float* x_dev, const float* gamma_dev, const float* gout_dev,
                        float* g_centers_dev, float* g_log_sigs_dev, float* g_kernel_dev, float* g_bias_dev, float* dgamma_dev,
                        int64_t B, void* workspace_dev, int64_t workspace_bytes, void* stream);
/* irbfn_net_vjp_x with caller-provided region weights gamma_dev [B,R] (`jax.vjp` of ClusterWCRBFNet's fused stage,
 * model.py:405-412, w.r.t. x at fixed gamma; nothing in the reference takes it): gx_dev [B,D] holds the RBF term only; if
 * dgamma_dev is not NULL it receives the cotangent of the weights, dgamma[b,r] = sum_k (gout W^T)[b,k] phi[b,r,k] (any O).
 * The softmax / Dense chain of the gate back to x is the caller's (a [B,R] x [R,D] product).  Always K5. */
int irbfn_net_vjp_x_gamma(irbfn_net* net, const float* x_dev, const float* gamma_dev, const float* gout_dev,
                          float* gx_dev, float* dgamma_dev, int64_t B, void* stream);
int64_t irbfn_cluster_gate_vjp_workspace_bytes(int D, int R);
int irbfn_cluster_gate_vjp(const float* x_dev, const float* gamma_dev, const float* dgamma_dev, const float* glogits_dev,
                           float* dlogits_dev, float* g_wc_dev, float* g_bc_dev, int64_t B, int D, int R,
                           void* workspace_dev, int64_t workspace_bytes, void* stream);
int irbfn_softmax_xent(const float* logits_dev, const float* labels_dev, float* glogits_dev, float* loss_dev,
                       float* partials_dev, int accumulate, int64_t B, int R, void* stream);

/* Dense head of DeeperWCRBFNet (src/irbfn_mpc/model.py:201-289; the model of IRBFNFrenetPlanner with
 * deeper=True, src/irbfn_mpc/irbfn_planner.py:286-298):  out = linear(relu(linear_pre2(relu(h1)))) with
 * h1 = linear_pre1(rbf_out) [B,H1] produced by irbfn_net_forward on a descriptor whose Dense layer is
 * linear_pre1.  w2[H1,H2], b2[H2], w3[H2,O], b3[O] device pointers; H1 = H2 = 64 (hard-coded in the
 * reference).  The VJP of the head is irbfn_mlp_head_vjp below.
 * For the three head entry points (irbfn_mlp_head_forward, irbfn_mlp_head_tick, irbfn_mlp_head_vjp):
 *   - h1_dev must be 16-byte aligned (its rows are read with 16-byte vector loads): IRBFN_ERR_BAD_ARG otherwise, for B > 0
 *     (irbfn_mlp_head_tick checks the address behind its shape checks: an unsupported shape stays IRBFN_ERR_UNSUPPORTED).  The
 *     other pointers need float alignment only (gradients may be views of a flat buffer at any float offset).
 *   - relu is max(v, 0) that propagates NaN, as jnp.maximum does: a NaN in a row of h1 gives a NaN output row (NaN controls
 *     from the tick) and NaN in the weight gradients it reaches; +Inf / -Inf follow IEEE arithmetic.
 *   - relu'(0) = 0 (jax.nn.relu): the VJP masks with h1 > 0 and z2 > 0; a NaN pre-activation masks to 0. */
int irbfn_mlp_head_forward(const float* h1_dev, const float* w2_dev, const float* b2_dev, const float* w3_dev,
                           const float* b3_dev, float* out_dev, int64_t B, int H1, int H2, int O, void* stream);

/* One planning tick of the Deeper planner behind its RBF stage: the head above -> negate the steer-velocity controls [T, 2T)
 * of mirrored rows (src/irbfn_mpc/irbfn_planner.py:203-204, :487-488) -> roll-out from state0 (:205-212), the chain
 * IRBFNFrenetPlanner(deeper=True) (:286-298) runs per pose, for B rows in ONE launch where O = 2T <= 16 (the reference's
 * cards: O = 2 and O = 10): the controls go from the output MFMAs through LDS to the wave's own roll-out, bit-equal to
 * irbfn_mlp_head_forward -> flip -> irbfn_rollout_forward.  Arguments as for irbfn_plan_tick: mirror_dev may be NULL (no
 * flip); states_dev may be NULL (controls only, with the flip; state0 / dyn unused; controls_dev required); controls_dev may
 * be NULL where irbfn_mlp_head_tick_needs_controls is 0.  Modes ST_SELECT, ST_KS, FULLINT, FRENET_LS; H1 = H2 = 64.
 * O > 16 runs head forward -> flip -> split-row roll-out through controls_dev, which is then required.
 * irbfn_mlp_head_tick_needs_controls: 1 if the tick goes through the caller's controls buffer (O > 16), 0 if it is one launch,
 * < 0 on a bad argument (no roll-out mode, T < 1, O != 2T): the counterpart of irbfn_net_tick_needs_controls. */
int irbfn_mlp_head_tick(const float* h1_dev, const float* w2_dev, const float* b2_dev, const float* w3_dev,
                        const float* b3_dev, int mode, const int32_t* mirror_dev /* or NULL */,
                        const float* state0_dev, const float* dyn_params_host,
                        float* controls_dev /* or NULL */, float* states_dev /* or NULL */,
                        int64_t B, int H1, int H2, int O, int T, void* stream);
int irbfn_mlp_head_tick_needs_controls(int mode, int O, int T);

/* VJP of that head (the reference trains the model: scripts/train_nmpc_frenet.py:339-421): gout [B,O] ->
 * gh1 [B,H1] (cotangent of linear_pre1's output = the seed of irbfn_net_vjp on the stage descriptor) and the
 * gradients of linear_pre2 (gw2 [H1,H2], gb2 [H2]) and linear (gw3 [H2,O], gb3 [O]).  O <= 16.  Deterministic. */
int64_t irbfn_mlp_head_vjp_workspace_bytes(int H1, int H2, int O);
int irbfn_mlp_head_vjp(const float* h1_dev, const float* w2_dev, const float* b2_dev, const float* w3_dev,
                       const float* gout_dev, float* gh1_dev, float* gw2_dev, float* gb2_dev, float* gw3_dev,
                       float* gb3_dev, int64_t B, int H1, int H2, int O, void* ws_dev, int64_t ws_bytes, void* stream);

/* float64 mode.  The reference trains and evaluates in float64 under --use_float64 (scripts/train_nmpc.py:41-42:
 * jax.config.update("jax_enable_x64", True); some of its checkpoints hold float64 centers / log_sigs).  These entry points
 * evaluate WCRBFNet.apply (model.py:169-198) and its parameter VJP (scripts/train_nmpc.py:297-298) in float64 on the f64
 * vector pipe, straight from the checkpoint-layout arrays: no descriptor, no packed records; the gate bounds are float64 too
 * (a float32 card would move gamma by delta * 4e-8).  All 13 bases.  The card is a host struct of sizes and DEVICE pointers:
 * lo / hi [nsplit][max_ranges], delta [nsplit], dim_ranges [n_ranges][nsplit] as for irbfn_net_create.
 * workspace: irbfn_f64_workspace_bytes(card, B, with_vjp) bytes (gamma [B][R], + the gradient slabs for the VJP).
 * irbfn_f64_vjp: cotangent gout [B,O] -> g_centers [R,K,D], g_log_sigs [R,K], g_kernel [K,O], g_bias [O]; O <= 16
 * (IRBFN_ERR_UNSUPPORTED above); deterministic.  Not a throughput path: plain lane-per-query / lane-per-centre kernels. */
typedef struct irbfn_f64_card {
  int D, R, K, O, basis, nsplit, max_ranges, n_ranges;
  const double* lo_dev;
  const double* hi_dev;
  const double* delta_dev;
  const int* dim_ranges_dev;
} irbfn_f64_card;
int64_t irbfn_f64_workspace_bytes(const irbfn_f64_card* card, int64_t B, int with_vjp);
int irbfn_f64_forward(const irbfn_f64_card* card, const double* centers_dev, const double* log_sigs_dev,
                      const double* kernel_dev, const double* bias_dev, const double* x_dev, double* out_dev, int64_t B,
                      void* workspace_dev, int64_t workspace_bytes, void* stream);
int irbfn_f64_vjp(const irbfn_f64_card* card, const double* centers_dev, const double* log_sigs_dev, const double* kernel_dev,
                  const double* x_dev, const double* gout_dev, double* g_centers_dev, double* g_log_sigs_dev,
                  double* g_kernel_dev, double* g_bias_dev, int64_t B, void* workspace_dev, int64_t workspace_bytes,
                  void* stream);
/* irbfn_net_vjp_x in float64 (`jax.vjp` of apply w.r.t. x under jax_enable_x64; nothing in the reference takes it):
 * gout [B,O] -> gx [B,D] (overwritten), RBF and gate term, the gate from the float64 card; any O, all 13 bases (the same
 * convention for a query on a centre).  One lane per query; needs no workspace: workspace_dev may be NULL. */
int irbfn_f64_vjp_x(const irbfn_f64_card* card, const double* centers_dev, const double* log_sigs_dev,
                    const double* kernel_dev, const double* x_dev, const double* gout_dev, double* gx_dev, int64_t B,
                    void* workspace_dev, int64_t workspace_bytes, void* stream);

/* k-means on a table: one Lloyd iteration per call (kmeans.hip).  The reference derives the centres of its fixed-centre nets
 * ("constraint clustering -> centre files") and the cluster labels of train_step_fullint_withcluster in notebooks that are
 * not in its snapshot: parity with its clustering is unpinned; the arithmetic below is pinned against a float64 statement.
 *   d2[n,k]  = the float32 chain d2 = fmaf(t, t, d2), t = x[n,d] - c[k,d], d = 0 .. D-1, from 0 (no Gram expansion);
 *   label[n] = argmin_k d2[n,k], ties to the lowest k; labels_dev [N] is read (for `moved`) and then overwritten: fill it with
 *              -1 before the first iteration.  d2_dev [N] (optional) = d2[n, label[n]].
 *   A row with a non-finite component, or whose float32 d2 to every centre is not finite, gets label -1 and d2 = NaN and
 *   enters no sum, no count and no statistic (the rule of irbfn_lut_nearest).  A centre with a non-finite component is never
 *   chosen.
 *   new_centers_dev [K,D] (optional; NULL = assign only) = the float32 mean of the rows labelled k: the sums are exact 64-bit
 *   integers on a per-column fixed-point grid of 2^-S max|x[:,d]| with S = 62 - bits(N), so the mean is within
 *   (2^-24 + 2^-S) max_n |x[n,d]| of the real one, in any order.  A cluster with no row keeps its old centre bit for bit and
 *   counts[k] = 0.  counts_dev [K] (optional) is exact.  new_centers_dev must not alias centers_dev.
 *   stats_dev [4] (float64): the number of finite rows; the inertia = sum of d2[n, label[n]] over them; moved = the number of
 *   them whose label differs from the value labels_dev held on entry; max_k ||new_k - old_k||^2 taken in float64 from the
 *   float32 centres (0 when new_centers_dev is NULL).
 *   Every output is bit-identical across repeats.
 * Supported: 1 <= D <= 16 (as irbfn_cluster_gate), 1 <= K <= 65536, any N >= 0 (grid-stride; no grid-limit refusal); outside it
 * IRBFN_ERR_UNSUPPORTED.  K < 1, D < 1, N < 0, a NULL x / centers / labels / stats with N > 0, or a workspace that is NULL,
 * not 8-byte aligned or smaller than irbfn_kmeans_workspace_bytes(N, K, D): IRBFN_ERR_BAD_ARG.  All of these are decided
 * before any HIP call.  N = 0: IRBFN_OK, no launch, the outputs untouched.  irbfn_kmeans_workspace_bytes returns the same
 * negative codes for sizes it refuses. */
int64_t irbfn_kmeans_workspace_bytes(int64_t N, int K, int D);
int irbfn_kmeans_step(const float* x_dev /*[N,D]*/, const float* centers_dev /*[K,D]*/, int32_t* labels_dev /*[N] in/out*/,
                      float* d2_dev /*[N] or NULL*/, float* new_centers_dev /*[K,D] or NULL = assign only*/,
                      int64_t* counts_dev /*[K] or NULL*/, double* stats_dev /*[4]*/, int64_t N, int K, int D,
                      void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Closed-form fit of the output layer (rbf_hidden.hip, syrk_f64.hip; irbfn_amd/linear_fit.py).  With the centres and widths held
 * fixed a net is linear in linear/kernel and linear/bias: the classical RBF construction takes them from linear least squares in
 * one pass over the table.  The reference has no counterpart (it reaches these weights by Adam alone): parity is unpinned; each
 * stage is pinned against a float64 statement of it.
 * irbfn_net_hidden: x_dev [B,D] -> h_dev[b * ldh + k] = sum_r gamma[b,r] phi(|x_b - c_rk| / sigma_rk), k < K, ldh >= K; columns
 *   >= K of a row are not written.  gamma is the net's own tanh gate; the bound linear leaves are ignored.  All-float32 VALU
 *   arithmetic as irbfn_net_forward's K1 (direct differences, the same basis and gate forms, the gate's exact zero); any net
 *   irbfn_net_create accepts.  Rows are independent (a NaN query stays in its row); no workspace; deterministic.  B = 0:
 *   IRBFN_OK, no launch.  IRBFN_ERR_BAD_ARG: NULL net, B < 0, and with B > 0 a NULL x / h or ldh < K; IRBFN_ERR_NO_PARAMS
 *   before irbfn_net_set_params.  irbfn_net_last_launch names it rbf_hidden<...>.
 * irbfn_syrk_f64: g[i][j] (+)= sum_n z[n * ldz + i] z[n * ldz + j], i, j < M: the float64 Gram matrix of float32 rows, both
 *   triangles of the full row-major [M][M] matrix, symmetric bit for bit.  accumulate = 0 overwrites g and never reads it (rows = 0
 *   zeroes it); accumulate = 1 adds onto it (rows = 0 leaves it untouched).  Every product is float32 x float32, exact in
 *   float64, and every sum is float64 (v_mfma_f64_16x16x4_f64): |g - exact| <= rows 2^-53 sum_n |z_ni z_nj|.  Rows past
 *   `rows` and columns in [M, ldz) are never read.  Non-finite values of z propagate by IEEE rules into the entries they touch.
 *   No atomics: bit-identical across repeats.  The workspace (irbfn_syrk_f64_workspace_bytes(rows, M) bytes, below 1 GiB, 8-byte
 *   aligned) need not be cleared.  IRBFN_ERR_BAD_ARG: M < 1, M > 8192, ldz < M, rows < 0, a NULL g, a NULL z with rows > 0, a
 *   workspace that is NULL, misaligned or too small; all decided before any HIP call.  irbfn_syrk_f64_workspace_bytes returns
 *   the same negative code for sizes it refuses. */
int irbfn_net_hidden(irbfn_net* net, const float* x_dev /*[B,D]*/, float* h_dev /*[B,ldh]*/, int64_t ldh, int64_t B, void* stream);
int64_t irbfn_syrk_f64_workspace_bytes(int64_t rows, int M);
int irbfn_syrk_f64(const float* z_dev /*[rows,ldz]*/, int64_t ldz, int64_t rows, int M, double* g_dev /*[M,M]*/, int accumulate,
                   void* ws_dev, int64_t ws_bytes, void* stream);

/* The p nearest centres of every row (knn.hip; irbfn_amd/widths.py): the core of the width rules that stand between k-means and
 * the closed-form fit.  The reference leaves its widths to Adam from log_sig = 0 and has no width rule: parity is unpinned; the
 * arithmetic below is pinned against a float64 statement.
 *   d2[n,k]  = the float32 chain d2 = fmaf(t, t, d2), t = q[n,d] - c[k,d], d = 0 .. D-1, from 0 (no Gram expansion): the chain of
 *              irbfn_kmeans_step, so p = 1 reproduces its label and d2 bit for bit.
 *   Row n gets its p smallest candidates in ascending order of the pair (d2, k): equal d2 goes to the lower k, and a centre at
 *   distance 0 is a neighbour like any other.  d2_dev[n,j] and idx_dev[n,j] (optional) are the j-th of them.
 *   A candidate whose d2 is NaN or Inf is never taken (a centre or a row with a non-finite component, an overflow).  self0 >= 0:
 *   row n never takes centre self0 + n (the rows are centres self0 .. self0 + N - 1 of the same set; an index >= K excludes
 *   nothing); self0 = -1: no exclusion.
 *   Slots for which no candidate is left (K minus the exclusions < p, non-finite centres, a non-finite row) get d2 = NaN and
 *   idx = -1, the k-means convention.
 *   split: the centres are cut into segments of whole tiles whose lists a second launch merges; 0 = the library chooses from N
 *   and K, s >= 1 = s segments (clamped to the number of tiles).  The order is total, so every output is bit-identical across
 *   repeats and across every value of split.  No atomics.
 * Supported: 1 <= D <= 16, 1 <= K <= 65536, 1 <= p <= 16, any N >= 0 (grid-stride); outside it IRBFN_ERR_UNSUPPORTED.  K < 1,
 * D < 1, p < 1, N < 0, self0 < -1, split < 0, a NULL q / c / d2 with N > 0, or a workspace that is NULL, not 8-byte aligned or
 * smaller than irbfn_knn_workspace_bytes(N, K, D, p, split): IRBFN_ERR_BAD_ARG, which wins over an unsupported size -- but for the
 * workspace that is too small: a size exists for supported shapes only, so that one test comes after the size limits.  All of
 * these are decided before any HIP call.  N = 0: IRBFN_OK, no launch, the outputs untouched.  The workspace need not be cleared.
 * Both launches are grid-stride loops: no N is refused for the grid it would need.
 * irbfn_knn_workspace_bytes returns the same negative codes for sizes it refuses; it grows with N, K, p and with split >= 1
 * (split = 0 lies between split = 1 and the number of tiles). */
int64_t irbfn_knn_workspace_bytes(int64_t N, int K, int D, int p, int split);
int irbfn_knn_d2(const float* q_dev /*[N,D]*/, const float* c_dev /*[K,D]*/, int64_t N, int K, int D, int p,
                 int64_t self0 /* -1: none; >= 0: row n never takes centre self0 + n */,
                 int split /* 0: the library chooses; s >= 1: the centres in s segments (clamped to the number of tiles) */,
                 float* d2_dev /*[N,p]*/, int32_t* idx_dev /*[N,p] or NULL*/, void* ws_dev, int64_t ws_bytes, void* stream);

/* Orthogonal least squares forward selection on a Gram matrix (ols.hip; irbfn_amd/ols.py): from a pool of M candidate centres,
 * repeatedly the one whose hidden-layer column removes the most of what is still unexplained in y (Chen, Cowan & Grant 1991).  The
 * reference places no centre by what it explains: parity is unpinned; the arithmetic below is pinned against a float64 statement.
 *   g_dev [Mg][Mg], Mg = M + 1 + O: G = Z^T Z of Z = [h | 1 | y] as irbfn_syrk_f64 leaves it (symmetric bit for bit; only read).
 *   A = G[:M+1,:M+1] with ridge_abs added to its first M diagonal entries, B = G[:M+1, M+1:]; n = M + 1 columns, or n = M with
 *   fit_bias = 0 (column M is then never read).  npad = M + 1 rounded up to a multiple of 64.
 *   State: d_dev [2][npad] = the running diagonal d and the first one d0; c_dev [npad][O] = the running right-hand side;
 *   l_dev [kmax + 1][npad] = the factor, one row per step; sel_dev [kmax + 1], gain_dev [kmax + 1][O], count_dev [1].
 *   irbfn_ols_begin: d = d0 = diag(A), c = B, count = 0, and the pivot of step 0.  Entries n .. npad - 1 of a row of d, c and l
 *   are never read or written.
 *   irbfn_ols_steps takes `steps` further pivots.  Step t = count:
 *     pivot   j = M in step 0 with fit_bias (the ones column), else the argmax over the columns i < M not yet taken with
 *             d[i] > tol d0[i] of score[i] = (sum_o c[i,o]^2) / d[i], ties to the lowest i; a NaN score never wins.  Without
 *             such a column, or with a best score that is not positive (or a ones column with d[M] <= 0), selection has ended:
 *             this and every later step is a no-op that writes nothing.  So is every step once count = kmax + fit_bias.
 *     column  l[t][i] = (A[i,j] - sum_{s<t} l[s][i] l[s][j]) / sqrt(d[j]) for the columns not yet taken, l[t][j] = sqrt(d[j]),
 *             0 for the columns taken earlier.
 *     update  ly = c[j,:] / sqrt(d[j]); gain[t,:] = ly^2; d[i] -= l[t][i]^2 and c[i,:] -= l[t][i] ly for every column not taken
 *             earlier, j included; sel[t] = j; count = t + 1.
 *   G_yy[o,o] - sum_{s<=t} gain[s,o] is the least of rss + ridge_abs |w|^2 over the weights of the first t + 1 pivots.
 *   All float64 on the vector pipe; the sum over s runs in a fixed order that depends on t alone, so every output is
 *   bit-identical across repeats and across how the steps are divided over calls.  A step is two launches (the column, update
 *   and per-block best scores; the pivot); no block waits for another, no atomics, and the pivot stays on the device.
 *   The workspace (irbfn_ols_workspace_bytes(M, O, kmax) bytes, 8-byte aligned) need not be cleared before irbfn_ols_begin and
 *   carries the selection's state from call to call, like the other buffers.
 * Supported: 1 <= M, 1 <= O, M + 1 + O <= 8192 (the limit of irbfn_syrk_f64), 1 <= kmax <= M.  Outside it, and for a NULL
 * pointer, a negative or NaN ridge_abs or tol, steps < 0, or a workspace that is not 8-byte aligned or too small:
 * IRBFN_ERR_BAD_ARG, decided before any HIP call.  steps = 0: IRBFN_OK, no launch.  irbfn_ols_workspace_bytes returns the same
 * negative code for sizes it refuses. */
int64_t irbfn_ols_workspace_bytes(int M, int O, int kmax);
int irbfn_ols_begin(const double* g_dev /*[Mg,Mg]*/, int M, int O, int fit_bias, double ridge_abs, double tol, int kmax,
                    double* l_dev /*[kmax+1][npad]*/, double* d_dev /*[2][npad]: d, d0*/, double* c_dev /*[npad][O]*/,
                    int32_t* sel_dev /*[kmax+1]*/, double* gain_dev /*[kmax+1][O]*/, int32_t* count_dev /*[1]*/, void* ws_dev,
                    int64_t ws_bytes, void* stream);
int irbfn_ols_steps(const double* g_dev /*[Mg,Mg]*/, int M, int O, int fit_bias, double tol, int kmax, double* l_dev, double* d_dev,
                    double* c_dev, int32_t* sel_dev, double* gain_dev, int32_t* count_dev, void* ws_dev, int64_t ws_bytes,
                    int steps, void* stream);

/* Leverages and predictions of the closed-form fit, row by row (rows_quad_f64.hip; irbfn_amd/loo.py): the pass over the rows behind
 * leave-one-out residuals, PRESS, GCV and the predictive variance factor of a query.  The reference has no counterpart: parity is
 * unpinned; the arithmetic below is pinned against integer and extended-precision statements of it.
 *   q[n]    = sum_{j<m} ( sum_{k<=j} z[n * ldz + k] p[k * ldp + j] )^2: the first m columns of p are an upper triangle (the host
 *             passes T^T, T = L^-1 diag(s) of the Cholesky factor of the scaled normal equations: q[n] = |T z_n|^2, the leverage).
 *   v[n,o]  = sum_{k<m} z[n * ldz + k] p[k * ldp + m + o], o < nd: nd dense columns (the host passes [W; b]: the prediction).
 *   Entries p[k][j] with k > j and j < m are never read, whatever they hold; neither are the columns [m, ldz) of z, the columns
 *   [m + nd, ldp) of p and the rows past `rows`.
 *   z is converted float32 -> float64 (exact); every product and sum is float64 (v_mfma_f64_16x16x4_f64).  Any-order bounds:
 *   |v - exact| <= (m + 1) 2^-53 sum_k |z_k p_ko| and |q - exact| <= (4 m + 8) 2^-53 sum_j (sum_k |z_k p_kj|)^2; integer data
 *   whose sums stay below 2^53 come out bit for bit.
 *   A block owns whole rows: no workspace, no atomics, one launch.  The order of every sum is fixed and the same for every row, so
 *   a row's q and v depend on that row's values, m, nd and p alone -- not on `rows`, on where the row sits in the call or on its
 *   neighbours: bit-identical across repeats and across any division of the rows over calls.  A non-finite value of z gives a
 *   non-finite q in its own row and touches no other row.
 * Supported: 1 <= m <= 8192 (the limit of irbfn_syrk_f64), 0 <= nd <= 256, ldz >= m, ldp >= m + nd, rows >= 0 (grid-stride: no row
 * count is refused for the grid it would need).  Outside it, and with rows > 0 for a NULL z, p or q or, with nd > 0, a NULL v:
 * IRBFN_ERR_BAD_ARG as irbfn_syrk_f64, decided before any HIP call.  rows = 0: IRBFN_OK, no launch, nothing is read or written.
 * nd = 0: v_dev is not used and may be NULL. */
int irbfn_rows_quad_f64(const float* z_dev /*[rows,ldz]*/, int64_t ldz, int64_t rows, int m, const double* p_dev /*[m,ldp]*/,
                        int64_t ldp, int nd, double* q_dev /*[rows]*/, double* v_dev /*[rows,nd] or NULL with nd = 0*/,
                        void* stream);

/* Closed-loop simulation of B cars on one race line (sim_advance.hip; irbfn_amd/simulate.py): plan, apply the first control,
 * move, plan again from where the car went.  One planning tick is irbfn_plan_tick (no roll-out) and ONE irbfn_sim_advance:
 * plant step(s), way-point search in a window around the car's last segment, look-ahead goal (the f1tenth pure-pursuit rule
 * of the reference's planners), statistics, and the next query with its mirror flag.  The reference runs this loop in the
 * gym (scripts/eval_dnmpc.py); parity of the loop is unpinned, every stage repeats, bit for bit, an entry point above.
 *
 * Per-car arrays that persist between calls (device, all in/out): state_dev [B,7] float32 (single-track state
 * [x, y, delta, v, psi, psi_dot, beta]), seg_dev [B] int32 (last nearest segment), status_dev [B] int32 (irbfn_sim_status),
 * record_dev [B, irbfn_sim_record_doubles()] float64 = [ticks, sum_d2, max_d, sum_dv, progress, s_last, fail_tick].  A fresh
 * record is all zero with fail_tick = -1.  A car whose status is not IRBFN_SIM_OK is FROZEN: the call reads and writes nothing
 * of its rows in any array.  Per call and car b:
 *  1. Plant, skipped when controls_dev is NULL (the call that prepares tick 0).  a = controls[b, 0], sv = controls[b, T]
 *     (rows [a_0..a_{T-1}, sv_0..sv_{T-1}]); n_sub >= 1 steps of the single-track step of `mode` (IRBFN_ROLLOUT_ST_SELECT or
 *     IRBFN_ROLLOUT_ST_KS) with the controls held and dt' = p[8] / n_sub (a float32 division); p = dyn_params_dev[b, 0:13]
 *     where that pointer is given (one parameter row per car), else dyn_params_host[13].  The new state has the bits of
 *     irbfn_rollout_forward(mode, [state, a x n_sub, sv x n_sub], p with p[8] = dt', T = n_sub)[:, -1, :].  A non-finite
 *     component: the state is stored, status = IRBFN_SIM_NONFINITE, fail_tick = tick, and the car stops here.
 *  2. Nearest segment i, parameter t and distance d of (double)state[0:2] on the polyline waypoints[:, 0:2], with the
 *     arithmetic of irbfn_nearest_point per segment (NaN distances skipped), over the segments seg[b] - win_back ..
 *     seg[b] + win_fwd: taken modulo N - 1 on a `wrap` track, else clipped to [0, N - 2] (seg[b] itself is clipped into that
 *     range first); each segment at most once, however large the window.  win_back = win_fwd = -1: every segment.  The
 *     smallest distance wins, ties go to the lowest segment index; nothing below infinity: d = inf, t = 0, i = 0.
 *  3. Statistics, float64, unfused, in this order: ticks += 1; sum_d2 += d * d; max_d = max(max_d, d);
 *     sum_dv += |(double)state[3] - waypoints[i,3]|; s = cum[i] + t * len[i]; unless this is the car's first call (ticks was
 *     0), e = s - s_last, on a wrap track e -= length if e > length / 2, else e += length if e <= -length / 2, and
 *     progress += e; then s_last = s.
 *  4. half_width > 0 and d > half_width: status = IRBFN_SIM_OFF_TRACK, fail_tick = tick, the car stops here.
 *  5. Goal.  d < lookahead: the search of irbfn_intersect_point from t_start = i + t with radius = (float)lookahead and the
 *     track's wrap, over the whole track in that function's order, first hit wins: goal = waypoints[(first_i + N) % N, :]; no
 *     hit: IRBFN_SIM_LOST.  Else d < max_reacquire: goal = waypoints[i, :].  Else IRBFN_SIM_LOST.  LOST sets fail_tick = tick
 *     and stops the car.
 *  6. x_dev[b, 0:7] and mirror_dev[b] = irbfn_plan_queries_cartesian of pose = (double)state[b] and this goal; seg[b] = i;
 *     goal_dev [B,4], dist_dev [B], t_dev [B] (float64, each optional) get the goal row, d and t.
 * A car that stops in steps 1, 4 or 5 has its state (and, from step 4 on, its record) stored, and nothing of step 6.
 * `tick` is only stored: simulate.closed_loop passes the number of plant steps taken so far, this call's included.
 * A car's result depends on that car alone: bit-identical across repeats and however the cars are divided over calls.  No atomics, no workspace; every loop is bounded by N.
 * IRBFN_ERR_BAD_ARG, decided before any HIP call: a NULL track, B < 0, N < 2, n_sub < 1, a window side below -1 or one side
 * -1 and the other not, T < 1 with controls given, a mode other than the two, a negative or NaN lookahead or max_reacquire,
 * a NaN half_width; and, with B > 0, a NULL waypoints / cum / len / state / seg / status / record / x / mirror pointer, or
 * controls without either dyn_params pointer.  B = 0: IRBFN_OK, no launch. */
typedef enum irbfn_sim_status {
  IRBFN_SIM_OK = 0,
  IRBFN_SIM_NONFINITE = 1,   /* the plant produced a non-finite state */
  IRBFN_SIM_OFF_TRACK = 2,   /* farther than half_width from the line */
  IRBFN_SIM_LOST = 3         /* no look-ahead goal: no intersection, or farther than max_reacquire */
} irbfn_sim_status;
typedef struct irbfn_sim_track {
  const double* waypoints_dev;   /* [N,4] x, y, theta, v */
  const double* cum_dev;         /* [N-1] arc length at the start of each segment */
  const double* len_dev;         /* [N-1] segment lengths */
  double length;                 /* of the whole line, the closing segment of a wrap track included */
  double lookahead, max_reacquire, half_width;
  int N, wrap, win_back, win_fwd;
} irbfn_sim_track;
int irbfn_sim_record_doubles(void);
int irbfn_sim_advance(const irbfn_sim_track* track, int mode, int tick, const float* controls_dev /*[B,2T] or NULL*/, int T,
                      const float* dyn_params_host /*[13]*/, const float* dyn_params_dev /*[B,13] or NULL*/, int n_sub,
                      float* state_dev, int32_t* seg_dev, int32_t* status_dev, double* record_dev, float* x_dev,
                      int32_t* mirror_dev, double* goal_dev, double* dist_dev, double* t_dev, int64_t B, void* stream);

/* Closed loop with the Frenet planner's 8-input nets (K14; the same kernel as above with one more template flag): the plant
 * stays the Cartesian single-track model, and the tick changes frame before it builds the query.  The reference takes the
 * Frenet pose from the gym's spline track, which is not available: parity is unpinned, the rule below is pinned against a
 * float64 statement of itself (tests/_frenet_sim_util.py), and the fused tick against the two stand-alone entry points.
 *
 * Track curvature curv_dev [N] float64, one value per way-point, from the caller (simulate.Track computes it once on the
 * host).  With wrap(e) = e - 2 pi rint(e / 2 pi), theta = waypoints[:, 2] and len the segment lengths, Track's rule is
 * kappa_i = wrap(theta_{i+1} - theta_{i-1}) / (len_{i-1} + len_i) at interior way-points; on a `wrap` track the two end
 * way-points use their neighbours across the seam and the closing segment's length; on an open track the ends are one-sided,
 * kappa_0 = wrap(theta_1 - theta_0) / len_0 and kappa_{N-1} = wrap(theta_{N-1} - theta_{N-2}) / len_{N-2}.
 *
 * Frenet pose of one car, state [x, y, delta, v, psi, psi_dot, beta] float32, from the nearest segment i, the parameter t
 * and the distance d of step 2 above.  Everything float64, no product fused into a sum:
 *   (dx, dy) = waypoints[i+1, 0:2] - waypoints[i, 0:2];  c = dx * (y - y_i) - dy * (x - x_i)
 *   ey = c >= 0 ? d : -d  (left of the line is positive; d = 0 gives +0 or -0, neither of which is mirrored)
 *   s = cum[i] + t * len[i]  (the value of step 3)
 *   theta_line = theta_i + t * wrap(theta_{i+1} - theta_i);  epsi = wrap(psi - theta_line)
 *   curv = kappa_i + t * (kappa_{i+1} - kappa_i)
 *   vx = v cos(beta), vy = v sin(beta), wz = psi_dot, delta = delta
 *   row = [s, ey, delta, vx, vy, wz, epsi, curv], the layout irbfn_plan_queries_frenet takes.
 * Way-point i + 1 never wraps: the polyline has N - 1 segments.  The frame is that of a polyline, not of a spline: crossing
 * a vertex at lateral offset ey, s jumps by about ey * dtheta and epsi by about ey * kappa * dtheta.
 *
 * irbfn_cartesian_to_frenet: the search of step 2 and the pose, nothing else (no status: every row is converted).  seg_dev
 * given: the track's window around seg_dev[b], exactly as step 2; NULL: every segment.  frenet_dev [B,8]; seg_out_dev [B], dist_dev
 * [B], t_dev [B] optional, get i, d, t.  seg_out_dev must not overlap seg_dev.  Nothing comparable (d = inf, i = 0) gives
 * ey = +-inf.
 *
 * irbfn_sim_advance_frenet: steps 1-5 of irbfn_sim_advance word for word; step 6 becomes: the pose above from the new state;
 * vx_goal = goal[3] (the goal way-point's speed); x_dev[b, 0:8] and mirror_dev[b] = irbfn_plan_queries_frenet of that pose and
 * vx_goal; seg[b] = i; frenet_dev [B,8] (optional) gets the pose, goal_dev / dist_dev / t_dev as above.  The record keeps its
 * 7 doubles.  A NaN curvature makes a NaN query, and the plant reports IRBFN_SIM_NONFINITE one tick later; there is no new
 * status.  state, seg, status, record, goal, dist and t have the bits irbfn_sim_advance gives them; frenet_dev has the bits of
 * irbfn_cartesian_to_frenet(new state, old seg); x and mirror those of irbfn_plan_queries_frenet(frenet_dev, goal[:, 3]).
 * IRBFN_ERR_BAD_ARG, decided before any HIP call: as irbfn_sim_advance (the conversion: the track's conditions and B < 0
 * only), and with B > 0 a NULL curv_dev (the conversion: or a NULL waypoints / cum / len / state / frenet pointer).  B = 0:
 * IRBFN_OK, no launch. */
int irbfn_cartesian_to_frenet(const irbfn_sim_track* track, const double* curv_dev /*[N]*/, const float* state_dev /*[B,7]*/,
                              const int32_t* seg_dev /*[B] or NULL = every segment*/, double* frenet_dev /*[B,8]*/,
                              int32_t* seg_out_dev /*[B] or NULL*/, double* dist_dev /*or NULL*/, double* t_dev /*or NULL*/,
                              int64_t B, void* stream);
int irbfn_sim_advance_frenet(const irbfn_sim_track* track, const double* curv_dev, int mode, int tick,
                             const float* controls_dev, int T, const float* dyn_params_host, const float* dyn_params_dev,
                             int n_sub, float* state_dev, int32_t* seg_dev, int32_t* status_dev, double* record_dev,
                             float* x_dev /*[B,8]*/, int32_t* mirror_dev, double* frenet_dev /*[B,8] or NULL*/, double* goal_dev,
                             double* dist_dev, double* t_dev, int64_t B, void* stream);

/* Batched NMPC solver (nmpc_solve.hip, K13; irbfn_amd/nmpc.py): for B independent (state, goal) pairs the control sequence
 * u [2T] = [a_0..a_{T-1}, sv_0..sv_{T-1}] that minimises a tracking cost through the roll-out model of `mode`
 * (IRBFN_ROLLOUT_ST_KS or IRBFN_ROLLOUT_ST_SELECT) inside the box |a_t| <= p[10], |sv_t| <= p[9].  The reference's labels come
 * from CasADi / IPOPT solvers that cannot be run here: parity is unpinned, the rule below is pinned against a float64 statement
 * of itself (tests/_nmpc_util.py).  One problem per lane, everything float32, no atomics, no workspace.
 *   States s_1..s_T: T steps of the model's one-step map from state0 -- the bits of irbfn_rollout_forward(mode, [state0 | u]).
 *   e_t = (x_t - g_x, y_t - g_y, wrap(psi_t - g_h), v_t - g_v), wrap(e) = e - 2 pi rint(e / 2 pi), slope 1.
 *   cost(u) = 1/2 [ sum_{t<T} q . e_t^2 + qf . e_T^2 + sum_t (r_a a_t^2 + r_sv sv_t^2)
 *                   + sum_{t<T-1} (rd_a (a_{t+1} - a_t)^2 + rd_sv (sv_{t+1} - sv_t)^2) ],
 *   the terms summed in this order (per step x, y, heading, speed).  With r the residuals (each term = r_i^2) and J = dr/du:
 *   g = J^T r, H = J^T J; J holds the mask V > 3 of ST_SELECT constant and gives the clips of delta and V slope 1/2 on a bound.
 *   u = clip(u0) (0 without u0), lambda = lambda0, c = cost(u).  Each of at most max_iter iterations: a variable is FIXED if
 *   (u <= lo and g > 0) or (u >= hi and g < 0); on the others (H + diag(lambda H_jj + eps max_j H_jj)) d = -g by Cholesky (a
 *   pivot <= 0 gives d = 0 in its variable), d = 0 on the fixed ones; u+ = clip(u + d).  cost(u+) < c: accept, lambda <-
 *   max(lambda / 10, lambda_min).  CONVERGED if |c - c+| <= tol c, accepted or not (a float32 cost at its minimum moves by
 *   rounding alone; a step that every bound stops leaves it where it is), or if c+ = 0.  Else, if not accepted, reject:
 *   lambda <- min(10 lambda, lambda_max), STALLED once lambda = lambda_max.  A start with c = 0 is CONVERGED with 0 iterations; a NaN / Inf in a row's state, goal,
 *   start, parameters or first cost is NONFINITE: u = the clipped start, both costs NaN, 0 iterations.
 *   Outputs: u_dev [B,2T]; cost_dev [B,2] = (cost of the clipped start, cost of u); info_dev [B,2] = (irbfn_nmpc_status,
 *   iterations); grad_dev [B,2T] (optional) = J^T r at u.  max_iter = 0: cost and gradient at the clipped start, status
 *   IRBFN_NMPC_MAX_ITER, nothing else.  A row's result depends on that row alone: bit-identical across repeats and however the
 *   rows are divided over calls.
 * p = dyn_params_dev[b, 0:13] where that pointer is given, else dyn_params_host[13] (as irbfn_sim_advance).
 * IRBFN_ERR_BAD_ARG, decided before any HIP call: B < 0, a mode other than the two, a NULL options pointer, a weight, lambda,
 * tol or eps that is negative or not finite, lambda_min > lambda_max, max_iter < 0; and, with B > 0, a NULL state0 / goal / u /
 * cost / info pointer or neither dyn_params pointer.  T outside 1..8: IRBFN_ERR_UNSUPPORTED.  B = 0: IRBFN_OK, no launch. */
typedef enum irbfn_nmpc_status {
  IRBFN_NMPC_CONVERGED = 0,
  IRBFN_NMPC_MAX_ITER = 1,
  IRBFN_NMPC_STALLED = 2,
  IRBFN_NMPC_NONFINITE = 3
} irbfn_nmpc_status;
typedef struct irbfn_nmpc_options {
  float q[4], qf[4];         /* stage and terminal weights of (x, y, heading, speed) */
  float r[2], rd[2];         /* weights of (a, sv) and of their differences */
  float lambda0, lambda_min, lambda_max, tol, eps;
  int max_iter;
} irbfn_nmpc_options;
int irbfn_nmpc_solve(int mode, int T, const float* state0_dev /*[B,7]*/, const float* goal_dev /*[B,4]*/,
                     const float* u0_dev /*[B,2T] or NULL*/, const float* dyn_params_host /*[13]*/,
                     const float* dyn_params_dev /*[B,13] or NULL*/, const irbfn_nmpc_options* opt, float* u_dev /*[B,2T]*/,
                     float* cost_dev /*[B,2]*/, int32_t* info_dev /*[B,2]*/, float* grad_dev /*[B,2T] or NULL*/, int64_t B,
                     void* stream);
/* The same solver through the Frenet low-speed model (K15; IRBFN_ROLLOUT_FRENET_LS, which irbfn_nmpc_solve keeps refusing): the
 * controller the Frenet planner's 8-input nets imitate -- lateral and heading error on a line of given curvature.  The
 * reference's CasADi / IPOPT generators cannot be run here: parity is unpinned, the rule is pinned against a float64 statement of
 * itself (tests/_nmpc_frenet_util.py).  The rule, the options struct, the outputs, the statuses and the meaning of max_iter = 0
 * are irbfn_nmpc_solve's word for word; what differs:
 *   State: state0_dev [B,8] = [s, ey, delta, vx, vy, wz, epsi, curv]; s_1..s_T are the bits of
 *   irbfn_rollout_forward(IRBFN_ROLLOUT_FRENET_LS, [state0 | u]).  vy, wz and curv never move.
 *   Residuals: e_t = (s_t - g_0, ey_t - g_1, wrap(epsi_t - g_2), vx_t - g_3), state components {0, 1, 6, 3}, weighted by q / qf
 *   and summed in the same order.
 *   Frame: the frame ends at the centre of curvature.  A roll-out that starts any of its steps from 1 - ey_t curv <= 0 has cost
 *   +inf: as the cost of the clipped start it makes the row IRBFN_NMPC_NONFINITE (u = the clipped start, both costs NaN, 0
 *   iterations); as the cost of a trial step it is rejected and lambda grows.
 *   Bounds and slopes: the box is |a_t| <= p[10], |sv_t| <= p[9], held by projection; the clip of delta has slope 1/2 on its
 *   bound; vx has no clip in this model.
 * IRBFN_ERR_BAD_ARG / IRBFN_ERR_UNSUPPORTED / B = 0: as irbfn_nmpc_solve, decided before any HIP call (there is no mode). */
int irbfn_nmpc_solve_frenet(int T, const float* state0_dev /*[B,8]*/, const float* goal_dev /*[B,4]*/,
                            const float* u0_dev /*[B,2T] or NULL*/, const float* dyn_params_host /*[13]*/,
                            const float* dyn_params_dev /*[B,13] or NULL*/, const irbfn_nmpc_options* opt,
                            float* u_dev /*[B,2T]*/, float* cost_dev /*[B,2]*/, int32_t* info_dev /*[B,2]*/,
                            float* grad_dev /*[B,2T] or NULL*/, int64_t B, void* stream);
/* Diagnostics */
int irbfn_abi_version(void);
int irbfn_device_count(void);
int irbfn_last_hip_error(void);
const char* irbfn_strerror(int status);
/* Name + launch geometry of the kernel the last forward call on this net used (for bench/profiles). */
int irbfn_net_last_launch(const irbfn_net* net, char* name_buf, int name_len, int* grid, int* block);

#ifdef __cplusplus
}
#endif
#endif /* IRBFN_HIP_H_ */
