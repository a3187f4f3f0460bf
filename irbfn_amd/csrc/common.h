// Shared declarations of libirbfn_hip.so (gfx950 only; see include/irbfn_hip.h for the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "dispatch.h"
#include "irbfn_hip.h"

namespace irbfn {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kMaxSplit = 8;       // nsplit <= 8 (gate dims)
constexpr int kMaxD = 8;
// blocks (= partial sums) of every two-stage loss / norm reduction: the size of the caller's `partials` buffer
// (irbfn_train_loss_partials) -- train_step.hip and the cross-entropy of the cluster gate (rbf_vjp.hip) share it
constexpr int kRedBlocks = 256;
// the loss / seed kernels (one roll-out + adjoint per row) run one row per thread up to this many blocks of 256: the
// caller's `partials` buffer holds kSeedBlocksMax floats
constexpr int kSeedBlocksMax = 1024;

// basis classes the hot loops are specialised on
enum BasisClass : int { BC_GAUSS = 0, BC_IQ = 1, BC_IMQ = 2, BC_GENERIC = 3 };

__host__ __device__ inline int basis_class(int basis) {
  switch (basis) {
    case IRBFN_GAUSSIAN:
    case IRBFN_GAUSSIAN_WIDE:
    case IRBFN_GAUSSIAN_WIDER: return BC_GAUSS;
    case IRBFN_INVERSE_QUADRATIC: return BC_IQ;
    case IRBFN_INVERSE_MULTIQUADRIC: return BC_IMQ;
    default: return BC_GENERIC;
  }
}

// Gaussian family exponent scale a in exp(-a d^2) (flax_rbf.py:35-47)
inline float gauss_scale(int basis) {
  return basis == IRBFN_GAUSSIAN_WIDE ? 0.1f : (basis == IRBFN_GAUSSIAN_WIDER ? 0.01f : 1.0f);
}

extern thread_local int g_last_hip_error;

#define IRBFN_HIP_CHECK(expr)                         \
  do {                                                \
    hipError_t e__ = (expr);                          \
    if (e__ != hipSuccess) {                          \
      ::irbfn::g_last_hip_error = (int)e__;           \
      return IRBFN_ERR_HIP;                           \
    }                                                 \
  } while (0)

constexpr int kMaxDevices = 64;     // devices the per-instance launch records cover (more: the attribute is set per launch)

// hipFuncAttributeMaxDynamicSharedMemorySize once per kernel instance and device, not per launch: `set` is the instance's own
// record of the largest size it has asked for on each device.  Per device because the attribute is the device's (the multi-GPU
// runs launch the same instance on every card), the size because one instance runs geometries of different LDS; a launch then
// costs one hipGetDevice (a thread-local read) and one relaxed load.  The saving itself is host time only and is not measured.
struct DynLdsSet { std::atomic<unsigned> bytes[kMaxDevices]; };
inline int ensure_dyn_lds(const void* kernel, size_t lds, DynLdsSet* set) {
  if (lds <= 48 * 1024) return IRBFN_OK;
  int dev = 0;
  IRBFN_HIP_CHECK(hipGetDevice(&dev));
  if (dev >= 0 && dev < kMaxDevices && set->bytes[dev].load(std::memory_order_relaxed) >= lds) return IRBFN_OK;
  IRBFN_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (dev >= 0 && dev < kMaxDevices) set->bytes[dev].store((unsigned)lds, std::memory_order_relaxed);
  return IRBFN_OK;
}

// The one launch of every kernel instance K: raise K's dynamic-LDS cap where this size needs it, launch, check.
template <auto K, class... Args>
int launch_kernel(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args) {
  static DynLdsSet set;
  if (const int rc = ensure_dyn_lds(reinterpret_cast<const void*>(K), lds, &set); rc != IRBFN_OK) return rc;
  hipLaunchKernelGGL(K, grid, block, lds, s, args...);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

// One value per thread of a 256-thread block, combined in a fixed tree through sm[256] (deterministic); every thread gets the
// result.  RESYNC: a barrier behind the read of sm[0], for a caller that writes sm again.
struct TreeSum { template <typename S> __device__ static S of(S a, S b) { return a + b; } };
struct TreeMax { template <typename S> __device__ static S of(S a, S b) { return b > a ? b : a; } };
template <typename Op, bool RESYNC, typename S>
__device__ __forceinline__ S block_tree_256(S v, S* sm) {
  const int t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const S o = sm[t + w];
      sm[t] = Op::of(sm[t], o);
    }
    __syncthreads();
  }
  const S r = sm[0];
  if constexpr (RESYNC) __syncthreads();
  return r;
}
template <typename S>
__device__ __forceinline__ S block_sum_256(S v, S* sm) { return block_tree_256<TreeSum, true>(v, sm); }

struct GateTables {        // device pointers owned by the descriptor
  const float* lo;         // [nsplit][max_ranges]
  const float* hi;         // [nsplit][max_ranges]
  const float* delta;      // [nsplit]
  const int* dim_ranges;   // [n_ranges][nsplit]
  int nsplit, max_ranges, n_ranges;
};

// Region 0's row of the gate tables by value (host mirror in the descriptor, filled by irbfn_net_create): what the kernels
// of one-region nets need of GateTables, without the pointer chase dim_ranges -> lo / hi.  lo[d] = lo_tab[d][dim_ranges[0][d]].
struct GateRow {
  float lo[kMaxSplit], hi[kMaxSplit], delta[kMaxSplit];
  int nsplit, n_ranges;
};

__host__ __device__ constexpr int mfma_cw(int D) { return (D + 1 + 3) & ~3; }   // K1m record: c[D], scale, pad

struct DynParams {         // dynamics.py:24-36
  float p[13];
};
struct DynParams64 {       // the same 13 entries for the float64 training steps (train_step.hip)
  double p[13];
};
// the DynParams a one-step map of scalar type S reads (rollout_step.h)
template <typename S> struct DynOf { using type = DynParams; };
template <> struct DynOf<double> { using type = DynParams64; };

}  // namespace irbfn

// The descriptor behind the opaque handle of the ABI.
struct irbfn_net {
  int D, R, K, O, basis, bclass;
  int DC;       // D padded to a compiled width (padding coordinates are 0 in x and c)
  int N;        // R*K centres
  int OP;       // O padded to a compiled accumulator width
  int S;        // floats per packed centre record: c[D], scale, W[OP], padded to a multiple of 4
  float* rec;   // [N][S]   packed records (device)
  float* bias;  // [OP]     (device, zero padded)
  float* sig2;  // [N]      exp(-2 log_sig) (device) -- VJP
  float* recm;  // [Npad][CW + 16*NT] records of the MFMA forward (K1m); NULL if not eligible
  int Npad;     // N rounded up to a multiple of 16 (MFMA chunk)
  unsigned char* f16_img;   // chunk images of the f16-split matrix-core forward (K1h); NULL if not eligible
  float* f16_oscale;        // [128] per-output power-of-two scale of the K1h weight split
  unsigned char* gram_img;  // chunk images of K1g (distances as a Gram expansion on the matrix cores); NULL if not eligible
  void* gram_hdr;           // K1g: origin and exponents of the expansion (device, written by the pack)
  int gram_ok;              // K1g: the parameters fit the expansion's exactness budget (read back by set_params)
  int gram_exp[5];          // K1g: exponents ex, ec, eq, ea, e2 (diagnostics)
  int gram_checked;         // K1g: gram_ok has been read back at least once (IRBFN_OPT_GRAM_STICKY)
  float* pack_part;         // K1g: partial statistics of the pack, one row per 1024 centres (pack_all.hip)
  int gamma_packed;         // K1g with region weights (rbf_forward_gram_gamma.hip): the images hold the parameters last bound
  int* vjp_flags;           // K2g: ring of 64 hand-over words (rbf_vjp.hip); zero at creation, never reset
  int vjp_gen;              // K2g: generation number of the last VJP call
  float* small_part;            // K1s workspace part[NB][B][OP] (small-batch latency kernel)
  unsigned int* small_ticket;   // K1s arrival counters [8192], zero between launches
  // raw parameter pointers are NOT kept: set_params copies what it needs
  float* gate_lo;
  float* gate_hi;
  float* gate_delta;
  int* gate_ranges;
  int nsplit, max_ranges, n_ranges;
  irbfn::GateRow gate0;     // region 0's gate row (K1g passes it with the kernel arguments)
  // region-sparse path (rbf_sparse.hip): tables of the card, built by irbfn_net_create where the net is eligible
  float* sp_img;            // the net as the region-sparse kernels hold it in LDS (rbf_sparse.hip, sp_img_layout): centre
                            // table [n_ranges][RS], region index words, region masks, factor entries, Dense weight rows
  int sp_ok, sp_E, sp_cap, sp_RS, sp_EW, sp_OPS;
  float sp_mean_active;     // expected number of regions with gamma != 0 for a query uniform over the card's bounds
  bool has_params;
  int opt[IRBFN_OPT_COUNT];     // irbfn_net_set_option
  char last_name[96];
  int last_grid, last_block;

  irbfn::GateTables gate() const {
    return irbfn::GateTables{gate_lo, gate_hi, gate_delta, gate_ranges, nsplit, max_ranges, n_ranges};
  }
};

namespace irbfn {
// The kernel a forward, planning tick or parameter VJP runs and its launch geometry, decided in one place (plan_forward /
// plan_tick, rbf_forward.hip; plan_vjp, rbf_vjp.hip); the launchers take the plan as it is.  record_launch writes irbfn_net_last_launch's name from it.
enum LaunchKind : int {
  LK_NONE = 0,       // nothing runs: `status` says why
  LK_K1S,            // rbf_fwd_clane: small batches
  LK_K1R,            // rbf_fwd_sparse: region-sparse gate (`roll`: the one-launch tick)
  LK_K1G,            // rbf_fwd_f16gram
  LK_K1G_WIDE,       // rbf_fwd_f16gram_wide
  LK_K1H,            // rbf_fwd_f16mfma
  LK_K1H_WIDE,       // rbf_fwd_f16mfma_wide[_pipe]
  LK_K1M,            // rbf_fwd_mfma
  LK_K1,             // rbf_fwd_qlane (`roll`: the roll-out epilogue)
  LK_TICK_K1G,       // rbf_tick_f16gram
  LK_TICK_K1H,       // rbf_tick_f16mfma
  LK_TICK_K1G_WIDE,  // rbf_tick_f16gram_wide
  LK_TICK_K1H_WIDE,  // rbf_tick_f16mfma_wide
  LK_K2G,            // rbf_vjp_f16gram, K2h behind it (plan_vjp, rbf_vjp.hip, chooses the VJP's kind; `mode`: the live leaves)
  LK_K2,             // rbf_vjp_kernel (`gated`: region weights per lane)
  LK_K2M,            // rbf_vjp_mfma (rbf_vjp_mfma.hip; Q: padded width OW, nw: centre tiles per wave, S: query slabs)
  LK_K1G_GAMMA,      // rbf_fwd_f16gram_gamma (caller-provided region weights)
  LK_TICK_K1G_GAMMA, // rbf_tick_f16gram_gamma
  LK_K2G_GAMMA,      // rbf_vjp_f16gram_gamma, the gated K2 behind it (irbfn_net_vjp_gamma under IRBFN_VJP_K2G_GAMMA; S: query slabs)
  LK_K2H,            // rbf_vjp_f16mfma and
  LK_K2R             // rbf_vjp_sparse: record_launch gives neither a name, the previous launch's stands
};

struct F16Geom {           // K1h's block geometry where the dispatch reached K1h (forced AUTO / K1H, its image, B >= 65)
  bool ok;
  int S, QG;               // centre slices (SW of the wide kernel) x query groups of 32
  bool pipe;               // wide: the pipelined ring fits
};

struct LaunchPlan {
  int kind = LK_NONE;
  int status = IRBFN_ERR_UNSUPPORTED;  // IRBFN_OK once a kernel is chosen
  int S = 0, QG = 0;       // K1h / K1g and their ticks: centre slices (SW of the wide forms) x query groups of 32; K2g: QSB
  int terms = 3;           // K1h narrow: 3 (hi, lo) f16 pairs, 1 plain f16, 2 plain bf16
  bool pipe = false;       // K1h wide: the pipelined kernel
  int Q = 1, QJ = 0;       // K1: queries per lane; K1m: query tiles per wave
  int nw = 0;              // K1 / K1m: waves per workgroup
  int QT = 1, nb = 0, cpl = 1;  // K1s: queries per tile, centre blocks, centres per lane
  int gc = 0;              // K1r: centre table gathered from global memory
  bool gated = false;      // K1: region weights
  bool roll = false;       // K1 / K1r: the roll-out epilogue of a planning tick
  bool split = false;      // tick: this forward into the caller's controls, then the split-row roll-out
  int mode = -1;           // ticks: irbfn_rollout_mode
  size_t lds = 0;
  int grid = 0, block = 0;
  F16Geom h = {};          // K1h's geometry behind the choice (K1g stands in front of K1h); the ticks read it
};
void record_launch(irbfn_net* net, const LaunchPlan& p);

// launchers implemented per translation unit
// K0 (pack_all.hip): every image of the net in two launches
int launch_pack_all(irbfn_net* net, const float* centers, const float* log_sigs, const float* kernel, const float* bias,
                    hipStream_t s);
size_t pack_partials_bytes(const irbfn_net* net);
int launch_forward(irbfn_net* net, const float* x, float* out, int64_t B, hipStream_t s);
int launch_forward_gamma(irbfn_net* net, const float* x, const float* gamma, float* out, int64_t B, hipStream_t s);
int launch_cluster_gate(const float* x, const float* wc, const float* bc, float* logits, float* gamma, int64_t B, int D,
                        int R, hipStream_t s);
bool mfma_eligible(const irbfn_net* net);
size_t mfma_record_floats(int D, int O);
size_t mfma_lds_bytes(const irbfn_net* net, int QJ, int nw);
int launch_forward_mfma(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s);
bool f16_eligible(const irbfn_net* net);
size_t f16_image_bytes(const irbfn_net* net);
// LDS bytes of K1h's narrow kernel (tick: the one-launch tick's control and state tiles on top) and of its wide kernels
size_t f16_lds_bytes(const irbfn_net* net, int S, int QG, bool tick);
size_t f16_wide_lds_bytes(const irbfn_net* net, int SW, int QG, bool pipe);
void f16_wide_normalize(const irbfn_net* net, int* SW, int* QG, bool* pipe);
int launch_forward_f16(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s);
bool gram_eligible(const irbfn_net* net);
size_t gram_image_bytes(const irbfn_net* net);
size_t gram_header_bytes();
size_t gram_lds_bytes(int S, int QG, bool tick, bool gamma = false);   // gamma: rbf_forward_gram_gamma.hip
size_t gram_wide_ring_bytes(const irbfn_net* net, int SW);
size_t gram_wide_lds_bytes(const irbfn_net* net, int SW, int QG, size_t extra_red_floats);
int launch_forward_gram(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s);
// K1g with caller-provided region weights (rbf_forward_gram_gamma.hip): regions padded to cpr chunks; select allocates the images
int gram_gamma_cpr(const irbfn_net* net);
bool gram_gamma_eligible(const irbfn_net* net);
int gram_gamma_select(irbfn_net* net);
bool gram_gamma_wanted(const irbfn_net* net);   // an option of the net selects a kernel that reads the padded images
int launch_forward_gram_gamma(irbfn_net* net, const LaunchPlan& p, const float* x, const float* gamma, float* out, int64_t B,
                              hipStream_t s);
int launch_tick_gram_gamma(irbfn_net* net, const LaunchPlan& p, const float* x, const float* gamma, const int* mirror,
                           const float* state0, const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s);
// the one-launch planning ticks: is an instance compiled for this net, mode and horizon; their LDS; the launchers
bool tick_narrow_compiled(const irbfn_net* net, int mode, int T);
bool tick_wide_compiled(const irbfn_net* net, int mode, int T);
size_t f16_wide_tick_lds_bytes(const irbfn_net* net, int SW, int QG);
size_t gram_wide_tick_lds_bytes(const irbfn_net* net, int SW, int QG);
int launch_tick_gram_narrow(irbfn_net* net, const LaunchPlan& p, const float* x, const int* mirror, const float* state0,
                            const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s);
int launch_tick_f16_narrow(irbfn_net* net, const LaunchPlan& p, const float* x, const int* mirror, const float* state0,
                           const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s);
int launch_tick_wide(irbfn_net* net, const LaunchPlan& p, const float* x, const int* mirror, const float* state0,
                     const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s);
int tick_needs_controls(const irbfn_net* net, int mode, int64_t B, int T);
size_t small_workspace_floats(int OP);
int small_ticket_count();
bool small_eligible(const irbfn_net* net, int64_t B);
void small_geometry(const irbfn_net* net, int64_t B, LaunchPlan* p);
int launch_forward_small(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s);
int launch_gate(irbfn_net* net, const float* x, float* gamma, int64_t B, hipStream_t s);
int64_t vjp_workspace_bytes(const irbfn_net* net, int64_t B);
// the parameter VJP.  gamma_ext: caller-provided region weights (irbfn_net_vjp_gamma), else null.  frozen: irbfn_net_vjp_frozen -- a null
// g_centers / g_log_sigs is a frozen leaf, neither computed (where K2g takes the net) nor written
int launch_vjp(irbfn_net* net, const float* x, const float* gout, float* g_centers, float* g_log_sigs, float* g_kernel,
               float* g_bias, int64_t B, void* ws, hipStream_t s, const float* gamma_ext, bool frozen);
// K2m (rbf_vjp_mfma.hip): one region, fast basis, padded d in {3, 4, 7, 8}, 16 < O <= 128
bool vjpm_eligible(const irbfn_net* net);
size_t vjpm_qrec_bytes(const irbfn_net* net, int64_t B);
int vjpm_groups(const irbfn_net* net);
int vjpm_slices(const irbfn_net* net, int64_t B, int max_qsb);
void vjpm_names(const irbfn_net* net, int* OW, int* CT);
int launch_vjp_mfma(irbfn_net* net, const float* x, const float* gout, int64_t B, float* qm, float* part, int QSB, int Npad,
                    hipStream_t s);
// irbfn_net_vjp_kernel_supported: 1 if `kernel` forced on this net takes a batch of B, else 0
int vjp_kernel_supported(const irbfn_net* net, int kernel, int64_t B);
// x-VJP (rbf_vjpx.hip): gamma null = the net's tanh gate (gate term included); else caller-provided region weights, the RBF term
// only and, if dgamma is not null, q[b,r]
int launch_vjp_x(irbfn_net* net, const float* x, const float* gamma, const float* gout, float* gx, float* dgamma, int64_t B,
                 hipStream_t s);
int launch_dgamma(irbfn_net* net, const float* x, const float* gout, float* dgamma, int64_t B, hipStream_t s);
int64_t cluster_gate_vjp_workspace_bytes(int D, int R);
int launch_cluster_gate_vjp(const float* x, const float* gamma, const float* dgamma, const float* glogits, float* dlogits,
                            float* g_wc, float* g_bc, int64_t B, int D, int R, float* ws, hipStream_t s);
int launch_softmax_xent(const float* logits, const float* labels, float* glogits, float* loss, float* partials, int accumulate,
                        int64_t B, int R, hipStream_t s);
int launch_rollout_forward(int mode, const float* x0u, const DynParams& dp, float* states, int64_t B,
                           int T, hipStream_t s);
int launch_rollout_forward_split(int mode, const float* state0, const float* controls, const DynParams& dp,
                                 float* states, int64_t B, int T, hipStream_t s);
int launch_rollout_vjp(int mode, const float* x0u, const DynParams& dp, const float* gstates,
                       float* g_x0u, int64_t B, int T, float clip_tie, hipStream_t s);
int launch_rollout_vjp_select(const float* x0u, const DynParams& dp, const float* gstates, float* g_x0u, int64_t B, int T,
                              float clip_tie, hipStream_t s);
// roll-out error statistics of a table (eval_errors.hip): M = S + 2 metrics per row, < 0 for a mode without controls
int eval_num_metrics(int mode);
int64_t eval_workspace_bytes(int mode);
int launch_eval_errors(int mode, const float* state0, const float* y_pred, const float* y, const DynParams& dp, int64_t B, int T,
                       int64_t row0, int accumulate, float* err, double* stats, int64_t* argmax, int64_t* hist, void* ws,
                       hipStream_t s);
int launch_unmirror(float* controls, const int* mirror, int64_t B, int O, int sv0, hipStream_t s);
// the head kernels read h1 rows with 16-byte vector loads: the three head entry points refuse any other h1_dev
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the tick of DeeperWCRBFNet's Dense head (mlp_head.hip): H1 = H2 = 64, O = 2T; states null = controls only
int launch_mlp_head_tick(const float* h1, const float* w2, const float* b2, const float* w3, const float* b3, int mode,
                         const int* mirror, const float* state0, const DynParams& dp, float* controls, float* states, int64_t B,
                         int O, int T, hipStream_t s);
int mlp_head_tick_needs_controls(int O);
// the tick of a net evaluated with caller-provided region weights gamma[B][R] (ClusterWCRBFNet)
int launch_forward_rollout_gamma(irbfn_net* net, int mode, const float* x, const float* gamma, const int* mirror,
                                 const float* state0, const DynParams& dp, float* controls, float* states, int64_t B, int T,
                                 hipStream_t s);
int launch_forward_rollout(irbfn_net* net, int mode, const float* x, const int* mirror, const float* state0,
                           const DynParams& dp, float* controls, float* states, int64_t B, int T,
                           hipStream_t s);
int padded_O(int O);
// region-sparse evaluation of multi-region nets (rbf_sparse.hip)
int sparse_setup(irbfn_net* net, const float* lo, const float* hi, const float* delta, const int* dim_ranges);
void sparse_free(irbfn_net* net);
bool sparse_preferred(const irbfn_net* net, int64_t B);
void sparse_pack_tables(const irbfn_net* net, float** ctab, float** wtab, int* wp);   // K1r / K2r tables packed by pack_all.hip (role P)
bool sparse_vjp_eligible(const irbfn_net* net);
bool sparse_vjp_lds_fits(const irbfn_net* net);
int sparse_vjp_slices(const irbfn_net* net, int64_t B);
size_t sparse_vjp_workspace_bytes(const irbfn_net* net, int64_t B);
int launch_vjp_sparse(irbfn_net* net, const float* x, const float* gout, int64_t B, void* spws, float* part, int SL, int Npad,
                      hipStream_t s);
// K1r's geometry for B queries (roll: the one-launch tick of `mode` / T): IRBFN_OK, IRBFN_ERR_UNSUPPORTED where it has no
// instance or its LDS image does not fit, IRBFN_ERR_HIP
int sparse_geometry(const irbfn_net* net, int64_t B, bool roll, int mode, int T, LaunchPlan* p);
int launch_forward_sparse(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, const int* mirror, int sv0,
                          int mode, const float* state0, const DynParams* dp, float* states, int T, hipStream_t s);
}  // namespace irbfn
