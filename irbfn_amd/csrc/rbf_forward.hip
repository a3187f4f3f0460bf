// K0 (pack), gate kernel and the K1 dispatcher -- see rbf_forward.h for the design of K1; the K1
// instantiations live in rbf_forward_kernels.hip (one object per compiled D).
#include <math.h>
#include "rbf_forward.h"
#include "rollout_step.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace irbfn {

int launch_forward_d3(const FwdArgs&, int, int, int, bool, bool, int, size_t, hipStream_t);
int launch_forward_d4(const FwdArgs&, int, int, int, bool, bool, int, size_t, hipStream_t);
int launch_forward_d7(const FwdArgs&, int, int, int, bool, bool, int, size_t, hipStream_t);
int launch_forward_d8(const FwdArgs&, int, int, int, bool, bool, int, size_t, hipStream_t);

static const int kCompiledOP[] = {2, 4, 5, 8, 10, 16, 32, 64, 100, 128};

int padded_O(int O) {
  for (int op : kCompiledOP)
    if (O <= op) return op;
  return -1;
}

int padded_D(int D) {
  if (D <= 3) return 3;
  if (D == 4) return 4;
  if (D <= 7) return 7;
  if (D == 8) return 8;
  return -1;
}

// ------------------------------------------------------------------------------------------------
// gate kernel: _region_activation (model.py:42-95) -> gamma[B][R].  One wave per 64 queries; the
// per-dimension factors are tabulated in LDS once, then every region is a product of nsplit
// look-ups.  Used by irbfn_net_gate and as the pre-pass of the VJP.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gate_kernel(const float* __restrict__ x, float* __restrict__ gamma,
                                                  GateTables gt, long B, int D, int R) {
  extern __shared__ float gtab[];                 // [E][64]
  const int lane = threadIdx.x;
  const long b = (long)blockIdx.x * kWave + lane;
  const long bb = b < B ? b : B - 1;
  const int E = gt.nsplit * gt.max_ranges;
  for (int e = 0; e < E; ++e) {
    const int d = e / gt.max_ranges;
    gtab[e * kWave + lane] = gate_factor(x[bb * D + d], gt.lo[e], gt.hi[e], gt.delta[d]);
  }
  // each lane only reads its own column: no barrier needed
  if (b >= B) return;
  for (int r = 0; r < R; ++r) {
    float g = 0.0f;
    if (r < gt.n_ranges) {
      g = 1.0f;
      for (int d = 0; d < gt.nsplit; ++d)
        g *= gtab[(d * gt.max_ranges + gt.dim_ranges[r * gt.nsplit + d]) * kWave + lane];
    }
    gamma[b * R + r] = g;
  }
}

int launch_gate(irbfn_net* net, const float* x, float* gamma, int64_t B, hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  const size_t lds = (size_t)net->nsplit * net->max_ranges * kWave * sizeof(float);
  if (lds > 64 * 1024) return IRBFN_ERR_UNSUPPORTED;
  const long grid = (B + kWave - 1) / kWave;
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)grid), dim3(kWave), lds, s, x, gamma, net->gate(), (long)B,
                     net->D, net->R);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

// ClusterWCRBFNet gate (model.py:402-404): logits = x Wc + bc, gamma = softmax(logits) (max-subtracted, as
// jax.nn.softmax).  One thread per query, two passes over the R regions; logits are part of the model's output.
__global__ __launch_bounds__(256) void cluster_gate_kernel(const float* __restrict__ x, const float* __restrict__ wc,
                                                           const float* __restrict__ bc, float* __restrict__ logits,
                                                           float* __restrict__ gamma, long B, int D, int R) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float xv[16];
  for (int d = 0; d < D; ++d) xv[d] = x[b * D + d];
  float mx = -INFINITY;
  for (int r = 0; r < R; ++r) {
    float l = bc[r];
    for (int d = 0; d < D; ++d) l = __builtin_fmaf(xv[d], wc[d * R + r], l);
    logits[b * R + r] = l;
    mx = fmaxf(mx, l);
  }
  float sum = 0.0f;
  for (int r = 0; r < R; ++r) {
    const float e = expf(logits[b * R + r] - mx);
    gamma[b * R + r] = e;
    sum += e;
  }
  const float inv = 1.0f / sum;
  for (int r = 0; r < R; ++r) gamma[b * R + r] *= inv;
}

int launch_cluster_gate(const float* x, const float* wc, const float* bc, float* logits, float* gamma, int64_t B, int D,
                        int R, hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  if (D < 1 || D > 16 || R < 1) return IRBFN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cluster_gate_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, x, wc, bc, logits, gamma,
                     (long)B, D, R);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

// ================================================================================================
// Kernel selection.  plan_forward and plan_tick decide, from the descriptor, its options (irbfn_net_set_option,
// include/irbfn_hip.h) and B, which kernel a forward / planning tick runs and with which geometry; the launchers take the
// plan and launch.  A HIP failure of the chosen kernel is returned, never covered by another kernel.  Nothing on the launch
// path reads the environment; outside the ABI entry that stores them, the options are read here and in the VJP's plan
// (rbf_vjp.hip) only.
// ================================================================================================
static int opt_or(const irbfn_net* net, int key, int dflt) {
  const int v = net->opt[key];
  return v > 0 ? v : dflt;           // geometry options: 0 = automatic
}

static int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

// K1: queries per lane Q, waves per workgroup NW, LDS
static LaunchPlan plan_qlane(const irbfn_net* net, int64_t B, bool gated, bool roll) {
  LaunchPlan p;
  const int OP = net->OP;
  // --- Q: two queries per lane halve the scalar-stream traffic per pair, but the kernel is VALU-issue
  // bound and more resident waves hide the scalar-load latency better (measured: Q=1,NW=16 152 us vs
  // Q=2,NW=16 175 us at cfg-2), so Q = 2 only once Q = 1 alone over-subscribes the chip.  The Q = 2 instances exist for
  // the fast bases only (launch_forward_d<D>, rbf_forward_kernels.hip): generic bases stay at Q = 1 at every B.
  int Q = 1;
  const bool q2_compiled = (OP == 2 || OP == 5 || OP == 10) && net->bclass != BC_GENERIC;
  if (q2_compiled && B >= (int64_t)kWave * 32768) Q = 2;
  const int ROWS = kWave * Q;
  const long tiles = (B + ROWS - 1) / ROWS;
  // --- NW: enough waves to cover the chip (1024 SIMDs) several times, >= 32 centres per wave
  const int max_threads = (OP * Q > 48) ? 512 : 1024;
  long want = (16384 + tiles - 1) / tiles;
  int nw = want < 1 ? 1 : (want > 16 ? 16 : (int)want);
  nw = pow2_floor(nw);
  while (nw > 1 && net->N / nw < 32) nw /= 2;
  // small nets (the reference's trained ones have 1000-1280 centres): fewer, longer waves once the launch still has
  // 8 waves per SIMD -- the per-block prologue / 16-wave reduction costs as much as 80 centres per wave
  // (128-region net, B = 65536: 95 -> 75 us; 12-region Frenet net 64 -> 49 us)
  while (nw > 1 && net->N / nw < 128 && tiles * (nw / 2) >= 8192) nw /= 2;
  while (nw * kWave > max_threads) nw /= 2;
  // --- LDS: max(stage, gate table) aliased with the reduction buffers
  const int OC = OP < 16 ? OP : 16;
  size_t stage = (size_t)ROWS * net->D;
  if (gated) stage += (size_t)net->nsplit * net->max_ranges * ROWS;
  size_t red = (size_t)nw * Q * OC * (kWave + 1) + ROWS;
  const size_t roll_floats = roll ? (size_t)ROWS * (net->O + 65) : 0;      // controls + the states staging tile (pitch 65)
  red += roll_floats;
  size_t lds = (stage > red ? stage : red) * sizeof(float);
  while (lds > 160 * 1024 && nw > 1) {
    nw /= 2;
    red = (size_t)nw * Q * OC * (kWave + 1) + ROWS + roll_floats;
    lds = (stage > red ? stage : red) * sizeof(float);
  }
  if (lds > 160 * 1024) return p;
  p.kind = LK_K1; p.status = IRBFN_OK;
  p.Q = Q; p.nw = nw; p.gated = gated; p.roll = roll; p.lds = lds;
  p.grid = (int)tiles; p.block = nw * kWave;
  return p;
}

// K1m (Phi x W on the f32 matrix cores).  Measured on MI355X at cfg-2 it is SLOWER than K1 (169-217 us vs 152 us): the
// f32-input MFMA runs at the fp32 vector rate and does not overlap with the VALU distance/basis work, so with O = 10 padded
// to a 16-wide tile it buys nothing.  Kept as the "reduction expressed as a dense GEMM" variant that BASELINE config 5 asks
// to report.  For WIDE outputs (O > 16: e.g. 50-step control sequences, O = 100) the picture flips: the weight FMAs
// dominate and the MFMA issues them ~1.8x more densely than SGPR-operand v_fmac (cfg-4 forward 342 -> 301 us), so K1m is
// preferred over K1 there (behind K1h where that is eligible).  IRBFN_FWD_K1 / IRBFN_FWD_K1M force K1 / K1m.
static bool prefer_mfma(const irbfn_net* net) {
  const int e = net->opt[IRBFN_OPT_FWD_KERNEL];
  if (!net->recm || e == IRBFN_FWD_K1) return false;
  return e == IRBFN_FWD_K1M || net->O > 16;
}

static bool plan_mfma(const irbfn_net* net, int64_t B, LaunchPlan* p) {
  const bool wide = net->O > 16;
  const int QJ = wide ? 2 : 4;                   // QJ = 4 is compiled for NT <= 4 only
  const long tiles = (B + 16 * QJ - 1) / (16 * QJ);
  long want = ((wide ? 2048 : 8192) + tiles - 1) / tiles;
  int nw = want < 1 ? 1 : (want > 16 ? 16 : (int)want);
  nw = pow2_floor(nw);
  const int chunks = net->Npad / 16;
  while (nw > 1 && chunks / nw < 2) nw /= 2;
  // the reduction tile [nw][16 QJ][16 NT + 1] grows with nw (NT = 7, 8 at nw = 16: 231 / 264 KB): fewer waves, as plan_qlane does
  size_t lds = mfma_lds_bytes(net, QJ, nw);
  while (lds > 160 * 1024 && nw > 1) {
    nw /= 2;
    lds = mfma_lds_bytes(net, QJ, nw);
  }
  if (lds > 160 * 1024) return false;
  const int NT = (net->O + 15) / 16;
  if (NT == 5 || NT == 6) return false;          // compiled for NT = 1..4, 7, 8
  p->kind = LK_K1M; p->status = IRBFN_OK;
  p->QJ = QJ; p->nw = nw; p->lds = lds; p->grid = (int)tiles; p->block = nw * kWave;
  return true;
}

// K1h (Phi x W on the f16 matrix cores at float32 accuracy, rbf_forward_f16.hip): one region, fast basis, O <= 128.  The
// default where eligible (cfg-2 131 vs 142 us, cfg-5 7.5 vs 8.9 ms against K1); IRBFN_OPT_FWD_KERNEL forces another kernel,
// IRBFN_OPT_FWD_F16_TERMS = 1 / 2 the reduced-precision single-product variants (reporting only).  Its block geometry
// where the dispatch reaches it; the one-launch ticks run the same geometry, so that they reduce the slices in the same order
// as the plain forward.
static F16Geom f16_geometry(const irbfn_net* net, int64_t B) {
  F16Geom g = {};
  const int e = net->opt[IRBFN_OPT_FWD_KERNEL];
  if (e != IRBFN_FWD_AUTO && e != IRBFN_FWD_K1H) return g;
  if (!net->f16_img || !f16_eligible(net) || B < 65) return g;
  const long groups = (B + 31) / 32;
  if (net->O > 16) {
    // wide outputs: block-shared W stream; SW = centre slices per block so that the grid covers the 256 CUs
    int SW = 1;
    while (SW < 4 && (groups * SW + 7) / 8 < 256) SW *= 2;
    SW = opt_or(net, IRBFN_OPT_FWD_F16_S, SW);
    if (SW != 1 && SW != 2 && SW != 4) SW = 1;
    int QG = opt_or(net, IRBFN_OPT_FWD_F16_QG, 8 / SW);
    f16_wide_normalize(net, &SW, &QG, &g.pipe);
    g.S = SW; g.QG = QG;
  } else {
    // narrow outputs: S centre slices x QG query groups of 32 per 8-wave block, S chosen so that the launch has >= 16384 waves
    long want = (16384 + groups - 1) / groups;           // measured at cfg-2: S = 8 (16384 waves) 131 us, S = 4 134 us
    int S = want < 1 ? 1 : (want > 8 ? 8 : (int)want);
    S = pow2_floor(S);
    if (S < want && S < 8) S *= 2;
    const int nchunks = (net->N + 31) / 32;
    while (S > 1 && nchunks / S < 2) S /= 2;
    // small nets: at least 8 chunks per wave once the launch still has 4 waves per SIMD (the slice reduction and the
    // prologue cost as much as a few chunks; N = 1000: 47.5 -> 44.5 us, N = 256: 23.6 -> 19.1 us at B = 65536)
    while (S > 1 && nchunks / S < 8 && groups * (S / 2) >= 4096) S /= 2;
    S = opt_or(net, IRBFN_OPT_FWD_F16_S, S);
    if (S > 8 || S > nchunks) S = 1;
    int QG = opt_or(net, IRBFN_OPT_FWD_F16_QG, 8 / S);
    if (S * QG > 8) QG = 1;
    g.S = S; g.QG = QG;
  }
  g.ok = true;
  return g;
}

static int f16_terms(const irbfn_net* net) {
  const int ot = net->opt[IRBFN_OPT_FWD_F16_TERMS];
  return (ot == 1 || ot == 2) ? ot : 3;          // 1: plain f16, 2: plain bf16 (both reporting only), 3: pairs
}

static bool plan_f16(const irbfn_net* net, int64_t B, LaunchPlan* p) {
  const F16Geom& h = p->h;
  size_t lds;
  if (net->O > 16) {
    lds = f16_wide_lds_bytes(net, h.S, h.QG, h.pipe);
    if (lds > 160 * 1024) return false;
    p->kind = LK_K1H_WIDE; p->pipe = h.pipe;
  } else {
    lds = f16_lds_bytes(net, h.S, h.QG, false);
    if (lds > 64 * 1024) return false;
    p->kind = LK_K1H; p->terms = f16_terms(net);
  }
  p->status = IRBFN_OK;
  p->S = h.S; p->QG = h.QG; p->lds = lds;
  p->grid = (int)(((B + 31) / 32 + h.QG - 1) / h.QG); p->block = h.S * h.QG * 64;
  return true;
}

// K1g (rbf_forward_gram.hip): where K1h's narrow kernel would run with its default operand pairs and the parameters fit the
// expansion (gram_ok, set by the pack)
static bool gram_preferred(const irbfn_net* net, int64_t B) {
  const int ot = net->opt[IRBFN_OPT_FWD_F16_TERMS];
  // below ~12k queries K1h's eight centre slices per query group finish sooner (config-2 net: B = 8192 27 vs 35 us,
  // B = 16384 44 vs 37 us)
  return net->gram_img && net->gram_ok && net->O <= 16 && (ot == 3 || ot == 0) && B >= 12288;
}

// K1g for wide outputs (rbf_forward_gram_wide.hip): d = 7 or 8, the parameters fit the expansion
static bool gram_wide_preferred(const irbfn_net* net, int64_t B) {
  return net->gram_img && net->gram_ok && net->O > 16 && net->O <= 128 && (net->DC == 7 || net->DC == 8) && B >= 2048 && net->N >= 256;
}

// S centre slices x QG query groups of 32 per block; the QG waves of a slice share one stream of chunk images (a ring of five,
// 35 KiB of LDS per slice).  Measured at the config-2 net (profiles/r03_gram_batch_sweep.txt; us at B = 16384 / 24576 / 32768 /
// 65536 / 131072 / 262144): S = 4, QG = 2: 38 / 70 / 72 / 139 / 275 / 547; S = 2, QG = 4: 53 / 53 / 55 / 82 / 155 / 298; S = 1, QG = 8:
// 88 / 88 / 88 / 88 / 142 / 273 -- more slices while the launch is short of waves, never more blocks than are resident at once.
// Between one and one and a half rounds of the S = 2 form (2048 < groups <= 3072: the reference's training batch of 80000) a
// second, thin round of blocks costs a wave's whole latency-bound pass over its slice; blocks of FOUR waves with all the centres
// (S = 1, QG = 4: four resident per CU, 4096 groups at once) spread the same work over the chip in one round
// (profiles/r03_gram_geometry_sweep.txt: N = 1000, B = 80000: 40.7 vs 47.4 us; N = 2048: 67 vs 73; N = 4096: 121 vs 122).
// S = 2 with more than 1024 groups would put two blocks of eight waves on a CU; ONE block of sixteen (S = 2, QG = 8) keeps the CU's
// sixteen waves and streams each chunk image into LDS once instead of twice: half the LDS-DMA requests per wave, whose issue is the
// largest cost of a step that is not arithmetic (profiles/k1g_setup_and_refills.txt: config 2 83.4 -> 81.4 us).  QG does not enter
// the order of any sum.  gram_default_qg is the one statement of the rule (plan_gram_gamma's forced S takes it too).
static int gram_default_qg(int S, long groups) {
  if (S == 1 && groups > 2048 && groups <= 3072) return 4;
  if (S == 2 && groups > 1024) return 8;
  return 8 / S > 0 ? 8 / S : 1;
}

static void gram_geometry(const irbfn_net* net, int64_t B, int nchunks, int* S_out, int* QG_out) {
  const long groups = (B + 31) / 32;
  int S = groups <= 512 ? 4 : (groups <= 2048 ? 2 : 1);
  while (S > 1 && nchunks / (2 * S) < 4) S /= 2;            // at least 8 chunks per wave
  S = opt_or(net, IRBFN_OPT_FWD_F16_S, S);
  if (S > 7 || S > nchunks) S = 1;
  int QG = opt_or(net, IRBFN_OPT_FWD_F16_QG, gram_default_qg(S, groups));
  if (S * QG > 16) QG = 1;
  *S_out = S; *QG_out = QG;
}

// block geometry of the wide K1g kernels: SW centre slices x QG query groups of 32, the slices' rings (three chunk images each)
// within the 160 KB of LDS
static void gram_wide_geometry(const irbfn_net* net, int64_t B, int* SW_out, int* QG_out) {
  const int nchunks = (net->N + 31) / 32;
  const long groups = (B + 31) / 32;
  int SW = 1;
  while (SW < 4 && (groups * SW + 7) / 8 < 256) SW *= 2;
  SW = opt_or(net, IRBFN_OPT_FWD_F16_S, SW);
  if (SW != 1 && SW != 2 && SW != 4) SW = 1;
  while (SW > 1 && (gram_wide_ring_bytes(net, SW) > 160 * 1024 || nchunks / SW < 2)) SW /= 2;
  // query groups per block, measured at config 4 (us; B = 8192 / 32768 / 262144): SW=2 QG=2: 88 / 173 / 1359; SW=2 QG=4: 109 / 117 / 863;
  // SW=1 QG=4: 133 / 136 / 698; SW=1 QG=8: 183 / 186 / 742 (K1h's wide kernel: 102 / 132 / 921)
  int QG = groups <= 384 ? 2 : (SW == 1 ? 4 : 8 / SW);
  QG = opt_or(net, IRBFN_OPT_FWD_F16_QG, QG);
  if (QG < 1 || SW * QG > 8) QG = 8 / SW;
  *SW_out = SW; *QG_out = QG;
}

// The narrow K1g kernels cut the chunk range into slices in 32-bit arithmetic (gram_body: c0, c1), so nchunks x S must stay below
// 2^31.  No net that exists gets there.  One-region kernels: irbfn_net_create accepts at most 2^30 centres, i.e. 2^25 chunks, and
// gram_geometry at most S = 7 slices: nchunks x S < 2^28.  Padded regions (caller-provided weights): nchunks = R x cpr can
// approach 2^30 at K = 1, but 2^31 / 7 chunk images of 7 KiB are 2 TB of device memory.
static bool gram_slices_fit(int nchunks, int S) { return (long)nchunks * S < (1L << 31); }

// K1g, narrow or wide: its image, the parameters inside the expansion's budget (checked by the caller), LDS
static bool plan_gram(const irbfn_net* net, int64_t B, LaunchPlan* p) {
  if (!net->f16_img || !gram_eligible(net)) return false;
  int S, QG;
  size_t lds;
  if (net->O > 16) {
    if ((net->DC != 7 && net->DC != 8) || net->O > 128) return false;
    gram_wide_geometry(net, B, &S, &QG);
    lds = gram_wide_lds_bytes(net, S, QG, 0);
    p->kind = LK_K1G_WIDE;
  } else {
    gram_geometry(net, B, (net->N + 31) / 32, &S, &QG);
    if (!gram_slices_fit((net->N + 31) / 32, S)) return false;
    lds = gram_lds_bytes(S, QG, false);
    p->kind = LK_K1G;
  }
  if (lds > 160 * 1024) {
    p->kind = LK_NONE;
    return false;
  }
  p->status = IRBFN_OK;
  p->S = S; p->QG = QG; p->lds = lds;
  p->grid = (int)(((B + 31) / 32 + QG - 1) / QG); p->block = S * QG * 64;
  return true;
}

// the forward's kernel for B > 0 queries
static LaunchPlan plan_forward(const irbfn_net* net, int64_t B) {
  LaunchPlan p;
  const int forced = net->opt[IRBFN_OPT_FWD_KERNEL];
  // K1s: small batches (planner ticks) -> centre-lane latency kernel
  if (forced == IRBFN_FWD_AUTO && small_eligible(net, B)) {
    small_geometry(net, B, &p);
    return p;
  }
  // K1r: several regions with a sparse gate -> every query visits only its non-zero regions (rbf_sparse.hip)
  if (forced == IRBFN_FWD_K1R || (forced == IRBFN_FWD_AUTO && sparse_preferred(net, B))) {
    p.status = sparse_geometry(net, B, false, 0, 0, &p);
    if (p.status != IRBFN_ERR_UNSUPPORTED || forced == IRBFN_FWD_K1R) return p;
  }
  if (forced == IRBFN_FWD_K1G) {
    if (net->gram_img && net->gram_ok) plan_gram(net, B, &p);
    return p;
  }
  p.h = f16_geometry(net, B);
  if (p.h.ok) {
    // K1g in front of K1h: the distances on the matrix cores as well
    const bool gram = net->O > 16 ? gram_wide_preferred(net, B) : gram_preferred(net, B);
    if (forced == IRBFN_FWD_AUTO && gram && plan_gram(net, B, &p)) return p;
    if (plan_f16(net, B, &p)) return p;
  }
  if (forced == IRBFN_FWD_K1H) return p;
  if (prefer_mfma(net) && plan_mfma(net, B, &p)) return p;
  if (forced == IRBFN_FWD_K1M) return p;
  const F16Geom h = p.h;
  p = plan_qlane(net, B, net->R > 1, false);
  p.h = h;
  return p;
}

// ---- planning tick ------------------------------------------------------------------------------------------------------
// K1h-wide's one-launch tick: an instance for this net / mode / horizon, the forward runs K1h-wide with the pipelined ring
static bool tick_wide_k1h(const irbfn_net* net, const LaunchPlan& fp, int mode, int64_t B, int T) {
  return net->opt[IRBFN_OPT_TICK_FUSED] != 0 && B > 64 && tick_wide_compiled(net, mode, T) && fp.h.ok && fp.h.pipe;
}

// K1h's narrow one-launch tick: an instance for this net / mode / horizon, the forward reaches K1h with the default operand
// pairs, the control and state tiles fit
static bool tick_narrow_k1h(const irbfn_net* net, const LaunchPlan& fp, int mode, int T, size_t* lds) {
  if (net->opt[IRBFN_OPT_TICK_FUSED] == 0 || !tick_narrow_compiled(net, mode, T)) return false;
  if (!fp.h.ok || net->O > 16 || f16_terms(net) != 3) return false;
  *lds = f16_lds_bytes(net, fp.h.S, fp.h.QG, true);
  return *lds <= 64 * 1024;
}

// the tick runs forward -> roll-out through a controls buffer (when the caller provides one): wide outputs, and narrow ones on
// K1h without a one-launch instance (K1h forward + K3 beat K1 with the roll-out in its epilogue: 134 + 17 vs 173 us at config 2's
// size; the 2 x B x O x 4 bytes of control traffic are noise next to the B x N pair work)
static bool tick_through_controls(const irbfn_net* net, const LaunchPlan& fp, int64_t B) {
  return B > 64 && (prefer_mfma(net) || (fp.h.ok && net->O <= 16));
}

// the tick's kernel for B > 0 queries, a states output, a roll-out mode with a fused form and O = 2T
static LaunchPlan plan_tick(const irbfn_net* net, int mode, int64_t B, int T, bool controls) {
  const LaunchPlan fp = plan_forward(net, B);
  if (fp.status == IRBFN_ERR_HIP) return fp;
  const int forced = net->opt[IRBFN_OPT_FWD_KERNEL];
  LaunchPlan t;
  t.mode = mode; t.status = IRBFN_OK;
  auto geometry = [&](int kind, int S, int QG) {
    t.kind = kind; t.S = S; t.QG = QG;
    t.grid = (int)(((B + 31) / 32 + QG - 1) / QG); t.block = S * QG * 64;
  };
  // the whole tick in one launch where the instance exists (wide: plan_tick_wide.hip; narrow: rbf_tick_f16mfma / rbf_tick_f16gram)
  if (tick_wide_k1h(net, fp, mode, B, T)) {
    // K1g's wide tick is tried only once K1h-wide's tick plan has passed, pipelined ring included
    if (fp.kind == LK_K1G_WIDE) {
      geometry(LK_TICK_K1G_WIDE, fp.S, fp.QG);
      t.lds = gram_wide_tick_lds_bytes(net, fp.S, fp.QG);
      if (t.lds <= 160 * 1024) return t;
    }
    geometry(LK_TICK_K1H_WIDE, fp.h.S, fp.h.QG);
    t.lds = f16_wide_tick_lds_bytes(net, fp.h.S, fp.h.QG);
    if (t.lds <= 160 * 1024) return t;
  }
  // a forced K1g below gram_preferred's batch floor runs in the forward, but the tick does not take it
  const bool gram_tick = fp.kind == LK_K1G && (forced != IRBFN_FWD_K1G || gram_preferred(net, B));
  if (gram_tick && net->opt[IRBFN_OPT_TICK_FUSED] != 0 && tick_narrow_compiled(net, mode, T)) {
    geometry(LK_TICK_K1G, fp.S, fp.QG);
    t.lds = gram_lds_bytes(fp.S, fp.QG, true);
    // S = 2, QG = 8 (gram_default_qg) is the largest tick: 117 KB.  A tick tile that grew past 160 KB would send the batches above 1024
    // groups to the K1h tick below without a word; tests/test_gpu_gram_setup.py asserts by name that they run rbf_tick_f16gram.
    if (t.lds <= 160 * 1024) return t;
  }
  if (tick_narrow_k1h(net, fp, mode, T, &t.lds)) {
    geometry(LK_TICK_K1H, fp.h.S, fp.h.QG);
    return t;
  }
  // several regions, sparse gate: forward + sign flip + roll-out in one launch of the region-sparse kernel
  if (fp.kind == LK_K1R) {
    LaunchPlan r;
    r.status = sparse_geometry(net, B, true, mode, T, &r);
    if (r.status != IRBFN_ERR_UNSUPPORTED) return r;
  }
  if (controls && tick_through_controls(net, fp, B)) {
    LaunchPlan f = fp;
    f.split = true;
    return f;
  }
  t = LaunchPlan();
  if (net->bclass == BC_GENERIC) return t;
  if (T * rollout_state_dim(mode) > 64) return t;      // the epilogue's staging tile holds 64 floats per row
  return plan_qlane(net, B, net->R > 1, true);
}

int tick_needs_controls(const irbfn_net* net, int mode, int64_t B, int T) {
  if (B <= 64) return 0;
  const LaunchPlan fp = plan_forward(net, B);
  size_t lds;
  if (tick_wide_k1h(net, fp, mode, B, T) || tick_narrow_k1h(net, fp, mode, T, &lds)) return 0;    // one launch, controls stay in LDS
  return tick_through_controls(net, fp, B) ? 1 : 0;   // forward + split-row roll-out through the caller's buffer
}

// ---- launch ---------------------------------------------------------------------------------------------------------------
void record_launch(irbfn_net* net, const LaunchPlan& p) {
  char* n = net->last_name;
  const size_t len = sizeof(net->last_name);
  const int NT = (net->O + 15) / 16, D = net->DC, BC = net->bclass;
  switch (p.kind) {
    case LK_K1S: snprintf(n, len, "rbf_fwd_clane<D=%d,OP=%d,BC=%d,QT=%d>", D, net->OP, BC, p.QT); break;
    case LK_K1R: snprintf(n, len, "rbf_fwd_sparse<D=%d,OP=%d,BC=%d,ROLL=%d,GC=%d>", D, net->sp_OPS, BC, (int)p.roll, p.gc); break;
    case LK_K1G: snprintf(n, len, "rbf_fwd_f16gram<D=%d,BC=%d,S=%d,QG=%d>", D, BC, p.S, p.QG); break;
    case LK_K1G_WIDE: snprintf(n, len, "rbf_fwd_f16gram_wide<D=%d,BC=%d,NT=%d,SW=%d,QG=%d>", D, BC, NT, p.S, p.QG); break;
    case LK_K1H:
      snprintf(n, len, "rbf_fwd_f16mfma<D=%d,BC=%d,TERMS=%s,S=%d,QG=%d>", D, BC,
               p.terms == 1 ? "1" : (p.terms == 2 ? "1,BF16" : "3"), p.S, p.QG);
      break;
    case LK_K1H_WIDE:
      snprintf(n, len, "rbf_fwd_f16mfma_wide%s<D=%d,BC=%d,NT=%d,SW=%d,QG=%d>", p.pipe ? "_pipe" : "", D, BC, NT, p.S, p.QG);
      break;
    case LK_K1M: snprintf(n, len, "rbf_fwd_mfma<D=%d,NT=%d,QJ=%d,BC=%d>", net->D, NT, p.QJ, BC); break;
    case LK_K1:
      snprintf(n, len, "rbf_fwd_qlane<D=%d,OP=%d,Q=%d,BC=%d,GATED=%d,ROLL=%d>", D, net->OP, p.Q, BC, (int)p.gated, (int)p.roll);
      break;
    case LK_TICK_K1G: snprintf(n, len, "rbf_tick_f16gram<D=%d,BC=%d,MODE=%d,S=%d,QG=%d>", D, BC, p.mode, p.S, p.QG); break;
    case LK_TICK_K1H: snprintf(n, len, "rbf_tick_f16mfma<D=%d,BC=%d,MODE=%d,S=%d,QG=%d>", D, BC, p.mode, p.S, p.QG); break;
    case LK_TICK_K1G_WIDE: snprintf(n, len, "rbf_tick_f16gram_wide<D=7,BC=%d,NT=7,MODE=%d,SW=%d,QG=%d>", BC, p.mode, p.S, p.QG); break;
    case LK_TICK_K1H_WIDE: snprintf(n, len, "rbf_tick_f16mfma_wide<D=7,BC=%d,NT=7,MODE=%d,SW=%d,QG=%d>", BC, p.mode, p.S, p.QG); break;
    case LK_K1G_GAMMA: snprintf(n, len, "rbf_fwd_f16gram_gamma<D=%d,BC=%d,S=%d,QG=%d>", D, BC, p.S, p.QG); break;
    case LK_TICK_K1G_GAMMA: snprintf(n, len, "rbf_tick_f16gram_gamma<D=%d,BC=%d,MODE=%d,S=%d,QG=%d>", D, BC, p.mode, p.S, p.QG); break;
    case LK_K2G:                 // mode: K2g's live leaves (irbfn_net_vjp_frozen) -- 1 no centres, 2 the Dense leaves only
      snprintf(n, len, "rbf_vjp_f16gram%s<D=%d,BC=%d,QSB=%d>", p.mode == 1 ? "/no_centres" : (p.mode == 2 ? "/linear" : ""), D, BC, p.S);
      break;
    case LK_K2G_GAMMA: snprintf(n, len, "rbf_vjp_f16gram_gamma<D=%d,BC=%d,QSB=%d>", D, BC, p.S); break;
    case LK_K2: snprintf(n, len, "rbf_vjp_kernel<D=%d,OP=%d,BC=%d,GATED=%d>", D, net->OP, BC, (int)p.gated); break;
    case LK_K2M: snprintf(n, len, "rbf_vjp_mfma<D=%d,OW=%d,BC=%d,CT=%d,QSB=%d>", D, p.Q, BC, p.nw, p.S); break;
    default: return;
  }
  net->last_grid = p.grid;
  net->last_block = p.block;
}

static void fill_args(irbfn_net* net, FwdArgs& a, const float* x, float* out, int64_t B) {
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.rec = net->rec;
  a.bias = net->bias;
  a.out = out;
  a.gate = net->gate();
  a.B = (long)B;
  a.Dreal = net->D;
  a.O = net->O;
  a.N = net->N;
  a.K = net->K;
  a.S = net->S;
  a.basis = net->basis;
  a.R = net->R;
}

static int launch_qlane(irbfn_net* net, const LaunchPlan& p, const FwdArgs& a, hipStream_t s) {
  switch (net->DC) {
    case 3: return launch_forward_d3(a, net->OP, p.Q, net->bclass, p.gated, p.roll, p.nw, p.lds, s);
    case 4: return launch_forward_d4(a, net->OP, p.Q, net->bclass, p.gated, p.roll, p.nw, p.lds, s);
    case 7: return launch_forward_d7(a, net->OP, p.Q, net->bclass, p.gated, p.roll, p.nw, p.lds, s);
    case 8: return launch_forward_d8(a, net->OP, p.Q, net->bclass, p.gated, p.roll, p.nw, p.lds, s);
    default: return IRBFN_ERR_UNSUPPORTED;
  }
}

// a forward plan into `out`
static int launch_planned(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s) {
  int rc;
  switch (p.kind) {
    case LK_K1S: rc = launch_forward_small(net, p, x, out, B, s); break;
    case LK_K1R: rc = launch_forward_sparse(net, p, x, out, B, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, s); break;
    case LK_K1G:
    case LK_K1G_WIDE: rc = launch_forward_gram(net, p, x, out, B, s); break;
    case LK_K1H:
    case LK_K1H_WIDE: rc = launch_forward_f16(net, p, x, out, B, s); break;
    case LK_K1M: rc = launch_forward_mfma(net, p, x, out, B, s); break;
    case LK_K1: {
      FwdArgs a;
      fill_args(net, a, x, out, B);
      rc = launch_qlane(net, p, a, s);
      break;
    }
    default: return p.status;
  }
  if (rc == IRBFN_OK) record_launch(net, p);
  return rc;
}

int launch_forward(irbfn_net* net, const float* x, float* out, int64_t B, hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  return launch_planned(net, plan_forward(net, B), x, out, B, s);
}

// K1g with caller-provided region weights (rbf_forward_gram_gamma.hip), selected by IRBFN_OPT_FWD_GAMMA_KERNEL = IRBFN_FWDG_K1G only.
// status: IRBFN_ERR_UNSUPPORTED for a net outside its instances or parameters outside the expansion's budget (the pack's verdict),
// IRBFN_ERR_NO_PARAMS while the images have not been packed since the option was set.  K1g's geometry over the R x cpr chunks of
// the padded regions; a forced S stands even where slices stay empty.
static LaunchPlan plan_gram_gamma(const irbfn_net* net, int64_t B, bool tick, int mode) {
  LaunchPlan p;
  if (!gram_gamma_eligible(net)) return p;
  const bool packed = net->gram_img && net->f16_img && (net->R == 1 || net->gamma_packed);
  if (!packed) { p.status = IRBFN_ERR_NO_PARAMS; return p; }
  if (!net->gram_ok) return p;
  const int nchunks = net->R * gram_gamma_cpr(net);
  int S, QG;
  gram_geometry(net, B, nchunks, &S, &QG);
  const int fs = net->opt[IRBFN_OPT_FWD_F16_S];
  if (fs > 0 && fs <= 7 && S != fs) {
    S = fs;
    QG = opt_or(net, IRBFN_OPT_FWD_F16_QG, gram_default_qg(S, (B + 31) / 32));
    if (S * QG > 16) QG = 1;
  }
  p.lds = gram_lds_bytes(S, QG, tick, true);
  if (p.lds > 160 * 1024 || !gram_slices_fit(nchunks, S)) return p;
  p.kind = tick ? LK_TICK_K1G_GAMMA : LK_K1G_GAMMA; p.status = IRBFN_OK; p.mode = mode;
  p.S = S; p.QG = QG;
  p.grid = (int)(((B + 31) / 32 + QG - 1) / QG); p.block = S * QG * 64;
  return p;
}

// forward with caller-provided region weights gamma[B][R] (ClusterWCRBFNet): the gated K1 unless the descriptor selects K1g
int launch_forward_gamma(irbfn_net* net, const float* x, const float* gamma, float* out, int64_t B, hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  if (net->opt[IRBFN_OPT_FWD_GAMMA_KERNEL] == IRBFN_FWDG_K1G) {
    const LaunchPlan g = plan_gram_gamma(net, B, false, -1);
    if (g.kind == LK_NONE) return g.status;
    const int rc = launch_forward_gram_gamma(net, g, x, gamma, out, B, s);
    if (rc == IRBFN_OK) record_launch(net, g);
    return rc;
  }
  const LaunchPlan p = plan_qlane(net, B, true, false);
  if (p.kind == LK_NONE) return p.status;
  FwdArgs a;
  fill_args(net, a, x, out, B);
  a.gamma_ext = gamma;
  const int rc = launch_qlane(net, p, a, s);
  if (rc == IRBFN_OK) record_launch(net, p);
  return rc;
}

// ---- pieces both ticks below share (gamma: the caller's region weights, null for the net's own gate) ----------------------
// controls only (no states asked for): any forward kernel, then the sign flip
static int forward_controls_only(irbfn_net* net, const float* x, const float* gamma, const int* mirror, float* controls, int64_t B,
                                 hipStream_t s) {
  if (!controls) return IRBFN_ERR_BAD_ARG;
  const int rc = gamma ? launch_forward_gamma(net, x, gamma, controls, B, s) : launch_forward(net, x, controls, B, s);
  if (rc != IRBFN_OK || !mirror) return rc;
  return launch_unmirror(controls, mirror, B, net->O, net->O / 2, s);
}

static int check_tick(const irbfn_net* net, int mode, int T) {
  if (mode != IRBFN_ROLLOUT_ST_SELECT && mode != IRBFN_ROLLOUT_ST_KS && mode != IRBFN_ROLLOUT_FULLINT &&
      mode != IRBFN_ROLLOUT_FRENET_LS)
    return IRBFN_ERR_UNSUPPORTED;
  return net->O != 2 * T ? IRBFN_ERR_BAD_ARG : IRBFN_OK;
}

// K1 with the roll-out in its epilogue
static int launch_qlane_tick(irbfn_net* net, const LaunchPlan& p, int mode, const float* x, const float* gamma, const int* mirror,
                             const float* state0, const DynParams& dp, float* controls, float* states, int64_t B, int T,
                             hipStream_t s) {
  FwdArgs a;
  fill_args(net, a, x, controls, B);
  a.gamma_ext = gamma;
  a.state0 = state0;
  a.states = states;
  a.T = T;
  a.mode = mode;
  a.dp = dp;
  a.mirror = mirror;
  a.sv0 = T;
  return launch_qlane(net, p, a, s);
}

int launch_forward_rollout(irbfn_net* net, int mode, const float* x, const int* mirror, const float* state0,
                           const DynParams& dp, float* controls, float* states, int64_t B, int T,
                           hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  if (states == nullptr) return forward_controls_only(net, x, nullptr, mirror, controls, B, s);
  if (const int rc = check_tick(net, mode, T); rc != IRBFN_OK) return rc;
  const LaunchPlan p = plan_tick(net, mode, B, T, controls != nullptr);
  if (p.split) {
    int rc = launch_planned(net, p, x, controls, B, s);
    if (rc == IRBFN_OK && mirror) rc = launch_unmirror(controls, mirror, B, net->O, T, s);
    if (rc != IRBFN_OK) return rc;
    return launch_rollout_forward_split(mode, state0, controls, dp, states, B, T, s);
  }
  int rc;
  switch (p.kind) {
    case LK_TICK_K1G_WIDE:
    case LK_TICK_K1H_WIDE: rc = launch_tick_wide(net, p, x, mirror, state0, dp, controls, states, B, T, s); break;
    case LK_TICK_K1G: rc = launch_tick_gram_narrow(net, p, x, mirror, state0, dp, controls, states, B, T, s); break;
    case LK_TICK_K1H: rc = launch_tick_f16_narrow(net, p, x, mirror, state0, dp, controls, states, B, T, s); break;
    case LK_K1R: rc = launch_forward_sparse(net, p, x, controls, B, mirror, T, mode, state0, &dp, states, T, s); break;
    case LK_K1: rc = launch_qlane_tick(net, p, mode, x, nullptr, mirror, state0, dp, controls, states, B, T, s); break;
    default: return p.status;
  }
  if (rc == IRBFN_OK) record_launch(net, p);
  return rc;
}

// the tick with caller-provided region weights gamma[B][R] (ClusterWCRBFNet, model.py:393-412): the gated K1 with the roll-out
// in its epilogue; where that plan cannot roll (generic basis, T x S > 64 floats of staging, LDS), forward -> sign flip ->
// split-row roll-out through the caller's controls buffer
int launch_forward_rollout_gamma(irbfn_net* net, int mode, const float* x, const float* gamma, const int* mirror,
                                 const float* state0, const DynParams& dp, float* controls, float* states, int64_t B, int T,
                                 hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  if (states == nullptr) return forward_controls_only(net, x, gamma, mirror, controls, B, s);
  if (const int rc = check_tick(net, mode, T); rc != IRBFN_OK) return rc;
  if (net->opt[IRBFN_OPT_FWD_GAMMA_KERNEL] == IRBFN_FWDG_K1G) {
    // K1g: one launch where the ROLL instance exists and its tiles fit, else its forward through the controls buffer below
    if (const LaunchPlan f = plan_gram_gamma(net, B, false, -1); f.kind == LK_NONE) return f.status;
    if (net->opt[IRBFN_OPT_TICK_FUSED] != 0 && tick_narrow_compiled(net, mode, T)) {
      const LaunchPlan g = plan_gram_gamma(net, B, true, mode);
      if (g.kind != LK_NONE) {
        const int rc = launch_tick_gram_gamma(net, g, x, gamma, mirror, state0, dp, controls, states, B, T, s);
        if (rc == IRBFN_OK) record_launch(net, g);
        return rc;
      }
    }
  } else if (net->bclass != BC_GENERIC && T * rollout_state_dim(mode) <= 64) {
    const LaunchPlan p = plan_qlane(net, B, true, true);
    if (p.kind == LK_K1) {
      const int rc = launch_qlane_tick(net, p, mode, x, gamma, mirror, state0, dp, controls, states, B, T, s);
      if (rc == IRBFN_OK) record_launch(net, p);
      return rc;
    }
  }
  if (!controls) return IRBFN_ERR_BAD_ARG;
  int rc = launch_forward_gamma(net, x, gamma, controls, B, s);
  if (rc == IRBFN_OK && mirror) rc = launch_unmirror(controls, mirror, B, net->O, T, s);
  if (rc != IRBFN_OK) return rc;
  return launch_rollout_forward_split(mode, state0, controls, dp, states, B, T, s);
}

}  // namespace irbfn
