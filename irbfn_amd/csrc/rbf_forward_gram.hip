// K1g: the narrow forward (one region, O <= 16, fast bases) with BOTH of its GEMM-shaped pieces on the f16 matrix cores:
// the squared distances as a Gram expansion and Phi x W (the hi/lo pairs of K1h).  Same mathematics as K1 / K1h
// (src/irbfn_mpc/model.py:169-198; RBF stage flax_rbf.py:258-285).
//
// Why: K1h is VALU-issue bound, and 14 of its ~21.5 VALU instructions per (query, centre) pair are the distance
// (x_i - c_i, fma) x 7.  With u = alpha_k |x - c_k|^2 + beta (the argument of the transcendental) written as
//     u = alpha_k Q  +  sum_i (-2 alpha_k c'_ki) x'_i  +  (alpha_k |c'_k|^2 + beta),      x' = x - r, c' = c - r, Q = |x'|^2
// it is a [centres x slots] x [slots x queries] product whose D layout (v_mfma: lane = query column, registers = 4 centre
// rows) is already the A layout of the Phi x W product: no shuffle between the two.  What is left on the VALU per pair is the
// transcendental and the hi/lo split of its result.
//
// Accuracy -- the expansion cancels (terms of size M = alpha (|x'|^2 + |c'|^2) sum to u <~ 30), and the matrix core adds its
// products in a tree of truncating ~24-bit adders (tools/probe_mfma_accum.hip, profiles/r03_mfma_accumulation_probe.txt), so a
// naive expansion carries an error of 2^-24 M.  Here the cancellation is EXACT:
//  * every factor v in {x'_i, Q, C_ki = -2 alpha_k c'_ki, alpha_k, c2_k} with |v| < 2^E is cut into a FIXED-POINT head
//    n0 = rint(v 2^(10-E)) 2^-10 (11 bits: exact in f16) and two float tails n1, n2 (f16 roundings of the scaled residuals:
//    v = 2^E (n0 + 2^-11 n1 + 2^-22 n2) to 2^(E-34)); c2 has two fixed-point heads;
//  * the head x head products of one (query, centre) element are integer multiples of one grid 2^(EX+EC-20) and their partial
//    sums stay below 2^24 grid units (checked at pack time): whatever the order of the adder tree, nothing is truncated;
//  * a tile takes TWO v_mfma_f32_16x16x32_f16.  The eleven heads sit in k 0..15 of the first (C = 0), i.e. in its lane groups
//    0 and 1: the matrix core sums the eight products of a lane group aligned to the group's largest and accumulates the four
//    groups in ascending k, so the two head groups give the cancelled head sum S1 exactly and everything behind them is added
//    to S1 -- what a 16x16x16 MFMA of the heads alone did until the heads were folded in (the model:
//    profiles/r03_mfma_accumulation_probe.txt; the fold itself: tools/probe_mfma_accum.hip fold, profiles/k1g_fold_heads.txt --
//    heads at the budget's edge alone are exact, and with tails behind them the result is bit for bit that of the three-MFMA form);
//  * the 47 tail products (each < 2^-10 of a head product) follow in k 16..31 of the first MFMA and in the second: truncation
//    there is 2^-24 of max(|u|, 2^-10 M).
// So u carries the error of a float32 evaluation of the direct form (a few 2^-24 |u|), not 2^-24 M.  Exponents EX .. E2 are
// chosen per net from the centres (pack_all.hip: statistics role, header per block); a query outside the representable box (|x'_i| >= 2^EX, non-finite)
// makes its WAVE take the VALU distances of K1h for its 32 queries (same records, same f16_arg): results there are K1h's.
// A net whose exponents do not fit (ok = 0 in the header, read back once by irbfn_net_set_params) is not dispatched here.
//
// Layout: v_mfma_f32_16x16x32_f16 with rows = 16 centres, k = slots (gram_fold_slot, rbf_forward_gram.h), columns = 16 queries.  A lane owns
// query (l & 15) of its wave's two query tiles; the D registers of centre tile ct hold centres 16 ct + 4 g + r (g = l >> 4),
// which become k-slots 8 g + 4 ct + r of the Phi x W product (the W rows of the image are permuted to match).
// Chunk image (32 centres, 6 KiB): distance operands [ct][operand][lane] 16 B, W hi, W lo (1 KiB each); the QG waves of a centre
// slice share an LDS ring of five images filled by LDS-DMA, one barrier per two chunks.  Per step a wave issues 14 MFMAs: 8 for
// the distances of its 2 x 2 tiles, 6 for Phi x W.  In memory K2g's unfolded records (5 KiB: rbf_vjp_gram.hip keeps the
// 16x16x16 head MFMA) lie behind each image; the forward kernels step over them (gram_chunk_stride).
// The kernel body is gram_body (rbf_forward_gram_body.h); rbf_forward_gram_gamma.hip instantiates it for nets of several regions
// evaluated with caller-provided region weights.
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rbf_forward_gram_body.h"

namespace irbfn {

template <int DC, int BC>
__global__ __launch_bounds__(1024, IRBFN_GRAM_WAVES) void rbf_fwd_f16gram(const GramArgs ga) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  gram_body<DC, BC, false>(ga, F16Roll{}, -1, lds);
}

// the planning tick of a narrow net in one launch (forward + sign flip + roll-out; irbfn_planner.py:203-212)
template <int DC, int BC>
__global__ __launch_bounds__(1024, IRBFN_GRAM_WAVES) void rbf_tick_f16gram(const GramArgs ga, const F16Roll rl, const int mode) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  gram_body<DC, BC, true>(ga, rl, mode, lds);
}

// ---- host side -------------------------------------------------------------------------------------------
static int gram_nt(const irbfn_net* net) { return (net->O + 15) / 16; }

bool gram_eligible(const irbfn_net* net) {
  return f16_eligible(net) && net->DC <= kGramDims;
}

size_t gram_image_bytes(const irbfn_net* net) {
  const int nchunks = (net->N + kF16Chunk - 1) / kF16Chunk;
  return (size_t)nchunks * gram_chunk_stride(gram_nt(net));
}

size_t gram_header_bytes() { return sizeof(GramHdr); }

#ifdef IRBFN_GRAM_STAMPS
extern "C" int irbfn_debug_gram_stamps(unsigned long long* out64) {
  return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_gram_stamps), sizeof(unsigned long long) * 64);
}
#endif

// S centre slices x QG query groups of 32 per block (tick: the one-launch tick's control and state tiles on top)
size_t gram_lds_bytes(int S, int QG, bool tick, bool gamma) {
  size_t ring = (size_t)S * kGramRing * kGramChunkBytes;
  if (gamma) ring += (size_t)S * QG * 128 * sizeof(float);   // a double-buffered tile of region weights per wave
  else ring += (size_t)QG * 32 * sizeof(float);              // the gate values of the block's queries, parked across the steps
  size_t red = (size_t)S * QG * 2 * 4 * 64 + (size_t)QG * 32;
  if (tick) red += (size_t)QG * 32 * (kTickNarrowCP + kTickNarrowSP);
  red *= sizeof(float);
  return ring > red ? ring : red;
}

int launch_forward_gram(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s) {
  if (p.kind == LK_K1G_WIDE) return launch_forward_gram_wide(net, p, x, out, B, s);
  GramArgs a;
  gram_fill_args(net, x, out, B, p.S, p.QG, &a);
  return dispatch<3, 4, 7, 8>(net->DC, [&](auto dc) {
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
      return launch_kernel<rbf_fwd_f16gram<dc(), bc()>>(dim3(p.grid), dim3(p.block), p.lds, s, a);
    });
  });
}

// The one-launch planning tick of a narrow net on K1g (rbf_tick_f16gram)
int launch_tick_gram_narrow(irbfn_net* net, const LaunchPlan& p, const float* x, const int* mirror, const float* state0,
                            const DynParams& dp, float* controls, float* states, int64_t B, int T, hipStream_t s) {
  GramArgs a;
  gram_fill_args(net, x, controls, B, p.S, p.QG, &a);
  F16Roll rl;
  rl.state0 = state0; rl.states = states; rl.mirror = mirror; rl.T = T; rl.wlds = 0; rl.dp = dp;
  return dispatch<7, 8>(net->DC, [&](auto dc) {
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
      return launch_kernel<rbf_tick_f16gram<dc(), bc()>>(dim3(p.grid), dim3(p.block), p.lds, s, a, rl, p.mode);
    });
  });
}

}  // namespace irbfn
