// K2h (rbf_vjp_f16.hip): interface towards the VJP launcher in rbf_vjp.hip.
#pragma once
#include "common.h"

namespace irbfn {

constexpr int vjph_rfq(int DC) { return DC <= 3 ? 4 : (DC <= 7 ? 8 : 12); }   // floats per packed query row (x, gamma)

bool vjph_eligible(const irbfn_net* net);
size_t vjph_block_bytes(const irbfn_net* net);
size_t vjph_lds_bytes(const irbfn_net* net);
// run_if: null, or a device word -- the kernels return at once unless it holds run_gen, the generation number K2g's pre-pass
// stores there when a query of this call lies outside the box (K2h as the fallback behind K2g; no reset between calls)
int launch_vjp_f16(irbfn_net* net, const float* x, const float* gout, int64_t B, unsigned char* qblk, const float* bmax,
                   int nbmax, float* scales, float* part, int QSB, int Npad, hipStream_t s, const int* run_if = nullptr, int run_gen = 0);

// K2g (rbf_vjp_gram.hip): u and the centre gradients on the matrix cores as well
bool vjpg_eligible(const irbfn_net* net);
size_t vjpg_block_bytes();
int launch_vjp_gram(irbfn_net* net, const float* x, const float* gout, int64_t B, unsigned char* qblk, const float* bmax, int nbmax,
                    float* scales, int* flag, int gen, float* part, int QSB, int Npad, hipStream_t s);
// K2g's live-leaf modes (irbfn_net_vjp_frozen): 0 all leaves, 1 no centres, 2 the Dense leaves only (rbf_vjp_gram.hip: VgMode)
int vjpg_waves(int mode, int O);                  // waves per SIMD of a mode's instance
int vjpg_slab_rows(int mode, int DC, int OP);     // slab rows of a mode: [d centers] [d log_sigs] d kernel
int launch_vjp_gram_live(irbfn_net* net, int mode, const float* x, const float* gout, int64_t B, unsigned char* qblk, const float* bmax,
                         int nbmax, float* scales, int* flag, int gen, float* part, int QSB, int Npad, hipStream_t s);
// rbf_vjp_f16gram_gamma (rbf_vjp_gram.hip): K2g over the R regions padded to whole chunks, caller-provided region weights gamma[B][R];
// slabs in the padded chunk order (Npad >= 32 R cpr), gtile: workspace of 32 R floats per 32-query block
bool vjpgg_eligible(const irbfn_net* net);        // the net's shape; the images and the pack's verdict are the planner's
int vjpgg_waves();
int launch_vjp_gram_gamma(irbfn_net* net, const float* x, const float* gamma, const float* gout, int64_t B, unsigned char* qblk,
                          float* gtile, const float* bmax, int nbmax, float* scales, int* flag, int gen, float* part, int QSB, int Npad,
                          hipStream_t s);

}  // namespace irbfn
