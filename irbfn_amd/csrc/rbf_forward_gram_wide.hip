// K1g for wide outputs (16 < O <= 128, d = 7 or 8): rbf_fwd_f16gram_wide -- see rbf_forward_gram_wide.h (the body) and
// rbf_forward_gram.hip (the expansion, its accuracy argument, the pack).  Same mathematics as K1 / K1h
// (src/irbfn_mpc/model.py:169-198; RBF stage flax_rbf.py:258-285).
#include "rbf_forward_gram_wide.h"

namespace irbfn {

template <int DC, int BC, int NT>
__global__ __launch_bounds__(512) void rbf_fwd_f16gram_wide(const GramArgs ga) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  wide_gram_body<DC, BC, NT, -1>(ga, F16Roll{}, lds);
}

// the rings of SW slices, three chunk images each
size_t gram_wide_ring_bytes(const irbfn_net* net, int SW) { return (size_t)SW * 3 * gram_chunk_bytes((net->O + 15) / 16); }

size_t gram_wide_lds_bytes(const irbfn_net* net, int SW, int QG, size_t extra_red_floats) {
  const size_t ring = gram_wide_ring_bytes(net, SW);
  const size_t red = ((size_t)SW * QG * 2 * 4 * 64 + (size_t)QG * 32 + extra_red_floats) * sizeof(float);
  return ring > red ? ring : red;
}

// chunks of the longest of the S slices [nchunks s / S, nchunks (s + 1) / S): the steps every wave of a narrow block walks
int gram_nsteps(int nchunks, int S) {
  int nsteps = 0;
  for (int s2 = 0; s2 < S; ++s2) {
    const int m = (int)((long)nchunks * (s2 + 1) / S) - (int)((long)nchunks * s2 / S);
    nsteps = m > nsteps ? m : nsteps;
  }
  return nsteps;
}

void gram_fill_args(const irbfn_net* net, const float* x, float* out, int64_t B, int S, int QG, GramArgs* a) {
  const int nchunks = (net->N + kF16Chunk - 1) / kF16Chunk;
  a->f.x = x; a->f.img = net->f16_img; a->f.oscale = net->f16_oscale; a->f.bias = net->bias; a->f.out = out; a->f.gate = net->gate();
  a->f.B = (long)B; a->f.Dreal = net->D; a->f.O = net->O; a->f.nchunks = nchunks; a->f.S = S; a->f.QG = QG;
  a->gimg = net->gram_img;
  a->hdr = reinterpret_cast<const GramHdr*>(net->gram_hdr);
  a->g0 = net->gate0;
  a->nsteps = gram_nsteps(nchunks, S);
}

int launch_forward_gram_wide(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s) {
  const int NT = (net->O + 15) / 16;
  GramArgs a;
  gram_fill_args(net, x, out, B, p.S, p.QG, &a);
  return dispatch<7, 8>(net->DC, [&](auto dc) {
    return dispatch<2, 3, 4, 5, 6, 7, 8>(NT, [&](auto nt) {
      return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
        return launch_kernel<rbf_fwd_f16gram_wide<dc(), bc(), nt()>>(dim3(p.grid), dim3(p.block), p.lds, s, a);
      });
    });
  });
}

}  // namespace irbfn
