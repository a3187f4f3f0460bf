// K5m: the x-VJP (rbf_vjpx.h) with hbar = gout W^T on the f32 matrix cores (gfx950).
//
// For wide outputs hbar is the bulk of the x-VJP (O = 100: 200 of ~240 flops per pair).  v_mfma_f32_16x16x4_f32 is an exact
// float32 fmaf chain on a pipe of its own (rbf_forward_mfma.hip).  The tile is K1m's turned round:
//
//     hbar^T[16 centres x 16 queries] += W[16 centres x 4 outputs] * gout^T[4 outputs x 16 queries]
//
// Lane l = (g = l >> 4, qs = l & 15) holds A[row = centre qs][k = g] and B[k = g][col = query qs]; which output sits in which
// k slot is free as long as A and B agree, so lane group g takes the CONTIGUOUS outputs [g OQ, (g + 1) OQ), OQ = OW / 4, and both
// operands are float4 loads.  The result leaves the lane D[row = centre 4 g + r][col = query qs], r = 0..3: one query column and
// four centre rows, so the lane's pair work (distance with the differences kept, one block of four transcendentals, D FMAs of
// s (x - c)) and its D running sums belong to ONE query, and the final reduction is over the four lane groups and the NW waves,
// in a fixed order.  The records are K1m's image (recm: centre, scale, padded weight row; centres past N have zero weight rows and
// contribute exactly 0); a wave reads its 16-centre chunks straight from L2 -- 16 B of weights per MFMA, the four centres of a
// lane group as 16-lane broadcasts -- there is no LDS ring.
//
// One region (gamma and its gradient factor out of the sums), the three fast basis classes, d = 2..8, O <= 128.
#include <string.h>

#include "rbf_vjpx.h"

namespace irbfn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct VjpxMfmaArgs {
  const float* __restrict__ x;      // [B][D]
  const float* __restrict__ g;      // [B][O]
  const float* __restrict__ recm;   // [Npad][CW + OW]
  float* __restrict__ gx;           // [B][D]
  GateTables gate;
  long B;
  int O, Npad;
};

template <int D, int NT, int BC>
__global__ __launch_bounds__(512) void rbf_vjpx_mfma(const VjpxMfmaArgs a) {
  extern __shared__ float lds[];
  constexpr int CW = mfma_cw(D);
  constexpr int OW = 16 * NT;
  constexpr int OQ = OW / 4;                     // outputs (= MFMA steps) per lane group
  constexpr int RS = CW + OW;
  constexpr int ROWS = 16;                       // queries per workgroup
  constexpr int LP = ROWS + 1;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nthreads = blockDim.x;
  const int nw = nthreads >> 6;
  const int qs = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * ROWS;
  const long left = a.B - row0;
  const int nvalid = left < ROWS ? (int)left : ROWS;
  const int O = a.O, GP = O | 1;
  const GateTables gt = a.gate;

  // ---- stage the query and cotangent tiles; the lane's query, its gate and its OQ cotangent entries go to registers
  float* xs = lds;                               // [ROWS][D]; the reduction buffer [nw * 4][D][LP] after the loop
  float* gs = xs + ROWS * D;                     // [ROWS][GP]
  {
    const float* xsrc = a.x + row0 * D;
    for (int i = tid; i < nvalid * D; i += nthreads) xs[i] = xsrc[i];
    const float* gsrc = a.g + row0 * O;
    for (int i = tid; i < nvalid * O; i += nthreads) {
      const int row = i / O;
      gs[row * GP + (i - row * O)] = gsrc[i];
    }
  }
  __syncthreads();
  const int rr = qs < nvalid ? qs : nvalid - 1;
  float xq[D], gb[OQ], dl[D];
#pragma unroll
  for (int j = 0; j < D; ++j) xq[j] = xs[rr * D + j];
#pragma unroll
  for (int s = 0; s < OQ; ++s) gb[s] = (g * OQ + s) < O ? gs[rr * GP + g * OQ + s] : 0.0f;
  float gam = gt.n_ranges > 0 ? 1.0f : 0.0f;     // model.py:70
#pragma unroll
  for (int d = 0; d < D; ++d) {
    dl[d] = 0.0f;
    if (d < gt.nsplit && gt.n_ranges > 0) {
      const int e = d * gt.max_ranges + gt.dim_ranges[d];
      float fac;
      dl[d] = gate_factor_dlog(xq[d], gt.lo[e], gt.hi[e], gt.delta[d], &fac);
      gam *= fac;
    }
  }

  // ---- hot loop: this wave's chunks of 16 centres
  const int chunks = a.Npad / 16;
  const int cpw = (chunks + nw - 1) / nw;
  const int c0 = wave * cpw < chunks ? wave * cpw : chunks;
  const int c1 = (c0 + cpw) < chunks ? (c0 + cpw) : chunks;
  float acc[D], q = 0.0f;
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = 0.0f;
  for (int c = c0; c < c1; ++c) {
    const float* base = a.recm + (size_t)c * 16 * RS;
    // A operand: W[centre qs][g OQ + s]
    float wa[OQ];
    {
      const float4* wp = reinterpret_cast<const float4*>(base + qs * RS + CW + g * OQ);
#pragma unroll
      for (int i = 0; i < OQ / 4; ++i) {
        const float4 v = wp[i];
        wa[4 * i + 0] = v.x; wa[4 * i + 1] = v.y; wa[4 * i + 2] = v.z; wa[4 * i + 3] = v.w;
      }
    }
    // two accumulators: a dependent 16x16x4 MFMA waits 40 cycles, an independent one issues after 32
    f32x4 h0 = {0.0f, 0.0f, 0.0f, 0.0f}, h1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < OQ; s += 2) {
      h0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], gb[s], h0, 0, 0, 0);
      h1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s + 1], gb[s + 1], h1, 0, 0, 0);
    }
    // the lane's four centres 4 g + i against its query (the MFMAs above run beside this on their own pipe)
    float t[4], df[4][D], sc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* rp = base + (4 * g + i) * RS;
      float cv[CW];
#pragma unroll
      for (int k = 0; k < CW / 4; ++k) {
        const float4 v = reinterpret_cast<const float4*>(rp)[k];
        cv[4 * k + 0] = v.x; cv[4 * k + 1] = v.y; cv[4 * k + 2] = v.z; cv[4 * k + 3] = v.w;
      }
      float r2 = 0.0f;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        df[i][j] = xq[j] - cv[j];
        r2 = __builtin_fmaf(df[i][j], df[i][j], r2);
      }
      sc[i] = cv[D];
      t[i] = basis_arg<BC>(r2, sc[i]);
    }
    trans_block<BC, 4>(t);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float hb = h0[i] + h1[i];            // hbar[centre 4 g + i][query qs]
      const float phi = t[i];
      q = __builtin_fmaf(hb, phi, q);
      const float s = hb * vjpx_fast_factor<BC>(phi) * sc[i];
#pragma unroll
      for (int j = 0; j < D; ++j) acc[j] = __builtin_fmaf(s, df[i][j], acc[j]);
    }
  }

  // ---- gamma, the gate term, and the fixed-order sum over lane groups and waves
  __syncthreads();                               // xs / gs are dead from here on
  float* red = xs;                               // [nw * 4][D][LP]
#pragma unroll
  for (int j = 0; j < D; ++j)
    red[((wave * 4 + g) * D + j) * LP + qs] = gam * __builtin_fmaf(vjpx_scale<BC>(), acc[j], q * dl[j]);
  __syncthreads();
  float* dst = a.gx + row0 * D;
  for (int idx = tid; idx < nvalid * D; idx += nthreads) {
    const int row = idx / D, j = idx - row * D;
    float s = 0.0f;
    for (int w = 0; w < nw * 4; ++w) s += red[(w * D + j) * LP + row];
    dst[idx] = s;
  }
}

// ------------------------------------------------------------------------------------------------
bool vjpxm_eligible(const irbfn_net* net) { return net->recm != nullptr && mfma_eligible(net); }

int vjpxm_width(const irbfn_net* net) { return 16 * ((net->O + 15) / 16); }

// IRBFN_VJPX_AUTO: K5m where it was measured ahead of K5 (profiles/vjp_x.txt, 4096 centres: O = 32 203 vs 234 us, O = 100
// 594 vs 789 us; level at O = 16, behind at O <= 10, where one 16-wide MFMA tile is mostly padding)
bool vjpxm_preferred(const irbfn_net* net, int64_t B, bool ext) {
  (void)B;
  return !ext && net->O > 16 && vjpxm_eligible(net);
}

static int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

VjpxPlan plan_vjpx_mfma(const irbfn_net* net, int64_t B) {
  VjpxPlan p;
  const long tiles = (B + 15) / 16;
  long want = (16384 + tiles - 1) / tiles;
  int nw = want < 1 ? 1 : (want > 8 ? 8 : (int)want);
  nw = pow2_floor(nw);
  const int chunks = net->Npad / 16;
  while (nw > 1 && chunks / nw < 2) nw /= 2;
  const size_t stage = (size_t)16 * net->D + (size_t)16 * (net->O | 1);
  const size_t red = (size_t)nw * 4 * net->D * 17;
  p.kind = VX_K5M; p.status = IRBFN_OK;
  p.nw = nw; p.lds = (stage > red ? stage : red) * sizeof(float); p.grid = tiles; p.block = nw * kWave;
  return p;
}

int launch_vjpx_mfma(irbfn_net* net, const VjpxPlan& p, const float* x, const float* gout, float* gx, int64_t B, hipStream_t s) {
  VjpxMfmaArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.g = gout; a.recm = net->recm; a.gx = gx; a.gate = net->gate(); a.B = (long)B;
  a.O = net->O; a.Npad = net->Npad;
  const int NT = (net->O + 15) / 16;
  const dim3 grid((unsigned)p.grid), block(p.block);
  return dispatch<2, 3, 4, 5, 6, 7, 8>(net->D, [&](auto d) {
    return dispatch<1, 2, 3, 4, 5, 6, 7, 8>(NT, [&](auto nt) {
      return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
        return launch_kernel<rbf_vjpx_mfma<d(), nt(), bc()>>(grid, block, p.lds, s, a);
      });
    });
  });
}

}  // namespace irbfn
