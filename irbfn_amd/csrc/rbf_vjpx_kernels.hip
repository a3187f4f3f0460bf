// K5 instantiations for ONE compiled input width D = IRBFN_INST_D (one object per D, as K1).  Design notes: rbf_vjpx.h.
#include "rbf_vjpx.h"

#ifndef IRBFN_INST_D
#error "compile with -DIRBFN_INST_D=<3|4|7|8>"
#endif

namespace irbfn {

typedef const float __attribute__((address_space(4)))* vx_crec_t;   // scalar (s_load) path of the records, see K1's group_body

// hbar[b,k] = sum_o gout[b,o] W[k,o] against the record's weight row (SGPRs), as two partial sums over output pairs: the form
// hipcc turns into v_pk_fma_f32 with an SGPR-pair operand, which the forward's weight FMAs were measured faster in than as
// single FMAs with an SGPR operand (build.py).  The pairs start at an even record index (an aligned SGPR pair).
typedef float vx_f2 __attribute__((ext_vector_type(2)));
template <int D, int OP>
__device__ __forceinline__ float vjpx_hbar(const vx_crec_t r, const float (&gq)[OP]) {
  constexpr int O0 = (D + 1) & 1;                // one single FMA in front when the weight row starts at an odd index
  float hb = 0.0f;
  if constexpr (O0 == 1) hb = gq[0] * r[D + 1];
  vx_f2 h2 = {0.0f, 0.0f};
#pragma unroll
  for (int o = O0; o + 1 < OP; o += 2)
    h2 = __builtin_elementwise_fma(vx_f2{gq[o], gq[o + 1]}, vx_f2{r[D + 1 + o], r[D + 2 + o]}, h2);
  if constexpr (((OP - O0) & 1) == 1) hb = __builtin_fmaf(gq[OP - 1], r[D + OP], hb);
  return hb + (h2.x + h2.y);
}

// one (query, centre) pair, any basis class.  `rp` is wave-uniform.
template <int D, int OP, int BC>
__device__ __forceinline__ void vjpx_pair(const float* __restrict__ rp_, const float (&xq)[D], const float (&gq)[OP], float gam,
                                          float (&acc)[D], float& q, int basis) {
  const vx_crec_t rp = (vx_crec_t)(uintptr_t)rp_;
  float df[D], r2 = 0.0f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    df[j] = xq[j] - rp[j];
    r2 = __builtin_fmaf(df[j], df[j], r2);
  }
  const float sc = rp[D];
  const float hb = vjpx_hbar<D, OP>(rp, gq);
  float phi, fac;
  if constexpr (BC == BC_GENERIC) {
    phi = basis_value_slope_finite(r2 * sc, basis, fac);
  } else {
    phi = basis_from_r2<BC>(r2, sc, basis);
    fac = vjpx_fast_factor<BC>(phi);
  }
  q = __builtin_fmaf(hb, phi, q);
  const float s = (hb * gam) * fac * sc;
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = __builtin_fmaf(s, df[j], acc[j]);
}

// G centres at once, fast classes: G distances (differences kept), the G transcendentals as one block (rbf_forward.h), then
// hbar and the D sums of each
template <int D, int OP, int BC, int G>
__device__ __forceinline__ void vjpx_group(const float* __restrict__ rp, int S, const float (&xq)[D], const float (&gq)[OP], float gam,
                                           float (&acc)[D], float& q) {
  float t[G], df[G][D];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const vx_crec_t r = (vx_crec_t)(uintptr_t)(rp + k * S);
    float r2 = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      df[k][j] = xq[j] - r[j];
      r2 = __builtin_fmaf(df[k][j], df[k][j], r2);
    }
    t[k] = basis_arg<BC>(r2, r[D]);
  }
  trans_block<BC, G>(t);
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const vx_crec_t r = (vx_crec_t)(uintptr_t)(rp + k * S);
    const float hb = vjpx_hbar<D, OP>(r, gq);
    const float phi = t[k];
    q = __builtin_fmaf(hb, phi, q);
    const float s = (hb * gam) * vjpx_fast_factor<BC>(phi) * r[D];
#pragma unroll
    for (int j = 0; j < D; ++j) acc[j] = __builtin_fmaf(s, df[k][j], acc[j]);
  }
}

template <int D, int OP, int BC>
__global__ __launch_bounds__((OP > 48) ? 512 : 1024) void rbf_vjpx_qlane(const VjpxArgs a) {
  extern __shared__ float lds[];
  constexpr int S = (D + 1 + OP + 3) & ~3;       // floats per record (RecLayout of K1)
  constexpr int LP = kWave + 1;                  // padded lane pitch of the reduction buffer
  constexpr int G = 4;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nthreads = blockDim.x;
  const int nw = nthreads >> 6;
  const long row0 = (long)blockIdx.x * kWave;
  const long left = a.B - row0;
  const int nvalid = left < kWave ? (int)left : kWave;
  const int Dr = a.Dreal, O = a.O;
  const int GP = O | 1;                          // odd row pitch of the staged cotangent tile
  const GateTables gt = a.gate;
  const bool ext = a.gamma_ext != nullptr;
  const int E = ext ? 0 : gt.nsplit * gt.max_ranges;

  float* gtab = lds;                             // [E][64] gate factors           (tanh gate)
  float* dtab = gtab + E * kWave;                // [E][64] d log(factor) / d x
  float* xs = dtab + E * kWave;                  // [64][Dr] query tile; the reduction buffer [nw][D][LP] once the loop is done
  float* gs = xs + kWave * Dr;                   // [64][GP] cotangent tile

  // ---- stage the query and cotangent tiles (contiguous in HBM -> coalesced) and pull the lane's rows into registers
  {
    const float* xsrc = a.x + row0 * Dr;
    for (int i = tid; i < nvalid * Dr; i += nthreads) xs[i] = xsrc[i];
    const float* gsrc = a.g + row0 * O;
    for (int i = tid; i < nvalid * O; i += nthreads) {
      const int row = i / O;
      gs[row * GP + (i - row * O)] = gsrc[i];
    }
  }
  __syncthreads();
  const int rr = lane < nvalid ? lane : nvalid - 1;
  float xq[D], gq[OP];
#pragma unroll
  for (int j = 0; j < D; ++j) xq[j] = j < Dr ? xs[rr * Dr + j] : 0.0f;
#pragma unroll
  for (int o = 0; o < OP; ++o) gq[o] = o < O ? gs[rr * GP + o] : 0.0f;

  // ---- smooth region gate and its logarithmic derivative per (split dimension, range) (model.py:74-85)
  for (int idx = tid; idx < E * kWave; idx += nthreads) {
    const int e = idx >> 6, row = idx & (kWave - 1);
    const int d = e / gt.max_ranges;
    const int r2 = row < nvalid ? row : nvalid - 1;
    float fac;
    dtab[idx] = gate_factor_dlog(xs[r2 * Dr + d], gt.lo[e], gt.hi[e], gt.delta[d], &fac);
    gtab[idx] = fac;
  }
  if (E > 0) __syncthreads();

  // ---- hot loop: this wave's slice of the centre records, region by region
  float acc[D], gacc[D];                         // RBF term (in units of vjpx_scale) and gate term
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = gacc[j] = 0.0f;
  int n0, n1;
  if (a.region_split) {
    const int per = (a.R + nw - 1) / nw;
    const long s0 = (long)wave * per * a.K, s1 = s0 + (long)per * a.K;
    n0 = s0 < a.N ? (int)s0 : a.N;
    n1 = s1 < a.N ? (int)s1 : a.N;
  } else {
    const int per = (a.N + nw - 1) / nw;
    n0 = wave * per < a.N ? wave * per : a.N;
    n1 = (n0 + per) < a.N ? (n0 + per) : a.N;
  }
  int n = n0;
  while (n < n1) {
    const int r = n / a.K;
    const int nend = ((r + 1) * a.K) < n1 ? ((r + 1) * a.K) : n1;
    float gam = 0.0f;
    if (ext) {
      gam = a.gamma_ext[(row0 + rr) * a.R + r];
    } else if (r < gt.n_ranges) {                // model.py:70: regions without a range stay 0
      gam = 1.0f;
      for (int d = 0; d < gt.nsplit; ++d)
        gam *= gtab[(d * gt.max_ranges + gt.dim_ranges[r * gt.nsplit + d]) * kWave + lane];
    }
    // no query of this wave is inside region r (as K1); dgamma = q is wanted whatever gamma is
    if (a.dgamma == nullptr && __ballot(gam != 0.0f) == 0ull) {
      n = nend;
      continue;
    }
    float q = 0.0f;
    if constexpr (BC != BC_GENERIC) {
      for (; n + G <= nend; n += G) vjpx_group<D, OP, BC, G>(a.rec + (size_t)n * S, S, xq, gq, gam, acc, q);
    }
    for (; n < nend; ++n) vjpx_pair<D, OP, BC>(a.rec + (size_t)n * S, xq, gq, gam, acc, q, a.basis);
    if (ext) {
      if (a.dgamma != nullptr && lane < nvalid) a.dgamma[(row0 + lane) * a.R + r] = q;
    } else {
      const float gq_r = gam * q;                // gamma_r q_r dlog_rd: 0 wherever gamma is 0 (dlog is bounded)
#pragma unroll
      for (int d = 0; d < D; ++d)
        if (d < gt.nsplit)
          gacc[d] = __builtin_fmaf(gq_r, dtab[(d * gt.max_ranges + gt.dim_ranges[r * gt.nsplit + d]) * kWave + lane], gacc[d]);
    }
  }

  // ---- combine the NW partial sums in a fixed order (deterministic) and store the tile
  __syncthreads();                               // xs / gs are dead from here on
  float* red = xs;                               // [nw][D][LP]
#pragma unroll
  for (int j = 0; j < D; ++j) red[(wave * D + j) * LP + lane] = __builtin_fmaf(vjpx_scale<BC>(), acc[j], gacc[j]);
  __syncthreads();
  float* dst = a.gx + row0 * Dr;
  for (int idx = tid; idx < nvalid * Dr; idx += nthreads) {
    const int row = idx / Dr, j = idx - row * Dr;
    float s = 0.0f;
    for (int w = 0; w < nw; ++w) s += red[(w * D + j) * LP + row];
    dst[idx] = s;
  }
}

#define IRBFN_CAT2(a, b) a##b
#define IRBFN_CAT(a, b) IRBFN_CAT2(a, b)

int IRBFN_CAT(launch_vjpx_d, IRBFN_INST_D)(const VjpxArgs& a, int OP, int bc, int nw, size_t lds, hipStream_t s) {
  constexpr int D = IRBFN_INST_D;
  const long tiles = (a.B + kWave - 1) / kWave;
  // the forward's compiled widths (padded_O)
  return dispatch<2, 4, 5, 8, 10, 16, 32, 64, 100, 128>(OP, [&](auto op) {
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ, BC_GENERIC>(bc, [&](auto bcv) {
      return launch_kernel<rbf_vjpx_qlane<D, op(), bcv()>>(dim3((unsigned)tiles), dim3(nw * kWave), lds, s, a);
    });
  });
}

}  // namespace irbfn
