// K2m: parameter VJP of a one-region WCRBFNet with the O-wide contractions on the f32 matrix cores (gfx950).
//
// The VJP analogue of K1m (rbf_forward_mfma.hip).  K2 (rbf_vjp.hip) keeps one centre per lane and runs the two O-wide
// sums of every (query, centre) pair on the VALU -- hbar = g . W[k,:] and dW[k,:] += gamma phi g -- 2 O FMAs per pair
// beside ~30 VALU instructions of distance, basis and centre sums.  K2m moves both sums onto v_mfma_f32_16x16x4_f32
// (full f32 operands, an fmaf chain per element) and keeps the rest on the VALU, which issues beside the matrix core.
//
// A wave owns CT tiles of 16 centres and walks 16-query tiles of its query slice.  Lane l = (i = l & 15, j = l >> 4):
//
//   hbar[q,k] = sum_o g[q,o] W[k,o]        D[16 q x 16 k] += A[q = i][o] B[o][k = i]         KS = OW/4 MFMAs per tile
//                                            lane group j holds the outputs o = j*KS + s of k-step s
//   distances, phi, dphi/dd2 on the VALU in the MFMA output layout: lane (i, j) holds centre i and queries 4j + r
//   dW[k,o]  += sum_q gamma phi[q,k] g[q,o]  D[16 k x 16 o] += A[k = i][q = 4j + r] B[q][o = i*NT + u]
//                                            the hbar result registers are the A operand as they are (k-step r takes the
//                                            queries 4j + r), 4 NT MFMAs per tile
//   centre / log-sigma sums: per lane over its queries, then a fixed xor tree across the four lane groups.
//
// The queries come from a pre-pass that writes one record per query, { g[0..OW) (zero padded), x[0..DC), gamma, 0.. },
// B rounded up to 16 zero records: every operand is an aligned vector load without bounds tests.  The four waves of a
// workgroup take different query slices of the same centres and are combined through LDS in a fixed order into K2's
// [slab][value][centre] layout, which vjp_reduce_kernel finishes: no atomics, a repeat call gives the same bits.
// Eligible: one region, the fast basis classes, padded d in {3, 4, 7, 8}, 16 < O <= 128 (padded to OW = 32, 64, 128).
#include "rbf_forward.h"

namespace irbfn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int vjpm_xw(int DC) { return (DC + 1 + 3) & ~3; }   // x[DC], gamma, padding

static int vjpm_ow(int O) { return O <= 32 ? 32 : (O <= 64 ? 64 : 128); }
static constexpr int vjpm_ct(int OW) { return OW <= 64 ? 2 : 1; }          // centre tiles per wave: the W and dW registers bound it

bool vjpm_eligible(const irbfn_net* net) {
  const bool d_ok = net->DC == 3 || net->DC == 4 || net->DC == 7 || net->DC == 8;
  return net->R == 1 && net->bclass != BC_GENERIC && d_ok && net->O > 16 && net->O <= 128;
}

size_t vjpm_qrec_bytes(const irbfn_net* net, int64_t B) {
  const int64_t bp = (B + 15) / 16 * 16;
  return (size_t)bp * (vjpm_ow(net->O) + vjpm_xw(net->DC)) * sizeof(float);
}

int vjpm_groups(const irbfn_net* net) {
  const int cw = 16 * vjpm_ct(vjpm_ow(net->O));
  return (net->N + cw - 1) / cw;
}

// query slabs: about 512 workgroups (two waves per SIMD), at least four 16-query tiles per wave, at most `max_qsb` (allocated)
int vjpm_slices(const irbfn_net* net, int64_t B, int max_qsb) {
  const long g = vjpm_groups(net);
  const long nt = (B + 15) / 16;
  long q = (512 + g - 1) / g;
  const long qmax = (nt + 15) / 16;
  if (q > qmax) q = qmax;
  if (q > max_qsb) q = max_qsb;
  if (q < 1) q = 1;
  return (int)q;
}

void vjpm_names(const irbfn_net* net, int* OW, int* CT) {
  *OW = vjpm_ow(net->O);
  *CT = vjpm_ct(*OW);
}

// records { g (OW), x (DC), gamma, 0 } of 64 queries per block; rows B .. Bpad16 are zero
__global__ __launch_bounds__(256) void vjpm_pack_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        float* __restrict__ qm, GateTables gt, long B, long Bp, int D, int DC,
                                                        int O, int OW, int QM) {
  __shared__ float gam[kWave];
  const int tid = threadIdx.x;
  const long b0 = (long)blockIdx.x * kWave;
  if (tid < kWave) {
    const long b = b0 + tid;
    float gm = 0.0f;
    if (b < B && gt.n_ranges > 0) {                // region 0 of the gate (model.py:70, 83-93), the product order of K2's pack
      gm = 1.0f;
      for (int d = 0; d < gt.nsplit; ++d) {
        const int e = d * gt.max_ranges + gt.dim_ranges[d];
        gm *= gate_factor(x[b * D + d], gt.lo[e], gt.hi[e], gt.delta[d]);
      }
    }
    gam[tid] = gm;
  }
  __syncthreads();
  const long left = Bp - b0;
  const int nv = left < kWave ? (int)left : kWave;
  float* dst = qm + b0 * QM;
  for (int idx = tid; idx < nv * QM; idx += 256) {
    const int q = idx / QM, c = idx - q * QM;
    const long b = b0 + q;
    float v = 0.0f;
    if (b < B) {
      if (c < OW) v = c < O ? g[b * O + c] : 0.0f;
      else if (c - OW < D) v = x[b * D + (c - OW)];
      else if (c - OW == DC) v = gam[q];
    }
    dst[idx] = v;
  }
}

struct VjpmArgs {
  const float* __restrict__ qm;     // [Bpad16][QM]
  const float* __restrict__ rec;    // [N][S] packed centre records { c[DC], scale, W[OP] }
  const float* __restrict__ sig2;   // [N]
  float* __restrict__ part;         // [QSB][V][Npad]
  long ntiles;                      // Bpad16 / 16
  int O, N, S, V, Npad, tiles_per_wave, basis;
  float gscale;
};

template <int D, int OW, int BC, int CT>
__global__ __launch_bounds__(256) void rbf_vjp_mfma(const VjpmArgs a) {
  extern __shared__ float red[];                 // [4][V][LP]
  constexpr int QM = OW + vjpm_xw(D);
  constexpr int KS = OW / 4;                     // hbar k-steps
  constexpr int NT = OW / 16;                    // dW output tiles
  constexpr int CW = 16 * CT;
  constexpr int LP = CW + 1;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), i = lane & 15, j = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nbase = blockIdx.x * CW;

  // this lane's centres (one per tile: centre nbase + 16 c + i) and the W operand of hbar
  float cc[CT][D], scv[CT], s2v[CT], wB[CT][KS];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    int n = nbase + 16 * c + i;
    n = n < a.N ? n : a.N - 1;
    const float* rp = a.rec + (size_t)n * a.S;
#pragma unroll
    for (int d = 0; d < D; ++d) cc[c][d] = rp[d];
    scv[c] = rp[D];
    s2v[c] = a.sig2[n];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int o = j * KS + s;
      wB[c][s] = o < a.O ? rp[D + 1 + o] : 0.0f;
    }
  }
  f32x4 accW[CT][NT];
  float gc[CT][D], gls[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    gls[c] = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) gc[c][d] = 0.0f;
#pragma unroll
    for (int u = 0; u < NT; ++u) accW[c][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  const long t0 = (long)(blockIdx.y * 4 + wave) * a.tiles_per_wave;
  long t1 = t0 + a.tiles_per_wave;
  t1 = t1 < a.ntiles ? t1 : a.ntiles;
  for (long t = t0; t < t1; ++t) {
    const float* qt = a.qm + t * 16 * QM;
    // hbar: A = g[query i][o = j KS + s]
    float gA[KS];
    {
      const float4* src = reinterpret_cast<const float4*>(qt + i * QM + j * KS);
#pragma unroll
      for (int s = 0; s < KS / 4; ++s) {
        const float4 v = src[s];
        gA[4 * s] = v.x; gA[4 * s + 1] = v.y; gA[4 * s + 2] = v.z; gA[4 * s + 3] = v.w;
      }
    }
    f32x4 hb[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      hb[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int s = 0; s < KS; ++s) hb[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(gA[s], wB[c][s], hb[c], 0, 0, 0);
    }
    // the pairs (query 4j + r, centre 16 c + i) on the VALU
    float gphi[CT][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* qr = qt + (4 * j + r) * QM + OW;
      float xr[vjpm_xw(D)];
#pragma unroll
      for (int s = 0; s < vjpm_xw(D) / 4; ++s) {
        const float4 v = reinterpret_cast<const float4*>(qr)[s];
        xr[4 * s] = v.x; xr[4 * s + 1] = v.y; xr[4 * s + 2] = v.z; xr[4 * s + 3] = v.w;
      }
      const float gam = xr[D];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        float diff[D];
        float r2 = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          diff[d] = xr[d] - cc[c][d];
          r2 = __builtin_fmaf(diff[d], diff[d], r2);
        }
        const float phi = basis_from_r2<BC>(r2, scv[c], a.basis);
        // K2's factoring: the centre's -2 / sigma^2 multiplies the finished sums
        const float tt = hb[c][r] * gam * basis_slope_fast<BC>(phi, a.gscale);
        gls[c] = __builtin_fmaf(tt, r2, gls[c]);
#pragma unroll
        for (int d = 0; d < D; ++d) gc[c][d] = __builtin_fmaf(tt, diff[d], gc[c][d]);
        gphi[c][r] = gam * phi;
      }
    }
    // dW: A = gamma phi (k-step r: queries 4j + r), B = g[query 4j + r][o = i NT + u]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float gB[NT];
      const float* qr = qt + (4 * j + r) * QM + i * NT;
      if constexpr (NT == 2) {
        const float2 v = *reinterpret_cast<const float2*>(qr);
        gB[0] = v.x; gB[1] = v.y;
      } else {
#pragma unroll
        for (int s = 0; s < NT / 4; ++s) {
          const float4 v = reinterpret_cast<const float4*>(qr)[s];
          gB[4 * s] = v.x; gB[4 * s + 1] = v.y; gB[4 * s + 2] = v.z; gB[4 * s + 3] = v.w;
        }
      }
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int u = 0; u < NT; ++u) accW[c][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(gphi[c][r], gB[u], accW[c][u], 0, 0, 0);
    }
  }

  // centre sums across the four lane groups (fixed tree), the factor -2 sigma^-2, then this wave's row of the LDS tile
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const float m2s = -2.0f * s2v[c];
    float v = gls[c];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (j == 0) red[(wave * a.V + D) * LP + 16 * c + i] = v * m2s;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      float w = gc[c][d];
      w += __shfl_xor(w, 16);
      w += __shfl_xor(w, 32);
      if (j == 0) red[(wave * a.V + d) * LP + 16 * c + i] = w * m2s;
    }
    // dW: lane (i, j) holds centres 16 c + 4 j + e, outputs i NT + u
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int o = i * NT + u;
      if (o < a.O)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[(wave * a.V + D + 1 + o) * LP + 16 * c + 4 * j + e] = accW[c][u][e];
    }
  }
  __syncthreads();
  const int rows = D + 1 + a.O;
  float* dst = a.part + (size_t)blockIdx.y * a.V * a.Npad + nbase;
  for (int idx = tid; idx < rows * CW; idx += 256) {
    const int v = idx / CW, l = idx - v * CW;
    const float s = (red[(0 * a.V + v) * LP + l] + red[(1 * a.V + v) * LP + l]) +
                    (red[(2 * a.V + v) * LP + l] + red[(3 * a.V + v) * LP + l]);
    dst[(size_t)v * a.Npad + l] = s;
  }
}

// qm: vjpm_qrec_bytes(net, B) of workspace; part: QSB slabs of V = DC + 1 + OP rows x Npad centres
int launch_vjp_mfma(irbfn_net* net, const float* x, const float* gout, int64_t B, float* qm, float* part, int QSB, int Npad,
                    hipStream_t s) {
  if (!vjpm_eligible(net) || B <= 0) return IRBFN_ERR_UNSUPPORTED;
  const int OW = vjpm_ow(net->O), CT = vjpm_ct(OW), DC = net->DC;
  const int QM = OW + vjpm_xw(DC);
  const long Bp = (B + 15) / 16 * 16;
  hipLaunchKernelGGL(vjpm_pack_kernel, dim3((unsigned)((Bp + kWave - 1) / kWave)), dim3(256), 0, s, x, gout, qm, net->gate(),
                     (long)B, Bp, net->D, DC, net->O, OW, QM);
  IRBFN_HIP_CHECK(hipGetLastError());
  VjpmArgs a;
  a.qm = qm; a.rec = net->rec; a.sig2 = net->sig2; a.part = part;
  a.ntiles = Bp / 16;
  a.O = net->O; a.N = net->N; a.S = net->S; a.V = DC + 1 + net->OP; a.Npad = Npad; a.basis = net->basis;
  a.tiles_per_wave = (int)((a.ntiles + (long)QSB * 4 - 1) / ((long)QSB * 4));
  a.gscale = gauss_scale(net->basis);
  const dim3 grid((unsigned)vjpm_groups(net), (unsigned)QSB);
  const size_t lds = (size_t)4 * a.V * (16 * CT + 1) * sizeof(float);     // <= 38.5 KB
  return dispatch<3, 4, 7, 8>(DC, [&](auto dc) {
    return dispatch<32, 64, 128>(OW, [&](auto ow) {
      return dispatch<BC_GAUSS, BC_IQ, BC_IMQ>(net->bclass, [&](auto bc) {
        return launch_kernel<rbf_vjp_mfma<dc(), ow(), bc(), vjpm_ct(ow())>>(grid, dim3(256), lds, s, a);
      });
    });
  });
}

}  // namespace irbfn
