// Hidden layer of a net (irbfn_net_hidden, include/irbfn_hip.h): h[b][k] = sum_r gamma[b][r] phi(|x_b - c_rk| / sigma_rk), what
// the forward kernels multiply by W inside their loops and never store.  It is the design matrix of the closed-form output-layer
// fit (irbfn_amd/linear_fit.py, K8 in syrk_f64.hip); the reference has no counterpart.
//
// All-float32 VALU, as K1 (rbf_forward.h): a query per lane (x in VGPRs), the packed records net->rec read through the scalar
// cache (c[DC], the folded scale; the weight row behind them is skipped), direct differences, basis_arg + trans_block for the
// fast bases and basis_from_r2 for the others, gate_factor for the gate.  A block of four waves owns 64 queries and walks the
// K centres in tiles of 64; wave w takes centres 16 w .. 16 w + 15 of the tile with 16 accumulators and sums the regions in
// order, skipping a region whose gamma is 0 for all of its 64 queries (as K1 does).  The 64 x 64 tile leaves through LDS so
// that the stores run along k.  The per-dimension gate factors are tabulated once per block in LDS (as gate_kernel's); a
// region's gamma is a product of nsplit look-ups.  No workspace, no atomics: deterministic, and rows are independent.
#include "rbf_forward.h"

#include <stdio.h>

namespace irbfn {

constexpr int kHidQ = 64;             // queries per block
constexpr int kHidTile = 64;          // centres per tile
constexpr int kHidPerWave = 16;       // centres of a tile per wave
constexpr int kHidPitch = kHidTile + 1;
constexpr int kHidG = 8;              // centres whose transcendentals are issued as one block

struct HiddenArgs {
  const float* __restrict__ x;        // [B][Dreal]
  const float* __restrict__ rec;      // [R K][S]
  float* __restrict__ h;              // [B][ldh]
  GateTables gate;
  long B, ldh;
  int Dreal, R, K, S, basis;
};

template <int D, int BC>
__global__ __launch_bounds__(256) void rbf_hidden(const HiddenArgs a) {
  extern __shared__ float lds[];
  typedef const float __attribute__((address_space(4)))* crec_t;      // scalar (s_load) path, see rbf_forward_kernels.hip
  float* tile = lds;                                // [kHidQ][kHidPitch]
  float* gtab = lds + kHidQ * kHidPitch;            // [nsplit * max_ranges][kHidQ]
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long row0 = (long)blockIdx.x * kHidQ;
  const long left = a.B - row0;
  const int nvalid = left < kHidQ ? (int)left : kHidQ;
  const GateTables gt = a.gate;
  const long bq = row0 + (lane < nvalid ? lane : nvalid - 1);         // a lane past the end repeats the last row

  float xq[D];
#pragma unroll
  for (int j = 0; j < D; ++j) xq[j] = j < a.Dreal ? a.x[bq * a.Dreal + j] : 0.0f;
  const int E = gt.nsplit * gt.max_ranges;
  for (int e = wave; e < E; e += 4) {
    const int d = e / gt.max_ranges;
    gtab[e * kHidQ + lane] = gate_factor(a.x[bq * a.Dreal + d], gt.lo[e], gt.hi[e], gt.delta[d]);
  }
  __syncthreads();

  for (int k0 = 0; k0 < a.K; k0 += kHidTile) {
    const int kw = k0 + wave * kHidPerWave;                           // this wave's first centre
    int nk = a.K - kw;
    nk = nk < 0 ? 0 : (nk < kHidPerWave ? nk : kHidPerWave);
    float acc[kHidPerWave];
#pragma unroll
    for (int i = 0; i < kHidPerWave; ++i) acc[i] = 0.0f;
    for (int r = 0; r < a.R && nk > 0; ++r) {
      float g = 0.0f;                                                 // model.py:70: regions without a range stay 0
      if (r < gt.n_ranges) {
        g = 1.0f;
        for (int d = 0; d < gt.nsplit; ++d) g *= gtab[(d * gt.max_ranges + gt.dim_ranges[r * gt.nsplit + d]) * kHidQ + lane];
      }
      if (__ballot(g != 0.0f) == 0ull) continue;                      // NaN != 0: a NaN query keeps its region
      const float* rp = a.rec + ((size_t)r * a.K + kw) * a.S;
#pragma unroll
      for (int i0 = 0; i0 < kHidPerWave; i0 += kHidG) {
        if (BC != BC_GENERIC && i0 + kHidG <= nk) {
          float t[kHidG];
#pragma unroll
          for (int i = 0; i < kHidG; ++i) {
            const crec_t c = (crec_t)(uintptr_t)(rp + (size_t)(i0 + i) * a.S);
            float r2 = 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) { const float dd = xq[j] - c[j]; r2 = __builtin_fmaf(dd, dd, r2); }
            t[i] = basis_arg<BC>(r2, c[D]);
          }
          if constexpr (BC != BC_GENERIC) trans_block<BC, kHidG>(t);
#pragma unroll
          for (int i = 0; i < kHidG; ++i) acc[i0 + i] = __builtin_fmaf(g, t[i], acc[i0 + i]);
        } else {
#pragma unroll
          for (int i = 0; i < kHidG; ++i) {
            if (i0 + i < nk) {
              const crec_t c = (crec_t)(uintptr_t)(rp + (size_t)(i0 + i) * a.S);
              float r2 = 0.0f;
#pragma unroll
              for (int j = 0; j < D; ++j) { const float dd = xq[j] - c[j]; r2 = __builtin_fmaf(dd, dd, r2); }
              acc[i0 + i] = __builtin_fmaf(g, basis_from_r2<BC>(r2, c[D], a.basis), acc[i0 + i]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kHidPerWave; ++i) tile[lane * kHidPitch + wave * kHidPerWave + i] = acc[i];
    __syncthreads();
    const int tk = a.K - k0 < kHidTile ? a.K - k0 : kHidTile;
    for (int idx = tid; idx < kHidQ * kHidTile; idx += 256) {
      const int q = idx >> 6, kk = idx & (kHidTile - 1);
      if (q < nvalid && kk < tk) a.h[(row0 + q) * a.ldh + k0 + kk] = tile[q * kHidPitch + kk];
    }
    __syncthreads();
  }
}

static int launch_hidden(irbfn_net* net, const float* x, float* h, int64_t ldh, int64_t B, hipStream_t s) {
  const size_t lds = ((size_t)kHidQ * kHidPitch + (size_t)net->nsplit * net->max_ranges * kHidQ) * sizeof(float);
  if (lds > 64 * 1024) return IRBFN_ERR_UNSUPPORTED;                  // as launch_gate
  const int64_t grid = (B + kHidQ - 1) / kHidQ;
  if (grid > 0x7fffffffLL) return IRBFN_ERR_UNSUPPORTED;
  HiddenArgs a;
  a.x = x; a.rec = net->rec; a.h = h; a.gate = net->gate();
  a.B = (long)B; a.ldh = (long)ldh;
  a.Dreal = net->D; a.R = net->R; a.K = net->K; a.S = net->S; a.basis = net->basis;
  const int rc = dispatch<3, 4, 7, 8>(net->DC, [&](auto d) {
    return dispatch<BC_GAUSS, BC_IQ, BC_IMQ, BC_GENERIC>(net->bclass, [&](auto bc) {
      return launch_kernel<rbf_hidden<d(), bc()>>(dim3((unsigned)grid), dim3(256), lds, s, a);
    });
  });
  if (rc == IRBFN_OK) {
    snprintf(net->last_name, sizeof(net->last_name), "rbf_hidden<D=%d,BC=%d>", net->DC, net->bclass);
    net->last_grid = (int)grid;
    net->last_block = 256;
  }
  return rc;
}

}  // namespace irbfn

using namespace irbfn;

extern "C" {

int irbfn_net_hidden(irbfn_net* net, const float* x_dev, float* h_dev, int64_t ldh, int64_t B, void* stream) {
  if (!net || B < 0) return IRBFN_ERR_BAD_ARG;
  if (B == 0) return IRBFN_OK;
  if (!x_dev || !h_dev || ldh < net->K) return IRBFN_ERR_BAD_ARG;
  if (!net->has_params) return IRBFN_ERR_NO_PARAMS;
  return launch_hidden(net, x_dev, h_dev, ldh, B, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
