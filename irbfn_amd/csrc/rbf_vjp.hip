// K2: parameter VJP of the WCRBFNet forward (hand-derived).
//
// Replaces jax.value_and_grad(loss_fn)(state.params) restricted to the network
// (scripts/train_nmpc.py:297-298, scripts/train_nmpc_frenet.py:388-389,416-417): given the
// cotangent g[B,O] of `out`, produce d/d{centers, log_sigs, kernel, bias}.
//
//   hbar[b,k]  = sum_o g[b,o] W[k,o]                      G[b,r,k] = hbar[b,k] * gamma[b,r]
//   d centers[r,k,:] = sum_b G * phi'(d2) * sig^-2 * (-2)(x_b - c_rk)
//   d log_sigs[r,k]  = sum_b G * phi'(d2) * (-2 d2)
//   d kernel[k,o]    = sum_b sum_r gamma[b,r] phi[b,r,k] g[b,o]         d bias[o] = sum_b g[b,o]
//
// Mapping ("centre-stationary"): one LANE owns one centre n = r*K + k: c, sigma^-2, W[k,:] and the
// D+1+O gradient accumulators stay in VGPRs; the queries (x_b, g_b, gamma_b) are wave-uniform and
// stream through the scalar cache into SGPRs.  A workgroup = 4 waves on the same 64 centres and
// different query sub-slices; grid = centre groups x query slices.  Partial sums are combined
// without atomics: LDS across the 4 waves, a [slice][value][centre] slab in the workspace, then a
// fixed-order reduce kernel -> bitwise reproducible gradients.
#include "rbf_forward.h"
#include "rbf_vjp_f16.h"

#include <climits>


namespace irbfn {

struct VjpArgs {
  const float* __restrict__ qrec;   // [B][QS] packed query records { x[0..D), gamma (R == 1), g[0..OP) }
  const float* __restrict__ gamma;  // [B][R]  (R > 1: per-lane region weight)
  const float* __restrict__ rec;    // [N][S]
  const float* __restrict__ sig2;   // [N]
  float* __restrict__ part;         // [QSB][V][Npad]
  long B;
  int Dreal, O, N, K, R, S, basis, Npad, per_wave;
  float gscale;
  const int* __restrict__ flag;     // GATED behind rbf_vjp_f16gram_gamma: run only if *flag == gen (null: always)
  int gen;
};

// Pre-pass: one packed, zero-padded record per query so that the hot loop reads ONE contiguous scalar
// stream (s_load_dwordx16 + x4) without per-element bounds branches:
//   qrec[b] = { x[b, 0..D) (padded to DC), gamma[b] (R == 1; model.py:42-95), g[b, 0..O) (padded to OP) }.
// For R > 1 the full gamma[B][R] matrix is written as well (per-lane region weights).
__global__ __launch_bounds__(256) void vjp_pack_queries_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                               float* __restrict__ qrec, float* __restrict__ gamma,
                                                               GateTables gt, long B, int D, int DC, int O, int OP,
                                                               int QS, int R) {
  // 64 queries per block, 256 threads; every global store runs over consecutive addresses (the first version gave a lane
  // one query: its R region weights went out as R dwords at a stride of R -- 87 us of the 128-region net's VJP at B = 80000)
  extern __shared__ float gtab[];                 // [E][64] gate factors, then [n_ranges][nsplit] table rows (as E * 64 offsets)
  const int tid = threadIdx.x;
  const long b0 = (long)blockIdx.x * kWave;
  const long left = B - b0;
  const int nv = left < kWave ? (int)left : kWave;
  const int E = gt.nsplit * gt.max_ranges;
  int* rows = reinterpret_cast<int*>(gtab + E * kWave);
  for (int idx = tid; idx < gt.n_ranges * gt.nsplit; idx += 256) {
    const int d = idx % gt.nsplit;
    rows[idx] = (d * gt.max_ranges + gt.dim_ranges[idx]) * kWave;
  }
  for (int idx = tid; idx < E * kWave; idx += 256) {
    const int e = idx >> 6, q = idx & (kWave - 1);
    const int d = e / gt.max_ranges;
    const long bb = b0 + (q < nv ? q : nv - 1);
    gtab[idx] = gate_factor(x[bb * D + d], gt.lo[e], gt.hi[e], gt.delta[d]);
  }
  __syncthreads();
  auto region_weight = [&](int q, int r) {        // model.py:70, 88-93
    if (r >= gt.n_ranges) return 0.0f;
    float gm = 1.0f;
    for (int d = 0; d < gt.nsplit; ++d) gm *= gtab[rows[r * gt.nsplit + d] + q];
    return gm;
  };
  // packed records: { x (padded to DC), gamma of region 0, g (padded to OP), zeros up to QS }
  float* qb = qrec + b0 * QS;
  for (int idx = tid; idx < nv * QS; idx += 256) {
    const int q = idx / QS, j = idx - q * QS;
    float v = 0.0f;
    if (j < D) v = x[(b0 + q) * D + j];
    else if (j == DC) v = region_weight(q, 0);
    else if (j > DC && j - DC - 1 < O) v = g[(b0 + q) * O + (j - DC - 1)];
    qb[idx] = v;
  }
  if (R > 1) {                                    // the full gamma[B][R] matrix (per-lane region weights of K2)
    float* gb = gamma + b0 * R;
    for (int idx = tid; idx < nv * R; idx += 256) {
      const int q = idx / R, r = idx - q * R;
      gb[idx] = region_weight(q, r);
    }
  }
}

template <int D, int OP, int BC, bool GATED>
__global__ __launch_bounds__(256) void rbf_vjp_kernel(const VjpArgs a) {
  extern __shared__ float lds[];
  constexpr int V = D + 1 + OP;
  constexpr int LP = kWave + 1;
  if constexpr (GATED)
    if (a.flag != nullptr && *a.flag != a.gen) return;       // the matrix-core kernel in front of this launch did the work
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x * kWave + lane;
  const int nn = n < a.N ? n : a.N - 1;

  // this lane's centre
  const float* rp = a.rec + (size_t)nn * a.S;
  float c[D], w[OP];
#pragma unroll
  for (int j = 0; j < D; ++j) c[j] = rp[j];
  const float sc = rp[D];
  const float s2 = a.sig2[nn];
#pragma unroll
  for (int o = 0; o < OP; ++o) w[o] = rp[D + 1 + o];
  const int r = nn / a.K;

  float gc[D], gw[OP], gls = 0.0f;
#pragma unroll
  for (int j = 0; j < D; ++j) gc[j] = 0.0f;
#pragma unroll
  for (int o = 0; o < OP; ++o) gw[o] = 0.0f;

  // this wave's query slice: records stream through the scalar cache (wave-uniform addresses)
  constexpr int QS = (D + 1 + OP + 3) & ~3;
  const long slice = (long)blockIdx.y * 4 + wave;
  const long b0 = slice * a.per_wave;
  long b1l = b0 + a.per_wave;
  b1l = b1l < a.B ? b1l : a.B;
  const int nq = b1l > b0 ? (int)(b1l - b0) : 0;
  const float* qp = a.qrec + b0 * QS;
  const float* gmp = a.gamma + b0 * a.R + r;     // GATED only
#pragma unroll 2
  for (int i = 0; i < nq; ++i, qp += QS) {
    float diff[D];
    float r2 = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      diff[j] = qp[j] - c[j];
      r2 = __builtin_fmaf(diff[j], diff[j], r2);
    }
    const float d2 = r2 * s2;
    float phi;
    if constexpr (BC == BC_GAUSS) phi = fast_exp2(r2 * sc);
    else phi = basis_from_r2<BC>(r2, sc, a.basis);
    float gam;
    if constexpr (GATED) gam = gmp[(long)i * a.R];
    else gam = qp[D];
    const float gphi = gam * phi;
    // hbar as two interleaved partial sums: hipcc's SLP turns the pair into v_pk_fma_f32 with an SGPR-pair
    // operand (4.7 cycles per two FMAs; a v_fmac with one SGPR and two VGPR reads costs 4.2 for one).
    // Measured and rejected: 4 queries per step with one block of 4 transcendentals (as in the forward
    // kernel): 90 VGPRs, 411 vs 404 us -- this kernel is bound by its ~38 VALU instructions per pair.
    float hb0 = 0.0f, hb1 = 0.0f;
#pragma unroll
    for (int o = 0; o + 1 < OP; o += 2) {
      const float g0 = qp[D + 1 + o], g1 = qp[D + 2 + o];
      hb0 = __builtin_fmaf(g0, w[o], hb0);
      hb1 = __builtin_fmaf(g1, w[o + 1], hb1);
      gw[o] = __builtin_fmaf(gphi, g0, gw[o]);
      gw[o + 1] = __builtin_fmaf(gphi, g1, gw[o + 1]);
    }
    if constexpr (OP & 1) {
      const float g0 = qp[D + OP];
      hb0 = __builtin_fmaf(g0, w[OP - 1], hb0);
      gw[OP - 1] = __builtin_fmaf(gphi, g0, gw[OP - 1]);
    }
    const float hbar = hb0 + hb1;
    // the centre's own factor -2 / sigma^2 multiplies the finished sums, not every pair:
    // d log_sig += t * (-2 d2) = (-2 s2) * t * r2,   d centre += (-2 t s2) * diff = (-2 s2) * t * diff
    float lsf;
    const float hg = hbar * gam;
    const float t = hg * basis_slope<BC>(phi, d2, r2, s2, a.gscale, a.basis, lsf);
    if constexpr (BC == BC_GAUSS || BC == BC_IQ || BC == BC_IMQ) gls = __builtin_fmaf(t, r2, gls);
    else gls = __builtin_fmaf(hg, lsf, gls);
#pragma unroll
    for (int j = 0; j < D; ++j) gc[j] = __builtin_fmaf(t, diff[j], gc[j]);
  }
  {
    const float m2s = -2.0f * s2;
    gls *= m2s;
#pragma unroll
    for (int j = 0; j < D; ++j) gc[j] *= m2s;
  }

  // combine the 4 waves through LDS (fixed order), write the slab row of this block
  float* red = lds;                            // [4][V][LP]
#pragma unroll
  for (int j = 0; j < D; ++j) red[(wave * V + j) * LP + lane] = gc[j];
  red[(wave * V + D) * LP + lane] = gls;
#pragma unroll
  for (int o = 0; o < OP; ++o) red[(wave * V + D + 1 + o) * LP + lane] = gw[o];
  __syncthreads();
  float* dst = a.part + (size_t)blockIdx.y * V * a.Npad + (size_t)blockIdx.x * kWave;
  for (int idx = tid; idx < V * kWave; idx += 256) {
    const int v = idx >> 6, l = idx & (kWave - 1);
    const float s = (red[(0 * V + v) * LP + l] + red[(1 * V + v) * LP + l]) +
                    (red[(2 * V + v) * LP + l] + red[(3 * V + v) * LP + l]);
    dst[(size_t)v * a.Npad + l] = s;
  }
}

// Reduce the slabs.  Stage 1: one thread per (value v, centre n) sums the query slices in slice order (consecutive threads
// = consecutive centres: coalesced) -> d centers, d log_sigs, and the per-CENTRE Dense gradient, which for one region IS
// d kernel and for R > 1 goes back into slab 0 (only this thread touches those words).  Stage 2 (R > 1): d kernel[k, o] =
// sum over the regions of the per-centre values, one wave per output, fixed tree.  (Round 1 summed R x QSB terms per
// output value in ONE thread: 100 threads x 128 regions x 24 slices of dependent loads = 2.2 ms of the 2.6 ms training
// step of the reference's 128-region net at its batch size of 80000.)
// Row V of the grid (blockIdx.y == V) is the second stage of the bias gradient: block o sums the per-block column sums of g
// (colsum_partial_kernel) -- a launch of its own until round 3.
//
// Where the slabs of a call live.  The primary buffer holds [slices][Vs][pitch]: the rows of K2g's live-leaf mode (rbf_vjp_gram.hip,
// VgMode: [d centers (0)] [d log_sigs (0, 1)] d kernel), full rows (mode 0) from every other kernel,
//     mode   crows   lrow   kb       Vs = kb + OP        (centre rows [0, crows), the width row, the first Dense row)
//     0      DC      DC     DC + 1   DC + 1 + OP = V
//     1      0       0      1        1 + OP
//     2      0       -1     0        OP
// and centre n in column n, or (cpr > 0: rbf_vjp_f16gram_gamma's padded chunk order) centre k of region r in column 32 cpr r + k,
// whose padding columns are never read.  Which kernel wrote the slabs can be known on the device only: where the flag holds `gen`
// the kernel in front handed the call over (it returned at once) and the one behind it wrote full rows in the plain order -- K2h
// behind a frozen-leaf K2g into the same buffer with the same slices, the gated K2 behind rbf_vjp_f16gram_gamma into `alt`, K2's own.
struct VjpSlabs {
  float* part;
  int slices, pitch, cpr, mode;
  float* alt;                       // cpr > 0: [alt_slices][V][alt_pitch]
  int alt_slices, alt_pitch;
  const int* flag;                  // null: no hand-over (never null with cpr > 0)
  int gen;
};

// grid row V of the slab reduce: block o sums the column sums of colsum_partial_kernel's blocks.  As a device function the last
// tree step compiles to two ds_read_b32 where the row written into the kernel had one ds_read2_b32 (+2 instructions); timed against
// that form on an MI355X (parent, parent again, this form; medians, us): 1000 centres at B = 80000 87.8 / 86.2 / 86.0, config 3
// 156.2 / 156.3 / 156.5, 128 regions 71.4 / 71.8 / 72.0 -- differences of the size two runs of one form show, so the row is
// stated once (profiles/vjp_reduce_fold.txt)
__device__ __forceinline__ void vjp_bias_row(const float* __restrict__ bpart, float* __restrict__ g_bias, int bias_blocks, int O,
                                             float* sm) {
  const int o = blockIdx.x, t = threadIdx.x;
  if (o >= O || bpart == nullptr) return;
  float sacc = 0.0f;
  for (int b = t; b < bias_blocks; b += 256) sacc += bpart[(size_t)b * O + o];
  sacc = block_tree_256<TreeSum, false>(sacc, sm);
  if (t == 0) g_bias[o] = sacc;
}

// What differs between the calls is compile-time: COLMAP the padded chunk order with its flag and second buffer, LIVE rows of a
// live-leaf mode, perhaps a flag, and leaves that may be null (a null g_centers / g_log_sigs is not written).  <false, false> runs
// in every training step: no load of a flag, no division.  The order of the sums is the contract: a handed-over call returns the
// bits of the kernel behind it run alone, a frozen call those of the all-live one.
template <bool COLMAP, bool LIVE>
__global__ __launch_bounds__(256) void vjp_reduce_kernel(const VjpSlabs sl, float* __restrict__ g_centers,
                                                         float* __restrict__ g_log_sigs, float* __restrict__ g_kernel, int V, int N,
                                                         int K, int R, int D, int DC, int O, int OP, const float* __restrict__ bpart,
                                                         float* __restrict__ g_bias, int bias_blocks) {
  // block = (value v, 64 consecutive centres) x 4 slice groups: thread (sg, l) sums slices sg, sg + 4, ... in order, the
  // four partial sums are added in a fixed order (small nets have few centre groups and hundreds of slices)
  __shared__ float sm[4][kWave];
  const int l = threadIdx.x & (kWave - 1), sg = threadIdx.x >> 6;
  if (blockIdx.y == (unsigned)V) return vjp_bias_row(bpart, g_bias, bias_blocks, O, &sm[0][0]);
  const int v = blockIdx.y, n = blockIdx.x * kWave + l;
  bool handed = false;                                      // the kernel behind the flag wrote the slabs
  if constexpr (COLMAP) handed = *sl.flag == sl.gen;
  else if constexpr (LIVE) handed = sl.flag != nullptr && *sl.flag == sl.gen;
  const int m = LIVE && !handed ? sl.mode : 0;
  const int crows = m == 0 ? DC : 0, lrow = m == 0 ? DC : (m == 1 ? 0 : -1), kb = m == 0 ? DC + 1 : (m == 1 ? 1 : 0);
  const int Vs = LIVE ? kb + OP : V;                         // slab stride of this layout
  // whole blocks leave: padded coordinate and output slots, and with LIVE a frozen leaf
  if constexpr (!LIVE) {
    if ((v >= D && v < DC) || v > DC + O) return;
  } else {
    if (!(v < crows ? (v < D && g_centers != nullptr) : (v == lrow ? g_log_sigs != nullptr : (v >= kb && v < kb + O)))) return;
  }
  const bool alt = COLMAP && handed;
  float* part = alt ? sl.alt : sl.part;
  const int QS = alt ? sl.alt_slices : sl.slices, Np = alt ? sl.alt_pitch : sl.pitch;
  int col = n;
  if constexpr (COLMAP)
    if (!alt) col = (n / K) * sl.cpr * 32 + n % K;
  float s = 0.0f;
  if (n < N)
    for (int q = sg; q < QS; q += 4) s += part[((size_t)q * Vs + v) * Np + col];
  sm[sg][l] = s;
  __syncthreads();
  if (sg != 0 || n >= N) return;
  s = (sm[0][l] + sm[1][l]) + (sm[2][l] + sm[3][l]);
  if (v < crows) g_centers[(size_t)n * D + v] = s;
  else if (v == lrow) g_log_sigs[n] = s;
  else if (R == 1) g_kernel[(size_t)n * O + (v - kb)] = s;
  else part[(size_t)v * Np + col] = s;                      // slab 0 of the buffer that was read (R > 1: full rows, kb = DC + 1)
}

// R > 1: d kernel[k, o] = the per-centre values of slab 0 summed over the regions, lanes over r and a fixed tree.  Only the padded
// order needs the flag here: a live-leaf call's two writers share buffer and pitch.
template <bool COLMAP>
__global__ __launch_bounds__(64) void vjp_reduce_regions_kernel(const VjpSlabs sl, float* __restrict__ g_kernel, int K, int R, int DC,
                                                                int O) {
  const int k = blockIdx.x, o = blockIdx.y, lane = threadIdx.x;
  const bool alt = COLMAP && *sl.flag == sl.gen;
  const float* part = alt ? sl.alt : sl.part;
  const int Np = alt ? sl.alt_pitch : sl.pitch, rs = COLMAP && !alt ? sl.cpr * 32 : K;
  float s = 0.0f;
  for (int r = lane; r < R; r += kWave) s += part[(size_t)(DC + 1 + o) * Np + (size_t)r * rs + k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);      // fixed tree: deterministic
  if (lane == 0) g_kernel[(size_t)k * O + o] = s;
}

// d bias[o] = sum_b g[b,o]: per-block column sums, then one block finishes (fixed order)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ g, float* __restrict__ part,
                                                              long B, int O, long rows_per_block,
                                                              float* __restrict__ bmax, const float* __restrict__ oscale) {
  extern __shared__ float sm[];                // [256]
  __shared__ float smax[256];
  float mx = 0.0f;                             // max FINITE |g| of this block's rows: the K2h / K2g operand scale (a NaN or Inf
                                               // reaches the f16 operands as such whatever the scale; split_cotangent_f16)
  float mo = 0.0f;                             // max finite |g[q,o]| s_o of these rows (bmax + gridDim.x + 8): the largest term of hbar
                                               // that is there -- K2g's scale of hbar's operands (rbf_vjp_gram.hip)
  const long r0 = (long)blockIdx.x * rows_per_block;
  long r1 = r0 + rows_per_block;
  r1 = r1 < B ? r1 : B;
  const long total = (r1 - r0) * O;
  const float* base = g + r0 * O;
  // thread t sums flat indices i = t + k*stride with stride a multiple of O -> fixed column per thread
  const int per = 256 / O > 0 ? 256 / O : 1;   // rows covered per sweep when O <= 256
  if (O <= 256) {
    const int stride = per * O;
    const int t = threadIdx.x;
    float s = 0.0f;
    if (t < stride) {
      for (long i = t; i < total; i += stride) {
        const float v = base[i];
        s += v;
        const float av = fabsf(v);
        mx = (av > mx && av <= 3.402823466e38f) ? av : mx;
      }
      if (bmax) mo = mx * oscale[t % O];         // one column per thread, its scale a power of two
    }
    sm[t] = t < stride ? s : 0.0f;
    __syncthreads();
    if (t < O) {
      float acc = 0.0f;
      for (int p = 0; p < per; ++p) acc += sm[p * O + t];
      part[(size_t)blockIdx.x * O + t] = acc;
    }
  } else {
    for (int o = threadIdx.x; o < O; o += 256) {
      float s = 0.0f;
      for (long rr = 0; rr < r1 - r0; ++rr) {
        const float v = base[rr * O + o];
        s += v;
        const float av = fabsf(v);
        mx = (av > mx && av <= 3.402823466e38f) ? av : mx;
        if (bmax) mo = fmaxf(mo, (av <= 3.402823466e38f ? av : 0.0f) * oscale[o]);
      }
      part[(size_t)blockIdx.x * O + o] = s;
    }
  }
  if (bmax) {                                  // block-uniform
    mx = block_tree_256<TreeMax, true>(mx, smax);
    mo = block_tree_256<TreeMax, false>(mo, smax);
    if (threadIdx.x == 0) {
      bmax[blockIdx.x] = mx;
      bmax[gridDim.x + 8 + blockIdx.x] = mo;
    }
  }
}

// ------------------------------------------------------------------------------------------------
struct VjpLayout {
  int groups, Npad, V, QS, bias_blocks;
  long rows_per_block;
  int QSB;         // dense slabs [QSB][V][Npad] allocated at off_part: K2 runs with all of them, K2h / K2g / K2m with at most as many
  int SL;          // K2r: slices per region = its own slabs [SL][V][Npad] at off_sp_part (0 where K2r cannot take the net)
  size_t off_gamma, off_part, off_bias, off_qrec, off_qblk, off_misc, total;
  size_t off_sp, off_sp_part, off_qm;   // K2r: pair lists, slabs; K2m: its query records
  // rbf_vjp_f16gram_gamma (a net that holds the padded images): slabs [QSG][V][NpadG] in the padded chunk order at off_gpart (one
  // region: the padded order is the plain one and the slabs are K2's), the region weights as tiles [nqb][R][32] at off_gtile
  int QSG, NpadG;
  size_t off_gtile, off_gpart;
};

// The VJP's workspace (irbfn_net_vjp_workspace_bytes): every kernel the net is eligible for has its part, whichever runs, so the
// layout reads the net and B > 0 alone -- no option, no region weights, no leaf mode.
static VjpLayout vjp_layout(const irbfn_net* net, int64_t B) {
  VjpLayout p;
  p.groups = (net->N + kWave - 1) / kWave;
  p.Npad = p.groups * kWave;
  p.V = net->DC + 1 + net->OP;
  long qsb = (8192 + (long)p.groups * 4 - 1) / ((long)p.groups * 4);
  long max_qsb = (B + 4 * 64 - 1) / (4 * 64);       // >= 64 queries per wave
  if (qsb > max_qsb) qsb = max_qsb;
  if (qsb > 4096) qsb = 4096;
  p.QSB = (int)qsb;
  p.bias_blocks = (int)(B < 256 * 64 ? (B + 63) / 64 : 256);
  p.rows_per_block = (B + p.bias_blocks - 1) / p.bias_blocks;
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t off = 0;
  p.off_gamma = off; off += al((size_t)(net->R > 1 ? B * net->R : 1) * sizeof(float));
  p.off_part = off;  off += al((size_t)p.QSB * p.V * p.Npad * sizeof(float));
  p.off_bias = off;  off += al((size_t)p.bias_blocks * net->O * sizeof(float));
  p.QS = (net->DC + 1 + net->OP + 3) & ~3;
  p.off_qrec = off;  off += al((size_t)B * p.QS * sizeof(float));
  // K2h / K2g: packed 32-query blocks + (absmax, scales)
  const size_t blkb = vjph_block_bytes(net) > vjpg_block_bytes() ? vjph_block_bytes(net) : vjpg_block_bytes();
  const bool gam = vjpgg_eligible(net) && net->gram_img != nullptr;
  p.off_qblk = off;  off += al(vjph_eligible(net) ? (size_t)((B + 31) / 32) * blkb : (gam ? (size_t)((B + 31) / 32) * vjpg_block_bytes() : 0));
  // [bias_blocks] max |g| per block, [8] (s_g, s_h, ...), [bias_blocks] max |g[q,o]| s_o per block (colsum_partial_kernel)
  p.off_misc = off;  off += al((size_t)(2 * p.bias_blocks + 8) * sizeof(float));
  p.SL = 0;
  p.off_sp = p.off_sp_part = off;
  if (sparse_vjp_eligible(net)) {
    off += al(sparse_vjp_workspace_bytes(net, B));
    p.SL = sparse_vjp_slices(net, B);
    p.off_sp_part = off;
    off += al((size_t)p.SL * p.V * p.Npad * sizeof(float));
  }
  p.off_qm = off;
  if (vjpm_eligible(net)) off += al(vjpm_qrec_bytes(net, B));
  p.QSG = 0; p.NpadG = 0;
  p.off_gtile = p.off_gpart = off;
  if (gam) {
    const long nqb = (B + 31) / 32, nch = (long)net->R * gram_gamma_cpr(net), gb = (nch + 3) / 4;
    long q = (256L * vjpgg_waves() + gb - 1) / gb;           // one resident round, at least 8 query blocks a slice: as vjpg_slices
    if (q > 64) q = 64;
    if (q * 8 > nqb) q = (nqb + 7) / 8;
    q = q < 1 ? 1 : q;
    off += al((size_t)nqb * net->R * 32 * sizeof(float));
    if (net->R == 1) {
      p.QSG = (int)(q < p.QSB ? q : p.QSB); p.NpadG = p.Npad;
      p.off_gpart = p.off_part;
    } else {
      p.QSG = (int)q; p.NpadG = (int)(nch * 32);
      p.off_gpart = off;
      off += al((size_t)p.QSG * p.V * p.NpadG * sizeof(float));
    }
  }
  p.total = off;
  return p;
}

// LDS of the gate tables that K2's query packing (vjp_pack_queries_kernel) stages
static size_t gate_tables_lds(const irbfn_net* net) {
  return ((size_t)net->nsplit * net->max_ranges * kWave + (size_t)net->n_ranges * net->nsplit) * sizeof(float);
}

// K2g's query slices.  A block = 4 waves = 128 centres; slices so that the launch is ONE resident round (3 or 4 waves per SIMD: 768 /
// 1024 blocks), at least 8 query blocks each (profiles/r03_vjp_qsb_sweep.txt: config 3 198 -> 195 us, the reference's 1000-centre
// net at B = 80000 107 -> 101 us against 1024 blocks)
static long vjpg_slices(const irbfn_net* net, int64_t B, int vg_mode, long blocks) {
  // rbf_vjp_gram.hip: 4 waves per SIMD where hbar is one MFMA (O <= 10), else 3 (the frozen-leaf modes: more, vjpg_waves)
  const long resident = vg_mode == 0 ? (net->O <= 10 ? 1024 : 768) : 256L * vjpg_waves(vg_mode, net->O);
  const long nqb = (B + 31) / 32;
  long q = (resident + blocks - 1) / blocks;
  if (q > 64) q = 64;                                  // small nets: the slab reduce grows with the slices (N = 1000, B = 80000: 64 slices 84 us, 96: 91)
  if (q * 8 > nqb) q = (nqb + 7) / 8;
  return q < 1 ? 1 : q;
}

// K2h's: fewer, longer query slices than K2 (3 waves per SIMD resident), which halves the slab traffic of the reduce kernel
static long vjph_slices(int64_t B, long blocks) {
  const long nqb = (B + 31) / 32;
  long q = (6144 + blocks * 4 - 1) / (blocks * 4);
  if (q * 4 > nqb) q = (nqb + 3) / 4;
  return q < 1 ? 1 : q;
}

// The VJP's kernel for B > 0 queries, decided here and nowhere else; written as plan_forward (rbf_forward.hip) is: the forced-only
// kernel first, then the automatic order, which the other options cut short.  `forced`: IRBFN_OPT_VJP_KERNEL, or the kernel
// irbfn_net_vjp_kernel_supported asks about.  gamma_ext: caller-provided region weights (irbfn_net_vjp_gamma); only the gated K2
// takes them.  vg_mode: the live leaves of an irbfn_net_vjp_frozen call (0: all), which K2g alone looks at.
// Returns kind + status (a plan without a kernel says IRBFN_ERR_UNSUPPORTED), p.S = the slabs the kernel runs with -- at most the
// layout's -- and what record_launch names (K2h and K2r have no name: the previous one stands).
static LaunchPlan plan_vjp(const irbfn_net* net, int64_t B, int forced, bool gamma_ext, int vg_mode, const VjpLayout& L) {
  LaunchPlan p;
  p.block = 256;
  auto take = [&](int kind, long slabs, long groups) {
    p.kind = kind; p.status = IRBFN_OK;
    p.S = (int)(slabs < L.QSB ? slabs : L.QSB);       // never more slabs than the layout allocated
    p.grid = (int)(groups * p.S);
  };
  // K2m: forced only -- IRBFN_VJP_AUTO never takes it, so every net keeps the kernel (and the bits) it had
  if (forced == IRBFN_VJP_K2M) {
    if (!vjpm_eligible(net) || gamma_ext) return p;
    take(LK_K2M, vjpm_slices(net, B, L.QSB), vjpm_groups(net));
    vjpm_names(net, &p.Q, &p.nw);
    return p;
  }
  // rbf_vjp_f16gram_gamma: forced only, irbfn_net_vjp_gamma only; any B.  The gated K2 stands behind it for a call with a query
  // outside K1g's box, so what K2 needs must hold as well.  NO_PARAMS: the images were allocated after the last irbfn_net_set_params
  if (forced == IRBFN_VJP_K2G_GAMMA) {
    if (!gamma_ext || !vjpgg_eligible(net) || L.QSG < 1 || net->vjp_flags == nullptr) return p;
    if (!(net->gram_img && net->f16_img && (net->R == 1 || net->gamma_packed))) { p.status = IRBFN_ERR_NO_PARAMS; return p; }
    if (!net->gram_ok || gate_tables_lds(net) > 64 * 1024) return p;
    p.kind = LK_K2G_GAMMA; p.status = IRBFN_OK;
    p.S = L.QSG;
    p.grid = (int)(((long)net->R * gram_gamma_cpr(net) + 3) / 4 * p.S);
    return p;
  }
  // K2h: every option but K2 reaches it, IRBFN_VJP_K2R included -- so IRBFN_VJP_K2H is a preference (below 2048 queries, or on a
  // net K2h cannot take, the call goes on to K2), and a forced K2r refuses only where K2h does not take the call
  if (vjph_eligible(net) && forced != IRBFN_VJP_K2 && B >= 2048 && !gamma_ext) {
    // K2g in front of K2h from 8192 queries and 2.5e7 (query, centre) pairs (tools/sweep_vjp_batch.py: 4096 centres: K2g 57.6 vs
    // K2h 64.3 us at B = 12288, a tie at 8192; 1000 centres: 50.1 vs 52.1 at 24576, 46.3 vs 45.0 at 16384)
    const bool gram = vjpg_eligible(net) &&
                      (forced == IRBFN_VJP_K2G || (forced == IRBFN_VJP_AUTO && B >= 8192 && (long long)B * net->N >= 25000000LL));
    if (forced == IRBFN_VJP_K2G && !gram) return p;
    if (vjph_lds_bytes(net) > 64 * 1024) return p;
    const long gh = (net->N + 31) / 32, gb = (gh + 3) / 4;      // K2h: blocks of 4 waves x 2 tiles of 16 centres; K2g: 128 centres
    if (gram) take(LK_K2G, vjpg_slices(net, B, vg_mode, gb), gb);
    else take(LK_K2H, vjph_slices(B, gh), gh);
    p.mode = vg_mode;
    return p;
  }
  if (forced == IRBFN_VJP_K2G) return p;
  // K2r: several regions with a sparse gate (automatic where the forward takes K1r).  Where its pair tables do not fit, K2 runs
  // instead, unless K2r was forced.  With caller-provided region weights the option is not looked at.
  if (!gamma_ext) {
    const bool sparse = sparse_vjp_eligible(net) && (forced == IRBFN_VJP_K2R || (forced == IRBFN_VJP_AUTO && sparse_preferred(net, B)));
    if (sparse && sparse_vjp_lds_fits(net)) {
      p.kind = LK_K2R; p.status = IRBFN_OK; p.S = L.SL;
      return p;
    }
    if (forced == IRBFN_VJP_K2R) return p;
  }
  // K2: every net; gated where the region weights differ between the lanes of a wave
  p.lds = gate_tables_lds(net);
  if (p.lds > 64 * 1024) return p;
  take(LK_K2, L.QSB, L.groups);
  p.gated = net->R > 1 || gamma_ext;
  return p;
}

// ---- ClusterWCRBFNet (src/irbfn_mpc/model.py:341-414): cotangent of the region weights ------------------------------
// d gamma[b,r] = sum_k hbar[b,k] phi[b,r,k],  hbar = g W^T  (the path from `out` back to the softmax gate; the tanh
// gate of WCRBFNet has no parameters, so K2 never needs it).  One lane per query, one wave per (64 queries, region):
// the region's K centre records are wave-uniform scalar streams, g[b,:] sits in registers.
template <int D, int OP>
__global__ __launch_bounds__(64) void dgamma_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                    const float* __restrict__ rec, float* __restrict__ dgamma, long B,
                                                    int Dreal, int O, int K, int R, int S, int bclass, int basis) {
  const int lane = threadIdx.x, r = blockIdx.y;
  const long b = (long)blockIdx.x * kWave + lane;
  const long bb = b < B ? b : B - 1;
  float xq[D], gq[OP];
#pragma unroll
  for (int j = 0; j < D; ++j) xq[j] = j < Dreal ? x[bb * Dreal + j] : 0.0f;
#pragma unroll
  for (int o = 0; o < OP; ++o) gq[o] = o < O ? g[bb * O + o] : 0.0f;
  float acc = 0.0f;
  const float* rp = rec + (size_t)r * K * S;
  for (int k = 0; k < K; ++k, rp += S) {
    float r2 = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float d = xq[j] - rp[j];
      r2 = __builtin_fmaf(d, d, r2);
    }
    float phi;
    switch (bclass) {
      case BC_GAUSS: phi = basis_from_r2<BC_GAUSS>(r2, rp[D], basis); break;
      case BC_IQ: phi = basis_from_r2<BC_IQ>(r2, rp[D], basis); break;
      case BC_IMQ: phi = basis_from_r2<BC_IMQ>(r2, rp[D], basis); break;
      default: phi = basis_from_r2<BC_GENERIC>(r2, rp[D], basis); break;
    }
    float hb = 0.0f;
#pragma unroll
    for (int o = 0; o < OP; ++o) hb = __builtin_fmaf(gq[o], rp[D + 1 + o], hb);
    acc = __builtin_fmaf(hb, phi, acc);
  }
  if (b < B) dgamma[b * R + r] = acc;
}

int launch_dgamma(irbfn_net* net, const float* x, const float* gout, float* dgamma, int64_t B, hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  const dim3 grid((unsigned)((B + kWave - 1) / kWave), net->R), block(kWave);
  return dispatch<3, 4, 7, 8>(net->DC, [&](auto dc) {
    return dispatch<2, 4, 5, 8, 10, 16>(net->OP, [&](auto op) {       // O <= 16
      return launch_kernel<dgamma_kernel<dc(), op()>>(grid, block, 0, s, x, gout, net->rec, dgamma, (long)B, net->D, net->O, net->K,
                                                      net->R, net->S, net->bclass, net->basis);
    });
  });
}

// softmax backward of the cluster gate (model.py:402-404): d logits = gamma * (d gamma - sum_s gamma_s d gamma_s)
// [+ the direct cotangent of the logits, e.g. of the cluster cross-entropy], one thread per query
__global__ __launch_bounds__(256) void cluster_dlogits_kernel(const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                              const float* __restrict__ glogits, float* __restrict__ dlogits,
                                                              long B, int R) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float dot = 0.0f;
  for (int r = 0; r < R; ++r) dot = __builtin_fmaf(gamma[b * R + r], dgamma[b * R + r], dot);
  for (int r = 0; r < R; ++r) {
    float v = gamma[b * R + r] * (dgamma[b * R + r] - dot);
    if (glogits) v += glogits[b * R + r];
    dlogits[b * R + r] = v;
  }
}

// d Wc[d,r] = sum_b x[b,d] dlogits[b,r] (d < D), d bc[r] = sum_b dlogits[b,r] (d == D).  Grid (region chunk, batch block):
// each of kGateBwdBlocks batch blocks walks the batch in 64-row tiles (coalesced copies into LDS) for one chunk of at most
// RC = gate_bwd_chunk(D) regions, whose (D + 1) * RC outputs fit in 256 threads x kGateBwdOut registers and whose
// xs[64][D + 1] + dl[64][RC] stage fits in 48 KiB of LDS, whatever R is.  Thread t owns the chunk's outputs t, t + 256, ...
// and adds the tile's rows in order; the per-block partial sums are added in block order by cluster_dense_final_kernel:
// deterministic, and each output's order does not depend on the chunking.  (The first version gave one block to an output
// and let it stride over the whole batch: 99 blocks, uncoalesced -- 102 us at 80000 rows.)
constexpr int kGateBwdBlocks = 256;
constexpr int kGateBwdOut = 8;                   // outputs per thread
constexpr int kGateBwdLdsFloats = 48 * 1024 / 4;
static int gate_bwd_chunk(int D) {
  const int by_regs = 256 * kGateBwdOut / (D + 1);
  const int by_lds = kGateBwdLdsFloats / kWave - (D + 1);
  return by_regs < by_lds ? by_regs : by_lds;
}
__global__ __launch_bounds__(256) void cluster_dense_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dlogits,
                                                                float* __restrict__ part, long B, int D, int R, int RC) {
  extern __shared__ float lds[];                 // xs[64][D + 1] (last column = 1), dl[64][nr]
  float* xs = lds;
  float* dl = lds + kWave * (D + 1);
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * RC;
  const int nr = R - r0 < RC ? R - r0 : RC;      // regions of this chunk
  const int nout = (D + 1) * nr;
  float acc[kGateBwdOut];
#pragma unroll
  for (int k = 0; k < kGateBwdOut; ++k) acc[k] = 0.0f;
  const long ntiles = (B + kWave - 1) / kWave;
  for (long tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
    const long b0 = tile * kWave;
    const long left = B - b0;
    const int nv = left < kWave ? (int)left : kWave;
    for (int i = tid; i < kWave * (D + 1); i += 256) {
      const int row = i / (D + 1), d = i - row * (D + 1);
      xs[i] = row < nv ? (d < D ? x[(b0 + row) * D + d] : 1.0f) : 0.0f;
    }
    for (int i = tid; i < kWave * nr; i += 256) {
      const int row = i / nr, r = i - row * nr;
      dl[i] = row < nv ? dlogits[(b0 + row) * R + r0 + r] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kGateBwdOut; ++k) {
      const int t = tid + k * 256;
      if (t < nout) {
        const int d = t / nr, r = t - d * nr;
        float s = acc[k];
        for (int row = 0; row < kWave; ++row) s = __builtin_fmaf(xs[row * (D + 1) + d], dl[row * nr + r], s);
        acc[k] = s;
      }
    }
    __syncthreads();
  }
  const size_t nall = (size_t)(D + 1) * R;
#pragma unroll
  for (int k = 0; k < kGateBwdOut; ++k) {
    const int t = tid + k * 256;
    if (t < nout) {
      const int d = t / nr, r = t - d * nr;
      part[(size_t)blockIdx.y * nall + (size_t)d * R + r0 + r] = acc[k];
    }
  }
}

__global__ __launch_bounds__(256) void cluster_dense_final_kernel(const float* __restrict__ part, float* __restrict__ g_wc,
                                                                  float* __restrict__ g_bc, int nblk, int D, int R) {
  // 16 outputs per block x 16 block groups: thread (sg, v) adds partials sg, sg + 16, ... in order, then a fixed tree
  __shared__ float sm[16][17];
  const int v = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const int t = blockIdx.x * 16 + v, nout = (D + 1) * R;
  float s = 0.0f;
  if (t < nout)
    for (int k = sg; k < nblk; k += 16) s += part[(size_t)k * nout + t];
  sm[sg][v] = s;
  __syncthreads();
  for (int w = 8; w > 0; w >>= 1) {
    if (sg < w) sm[sg][v] += sm[sg + w][v];
    __syncthreads();
  }
  if (sg != 0 || t >= nout) return;
  if (t < D * R) g_wc[t] = sm[0][v];
  else g_bc[t - D * R] = sm[0][v];
}

int64_t cluster_gate_vjp_workspace_bytes(int D, int R) { return (int64_t)kGateBwdBlocks * (D + 1) * R * (int64_t)sizeof(float); }

int launch_cluster_gate_vjp(const float* x, const float* gamma, const float* dgamma, const float* glogits, float* dlogits,
                            float* g_wc, float* g_bc, int64_t B, int D, int R, float* ws, hipStream_t s) {
  if (B == 0) {
    IRBFN_HIP_CHECK(hipMemsetAsync(g_wc, 0, (size_t)D * R * sizeof(float), s));
    IRBFN_HIP_CHECK(hipMemsetAsync(g_bc, 0, (size_t)R * sizeof(float), s));
    return IRBFN_OK;
  }
  if (D < 1 || D > 16 || R < 1 || (int64_t)(D + 1) * R > INT_MAX) return IRBFN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cluster_dlogits_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, gamma, dgamma, glogits, dlogits,
                     (long)B, R);
  IRBFN_HIP_CHECK(hipGetLastError());
  const int RC = gate_bwd_chunk(D);
  const int nchunk = (R + RC - 1) / RC;
  const size_t lds = (size_t)kWave * (D + 1 + (R < RC ? R : RC)) * sizeof(float);
  const long ntiles = (B + kWave - 1) / kWave;
  const int nblk = ntiles < kGateBwdBlocks ? (int)ntiles : kGateBwdBlocks;
  hipLaunchKernelGGL(cluster_dense_bwd_kernel, dim3((unsigned)nchunk, (unsigned)nblk), dim3(256), lds, s, x, dlogits, ws,
                     (long)B, D, R, RC);
  IRBFN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(cluster_dense_final_kernel, dim3(((D + 1) * R + 15) / 16), dim3(256), 0, s, ws, g_wc, g_bc, nblk, D, R);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

// optax.softmax_cross_entropy(logits, labels).mean() (scripts/train_nmpc_frenet.py:431) and its cotangent of the logits:
// loss_b = -sum_r labels[b,r] log_softmax(logits)[b,r];  d loss / d logits = (softmax * sum_r labels - labels) / B.
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                           float* __restrict__ glogits, float* __restrict__ loss_part, long B,
                                                           int R) {
  __shared__ float sm[256];
  float lsum = 0.0f;
  const float invB = 1.0f / (float)B;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long)gridDim.x * 256) {
    float mx = -INFINITY;
    for (int r = 0; r < R; ++r) mx = fmaxf(mx, logits[b * R + r]);
    float se = 0.0f, sl = 0.0f;
    for (int r = 0; r < R; ++r) { se += expf(logits[b * R + r] - mx); sl += labels[b * R + r]; }
    const float lse = mx + logf(se);
    for (int r = 0; r < R; ++r) {
      const float lp = logits[b * R + r] - lse;
      lsum += -labels[b * R + r] * lp * invB;
      glogits[b * R + r] = (expf(lp) * sl - labels[b * R + r]) * invB;
    }
  }
  lsum = block_tree_256<TreeSum, false>(lsum, sm);
  if (threadIdx.x == 0) loss_part[blockIdx.x] = lsum;
}

__global__ __launch_bounds__(256) void xent_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out, int accumulate) {
  __shared__ float sm[256];
  float v = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) v += part[i];
  v = block_tree_256<TreeSum, false>(v, sm);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + v : v;
}

int launch_softmax_xent(const float* logits, const float* labels, float* glogits, float* loss, float* partials, int accumulate,
                        int64_t B, int R, hipStream_t s) {
  hipLaunchKernelGGL(softmax_xent_kernel, dim3(kRedBlocks), dim3(256), 0, s, logits, labels, glogits, partials, (long)B, R);
  IRBFN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(xent_final_kernel, dim3(1), dim3(256), 0, s, partials, kRedBlocks, loss, accumulate);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

int vjp_kernel_supported(const irbfn_net* net, int kernel, int64_t B) {
  if (B < 1) B = 1;
  return plan_vjp(net, B, kernel, false, 0, vjp_layout(net, B)).status == IRBFN_OK ? 1 : 0;
}

int64_t vjp_workspace_bytes(const irbfn_net* net, int64_t B) { return B <= 0 ? 0 : (int64_t)vjp_layout(net, B).total; }

// One parameter-VJP call as its launch sequences see it
struct VjpCall {
  irbfn_net* net;
  const float *x, *gout, *gamma_ext;
  float *g_centers, *g_log_sigs, *g_kernel, *g_bias;   // a null g_centers / g_log_sigs: a frozen leaf (irbfn_net_vjp_frozen)
  int64_t B;
  char* ws;
  hipStream_t s;
  template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
};

// the bias column sums per block; bmax: the block maxima of |g|, and behind them and the scales those of |g| s_o, as well (K2h / K2g
// pack g to f16 with them)
static int bias_partials(const VjpCall& c, const VjpLayout& L, float* bmax) {
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(L.bias_blocks), dim3(256), 256 * sizeof(float), c.s, c.gout, c.at<float>(L.off_bias),
                     (long)c.B, c.net->O, L.rows_per_block, bmax, bmax ? c.net->f16_oscale : nullptr);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

// The slab reduce of every call: V value rows and the bias row over max(centre groups, O) blocks, then for R > 1 the region stage.
// The instance follows from the slabs and the leaves; full rows of one buffer with every leaf live take the one without a flag load.
static int launch_vjp_reduce(const VjpCall& c, const VjpLayout& L, const VjpSlabs& sl) {
  const irbfn_net* net = c.net;
  unsigned gx = (unsigned)((net->N + kWave - 1) / kWave);
  if (gx < (unsigned)net->O) gx = (unsigned)net->O;
  const bool colmap = sl.cpr > 0, live = sl.flag != nullptr || sl.mode != 0 || !c.g_centers || !c.g_log_sigs;
  auto stage1 = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(gx, L.V + 1), dim3(256), 0, c.s, sl, c.g_centers, c.g_log_sigs, c.g_kernel, L.V, net->N, net->K, net->R,
                       net->D, net->DC, net->O, net->OP, c.at<float>(L.off_bias), c.g_bias, L.bias_blocks);
  };
  if (colmap) stage1(vjp_reduce_kernel<true, false>);
  else if (live) stage1(vjp_reduce_kernel<false, true>);
  else stage1(vjp_reduce_kernel<false, false>);
  IRBFN_HIP_CHECK(hipGetLastError());
  if (net->R > 1) {
    auto stage2 = colmap ? vjp_reduce_regions_kernel<true> : vjp_reduce_regions_kernel<false>;
    hipLaunchKernelGGL(stage2, dim3(net->K, net->O), dim3(kWave), 0, c.s, sl, c.g_kernel, net->K, net->R, net->DC, net->O);
    IRBFN_HIP_CHECK(hipGetLastError());
  }
  return IRBFN_OK;
}

// full rows [slices][V][Npad] of one writer in the plain order
static VjpSlabs plain_slabs(const VjpLayout& L, float* slabs, int slices) {
  return {slabs, slices, L.Npad, 0, 0, nullptr, 0, 0, nullptr, 0};
}

// the tail of K2m, K2r and K2: the bias column sums (no block maxima: nobody packs g to f16 there), then the slab reduce
static int bias_and_reduce(const VjpCall& c, const VjpLayout& L, float* slabs, int slices) {
  const int rc = bias_partials(c, L, nullptr);
  return rc != IRBFN_OK ? rc : launch_vjp_reduce(c, L, plain_slabs(L, slabs, slices));
}

// K2h, or K2g with K2h behind it
static int launch_vjp_k2h(const VjpCall& c, const VjpLayout& L, const LaunchPlan& p) {
  irbfn_net* net = c.net;
  float* part = c.at<float>(L.off_part);
  unsigned char* qblk = c.at<unsigned char>(L.off_qblk);
  float* bmax = c.at<float>(L.off_misc);         // [bias_blocks] max |g| per block
  float* scales = bmax + L.bias_blocks;          // [2]
  int rc = bias_partials(c, L, bmax);
  if (rc != IRBFN_OK) return rc;
  const bool gram = p.kind == LK_K2G, live = gram && p.mode != 0;      // live: slabs of the live rows only (they fit in the full-row slabs)
  const int* run_if = nullptr;
  int run_gen = 0;
  if (gram) {
    // K2g first; a query outside its representable box raises the flag, K2g returns at once and K2h -- launched behind it
    // with the complementary test -- does the work
    // The flag is a generation number in a small ring of net-owned words (zero at creation): call `gen` stores gen into word
    // gen % 64 when it has such a query, nobody resets anything -- a memset per call was a launch of its own.
    if (++net->vjp_gen <= 0) net->vjp_gen = 1;
    run_gen = net->vjp_gen;
    int* flag = net->vjp_flags + (run_gen & 63);
    record_launch(net, p);
    rc = live ? launch_vjp_gram_live(net, p.mode, c.x, c.gout, c.B, qblk, bmax, L.bias_blocks, scales, flag, run_gen, part, p.S, L.Npad, c.s)
              : launch_vjp_gram(net, c.x, c.gout, c.B, qblk, bmax, L.bias_blocks, scales, flag, run_gen, part, p.S, L.Npad, c.s);
    if (rc != IRBFN_OK) return rc;
    run_if = flag;
  }
  rc = launch_vjp_f16(net, c.x, c.gout, c.B, qblk, bmax, L.bias_blocks, scales, part, p.S, L.Npad, c.s, run_if, run_gen);
  if (rc != IRBFN_OK) return rc;
  VjpSlabs sl = plain_slabs(L, part, p.S);
  if (live) { sl.mode = p.mode; sl.flag = run_if; sl.gen = run_gen; }   // K2g's live rows, or K2h's full ones where the flag holds gen
  return launch_vjp_reduce(c, L, sl);
}

static int launch_vjp_k2m(const VjpCall& c, const VjpLayout& L, const LaunchPlan& p) {
  float* part = c.at<float>(L.off_part);
  record_launch(c.net, p);
  const int rc = launch_vjp_mfma(c.net, c.x, c.gout, c.B, c.at<float>(L.off_qm), part, p.S, L.Npad, c.s);
  return rc != IRBFN_OK ? rc : bias_and_reduce(c, L, part, p.S);
}

// K2r: pair lists per region -> one wave per (region, slice) -> the same fixed-order slab reduce; no query packing
static int launch_vjp_k2r(const VjpCall& c, const VjpLayout& L, const LaunchPlan& p) {
  float* part = c.at<float>(L.off_sp_part);
  const int rc = launch_vjp_sparse(c.net, c.x, c.gout, c.B, c.ws + L.off_sp, part, p.S, L.Npad, c.s);
  return rc != IRBFN_OK ? rc : bias_and_reduce(c, L, part, p.S);
}

// K2's query packing and main kernel.  run_if: behind rbf_vjp_f16gram_gamma (caller-provided region weights, so the packing writes
// none of its own) the main kernel runs only where the word holds run_gen
static int launch_vjp_k2_main(const VjpCall& c, const VjpLayout& L, const LaunchPlan& p, const int* run_if = nullptr, int run_gen = 0) {
  irbfn_net* net = c.net;
  float *qrec = c.at<float>(L.off_qrec), *gamma = c.at<float>(L.off_gamma), *part = c.at<float>(L.off_part);
  hipLaunchKernelGGL(vjp_pack_queries_kernel, dim3((unsigned)((c.B + kWave - 1) / kWave)), dim3(256), p.lds, c.s, c.x, c.gout, qrec, gamma,
                     net->gate(), (long)c.B, net->D, net->DC, net->O, net->OP, L.QS, run_if ? 1 : net->R);
  IRBFN_HIP_CHECK(hipGetLastError());
  VjpArgs a;
  a.flag = run_if; a.gen = run_gen;
  a.qrec = qrec; a.gamma = c.gamma_ext ? c.gamma_ext : gamma; a.rec = net->rec; a.sig2 = net->sig2; a.part = part;
  a.B = (long)c.B; a.Dreal = net->D; a.O = net->O; a.N = net->N; a.K = net->K; a.R = net->R; a.S = net->S;
  a.basis = net->basis; a.Npad = L.Npad; a.gscale = gauss_scale(net->basis);
  a.per_wave = (int)((c.B + p.S * 4L - 1) / (p.S * 4L));      // four waves per slab, each its share of the queries
  const dim3 grid(L.groups, p.S);
  if (!run_if) record_launch(net, p);
  return dispatch<3, 4, 7, 8>(net->DC, [&](auto dc) {
    return dispatch<2, 4, 5, 8, 10, 16, 32, 64, 100, 128>(net->OP, [&](auto op) {
      constexpr int V = dc() + 1 + op();
      const size_t lds = (size_t)4 * V * (kWave + 1) * sizeof(float);
      return dispatch<BC_GAUSS, BC_IQ, BC_IMQ, BC_GENERIC>(net->bclass, [&](auto bc) {
        return p.gated ? launch_kernel<rbf_vjp_kernel<dc(), op(), bc(), true>>(grid, dim3(256), lds, c.s, a)
                       : launch_kernel<rbf_vjp_kernel<dc(), op(), bc(), false>>(grid, dim3(256), lds, c.s, a);
      });
    });
  });
}

static int launch_vjp_k2(const VjpCall& c, const VjpLayout& L, const LaunchPlan& p) {
  const int rc = launch_vjp_k2_main(c, L, p);
  return rc != IRBFN_OK ? rc : bias_and_reduce(c, L, c.at<float>(L.off_part), p.S);
}

// rbf_vjp_f16gram_gamma, the gated K2 behind it: a query outside K1g's box raises this call's flag (as for K2g, launch_vjp_k2h), the
// matrix-core kernel returns at once and K2 -- launched behind it with the complementary test -- does the work
static int launch_vjp_k2g_gamma(const VjpCall& c, const VjpLayout& L, const LaunchPlan& p) {
  irbfn_net* net = c.net;
  const LaunchPlan pk = plan_vjp(net, c.B, IRBFN_VJP_K2, true, 0, L);
  if (pk.kind != LK_K2) return pk.status;
  float* bmax = c.at<float>(L.off_misc);         // [bias_blocks] max |g| per block
  float* scales = bmax + L.bias_blocks;          // [2]
  int rc = bias_partials(c, L, bmax);
  if (rc != IRBFN_OK) return rc;
  if (++net->vjp_gen <= 0) net->vjp_gen = 1;
  const int gen = net->vjp_gen;
  int* flag = net->vjp_flags + (gen & 63);
  record_launch(net, p);
  rc = launch_vjp_gram_gamma(net, c.x, c.gamma_ext, c.gout, c.B, c.at<unsigned char>(L.off_qblk), c.at<float>(L.off_gtile), bmax,
                             L.bias_blocks, scales, flag, gen, c.at<float>(L.off_gpart), p.S, L.NpadG, c.s);
  if (rc != IRBFN_OK) return rc;
  rc = launch_vjp_k2_main(c, L, pk, flag, gen);
  if (rc != IRBFN_OK) return rc;
  // the matrix-core kernel's slabs in the padded chunk order, or K2's own where the flag holds gen
  return launch_vjp_reduce(c, L, {c.at<float>(L.off_gpart), p.S, L.NpadG, gram_gamma_cpr(net), 0, c.at<float>(L.off_part), pk.S, L.Npad, flag, gen});
}

int launch_vjp(irbfn_net* net, const float* x, const float* gout, float* g_centers, float* g_log_sigs, float* g_kernel,
               float* g_bias, int64_t B, void* ws, hipStream_t s, const float* gamma_ext, bool frozen) {
  if (B == 0) {
    if (g_centers) IRBFN_HIP_CHECK(hipMemsetAsync(g_centers, 0, (size_t)net->N * net->D * sizeof(float), s));
    if (g_log_sigs) IRBFN_HIP_CHECK(hipMemsetAsync(g_log_sigs, 0, (size_t)net->N * sizeof(float), s));
    IRBFN_HIP_CHECK(hipMemsetAsync(g_kernel, 0, (size_t)net->K * net->O * sizeof(float), s));
    IRBFN_HIP_CHECK(hipMemsetAsync(g_bias, 0, (size_t)net->O * sizeof(float), s));
    return IRBFN_OK;
  }
  // K2g's mode: the centres frozen -> NO_CENTRES, the widths too -> LINEAR; live centres with frozen widths take the full
  // computation (no upstream layer class freezes the widths alone)
  const int vg_mode = !frozen || g_centers ? 0 : (g_log_sigs ? 1 : 2);
  const VjpLayout L = vjp_layout(net, B);
  const LaunchPlan p = plan_vjp(net, B, net->opt[IRBFN_OPT_VJP_KERNEL], gamma_ext != nullptr, vg_mode, L);
  const VjpCall c = {net, x, gout, gamma_ext, g_centers, g_log_sigs, g_kernel, g_bias, B, static_cast<char*>(ws), s};
  switch (p.kind) {
    case LK_K2G:
    case LK_K2H: return launch_vjp_k2h(c, L, p);
    case LK_K2M: return launch_vjp_k2m(c, L, p);
    case LK_K2R: return launch_vjp_k2r(c, L, p);
    case LK_K2: return launch_vjp_k2(c, L, p);
    case LK_K2G_GAMMA: return launch_vjp_k2g_gamma(c, L, p);
    default: return p.status;
  }
}

}  // namespace irbfn
