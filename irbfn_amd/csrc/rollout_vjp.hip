// K4: hand-derived VJPs of the roll-outs (reverse sweeps).  One lane per trajectory: the forward is
// recomputed, the few pre-step quantities the adjoint needs are parked in LDS ([T][NP][64], one
// column per lane -> conflict-free), then the sweep runs backwards accumulating the seeds of every
// step's state (`all_states` is the differentiated output).
//
// Replaces JAX's transpose of the scans under value_and_grad: scripts/train_nmpc.py:275-276
// (dynamic_st_onestep_aux), :356-374 (inline bicycle), scripts/train_nmpc_frenet.py:408-409
// (integrate_frenet_mult), deprecated/train_newlut.py:194-199 (integrate_path_mult).
// clip() gradient: 1 strictly inside, 0 strictly outside, `tie` on a bound (jnp.clip is
// minimum(maximum(.)), whose tie rule is 1/2).
#include "common.h"
#include "rollout_step.h"
#include "rollout_adjoint.h"

namespace irbfn {

struct RollVjpArgs {
  const float* __restrict__ x0u;      // [B][L]
  const float* __restrict__ gstates;  // [B][T][S]
  float* __restrict__ gx0u;           // [B][L]
  long B;
  int T, L;
  float tie;
  DynParams dp;
};

// ---- the control-driven models (dynamics.py:103-187, scripts/train_nmpc.py:329-374, dynamics.py:190-290) ---------
// The forward's pre-step quantities (vjp_park: NP floats per step) are parked in LDS, [T][NP][64], one column per lane.
template <int MODE>
__global__ __launch_bounds__(64) void rollout_vjp_park_kernel(const RollVjpArgs a) {
  constexpr int S = ModeTraits<MODE>::S, S0 = ModeTraits<MODE>::S0, NP = ModeTraits<MODE>::NP;
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const long b = (long)blockIdx.x * kWave + lane;
  if (b >= a.B) return;
  const int T = a.T;
  const float* row = a.x0u + b * a.L;
  const float* u = row + S0;                     // a_t = u[t], sv_t = u[T + t]
  float* grow = a.gx0u + b * a.L;
  const float* gs = a.gstates + b * (long)T * S;
  float s[S];
  roll_init<MODE>(row, s);
  [[maybe_unused]] const float cur = MODE == IRBFN_ROLLOUT_FRENET_LS ? s[S - 1] : 0.0f;   // Frenet: the curvature
  for (int t = 0; t < T; ++t) {
    float pk[NP];
    vjp_park<MODE>(s, pk);
#pragma unroll
    for (int i = 0; i < NP; ++i) lds[(t * NP + i) * kWave + lane] = pk[i];
    roll_step<MODE>(s, u[t], u[T + t], a.dp);
  }
  float lam[S];
#pragma unroll
  for (int i = 0; i < S; ++i) lam[i] = 0.0f;
  for (int t = T - 1; t >= 0; --t) {
#pragma unroll
    for (int i = 0; i < S; ++i) lam[i] += gs[t * S + i];
    float pk[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) pk[i] = lds[(t * NP + i) * kWave + lane];
    float ga, gsv;
    vjp_back_step<MODE>(pk, u[t], u[T + t], lam, cur, a.tie, a.dp, ga, gsv);
    grow[S0 + t] = ga;
    grow[S0 + T + t] = gsv;
  }
  float g0[S0];
  roll_init_grad<MODE>(row, lam, a.tie, g0);
#pragma unroll
  for (int i = 0; i < S0; ++i) grow[i] = g0[i];
}

// ---- cubic spiral (planner_utils.py:20-77); T = number of samples N <= 256 ------------------------------------------------
// Per-lane seed dwords at a stride of N * 24 bytes and a park of theta / dx / dy of all N samples in LDS measured 0.75 TB/s
// (B = 262144, N = 100).  Here one wave owns 64 consecutive paths -- their seeds are ONE contiguous block of HBM -- and walks
// the samples in chunks of G = 8, last chunk first:
//  * the chunk's seeds (64 rows x 48 floats) are read by the whole wave as consecutive dwords (256 contiguous bytes per
//    instruction, runs of 192 bytes per row) into an LDS tile of odd pitch and read back per row without bank conflicts;
//  * no park of all samples: the forward pass keeps a checkpoint (theta, dx, dy before the chunk: 3 floats) per chunk in LDS,
//    the reverse pass re-runs one chunk from its checkpoint into registers -- the forward's own values, same step function --
//    and sweeps it backwards.
constexpr int kSpiralG = 8;
constexpr int kSpiralPitch = kSpiralG * 6 + 1;     // odd
__global__ __launch_bounds__(64) void rollout_vjp_spiral_staged(const RollVjpArgs a) {
  extern __shared__ float lds[];
  constexpr int G = kSpiralG, PITCH = kSpiralPitch;
  const int lane = threadIdx.x;
  const long b0 = (long)blockIdx.x * kWave;
  const long left = a.B - b0;
  const int nvalid = left < kWave ? (int)left : kWave;
  const int N = a.T;
  const int nch = (N + G - 1) / G;
  float* tile = lds;                             // [64][PITCH]
  float* ck = lds + kWave * PITCH;               // [nch][3][64]
  const long b = b0 + (lane < nvalid ? lane : nvalid - 1);
  const float* row = a.x0u + b * 5;
  float q[5], c[4];
#pragma unroll
  for (int i = 0; i < 5; ++i) q[i] = row[i];
  spiral_coefs(q, c);
  const float slen = q[4];
  {                                              // forward pass: checkpoints only
    float st[6] = {0.0f, 0.0f, 0.0f, c[0], 0.0f, 0.0f};
    float sc[2] = {0.0f, 1.0f};
    for (int i = 0; i < N; ++i) {
      if (i % G == 0) {
        const int g = i / G;
        ck[(g * 3 + 0) * kWave + lane] = st[2];
        ck[(g * 3 + 1) * kWave + lane] = st[4];
        ck[(g * 3 + 2) * kWave + lane] = st[5];
      }
      spiral_step(st, c, slen, i, N, sc);
    }
  }
  const float* gs_tile = a.gstates + b0 * (long)N * 6;
  const long rs = (long)N * 6;
  float gc[4] = {0, 0, 0, 0};
  float g_s = 0.0f, ldx = 0.0f, ldy = 0.0f, lth = 0.0f;
#pragma unroll 1
  for (int g = nch - 1; g >= 0; --g) {
    const int i0 = g * G;
    const int n = (N - i0) < G ? (N - i0) : G;
    const int nf = n * 6;
    // the chunk's seeds: consecutive lanes = consecutive floats of a row's segment
    const float rnf = 1.0f / (float)nf;           // idx < 64 * 48: (idx + 0.5) / nf in float32 floors to the exact quotient
    for (int idx = lane; idx < nvalid * nf; idx += kWave) {
      const int r = (int)(((float)idx + 0.5f) * rnf), j = idx - r * nf;
      tile[r * PITCH + j] = gs_tile[r * rs + (long)i0 * 6 + j];
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // re-run the chunk from its checkpoint
    float st[6] = {0.0f, 0.0f, ck[(g * 3 + 0) * kWave + lane], 0.0f, ck[(g * 3 + 1) * kWave + lane], ck[(g * 3 + 2) * kWave + lane]};
    // parked per sample: sin / cos of its heading and of the previous one (the step's own evaluations: the adjoint below
    // needs no trigonometry of its own -- four ocml sinf / cosf calls per sample made this kernel compute-bound), dx, dy
    float psn[G], pcs[G], psp[G], pcp[G], pdx[G], pdy[G];
    float sc[2];
    sincos_fast(st[2], sc[0], sc[1]);
#pragma unroll
    for (int tt = 0; tt < G; ++tt) {
      psp[tt] = sc[0]; pcp[tt] = sc[1];
      if (tt < n) spiral_step(st, c, slen, i0 + tt, N, sc);
      psn[tt] = sc[0]; pcs[tt] = sc[1]; pdx[tt] = st[4]; pdy[tt] = st[5];
    }
    const float* mine = tile + (lane < nvalid ? lane : nvalid - 1) * PITCH;
#pragma unroll
    for (int tt = G - 1; tt >= 0; --tt) {
      if (tt < n) {
        const int i = i0 + tt;
        const float tau = (i < N - 1) ? fdiv_fast((float)i, (float)(N - 1)) : (i > 0 ? 1.0f : 0.0f);    // as spiral_step
        const float sk = (i < N - 1) ? slen * tau : (i > 0 ? slen : 0.0f);
        const float k = (float)(i + 1);
        const float rk = fdiv_fast(1.0f, k);
        const float dx = pdx[tt], dy = pdy[tt];
        const float gx = mine[tt * 6 + 0], gy = mine[tt * 6 + 1], gth = mine[tt * 6 + 2], gka = mine[tt * 6 + 3],
                    gdx = mine[tt * 6 + 4], gdy = mine[tt * 6 + 5];
        const float Gdx = gdx + ldx + sk * gx;
        const float Gdy = gdy + ldy + sk * gy;
        float gsk = gx * dx + gy * dy;
        const float Gth = gth + lth + (Gdx * (-psn[tt]) + Gdy * pcs[tt]) * (0.5f * rk);
        lth = (Gdx * (-psp[tt]) + Gdy * pcp[tt]) * (0.5f * rk);     // sample 0: previous heading 0 -> (sin, cos) = (0, 1)
        ldx = Gdx * (1.0f - rk);
        ldy = Gdy * (1.0f - rk);
        const float rj[4] = {1.0f, 0.5f, 1.0f / 3.0f, 0.25f};
        float pw = 1.0f, kap = 0.0f, dkap = 0.0f, pwm1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gc[j] += Gth * (pw * sk) * rj[j] + gka * pw;
          kap += c[j] * pw;
          dkap += (float)j * c[j] * pwm1;
          pwm1 = pw;
          pw = pw * sk;
        }
        gsk += Gth * kap + gka * dkap;
        g_s += gsk * tau;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();               // the tile is overwritten by the next chunk
  }
  const float PM[4][4] = {{1.0f, 0.0f, 0.0f, 0.0f},
                          {-11.0f / 2, 9.0f, -9.0f / 2, 1.0f},
                          {9.0f, -45.0f / 2, 18.0f, -9.0f / 2},
                          {-9.0f / 2, 27.0f / 2, -27.0f / 2, 9.0f / 2}};
  float inv = 1.0f;
  float gq[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int m = 0; m < 4; ++m) gq[m] += gc[r] * PM[r][m] * inv;
    g_s += -(float)r * c[r] / slen * gc[r];
    inv = inv / slen;
  }
  if (lane < nvalid) {
    float* grow = a.gx0u + (b0 + lane) * 5;
#pragma unroll
    for (int m = 0; m < 4; ++m) grow[m] = gq[m];
    grow[4] = g_s;
  }
}

// ---- K4: the same reverse sweeps with the memory machinery of the forward roll-out (T <= 50) ---------------------
// The park kernel above touches HBM through per-lane strided dwords (measured 0.5-0.9 TB/s at T = 50).  Here:
//  * input rows: whole-tile LDS-DMA, the 2T controls of a trajectory live in registers (as in rollout.hip);
//  * no [T][3][64] park: the forward pass keeps a CHECKPOINT of the few state components the adjoint needs every
//    G = 10 steps (15 registers); the reverse pass re-runs one 10-step segment at a time into registers
//    (exactly the forward's values: same step function) and sweeps it backwards;
//  * the segment's seeds gstates[b, t0 .. t0+G, :] (G*S floats per row) are fetched as aligned 16-byte pieces by
//    the whole wave into an LDS tile and read back per row;
//  * the control gradients overwrite the controls IN PLACE in the registers -- the arrays rotate circularly by G
//    per segment so that every access has a static register index and the gradients end in natural order -- and
//    leave with the state cotangent as ONE contiguous tile through LDS (whole 128-byte lines, non-temporal).
typedef const __attribute__((address_space(1))) void* vgptr_t;
typedef __attribute__((address_space(3))) void* vlptr_t;
typedef float vf4 __attribute__((ext_vector_type(4)));

struct RollVjp2Args {
  const float* __restrict__ x0u;      // [B][L]
  const float* __restrict__ gstates;  // [B][T][S]
  float* __restrict__ gx0u;           // [B][L]
  long B;
  int T, L, wlds, dma_ok;
  float tie;
  DynParams dp;
};

constexpr int kVjpWaves = 2, kVjpRPP = 16;
constexpr int vjp_group(int TCH) { return TCH >= 10 ? 5 : TCH; }
// a row's seed chunk (G*S floats + up to 3 in front for the 16-byte alignment) as NPC 16-byte pieces; the tile is filled by
// LDS-DMA, so a row is NPC * 4 floats and NPC is odd (rows of an even number of pieces would fall on 4 or 8 banks)
constexpr int vjp_pieces(int S, int G) { return ((G * S + 6) / 4) | 1; }
constexpr int vjp_pitch(int S, int G) { return 4 * vjp_pieces(S, G); }

template <int MODE, int TCH>
__global__ __launch_bounds__(64 * kVjpWaves, 2) void rollout_vjp_regs_kernel(const RollVjp2Args a) {
  extern __shared__ float lds[];
  constexpr int S = ModeTraits<MODE>::S, S0 = ModeTraits<MODE>::S0, NP = ModeTraits<MODE>::NP;
  constexpr int G = vjp_group(TCH), NG = TCH / G;
  constexpr int PITCH = vjp_pitch(S, G);
  constexpr int NPC = vjp_pieces(S, G);          // 16-byte pieces of a row's aligned seed chunk
  constexpr int RPP = kVjpRPP;
  static_assert(TCH % G == 0, "whole groups");
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long b0 = ((long)blockIdx.x * kVjpWaves + wave) * kWave;
  if (b0 >= a.B) return;
  const long left = a.B - b0;
  const int nvalid = left < kWave ? (int)left : kWave;
  const int T = a.T, L = a.L;
  float* tile = lds + (size_t)wave * a.wlds;
  float* mine = tile + lane * PITCH;
  auto lds_drain = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  };
  const bool dma = nvalid == kWave && a.dma_ok;

  // ---- prologue: my row -> registers ---------------------------------------------------------------------------
  float q0[S0], ua[TCH], us[TCH];
#pragma unroll
  for (int t = 0; t < TCH; ++t) { ua[t] = 0.0f; us[t] = 0.0f; }
  if (dma) {
#pragma unroll 1
    for (int p = 0; p < kWave / RPP; ++p) {
      const float* src = a.x0u + (b0 + (long)p * RPP) * L;
      const int nf = RPP * L;
      for (int v = lane * 4; v < nf; v += 256)
        __builtin_amdgcn_global_load_lds((vgptr_t)(src + v), (vlptr_t)(tile + (v - lane * 4)), 16, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      if ((lane / RPP) == p) {
        const float* rr = tile + (lane % RPP) * L;
#pragma unroll
        for (int i = 0; i < S0; ++i) q0[i] = rr[i];
#pragma unroll
        for (int t = 0; t < TCH; ++t) { ua[t] = rr[S0 + t]; us[t] = rr[S0 + T + t]; }     // slots t >= T are never used
      }
      lds_drain();
    }
  } else {
    const float* row = a.x0u + (b0 + (lane < nvalid ? lane : nvalid - 1)) * L;
#pragma unroll
    for (int i = 0; i < S0; ++i) q0[i] = row[i];
#pragma unroll
    for (int t = 0; t < TCH; ++t)
      if (t < T) { ua[t] = row[S0 + t]; us[t] = row[S0 + T + t]; }
  }
  float s[S];
  roll_init<MODE>(q0, s);
  [[maybe_unused]] float cur = 0.0f;
  if constexpr (MODE == IRBFN_ROLLOUT_FRENET_LS) cur = s[7];

  const float* gs_tile = a.gstates + b0 * (long)T * S;
  const long rs = (long)T * S;
  const int g4 = (int)((reinterpret_cast<uintptr_t>(gs_tile) >> 2) & 3);
  // The seeds of a group are requested ONE GROUP AHEAD by LDS-DMA (global_load_lds_dwordx4, gathered 16-byte pieces: no
  // staging VGPRs) into the other of two row tiles: fetched at the top of the group that needs them they cost half the
  // kernel (157 us without the seeds against 315 us with them, at B = 262144, T = 50) -- the latency of a dependent
  // global -> register -> LDS round trip per group with two waves per SIMD to hide it.
  float* tile2 = tile + kWave * PITCH;
  auto request = [&](int gq, float* dst) {       // seeds of group gq -> dst (asynchronous; retired by vmcnt)
    const int tq = gq * G;
    const int nq = (T - tq) < G ? (T - tq) : G;
    int ln = lane;
    // NP = 5 (ST_SELECT): the NPC piece addresses, loop-invariant up to tq, were hoisted out of pass 2 into 34 VGPRs the sweeps
    // have no room for, and came back from scratch in every group.  Opaque lane: they are computed where they are used
    // (a dozen integer instructions per piece and group).
    if constexpr (NP > 4) asm volatile("" : "+v"(ln));
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int idx = j * kWave + (NP > 4 ? ln : lane);      // the other modes: `lane` itself, their code as it was
      const int r = idx / NPC, part = idx - r * NPC;
      const int C = (g4 + (int)((r * rs + (long)tq * S) & 3)) & 3;
      const float* src = gs_tile + r * rs + (long)tq * S - C + 4 * part;        // 16-byte aligned, inside the tile
      if (4 * part < C + nq * S)
        __builtin_amdgcn_global_load_lds((vgptr_t)src, (vlptr_t)(dst + j * 256), 16, 0, 0);
    }
  };
  const int g_last = (T - 1) / G;                // the last group with steps
  int cbuf = 0;
  if (dma) request(g_last, tile);                // in flight during the whole forward pass

  // ---- pass 1: forward, one checkpoint per group; the arrays (and the checkpoint list) rotate DOWN circularly:
  //      static register indices inside the rolled loop, natural order after NG groups
  float ck[NG][NP];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int i = 0; i < NP; ++i) ck[g][i] = 0.0f;
#pragma unroll 1
  for (int gI = 0; gI < NG; ++gI) {
    {
      float pk[NP];
      vjp_park<MODE>(s, pk);
#pragma unroll
      for (int g = 0; g + 1 < NG; ++g)
#pragma unroll
        for (int i = 0; i < NP; ++i) ck[g][i] = ck[g + 1][i];
#pragma unroll
      for (int i = 0; i < NP; ++i) ck[NG - 1][i] = pk[i];     // after the remaining rotations: group g at ck[g]
    }
#pragma unroll
    for (int tt = 0; tt < G; ++tt)
      if (gI * G + tt < T) roll_step<MODE>(s, ua[tt], us[tt], a.dp);
    if constexpr (NG > 1) {
      float ta[G], ts[G];
#pragma unroll
      for (int i = 0; i < G; ++i) { ta[i] = ua[i]; ts[i] = us[i]; }
#pragma unroll
      for (int i = 0; i + G < TCH; ++i) { ua[i] = ua[i + G]; us[i] = us[i + G]; }
#pragma unroll
      for (int i = 0; i < G; ++i) { ua[TCH - G + i] = ta[i]; us[TCH - G + i] = ts[i]; }
    }
  }

  // ---- pass 2: segments in reverse; the group's controls sit at [TCH - G, TCH) ---------------------------------
  float lam[S];
#pragma unroll
  for (int i = 0; i < S; ++i) lam[i] = 0.0f;
#pragma unroll 1
  for (int gI = NG - 1; gI >= 0; --gI) {
    const int t0 = gI * G;
    if (t0 < T) {                                // wave-uniform
      const int n = (T - t0) < G ? (T - t0) : G;
      float* cur_tile = cbuf ? tile2 : tile;
      const float* mine = cur_tile + lane * PITCH;
      const int myC = (g4 + (int)((lane * rs + (long)t0 * S) & 3)) & 3;
      if (dma) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this group's seeds have landed
        __builtin_amdgcn_wave_barrier();
        if (gI > 0) request(gI - 1, cbuf ? tile : tile2);    // the other tile was last read two groups ago
      } else {
        const float* src = gs_tile + (lane < nvalid ? lane : nvalid - 1) * rs + (long)t0 * S;
        float* d = cur_tile + lane * PITCH + myC;
        for (int i = 0; i < n * S; ++i) d[i] = src[i];
      }
      cbuf ^= 1;
      lds_drain();
      // re-run the segment from its checkpoint: pre-step quantities of every step into registers
      float ss[S], park[G][NP], pk[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) pk[i] = ck[NG - 1][i];
#pragma unroll
      for (int i = 0; i < S; ++i) ss[i] = 0.0f;
      if constexpr (MODE == IRBFN_ROLLOUT_FRENET_LS) { ss[1] = pk[0]; ss[2] = pk[1]; ss[3] = pk[2]; ss[6] = pk[3]; ss[7] = cur; }
      else if constexpr (MODE == IRBFN_ROLLOUT_ST_SELECT) { ss[2] = pk[0]; ss[3] = pk[1]; ss[4] = pk[2]; ss[5] = pk[3]; ss[6] = pk[4]; }
      else { ss[2] = pk[0]; ss[3] = pk[1]; ss[4] = pk[2]; }
#pragma unroll
      for (int tt = 0; tt < G; ++tt) {
        vjp_park<MODE>(ss, park[tt]);
        if (tt < n) roll_step<MODE>(ss, ua[TCH - G + tt], us[TCH - G + tt], a.dp);
      }
#pragma unroll
      for (int tt = G - 1; tt >= 0; --tt) {
        if (tt < n) {
#pragma unroll
          for (int i = 0; i < S; ++i) lam[i] += mine[myC + tt * S + i];
          float ga, gsv;
          vjp_back_step<MODE>(park[tt], ua[TCH - G + tt], us[TCH - G + tt], lam, cur, a.tie, a.dp, ga, gsv);
          ua[TCH - G + tt] = ga;                 // the control is dead from here on: its slot takes the gradient
          us[TCH - G + tt] = gsv;
        }
      }
      lds_drain();
    }
    if constexpr (NG > 1) {                      // rotate UP circularly: the next (earlier) group moves to [TCH - G, TCH)
#pragma unroll
      for (int g = NG - 1; g > 0; --g)
#pragma unroll
        for (int i = 0; i < NP; ++i) ck[g][i] = ck[g - 1][i];
      float ta[G], ts[G];
#pragma unroll
      for (int i = 0; i < G; ++i) { ta[i] = ua[TCH - G + i]; ts[i] = us[TCH - G + i]; }
#pragma unroll
      for (int i = TCH - 1; i >= G; --i) { ua[i] = ua[i - G]; us[i] = us[i - G]; }
#pragma unroll
      for (int i = 0; i < G; ++i) { ua[i] = ta[i]; us[i] = ts[i]; }
    }
  }
  // cotangent of the initial state
  float g0[S0];
  roll_init_grad<MODE>(q0, lam, a.tie, g0);

  // ---- epilogue: gradient rows -> HBM, RPP rows per pass as one contiguous block of whole lines -----------------
  float* gout = a.gx0u + b0 * L;
  if (dma) {
#pragma unroll 1
    for (int p = 0; p < kWave / RPP; ++p) {
      if ((lane / RPP) == p) {
        float* rr = tile + (lane % RPP) * L;
#pragma unroll
        for (int i = 0; i < S0; ++i) rr[i] = g0[i];
#pragma unroll
        for (int t = 0; t < TCH; ++t)
          if (t < T) { rr[S0 + t] = ua[t]; rr[S0 + T + t] = us[t]; }
      }
      lds_drain();
      float* dst = gout + (long)p * RPP * L;
      const int nf = RPP * L;                    // multiple of 4 floats; dst is 16-byte aligned
      for (int v = lane * 4; v < nf; v += 256) {
        const vf4 val = *reinterpret_cast<const vf4*>(tile + v);
        __builtin_nontemporal_store(val, reinterpret_cast<vf4*>(dst + v));
      }
      lds_drain();
    }
  } else if (lane < nvalid) {
    float* grow = gout + (long)lane * L;
#pragma unroll
    for (int i = 0; i < S0; ++i) grow[i] = g0[i];
#pragma unroll
    for (int t = 0; t < TCH; ++t)
      if (t < T) { grow[S0 + t] = ua[t]; grow[S0 + T + t] = us[t]; }
  }
}

template <int MODE>
static int launch_vjp_regs(const RollVjpArgs& v, hipStream_t s) {
  constexpr int S = ModeTraits<MODE>::S;
  RollVjp2Args a;
  a.x0u = v.x0u; a.gstates = v.gstates; a.gx0u = v.gx0u; a.B = v.B; a.T = v.T; a.L = v.L;
  a.tie = v.tie; a.dp = v.dp;
  const int TCH = a.T <= 8 ? 8 : 50;
  const int G = vjp_group(TCH);
  long w = (TCH / G > 1 ? 2L : 1L) * kWave * vjp_pitch(S, G);     // two seed tiles where there is a next group to prefetch
  if ((long)kVjpRPP * a.L > w) w = (long)kVjpRPP * a.L;
  a.wlds = (int)((w + 3) & ~3L);
  a.dma_ok = ((reinterpret_cast<uintptr_t>(a.x0u) | reinterpret_cast<uintptr_t>(a.gstates) | reinterpret_cast<uintptr_t>(a.gx0u)) & 15) == 0;
  const size_t lds = (size_t)kVjpWaves * a.wlds * sizeof(float);
  if (lds > 64 * 1024) return IRBFN_ERR_UNSUPPORTED;
  const long waves = (a.B + kWave - 1) / kWave;
  const dim3 grid((unsigned)((waves + kVjpWaves - 1) / kVjpWaves)), block(kWave * kVjpWaves);
  if (TCH == 8) hipLaunchKernelGGL((rollout_vjp_regs_kernel<MODE, 8>), grid, block, lds, s, a);
  else hipLaunchKernelGGL((rollout_vjp_regs_kernel<MODE, 50>), grid, block, lds, s, a);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

template <int MODE>
static int launch_vjp_park(const RollVjpArgs& a, hipStream_t s) {
  const size_t lds = (size_t)a.T * ModeTraits<MODE>::NP * kWave * sizeof(float);
  if (lds > 150 * 1024) return IRBFN_ERR_UNSUPPORTED;
  return launch_kernel<rollout_vjp_park_kernel<MODE>>(dim3((unsigned)((a.B + kWave - 1) / kWave)), dim3(kWave), lds, s, a);
}

// K4 up to T = 50, the park kernel beyond
template <int MODE>
static int launch_vjp_mode(const RollVjpArgs& a, hipStream_t s) {
  if (a.T <= 50) {
    const int rc = launch_vjp_regs<MODE>(a, s);
    if (rc != IRBFN_ERR_UNSUPPORTED) return rc;
  }
  return launch_vjp_park<MODE>(a, s);
}

// ST_SELECT with the mask V > 3 held constant (rollout_adjoint.h): the same two kernels; the park kernel's LDS bound gives
// T <= 120 at NP = 5
int launch_rollout_vjp_select(const float* x0u, const DynParams& dp, const float* gstates, float* g_x0u, int64_t B, int T,
                              float clip_tie, hipStream_t s) {
  constexpr int MODE = IRBFN_ROLLOUT_ST_SELECT;
  if (B == 0) return IRBFN_OK;
  if (T == 0) {
    IRBFN_HIP_CHECK(hipMemsetAsync(g_x0u, 0, (size_t)B * ModeTraits<MODE>::S0 * sizeof(float), s));
    return IRBFN_OK;
  }
  RollVjpArgs a;
  a.x0u = x0u; a.gstates = gstates; a.gx0u = g_x0u; a.B = (long)B; a.T = T;
  a.L = rollout_input_dim(MODE, T); a.tie = clip_tie; a.dp = dp;
  return launch_vjp_mode<MODE>(a, s);
}

int launch_rollout_vjp(int mode, const float* x0u, const DynParams& dp, const float* gstates,
                       float* g_x0u, int64_t B, int T, float clip_tie, hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  // ST_SELECT: the reference never differentiates it (SURVEY B-5); launch_rollout_vjp_select is this project's own adjoint
  if (mode == IRBFN_ROLLOUT_ST_SELECT || rollout_state_dim(mode) < 0) return IRBFN_ERR_UNSUPPORTED;
  if (T == 0) {                                  // no step: the rows are the initial states, and nothing depends on them
    IRBFN_HIP_CHECK(hipMemsetAsync(g_x0u, 0, (size_t)B * mode_dims(mode).S0 * sizeof(float), s));
    return IRBFN_OK;
  }
  RollVjpArgs a;
  a.x0u = x0u; a.gstates = gstates; a.gx0u = g_x0u; a.B = (long)B; a.T = T;
  a.L = rollout_input_dim(mode, T); a.tie = clip_tie; a.dp = dp;
  switch (mode) {
    case IRBFN_ROLLOUT_ST_KS: return launch_vjp_mode<IRBFN_ROLLOUT_ST_KS>(a, s);
    case IRBFN_ROLLOUT_FULLINT: return launch_vjp_mode<IRBFN_ROLLOUT_FULLINT>(a, s);
    case IRBFN_ROLLOUT_FRENET_LS: return launch_vjp_mode<IRBFN_ROLLOUT_FRENET_LS>(a, s);
    default: break;
  }
  if (T > 256) return IRBFN_ERR_UNSUPPORTED;     // the spiral: 37 KB of LDS at N = 256
  const size_t lds = ((size_t)kWave * kSpiralPitch + (size_t)((T + kSpiralG - 1) / kSpiralG) * 3 * kWave) * sizeof(float);
  hipLaunchKernelGGL(rollout_vjp_spiral_staged, dim3((unsigned)((B + kWave - 1) / kWave)), dim3(kWave), lds, s, a);
  IRBFN_HIP_CHECK(hipGetLastError());
  return IRBFN_OK;
}

}  // namespace irbfn
