// K1g's narrow kernel body (rbf_forward_gram.hip: the description of the scheme), shared by the one-region instances
// (rbf_fwd_f16gram / rbf_tick_f16gram, GAMMA = false) and the instances for nets evaluated with caller-provided region weights
// gamma[B][R] (rbf_forward_gram_gamma.hip, GAMMA = true).
#pragma once

#include "rbf_forward_gram.h"

namespace irbfn {

// GAMMA: the region weights of the call.  The chunk range is R regions of cpr = ceil(K / 32) chunks each (a region's last chunk
// padded with centres that contribute exactly 0: pack_all.hip), chunk c belongs to region c / cpr.
struct GramGamma {
  const float* __restrict__ gamma;        // [B][R]
  int R, cpr;
};

// ---- kernel ----------------------------------------------------------------------------------------------
template <int DC, int BC, bool ROLL, bool GAMMA = false>
__device__ __forceinline__ void gram_body(const GramArgs& ga, const F16Roll& rl, int mode, unsigned char* lds,
                                          [[maybe_unused]] const GramGamma gm = GramGamma{nullptr, 1, 1}) {
  static_assert(DC <= kGramDims, "eight coordinate slots");
  const F16Args& a = ga.f;
  constexpr int CBL = f16_chunk_bytes(DC);                   // K1h's chunk image (the VALU path reads its records)
  constexpr int CB = kGramChunkBytes;                        // what a ring slot holds of a chunk image
  constexpr int CST = gram_chunk_stride(1);                  // chunk image to chunk image in memory (K2g's records lie between)
  const int tid = threadIdx.x, lane = tid & 63;
  IRBFN_GRAM_PHASE(GP_ENTRY);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = a.S, QG = a.QG;
  // slice = wave / QG, qg = wave % QG (the QG waves of a slice are adjacent and share its ring) without a division: S <= 7
  // (gram_geometry), so seven scalar compares
  int slice = 0;
#pragma unroll
  for (int s2 = 1; s2 < 8; ++s2) slice += wave >= s2 * QG ? 1 : 0;
  const int qg = wave - slice * QG;
  const int g = lane >> 4, n = lane & 15;
  const long q0 = ((long)blockIdx.x * QG + qg) * 32;
  const GramHdr* hp = ga.hdr;
  long qrow[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    long q = q0 + t * 16 + n;
    q = q < a.B ? q : a.B - 1;
    qrow[t] = q < 0 ? 0 : q;
  }
  // ---- query-side operands: B[k = slot][column = query].  Every x load of the lane -- the operands' four and, in the slice-0
  // waves, the gate's -- is issued before the first of them is waited for.
  float xop[2][2], rop[2];
  gram_query_loads<DC>(a, hp, qrow, g, xop, rop);
  // ---- smooth region gate of the single region (model.py:42-95), one value per query: evaluated here by the slice-0 waves from
  // region 0's row of the tables (GateRow, with the kernel arguments) and parked in an LDS tile of QG x 32 floats BEHIND the rings
  // (the rings are overwritten during the steps, and the kernel has no vector register to spare across them); the tail reads
  // the two values of a lane back.  A wave reads what its own lanes wrote: no barrier.
  [[maybe_unused]] float* gpark = reinterpret_cast<float*>(lds + (size_t)S * kGramRing * CB) + qg * 32;
  if constexpr (!GAMMA) {
    if (slice == 0) {
      const GateRow& gr = ga.g0;
      float xg[2][DC];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int d = 0; d < DC; ++d) xg[t][d] = a.x[qrow[t] * a.Dreal + (d < gr.nsplit ? d : 0)];   // nsplit <= Dreal: inside the row
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float gv = gr.n_ranges > 0 ? 1.0f : 0.0f;            // model.py:70
#pragma unroll
        for (int d = 0; d < DC; ++d)
          if (d < gr.nsplit && gr.n_ranges > 0) gv *= gate_factor(xg[t][d], gr.lo[d], gr.hi[d], gr.delta[d]);
        if (g == 0) gpark[t * 16 + n] = gv;
      }
    }
  }
  h8_t bq[2][2];
  const bool bad = gram_query_operands_fold<DC>(a, hp, xop, rop, g, bq);
  // wave-uniform: the VALU distances for these 32 queries (through readfirstlane, which tells the compiler so)
  const bool wave_bad = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(bad) != 0ull ? 1 : 0) != 0;
#ifdef IRBFN_GRAM_STAMPS
  asm volatile("" ::"s"((int)wave_bad), "v"(bq[1][0]), "v"(bq[1][1]));
#endif
  IRBFN_GRAM_PHASE(GP_OPERANDS);

  // chunks [c0, c1) of the slice in 32-bit arithmetic: nchunks * S < 2^31 (checked where the plan is made)
  const unsigned nch = (unsigned)a.nchunks;
  const int c0 = (int)(nch * (unsigned)slice / (unsigned)S), c1 = (int)(nch * (unsigned)(slice + 1) / (unsigned)S);
  const int na = c1 - c0;
  const int nsteps = ga.nsteps;                              // every wave of the block walks the longest slice (barriers): gram_fill_args
  // Ring of kGramRing chunk images per slice: during step i the waves read the distance operands of chunk i + 1 and the W
  // operands of chunk i while later chunks land (end_of_step below).
  unsigned char* ring = lds + (size_t)slice * kGramRing * CB;
  constexpr int NVI = CB / 1024;                             // 6 wave-instructions per chunk image
  // The one-region instances carry the address of their refills: a wave requests pieces qg, qg + QG, ... of every chunk image of
  // its slice, and the chunks are staged in order (k = 0, 1, 2, ... from the prologue on), so gnext is the lane's 16 bytes of piece
  // qg of the NEXT chunk to stage, advanced by one image per staged chunk: one 64-bit add per chunk where the address built from k
  // costs a 64-bit multiply-add per chunk and an add per piece.  Past the slice (k >= na) nothing is staged, and nothing after it
  // either: the pointer stays.  The GAMMA instances, which have no register to spare (they spill already), build it from k.
  [[maybe_unused]] int npc = 0;                              // pieces of a chunk image this wave requests
#pragma unroll
  for (int p = 0; p < NVI; ++p) npc += qg + p * QG < NVI ? 1 : 0;
  [[maybe_unused]] const unsigned char* gnext = ga.gimg + (size_t)c0 * CST + qg * 1024 + lane * 16;
  auto stage = [&](int k, int buf) __attribute__((always_inline)) {   // chunk c0 + k of the slice -> ring slot buf; the QG waves share the copy
    if (k >= na) return;
    unsigned char* dst = ring + buf * CB;
    if constexpr (GAMMA) {
      const unsigned char* gp = ga.gimg + (size_t)(c0 + k) * CST + lane * 16;
      for (int v = qg; v < NVI; v += QG)
        __builtin_amdgcn_global_load_lds((gptr_t)(gp + v * 1024), (lptr_t)(dst + v * 1024), 16, 0, 0);
    } else {
      // piece qg from the pointer itself; QG < 6: the further pieces in a rolled loop, one add each as before (unrolled to
      // all pieces with their LDS addresses as constants the ten-step trip wants 70 scalar registers and spills them)
      if (npc > 0) {
        const unsigned char* gp = gnext;
        unsigned char* lp = dst + qg * 1024;
        __builtin_amdgcn_global_load_lds((gptr_t)gp, (lptr_t)lp, 16, 0, 0);
        for (int p = 1; p < npc; ++p) {
          gp += QG * 1024;
          lp += QG * 1024;
          __builtin_amdgcn_global_load_lds((gptr_t)gp, (lptr_t)lp, 16, 0, 0);
        }
      }
      gnext += CST;
    }
  };
  auto step_barrier = [&]() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  auto next3 = [&](int b3) { return b3 == kGramRing - 1 ? 0 : b3 + 1; };
  // A step touches chunks i (W) and i + 1 (distance operands).  One barrier per kGramPer = (kGramRing - 1) / 2 steps: behind it chunks
  // i + 1 .. i + kGramPer + 1 are resident and the next kGramPer are requested into the slots of the chunks everybody has left
  // (kGramRing = 3: a barrier per chunk; 5: one per two chunks).
  constexpr int kGramPer = (kGramRing - 1) / 2;
  static_assert(kGramRing == 2 * kGramPer + 1 && kGramPer >= 1, "ring = 2 x (steps per barrier) + 1");
  // GAMMA: the lane's two region weights (one per query tile: the lane owns query n of both) are multiplied onto the 16 basis
  // values of a step in front of the hi / lo split, so a chunk's contribution to both accumulators carries gamma of its region.
  // |gamma| <= 1 keeps the products inside the f16 range of the split.  gamma rows lie R floats apart, so the weights travel as the
  // chunk images do: behind each step barrier every wave requests, by one LDS-DMA dword per lane, the weights of its 32 queries
  // for the kGramPer steps of the period after the next (lane = 32 x step-in-period + query) into its own double-buffered tile
  // behind the rings; the vmcnt(0) of the following barrier, which the ring's copies need anyway, covers them, and a step reads its
  // two values from LDS: no step waits for a load it has just issued, and no register is the target of a load in flight.
  [[maybe_unused]] float* gtile = nullptr;                   // [2 periods][kGramPer <= 2 steps][32 queries] of this wave
  [[maybe_unused]] const float* grow = nullptr;              // gamma row of the wave's first query (wave-uniform)
  [[maybe_unused]] int glim = 0;                             // rows of the batch behind it, at most 31
  if constexpr (GAMMA) {
    static_assert(kGramPer <= 2, "a period's weights are one dword per lane");
    gtile = reinterpret_cast<float*>(lds + (size_t)S * kGramRing * CB) + wave * 128;
    const long qb = q0 < a.B ? q0 : a.B - 1;                 // the rows past the batch read the last row (as qrow)
    grow = gm.gamma + qb * (long)gm.R;
    glim = a.B - 1 - qb < 31 ? (int)(a.B - 1 - qb) : 31;
  }
  auto gamma_stage = [&](int period) {                       // the weights of steps period * kGramPer + (0, 1)
    if constexpr (GAMMA) {
      // no request past the block's last step: the epilogue reuses this LDS, and no barrier would wait for the copy
      if (period * kGramPer >= nsteps) return;
      // the lane's number from the execution mask, its row offset recomputed per request: nothing of this lives in a vector
      // register across the steps (the kernel has none to spare)
      int l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      asm volatile("" : "+v"(l));
      const int st = period * kGramPer + ((l >> 5) < kGramPer ? (l >> 5) : kGramPer - 1);
      int reg = (c0 + st) / gm.cpr;                          // chunk c belongs to region c / cpr; past the slice: any valid region
      reg = reg < gm.R ? reg : gm.R - 1;
      const int ql = (l & 31) < glim ? (l & 31) : glim;
      __builtin_amdgcn_global_load_lds((gptr_t)(grow + (unsigned)(ql * gm.R + reg)), (lptr_t)(gtile + (period & 1) * 64), 4, 0, 0);
    }
  };
  [[maybe_unused]] float gcur[2] = {1.0f, 1.0f};
  auto gamma_read = [&](int i) {                             // step i's two weights
    if constexpr (GAMMA) {
      const float* gp = gtile + ((i / kGramPer) & 1) * 64 + (i % kGramPer) * 32 + n;
      gcur[0] = gp[0];
      gcur[1] = gp[16];
    }
  };

#ifdef IRBFN_GRAM_STAMPS
  unsigned long long t_refill = 0;                           // s_memtime behind the step barrier, 0 in a step without one
#endif
  // par = i % kGramPer, which the caller knows without a division
  auto end_of_step = [&](int i, int b0, int par) __attribute__((always_inline)) {
    if (par != kGramPer - 1) return;
    step_barrier();
#ifdef IRBFN_GRAM_STAMPS
    t_refill = IRBFN_GRAM_T();
#endif
#pragma unroll
    for (int j = 0; j < kGramPer; ++j) {
      int slot = b0 - (kGramPer - 1) + j;                    // slot of chunk i - (kGramPer - 1) + j
      slot = slot < 0 ? slot + kGramRing : slot;
      stage(i + kGramPer + 2 + j, slot);
    }
    gamma_stage(i / kGramPer + 2);                           // into the tile of the period that has just ended
  };

  f4_t acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};                // A1: ph * wh
  f4_t acl[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};                // A2: pls * wh + ph * wls
  // transcendental, hi / lo split and Phi x W of the 16 pairs in t16 with the W operands of chunk `buf`
  // (`l16`: the lane's 16 bytes at the start of the image, buf + lane * 16)
  auto products = [&](float (&t16)[16], const unsigned char* l16, auto pre) __attribute__((always_inline)) {
    const h8_t bh = *reinterpret_cast<const h8_t*>(l16 + kGramOpBytes);
    const h8_t bl = *reinterpret_cast<const h8_t*>(l16 + kGramOpBytes + kF16WBytes);
    pre(t16);                                                // P = 2^kPhiExp * phi for the step's 16 pairs
    if constexpr (GAMMA) {
#pragma unroll
      for (int j = 0; j < 16; ++j) t16[j] *= gcur[j >> 3];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      unsigned wh[4], wl[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) split_pair_mix(t16[t * 8 + 2 * jj], t16[t * 8 + 2 * jj + 1], wh[jj], wl[jj]);
      const h8_t ah = __builtin_bit_cast(h8_t, u4_t{wh[0], wh[1], wh[2], wh[3]});
      const h8_t al = __builtin_bit_cast(h8_t, u4_t{wl[0], wl[1], wl[2], wl[3]});
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc[t], 0, 0, 0);
      acl[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acl[t], 0, 0, 0);
      acl[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acl[t], 0, 0, 0);
    }
  };

#pragma unroll
  for (int k = 0; k <= kGramPer; ++k) stage(k, k);
  gamma_stage(0);
  step_barrier();                                            // the first kGramPer + 1 chunks are there
  IRBFN_GRAM_PHASE(GP_BARRIER1);
#pragma unroll
  for (int k = kGramPer + 1; k < kGramRing; ++k) stage(k, k);
  gamma_stage(1);
  IRBFN_GRAM_PHASE(GP_LOOP0);
  if (!wave_bad) {
    // the distances of chunk i + 1 are issued in front of the VALU work on chunk i: ua / ub hold them in turn
    f4_t ua[2][2], ub[2][2];
    if (na > 0) gram_distances(ring, lane, bq, ua);
    // trans16 is inline asm: the hazard recogniser does not see it read MFMA results.  In the loop the 8 distance MFMAs of the
    // next chunk lie in front of it; a slice of ONE chunk reads them right away: explicit wait states, once
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    [[maybe_unused]] unsigned long long tph[5] = {0, 0, 0, 0, 0};
    // The lane's base into the slice's ring (16-byte operand and W records).  The one-region instances hold it as a register the
    // compiler takes as given: with the slot a constant (below) every LDS read of a step is the base plus an immediate, at most
    // (kGramRing - 1) x 6144 + 5120 -- no vector add per read group.
    unsigned o16 = (unsigned)(slice * kGramRing * CB) + lane * 16;
    if constexpr (!GAMMA) asm volatile("" : "+v"(o16));
    const unsigned char* const r16 = lds + o16;
    static_assert((kGramRing - 1) * CB + kGramOpBytes + kF16WBytes + 16 <= 65536, "the offset field of ds_read has 16 bits");
    // step i: chunk i in ring slot b0, chunk i + 1 in the next slot; par = i % kGramPer; all: the caller knows i + 1 < na
    auto one_step = [&](int i, int b0, int par, f4_t (&ucur)[2][2], f4_t (&unxt)[2][2], bool all = false) __attribute__((always_inline)) {
      const int b1 = next3(b0);
      [[maybe_unused]] const unsigned long long t0 = IRBFN_GRAM_T();
      if (all || i + 1 < na) gram_distances_at(r16 + b1 * CB, bq, unxt);   // issued in front of the VALU work on chunk i
      if (all || i < na) {
        gamma_read(i);
        float t16[16];
        products(t16, r16 + b0 * CB, [&](float (&o)[16]) { trans16<BC>(ucur, o); });
      }
      [[maybe_unused]] const unsigned long long t2 = IRBFN_GRAM_T();
#ifdef IRBFN_GRAM_STAMPS
      t_refill = 0;
#endif
      end_of_step(i, b0, par);
      [[maybe_unused]] const unsigned long long t4 = IRBFN_GRAM_T();
#ifdef IRBFN_GRAM_STAMPS
      // the refill requests behind the barrier (address arithmetic and one LDS-DMA issue per piece) are stamped on their own
      const unsigned long long t3 = t_refill != 0 ? t_refill : t4;
      tph[1] += t2 - t0; tph[2] += t3 - t2; tph[3] += t4 - t3; tph[4] += 1;
#endif
    };
    static_assert(2 % kGramPer == 0, "a pair of steps is a whole number of barrier periods");
    int i = 0;
    // One-region instances: trips of kGramTrip = 2 x kGramRing steps.  After that many the ring slot is 0 again, ua / ub have the
    // roles of the first step and a barrier period has just ended, so the slot, the roles and the place in the period of each
    // step of a trip are constants.  A wave takes a trip only while its OWN slice reaches past it (i + kGramTrip < na), so the
    // steps of a trip ask for no chunk that is not there and carry no branch around their halves: two steps between barriers are
    // one block of straight code.  Which loop runs a step does not matter to the block: every wave passes the barrier of every
    // odd step either way.  (The GAMMA instances keep the rolled loop below for all their steps: the long trip costs them
    // spills.)
    if constexpr (!GAMMA) {
      constexpr int kGramTrip = 2 * kGramRing;
      for (; i + kGramTrip <= nsteps && i + kGramTrip < na; i += kGramTrip) {
#pragma unroll
        for (int j = 0; j < kGramTrip; j += 2) {
          one_step(i + j, j % kGramRing, j % kGramPer, ua, ub, true);
          one_step(i + j + 1, (j + 1) % kGramRing, (j + 1) % kGramPer, ub, ua, true);
        }
      }
    }
    // the steps that are left (the end of the slice, a short slice, the steps past a shorter slice), two per trip, from slot 0 on
    int b0 = 0;                                              // ring slot of chunk i
    for (; i < nsteps; i += 2) {
      one_step(i, b0, 0, ua, ub);
      b0 = next3(b0);
      if (i + 1 < nsteps) {
        one_step(i + 1, b0, 1 % kGramPer, ub, ua);
        b0 = next3(b0);
      }
    }
#ifdef IRBFN_GRAM_STAMPS
    if (blockIdx.x < 2 && tid == 0)
      for (int k = 0; k < 5; ++k) g_gram_stamps[blockIdx.x * 32 + k] = tph[k];
#endif
  } else {
    // a query of this wave lies outside the representable box (or is not finite): K1h's distances for its 32 queries,
    // same barriers and the same share of the copies
    int b0 = 0;
    for (int i = 0; i < nsteps; ++i) {
      if (i < na) {
        gamma_read(i);
        float t16[16];
        gram_valu_args<DC, BC, GAMMA>(a, qrow, g, reinterpret_cast<const float*>(a.img + (size_t)(c0 + i) * CBL), t16);
        products(t16, ring + b0 * CB + lane * 16, [&](float (&o)[16]) { trans_block<BC, 16>(o); });
      }
      end_of_step(i, b0, i % kGramPer);
      b0 = next3(b0);
    }
  }
  IRBFN_GRAM_PHASE(GP_LOOP1);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = __builtin_fmaf(acl[t][r], kLoScale, acc[t][r]);   // A1 + 2^-11 A2

  // ---- the gate values parked by the prologue
  float gam[2] = {0.0f, 0.0f};
  if constexpr (GAMMA) {
    gam[0] = gam[1] = 1.0f;                                  // the region weights are inside the sums
  } else if (slice == 0) {
    gam[0] = gpark[n];
    gam[1] = gpark[16 + n];
  }
#ifdef IRBFN_GRAM_STAMPS
  asm volatile("" ::"v"(gam[0]), "v"(gam[1]));
#endif
  IRBFN_GRAM_PHASE(GP_GATE);
  narrow_epilogue<ROLL>(a, rl, mode, lds, acc, gam, S, slice, qg, q0, 1.0f / (gram_phi_scale<BC>() * kWScale));
  IRBFN_GRAM_PHASE(GP_STORED);
}

}  // namespace irbfn
