// K1g -- shared pieces of the matrix-core forward kernels that evaluate the squared distances as a Gram expansion
// (rbf_forward_gram.hip: narrow nets, the description of the scheme; rbf_forward_gram_wide.h: 16 < O <= 128): header of the
// expansion, slot tables, the query-side operands, the distance MFMAs, the VALU fallback, the 3-instruction operand split.
#pragma once

#include "rbf_forward_f16_narrow.h"

namespace irbfn {

typedef _Float16 h4_t __attribute__((ext_vector_type(4)));

constexpr int kGramOpBytes = 2 * 2 * 64 * 16;                    // [ct][operand][lane] 8 halfs: 4 KiB of distance operands per chunk
constexpr int gram_chunk_bytes(int NT = 1) { return kGramOpBytes + NT * 2 * kF16WBytes; }   // + W hi, W lo per column tile
constexpr int kGramChunkBytes = gram_chunk_bytes(1);                              // 6 KiB (narrow nets): what a ring slot holds
// K2g (rbf_vjp_gram.hip) keeps the unfolded form -- a 16x16x16 MFMA of the heads, two 16x16x32 of the tails -- and reads its
// centre-side records behind each chunk image: the forward kernels never copy them
constexpr int kGramHeadBytes = 2 * 64 * 8;                       // [ct][lane] 4 halfs
constexpr int kGramTailBytes = 2 * 2 * 64 * 16;                  // [ct][half][lane] 8 halfs
constexpr int kGramVjpBytes = kGramHeadBytes + kGramTailBytes;   // 5 KiB
constexpr int gram_chunk_stride(int NT = 1) { return gram_chunk_bytes(NT) + kGramVjpBytes; }   // chunk image to chunk image in memory
constexpr int kGramDims = 8;                                    // coordinates the slot tables hold (d <= 8: the Frenet nets have 8)
#ifndef IRBFN_GRAM_RING
#define IRBFN_GRAM_RING 5       // chunk images per centre slice in the LDS ring of the narrow kernel: 3 (a barrier per chunk) or 5 (one per two)
#endif
constexpr int kGramRing = IRBFN_GRAM_RING;
#ifndef IRBFN_GRAM_WAVES
#define IRBFN_GRAM_WAVES 4     // waves per SIMD the register allocation must allow
#endif

struct GramHdr {
  float r[8];                 // origin (midpoint of the centres' box)
  int ex, ec, eq, ea, e2;     // |x'_i| < 2^ex, |C| < 2^ec, Q < 2^eq, |alpha| < 2^ea, |c2| < 2^e2
  int ok;
  float cabs, amax, cmax, c2max;
};

// ---- the slot tables: which product sits in which k-slot ---------------------------------------------------------
// The forward kernels: two k = 32 operands per 16 x 16 tile (gram_fold_slot below).  K2g: the unfolded tables, which follow.
// A lane of an unfolded operand holds the slots of ONE lane group g = lane >> 4: head slots 4 g + j (j < 4), tail slots 32 hf + 8 g + j (j < 8).
// The products of coordinate i live with group i / 2 -- its head in head slot 4 (i / 2) + (i & 1), its five tail combinations in tail
// slots 32 (i & 1) + 8 (i / 2) + m -- so a lane of the query side splits just ITS two coordinates (gram_query_operands); the
// Q x alpha and 1 x c2 products fill free slots of the groups 0..2.  (Until round 3's last version the slots ran coordinate by
// coordinate across the groups: every lane split all eight coordinates and selected -- 700 instructions of prologue per wave.)
struct GramSlot { int kind, dim, p, q; };        // kind: 0 empty, 1 x'_dim part p x C part q, 2 Q part p x alpha part q, 3 1 x c2 part p
__host__ __device__ constexpr int gram_comb_p(int m) { return m == 0 ? 0 : (m == 1 ? 1 : (m == 2 ? 0 : (m == 3 ? 2 : 1))); }
__host__ __device__ constexpr int gram_comb_q(int m) { return m == 0 ? 1 : (m == 1 ? 0 : (m == 2 ? 2 : (m == 3 ? 0 : 1))); }
__host__ __device__ constexpr GramSlot gram_head_slot(int s) {
  const int g = s >> 2, j = s & 3;
  return j < 2 ? GramSlot{1, 2 * g + j, 0, 0}
               : (j == 2 ? (g == 0 ? GramSlot{2, 0, 0, 0} : (g == 1 ? GramSlot{3, 0, 0, 0} : (g == 2 ? GramSlot{3, 0, 1, 0} : GramSlot{0, 0, 0, 0})))
                         : GramSlot{0, 0, 0, 0});
}
__host__ __device__ constexpr GramSlot gram_tail_slot(int s) {
  const int hf = s >> 5, g = (s >> 3) & 3, j = s & 7;
  const int m = hf * 3 + (j - 5);                            // free slots of group 0: Q x alpha combinations 0..4, then the third c2 part
  return j < 5 ? GramSlot{1, 2 * g + hf, gram_comb_p(j), gram_comb_q(j)}
               : (g == 0 ? (m < 5 ? GramSlot{2, 0, gram_comb_p(m), gram_comb_q(m)} : GramSlot{3, 0, 2, 0})
                         : (g == 1 && hf == 0 && j == 5 ? GramSlot{3, 0, 3, 0} : GramSlot{0, 0, 0, 0}));
}
static_assert(kGramDims == 8, "four lane groups x two coordinates");

// The folded tables of the forward kernels: slot k of operand o (two v_mfma_f32_16x16x32_f16 per tile, the first with C = 0).
// A lane of group g holds k = 8 g + j (j < 8) of BOTH operands.
//   operand 0, k 0..15 (groups 0, 1): the eleven HEADS and nothing else.  The MFMA sums the eight products of a lane group
//     aligned to the group's largest and accumulates the groups in ascending k: two groups of fixed-point heads on one grid
//     inside the 2^24-unit budget are summed and accumulated exactly, and the tails behind them (groups 2, 3, then operand 1)
//     meet the CANCELLED head sum, as they did behind the 16x16x16 MFMA (tools/probe_mfma_accum.hip fold,
//     profiles/k1g_fold_heads.txt: a million tiles bit-identical to the unfolded form).
//   operand 0, k 16..31 and operand 1: the 47 tails.
// Group g splits coordinates 2 g and 2 g + 1 (gram_query_operands_fold).  Groups 0 / 1 keep their own two heads and take
// those of groups 2 / 3 (coordinates 4, 5 / 6, 7); their ten tails overflow their eight slots of operand 1 by the (1, 1)
// combinations, which groups 2 / 3 take in return: ONE exchange across lane ^ 32 per query tile.  Q is known to every lane (the
// butterfly), so Q x alpha and the c2 parts sit wherever a slot is free.
__host__ __device__ constexpr GramSlot gram_fold_slot(int o, int k) {
  const int g = k >> 3, j = k & 7;
  if (o == 0 && g < 2)
    return j < 2 ? GramSlot{1, 2 * g + j, 0, 0}
                 : (j < 4 ? GramSlot{1, 4 + 2 * g + (j - 2), 0, 0}
                          : (g == 0 ? (j == 4 ? GramSlot{2, 0, 0, 0} : GramSlot{0, 0, 0, 0})
                                    : (j == 4 ? GramSlot{3, 0, 0, 0} : (j == 5 ? GramSlot{3, 0, 1, 0} : GramSlot{0, 0, 0, 0}))));
  if (o == 0)                                                // groups 2, 3: coordinate 2 g, the (1, 1) tails of 2 (g - 2) and 2 (g - 2) + 1
    return j < 5 ? GramSlot{1, 2 * g, gram_comb_p(j), gram_comb_q(j)}
                 : (j < 7 ? GramSlot{1, 2 * (g - 2) + (j - 5), 1, 1} : (g == 2 ? GramSlot{3, 0, 3, 0} : GramSlot{0, 0, 0, 0}));
  if (g < 2) return GramSlot{1, 2 * g + (j >> 2), gram_comb_p(j & 3), gram_comb_q(j & 3)};      // four tails of each of its two
  if (j < 5) return GramSlot{1, 2 * g + 1, gram_comb_p(j), gram_comb_q(j)};
  const int m = (g - 2) * 3 + (j - 5);                       // Q x alpha combinations 0..4, then the third c2 part
  return m < 5 ? GramSlot{2, 0, gram_comb_p(m), gram_comb_q(m)} : GramSlot{3, 0, 2, 0};
}
// every product of the expansion exactly once, heads (p = q = 0; c2: p < 2) in k < 16 of operand 0 and nowhere else
__host__ __device__ constexpr bool gram_slot_is_head(const GramSlot sl) { return sl.kind == 3 ? sl.p < 2 : (sl.kind != 0 && sl.p + sl.q == 0); }
__host__ __device__ constexpr int gram_fold_count(int kind, int dim, int p, int q) {
  int c = 0;
  for (int o = 0; o < 2; ++o)
    for (int k = 0; k < 32; ++k) {
      const GramSlot sl = gram_fold_slot(o, k);
      c += (sl.kind == kind && sl.dim == dim && sl.p == p && sl.q == q) ? 1 : 0;
    }
  return c;
}
__host__ __device__ constexpr bool gram_fold_tables_ok() {
  int used = 0;
  for (int o = 0; o < 2; ++o)
    for (int k = 0; k < 32; ++k) {
      const GramSlot sl = gram_fold_slot(o, k);
      used += sl.kind != 0 ? 1 : 0;
      if (sl.kind != 0 && gram_slot_is_head(sl) != (o == 0 && k < 16)) return false;       // no head at k >= 16, no tail below
    }
  if (used != 8 * 6 + 6 + 4) return false;                   // nothing twice, given that everything below is there once
  for (int p = 0; p < 3; ++p)
    for (int q = 0; p + q < 3; ++q) {
      for (int d = 0; d < kGramDims; ++d)
        if (gram_fold_count(1, d, p, q) != 1) return false;
      if (gram_fold_count(2, 0, p, q) != 1) return false;
    }
  for (int p = 0; p < 4; ++p)
    if (gram_fold_count(3, 0, p, 0) != 1) return false;
  return true;
}
static_assert(gram_fold_tables_ok(), "folded slot tables");
// power-of-two weight of a slot's product and its split between the two operands (both kept near 2^(T/2))
__host__ __device__ inline int gram_T(const GramHdr& h, const GramSlot sl) {
  return sl.kind == 1 ? h.ex + h.ec - 11 * (sl.p + sl.q) : (sl.kind == 2 ? h.eq + h.ea - 11 * (sl.p + sl.q) : h.e2 - 11 * sl.p);
}
__host__ __device__ inline int gram_ax(int T) { return (T + 1) >> 1; }      // query-side exponent; centre side: T - ax

// The inverse multiquadric arrives as P = 2^7 phi here (K1h: 2^14 phi, argument 2^-28 (1 + t)): an argument scaled by 2^-28
// would push the tail operands of the expansion -- 2^-11 and 2^-22 of the heads -- below the f16 normal range.  2^7 phi is a
// normal f16 number down to phi = 2^-21, which an algebraically decaying basis does not reach.
template <int BC>
__host__ __device__ constexpr float gram_phi_scale() { return BC == BC_IMQ ? 128.0f : kPhiScale; }

// Diagnosis build only (tools/build_variant.py ... -DIRBFN_GRAM_STAMPS): wave 0 of blocks 0 and 1 add up s_memtime per
// phase of the step (words 0..4 of the block's 32) and stamp the phases of the launch (words 8 + k: s_memtime at kernel
// entry, query operands ready, first barrier passed, loop start, loop end, gate done, last store; words 16 / 17:
// s_memrealtime at entry and behind the last store); no output depends on it and the regular build contains none of it.
#ifdef IRBFN_GRAM_STAMPS
__device__ unsigned long long g_gram_stamps[64];
#define IRBFN_GRAM_T() __builtin_amdgcn_s_memtime()
// every load and LDS access issued so far has returned when the stamp is taken
#define IRBFN_GRAM_PHASE(k)                                                                            \
  do {                                                                                                 \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                        \
    if (blockIdx.x < 2 && threadIdx.x == 0) {                                                          \
      g_gram_stamps[blockIdx.x * 32 + 8 + (k)] = __builtin_amdgcn_s_memtime();                         \
      if ((k) == 0 || (k) == 6) g_gram_stamps[blockIdx.x * 32 + 16 + (k) / 6] = __builtin_amdgcn_s_memrealtime(); \
    }                                                                                                  \
  } while (0)
#else
#define IRBFN_GRAM_T() 0ull
#define IRBFN_GRAM_PHASE(k) do { } while (0)
#endif
enum GramPhase : int { GP_ENTRY = 0, GP_OPERANDS, GP_BARRIER1, GP_LOOP0, GP_LOOP1, GP_GATE, GP_STORED };

// ---- kernel ----------------------------------------------------------------------------------------------
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef unsigned u2_t __attribute__((ext_vector_type(2)));

// The (hi, lo) pair of f16_split.h in five instructions per value pair instead of eight: hi = the packed round-toward-zero
// conversion itself (the leading 11 bits of P wherever P is a normal f16 number), lo = 2^11 (P - hi) with the residual from one
// v_fma_mix_f32 per value that reads hi as the f16 number it is (exact: every term a multiple of the last bit of P).
// (v_pk_add_f32 / v_pk_mul_f32 for the subtraction and the gain: measured slower -- packed f32 VALU costs more than the two
// plain instructions it replaces, MI355X_MICROARCH.md constants table.  v_fma_mixlo_f16 + v_fma_mixhi_f16 writing the two halves of
// the lo pair directly -- 2 instructions instead of 3 -- measured 5 % SLOWER at config 2: 92.1 vs 87.4 us, profiles/r03_gram_experiments.txt.)
//
// The 2^11 gain of a value PAIR is one instruction: the residuals d = P - hi come out of the two v_fma_mix_f32 unscaled
// (fma(hi, -1, P): exact, the low bits of P) into an aligned register pair, and one v_lshl_add_u64 adds 11 to both exponent
// fields (bits(2048 d) = bits(d) + (11 << 23) for a normal d of either sign with room in the exponent; |d| < 2^4 here, so
// neither dword carries: the low one not into the high one).  Five instructions per pair instead of six (beside MFMAs the add
// costs 4.4 cycles per pair and SIMD, the two multiplies 8.4: tools/ubench.hip split, profiles/k1g_split_gain.txt; the inline
// constant of the mixes costs what their SGPR operand did).  The pair is bit-identical to the form with the two multiplies (ADD64 = false: q = 2048 P, then
// fma(hi, -2048, q)) for every P the kernels produce (tests/test_split_gain_cpu.py sweeps it):
//   - d == 0 (P has no bits below hi's last; P = +-0, where fma(-0, -1, -0) = +0 as fma(-0, -2048, -0) did): the add makes
//     2^-116 of +0, which the round-toward-zero conversion turns into the +0 the other form has;
//   - P subnormal or below 2^-103, where d is a subnormal float and the add does not scale it: both forms give a value
//     below 2^-115 with the sign of P, and the conversion its signed zero.
//   (Adding the gain to P in front of the mixes -- in place, P being dead behind the hi conversion -- costs the same five
//   instructions but turns P = -0, which the region-weighted instances produce (an underflowed basis value times a negative
//   weight), into -2^-116 and its lo into -0 where the multiplies give +0.)
// P infinite does not arise (the arguments of the reciprocal bases are >= 1, the exponential's are <= 14), and a NaN -- a
// NaN query, which takes the VALU distances -- stays a NaN in hi and so in its row's output, whatever the add makes of lo.
#ifndef IRBFN_SPLIT_ADD64
#define IRBFN_SPLIT_ADD64 1     // 0: the gain as two v_mul_f32 (A/B builds: tools/build_variant.py ... -DIRBFN_SPLIT_ADD64=0)
#endif
constexpr unsigned long long kLoGainBits2 = 0x0580000005800000ull;      // 11 << 23 in both dwords
template <bool ADD64 = (IRBFN_SPLIT_ADD64 != 0)>
__device__ __forceinline__ void split_pair_mix(float p0, float p1, unsigned& hi, unsigned& lo) {
  hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(p0, p1));
  if constexpr (ADD64) {
    float d0, d1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hi), "v"(p0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hi), "v"(p1));
    f2_t d = {d0, d1};
    // plain C++ (u64 + constant) may lower to v_add_co + v_addc_co: the instruction is named
    asm("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(d) : "s"(kLoGainBits2));
    lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(d[0], d[1]));
  } else {
    const float q0 = p0 * kLoGain, q1 = p1 * kLoGain;
    const float ng = -kLoGain;
    float d0, d1;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hi), "s"(ng), "v"(q0));
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hi), "s"(ng), "v"(q1));
    lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(d0, d1));
  }
}

// the step's 16 transcendentals back to back (rbf_forward.h, trans_block), from the MFMA result registers into fresh ones
template <int BC>
__device__ __forceinline__ void trans16(const f4_t (&u)[2][2], float (&o)[16]) {
#define IRBFN_T8(OP, T)                                                                                                          \
  asm volatile(OP " %0, %8\n " OP " %1, %9\n " OP " %2, %10\n " OP " %3, %11\n " OP " %4, %12\n " OP " %5, %13\n " OP " %6, %14\n " OP     \
               " %7, %15" IRBFN_T8_TAIL##T                                                                                       \
               : "=&v"(o[8 * T]), "=&v"(o[8 * T + 1]), "=&v"(o[8 * T + 2]), "=&v"(o[8 * T + 3]), "=&v"(o[8 * T + 4]),           \
                 "=&v"(o[8 * T + 5]), "=&v"(o[8 * T + 6]), "=&v"(o[8 * T + 7])                                                   \
               : "v"(u[T][0][0]), "v"(u[T][0][1]), "v"(u[T][0][2]), "v"(u[T][0][3]), "v"(u[T][1][0]), "v"(u[T][1][1]),           \
                 "v"(u[T][1][2]), "v"(u[T][1][3]));
#define IRBFN_T8_TAIL0 ""
#define IRBFN_T8_TAIL1 "\n s_nop 7"
  if constexpr (BC == BC_GAUSS) { IRBFN_T8("v_exp_f32_e32", 0) IRBFN_T8("v_exp_f32_e32", 1) }
  else if constexpr (BC == BC_IQ) { IRBFN_T8("v_rcp_f32_e32", 0) IRBFN_T8("v_rcp_f32_e32", 1) }
  else { IRBFN_T8("v_rsq_f32_e32", 0) IRBFN_T8("v_rsq_f32_e32", 1) }
#undef IRBFN_T8
#undef IRBFN_T8_TAIL0
#undef IRBFN_T8_TAIL1
}

struct GramArgs {
  F16Args f;                              // x, img = K1h's image (records of the VALU path), oscale, bias, out, gate, B, ...
  const unsigned char* __restrict__ gimg; // [nchunks][gram_chunk_stride]: a chunk's image, then K2g's records
  const GramHdr* __restrict__ hdr;
  GateRow g0;                             // the narrow kernels' gate: region 0's row by value, with the kernel arguments
  int nsteps;                             // chunks of the longest of the S slices: the steps every wave of a block walks
};

// |v| < 2^E given as vh + vl -> normalised parts (float), as gram_parts_d
__device__ __forceinline__ void gram_parts_f(float vh, float vl, float inv, float (&n)[3]) {
  const float a = vh * inv, b = vl * inv;                    // exact (power of two)
  n[0] = __builtin_rintf(a * 1024.0f) * (1.0f / 1024.0f);
  const float r1 = ((a - n[0]) + b) * 2048.0f;               // a - n0 is exact
  n[1] = (float)(_Float16)r1;
  const float r2 = (r1 - n[1]) * 2048.0f;
  n[2] = (float)(_Float16)r2;
}

// Query-side operands of the expansion for the wave's two query tiles (rows qrow[t] of x): B[k = slot][column = query (lane & 15)],
// a lane holding the slots of its group g = lane >> 4 (forward: 8 g + j of both operands, gram_query_operands_fold; K2g: 4 g + j
// of the head MFMA, 32 hf + 8 g + j of the tail MFMAs, gram_query_operands).  A lane splits the two coordinates 2 g and
// 2 g + 1 of its queries (gram_query_parts; the slot tables above put their products into its slots, but for the one exchange of
// the folded form); Q = |x'|^2 is summed in double-float
// over the four lanes that hold a query's coordinates (a commutative butterfly: the four lanes end with the same bits).  Returns
// whether THIS lane's coordinates fall outside the representable box (|x'_i| >= 2^ex, Q >= 2^eq, NaN, Inf) or the header says the
// net does not fit -- the callers take the ballot of the wave.
// The lane's four coordinates xv[t][c] (query tile t, coordinate 2 g + c; 0 past the net's dimension) come from gram_query_loads:
// one address per value, known at kernel entry, so the four loads -- and whatever else the caller loads between the two
// calls -- are in flight together and the operands wait once.
template <int DC>
__device__ __forceinline__ void gram_query_loads(const F16Args& a, const GramHdr* hp, const long (&qrow)[2], int g, float (&xv)[2][2],
                                                 float (&rv)[2]) {
  // the origin's two coordinates of the lane go out with the x loads (r holds eight entries: no branch around the load)
#pragma unroll
  for (int c = 0; c < 2; ++c) rv[c] = hp->r[2 * g + c];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int i = 2 * g + c;
      const bool in = i < DC && i < a.Dreal;
      const float v = a.x[qrow[t] * a.Dreal + (in ? i : 0)];  // always inside the row: no branch around the load
      xv[t][c] = in ? v : 0.0f;
    }
}

// the normalised parts of the lane's two coordinates (nx[t][c][part]) and of Q (nq[t][part]) for the two query tiles
template <int DC>
__device__ __forceinline__ bool gram_query_parts(const GramHdr* hp, const float (&xin)[2][2], const float (&rin)[2], int g,
                                                 float (&nx)[2][2][3], float (&nq)[2][3]) {
  // The error-free sums below are written operation by operation: contracted into FMAs (hipcc's default, -ffp-contract=fast:
  // th = qh + sh * sh as one fma, tb = th - qh as fma(-sh', sh', th) when qh is itself a product) they lose the low word of Q --
  // 6e-8 of |x'|^2, which the cancellation against 2 c'x' and |c'|^2 turns into 4e-5 of the result for a query 28 widths from
  // the origin of the expansion (tests/test_gpu_gram.py::test_gram_ill_conditioned_columns[outlier_far_centre])
#pragma clang fp contract(off)
  static_assert(DC <= kGramDims, "eight coordinate slots");
  const int ex = hp->ex, eq = hp->eq;
  bool bad = hp->ok == 0;
  const float xinv = __builtin_ldexpf(1.0f, -ex), qinv = __builtin_ldexpf(1.0f, -eq);
  const float xlim = __builtin_ldexpf(1.0f, ex) * 0.999f, qlim = __builtin_ldexpf(1.0f, eq) * 0.999f;
  float rr[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    rr[c] = (2 * g + c < DC) ? -rin[c] : 0.0f;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float qh = 0.0f, ql = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float xv = xin[t][c];
      const float sh = xv + rr[c];                           // TwoSum: x' = sh + sl exactly
      const float bb = sh - xv;
      const float sl = (xv - (sh - bb)) + (rr[c] - bb);
      bad = bad || !(__builtin_fabsf(sh) < xlim);            // NaN / Inf / outside the box
      gram_parts_f(sh, sl, xinv, nx[t][c]);
      const float ph = sh * sh;                              // Q += x'^2 in double-float
      const float pl = __builtin_fmaf(sh, sh, -ph) + 2.0f * sh * sl;
      const float th = qh + ph;
      const float tb = th - qh;
      ql += ((qh - (th - tb)) + (ph - tb)) + pl;
      qh = th;
    }
#pragma unroll
    for (int off = 16; off <= 32; off *= 2) {                // the other lane groups' coordinates
      const float oh = __shfl_xor(qh, off), ol = __shfl_xor(ql, off);
      const float th = qh + oh;
      const float tb = th - qh;
      ql = ((qh - (th - tb)) + (oh - tb)) + (ql + ol);
      qh = th;
    }
    bad = bad || !(qh < qlim);
    gram_parts_f(qh, ql, qinv, nq[t]);
  }
  return bad;
}

// K2g's operands (the unfolded tables): B[k = slot][column = query], slots 4 g + j of the head MFMA, 32 hf + 8 g + j of the tail MFMAs
template <int DC>
__device__ __forceinline__ bool gram_query_operands(const F16Args& a, const GramHdr* hp, const float (&xin)[2][2], const float (&rin)[2],
                                                    int g, h4_t (&bhd)[2], h8_t (&btl)[2][2]) {
  GramHdr hx;                                                // exponents only (gram_T)
  hx.ex = hp->ex; hx.ec = hp->ec; hx.eq = hp->eq; hx.ea = hp->ea; hx.e2 = hp->e2;
  auto scale_of = [&](const GramSlot sl) -> float { return sl.kind == 0 ? 0.0f : __builtin_ldexpf(1.0f, gram_ax(gram_T(hx, sl))); };
  float nxa[2][2][3], nqa[2][3];
  const bool bad = gram_query_parts<DC>(hp, xin, rin, g, nxa, nqa);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float (&nx)[2][3] = nxa[t];
    const float (&nq)[3] = nqa[t];
    // head slots 4 g + j: the two coordinates' heads, then (group 0) Q x alpha, (groups 1, 2) the two c2 heads
    {
      const float sc = scale_of(gram_head_slot(0));          // kind 1, p = q = 0: the same weight in every group
      const float f2 = g == 0 ? nq[0] * scale_of(gram_head_slot(2))
                              : (g == 1 ? scale_of(gram_head_slot(4 + 2)) : (g == 2 ? scale_of(gram_head_slot(8 + 2)) : 0.0f));
      bhd[t][0] = (_Float16)(nx[0][0] * sc);
      bhd[t][1] = (_Float16)(nx[1][0] * sc);
      bhd[t][2] = (_Float16)f2;
      bhd[t][3] = (_Float16)0.0f;
    }
    // tail slots 32 hf + 8 g + j: j < 5 the combinations of coordinate 2 g + hf; j >= 5: group 0 the Q x alpha combinations and
    // the third c2 part, group 1 (hf = 0, j = 5) the fourth
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const GramSlot sl = gram_tail_slot(32 * hf + j);     // group 0's entry: p, q and the weight do not depend on the group
        btl[t][hf][j] = (_Float16)(nx[hf][sl.p] * scale_of(sl));
      }
#pragma unroll
      for (int j = 5; j < 8; ++j) {
        const GramSlot s0 = gram_tail_slot(32 * hf + j), s1 = gram_tail_slot(32 * hf + 8 + j);
        const float v0 = s0.kind == 2 ? nq[s0.p] * scale_of(s0) : scale_of(s0);      // kind 3 / empty: the weight itself / 0
        const float v1 = scale_of(s1);                                                // kind 3 or empty
        btl[t][hf][j] = (_Float16)(g == 0 ? v0 : (g == 1 ? v1 : 0.0f));
      }
    }
  }
  return bad;
}

// The forward kernels' operands (gram_fold_slot): bq[t][o][j] = slot 8 g + j of operand o for query tile t.  A lane converts the
// parts of its own two coordinates; what its slots hold of another group's comes as one dword per tile from lane ^ 32:
// groups 2 / 3 send their two heads, groups 0 / 1 their two (1, 1) tails.
template <int DC>
__device__ __forceinline__ bool gram_query_operands_fold(const F16Args& a, const GramHdr* hp, const float (&xin)[2][2],
                                                         const float (&rin)[2], int g, h8_t (&bq)[2][2]) {
  typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
  GramHdr hx;                                                // exponents only (gram_T)
  hx.ex = hp->ex; hx.ec = hp->ec; hx.eq = hp->eq; hx.ea = hp->ea; hx.e2 = hp->e2;
  auto scale_of = [&](const GramSlot sl) -> float { return sl.kind == 0 ? 0.0f : __builtin_ldexpf(1.0f, gram_ax(gram_T(hx, sl))); };
  float nxa[2][2][3], nqa[2][3];
  const bool bad = gram_query_parts<DC>(hp, xin, rin, g, nxa, nqa);
  const bool lower = g < 2;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float (&nx)[2][3] = nxa[t];
    const float (&nq)[3] = nqa[t];
    const float sc0 = scale_of(GramSlot{1, 0, 0, 0}), sc11 = scale_of(GramSlot{1, 0, 1, 1});
    const h2_t mine = lower ? h2_t{(_Float16)(nx[0][1] * sc11), (_Float16)(nx[1][1] * sc11)}
                            : h2_t{(_Float16)(nx[0][0] * sc0), (_Float16)(nx[1][0] * sc0)};
    const h2_t theirs = __builtin_bit_cast(h2_t, __shfl_xor(__builtin_bit_cast(int, mine), 32));
    // the value of a slot as group gg has it, from this lane's parts (the select below keeps the lane's own group's)
    auto value = [&](const GramSlot sl, int gg) -> float {
      if (sl.kind == 0) return 0.0f;
      if (sl.kind == 2) return nq[sl.p] * scale_of(sl);
      if (sl.kind == 3) return scale_of(sl);
      return nx[sl.dim & 1][sl.p] * scale_of(sl);            // an own coordinate: dim = 2 gg or 2 gg + 1
    };
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        _Float16 v[4];
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const GramSlot sl = gram_fold_slot(o, 8 * gg + j);
          const bool foreign = sl.kind == 1 && (sl.dim >> 1) != gg;       // arrives from lane ^ 32, in the order it was packed
          v[gg] = foreign ? theirs[sl.dim & 1] : (_Float16)value(sl, gg);
        }
        bq[t][o][j] = g == 0 ? v[0] : (g == 1 ? v[1] : (g == 2 ? v[2] : v[3]));
      }
  }
  return bad;
}
template <int DC>
__device__ __forceinline__ bool gram_query_operands(const F16Args& a, const GramHdr* hp, const long (&qrow)[2], int g, h4_t (&bhd)[2],
                                                    h8_t (&btl)[2][2]) {
  float xv[2][2], rv[2];
  gram_query_loads<DC>(a, hp, qrow, g, xv, rv);
  return gram_query_operands<DC>(a, hp, xv, rv, g, bhd, btl);
}
template <int DC>
__device__ __forceinline__ bool gram_query_operands_fold(const F16Args& a, const GramHdr* hp, const long (&qrow)[2], int g, h8_t (&bq)[2][2]) {
  float xv[2][2], rv[2];
  gram_query_loads<DC>(a, hp, qrow, g, xv, rv);
  return gram_query_operands_fold<DC>(a, hp, xv, rv, g, bq);
}
// the tables say what the code above assumes
static_assert(gram_head_slot(0).kind == 1 && gram_head_slot(4 * 3 + 1).dim == 7 && gram_head_slot(2).kind == 2 && gram_head_slot(6).kind == 3 &&
              gram_head_slot(10).kind == 3 && gram_head_slot(10).p == 1 && gram_head_slot(14).kind == 0 && gram_head_slot(3).kind == 0, "head slots");
static_assert(gram_tail_slot(32 + 8 * 2 + 4).kind == 1 && gram_tail_slot(32 + 8 * 2 + 4).dim == 5 && gram_tail_slot(5).kind == 2 &&
              gram_tail_slot(32 + 6).kind == 2 && gram_tail_slot(32 + 7).kind == 3 && gram_tail_slot(32 + 7).p == 2 && gram_tail_slot(8 + 5).kind == 3 &&
              gram_tail_slot(8 + 5).p == 3 && gram_tail_slot(8 + 6).kind == 0 && gram_tail_slot(16 + 5).kind == 0 && gram_tail_slot(32 + 8 + 5).kind == 0, "tail slots");

// K2g's exact head sums (v_mfma_f32_16x16x16_f16, C = 0), each as ONE asm block that ends in five wait states.  gfx950 does NOT
// interlock a 16x16x32 MFMA that accumulates onto the result of a 16x16x16 one, and hipcc does not pad the pair: with fewer than 5 wait states (or one other MFMA) between the two the second reads a stale accumulator --
// half of its outputs wrong, tools/probe_mfma_dependent.hip (16x16x32 -> 16x16x32, 16x16x16 -> 16x16x16 and MFMA -> VALU are
// interlocked).  The compiler's schedule had kept the pairs apart in the shipped kernels and put them back to back in faster
// variants of K2g (four waves per SIMD: all 24 instances wrong), which is how this was found.
// one query half against two centre tiles: u[ct] = A x B[ct]
__device__ __forceinline__ void gram_heads2(const h4_t& a, const h4_t (&b)[2], f4_t (&u)[2]) {
  asm("v_mfma_f32_16x16x16_f16 %0, %2, %3, 0\n v_mfma_f32_16x16x16_f16 %1, %2, %4, 0\n s_nop 4"
      : "=&v"(u[0]), "=&v"(u[1])
      : "v"(a), "v"(b[0]), "v"(b[1]));
}

// ... with a start value c in the accumulator (K2g, gaussian: c = -14 takes the 2^14 of the basis value out again, so that the
// result IS alpha d^2; a multiple of the head grid and inside the budget that holds the +14 of c2, hence still exact)
__device__ __forceinline__ void gram_heads2c(const h4_t& a, const h4_t (&b)[2], const f4_t& c, f4_t (&u)[2]) {
  asm("v_mfma_f32_16x16x16_f16 %0, %2, %3, %5\n v_mfma_f32_16x16x16_f16 %1, %2, %4, %5\n s_nop 4"
      : "=&v"(u[0]), "=&v"(u[1])
      : "v"(a), "v"(b[0]), "v"(b[1]), "v"(c));
}

// the argument of the transcendental for the 2 x 2 tiles (query tile t, centre tile ct) of the chunk image at `buf`: operand 0
// (C = 0: the exact head sum, then its 16 tails), then operand 1 -- the four independent MFMAs first, so that no MFMA follows
// the one it accumulates onto (16x16x32 onto 16x16x32 is interlocked either way: tools/probe_mfma_dependent.hip)
// (`l16`: the lane's 16 bytes at the start of the image, buf + lane * 16)
__device__ __forceinline__ void gram_distances_at(const unsigned char* l16, const h8_t (&bq)[2][2], f4_t (&u)[2][2]) {
  h8_t aq[2][2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int o = 0; o < 2; ++o) aq[ct][o] = *reinterpret_cast<const h8_t*>(l16 + (ct * 2 + o) * 1024);
  const f4_t z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) u[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq[ct][0], bq[t][0], z, 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) u[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq[ct][1], bq[t][1], u[t][ct], 0, 0, 0);
}
__device__ __forceinline__ void gram_distances(const unsigned char* buf, int lane, const h8_t (&bq)[2][2], f4_t (&u)[2][2]) {
  gram_distances_at(buf + lane * 16, bq, u);
}

// The same arguments on the VALU from K1h's centre records `recs` of the chunk (a wave with a query outside the box): t16[t * 8 + j] for
// centre 16 (j >> 2) + 4 g + (j & 3) -- the k order of the Phi x W product here.  FINITE_R2: an infinite squared distance (a query
// with an Inf coordinate) enters as 3e38, so that a padding centre (scale 0) gives its finite P and not Inf x 0 -- the kernels
// whose regions all end in padding centres (rbf_forward_gram_gamma.hip) answer such a row as K1 does, with phi = 0
template <int DC, int BC, bool FINITE_R2 = false>
__device__ __forceinline__ void gram_valu_args(const F16Args& a, const long (&qrow)[2], int g, const float* recs, float (&t16)[16]) {
  constexpr int RF = f16_rf(DC);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float xq[DC];
#pragma unroll
    for (int d = 0; d < DC; ++d) xq[d] = d < a.Dreal ? a.x[qrow[t] * a.Dreal + d] : 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float* rp = recs + ((j >> 2) * 16 + 4 * g + (j & 3)) * RF;
      float r2 = 0.0f;
#pragma unroll
      for (int d = 0; d < DC; ++d) {
        const float df = xq[d] - rp[d];                      // flax_rbf.py:280
        r2 = __builtin_fmaf(df, df, r2);
      }
      if constexpr (FINITE_R2) r2 = r2 == __builtin_inff() ? 3.0e38f : r2;
      float arg = f16_arg<BC>(r2, rp[RF - 1]);
      if constexpr (BC == BC_IMQ) arg *= kPhiScale;          // 2^7 phi here (gram_phi_scale), K1h's records are scaled for 2^14 phi
      t16[t * 8 + j] = arg;
    }
  }
}

// host side (rbf_forward_gram.hip, rbf_forward_gram_wide.hip, plan_tick_wide.hip)
int gram_nsteps(int nchunks, int S);
void gram_fill_args(const irbfn_net* net, const float* x, float* out, int64_t B, int S, int QG, GramArgs* a);
int launch_forward_gram_wide(irbfn_net* net, const LaunchPlan& p, const float* x, float* out, int64_t B, hipStream_t s);

}  // namespace irbfn
