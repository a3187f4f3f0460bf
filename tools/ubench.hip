// VALU issue-rate microbenchmark for gfx950: v_fma_f32 vs v_pk_fma_f32 vs v_exp_f32 (+ SGPR operand
// forms), at 1..8 waves per SIMD; `ubench split`: the 2^11 gain of the K1g operand split (v_lshl_add_u64 against two v_mul_f32, alone and beside MFMAs).
// hipcc --offload-arch=gfx950 -O3 tools/ubench.hip -o /tmp/ubench
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#define REP 64
#define ITERS 2000

template <int MODE>
__global__ void k(float* out, float sv, unsigned long long* cyc) {
  float a0 = threadIdx.x * 1e-3f, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  float b = 1.0001f;
  unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < ITERS; ++it) {
#pragma unroll
    for (int r = 0; r < REP / 8; ++r) {
      if (MODE == 0) {   // v_fma_f32, VGPR operands, 8 independent chains
        asm volatile("v_fma_f32 %0, %0, %8, %0\n v_fma_f32 %1, %1, %8, %1\n v_fma_f32 %2, %2, %8, %2\n v_fma_f32 %3, %3, %8, %3\n"
                     "v_fma_f32 %4, %4, %8, %4\n v_fma_f32 %5, %5, %8, %5\n v_fma_f32 %6, %6, %8, %6\n v_fma_f32 %7, %7, %8, %7\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
      } else if (MODE == 1) {   // v_fma_f32 with an SGPR operand
        asm volatile("v_fma_f32 %0, %0, %8, %0\n v_fma_f32 %1, %1, %8, %1\n v_fma_f32 %2, %2, %8, %2\n v_fma_f32 %3, %3, %8, %3\n"
                     "v_fma_f32 %4, %4, %8, %4\n v_fma_f32 %5, %5, %8, %5\n v_fma_f32 %6, %6, %8, %6\n v_fma_f32 %7, %7, %8, %7\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "s"(sv));
      } else if (MODE == 2) {   // v_pk_fma_f32 (4 independent register pairs)
        asm volatile("v_pk_fma_f32 %0, %0, %4, %0\n v_pk_fma_f32 %1, %1, %4, %1\n v_pk_fma_f32 %2, %2, %4, %2\n v_pk_fma_f32 %3, %3, %4, %3\n"
                     "v_pk_fma_f32 %0, %0, %4, %0\n v_pk_fma_f32 %1, %1, %4, %1\n v_pk_fma_f32 %2, %2, %4, %2\n v_pk_fma_f32 %3, %3, %4, %3\n"
                     : "+v"(*(double*)&a0), "+v"(*(double*)&a2), "+v"(*(double*)&a4), "+v"(*(double*)&a6) : "v"(*(double*)&b));
      } else if (MODE == 3) {   // v_exp_f32
        asm volatile("v_exp_f32 %0, %0\n v_exp_f32 %1, %1\n v_exp_f32 %2, %2\n v_exp_f32 %3, %3\n"
                     "v_exp_f32 %4, %4\n v_exp_f32 %5, %5\n v_exp_f32 %6, %6\n v_exp_f32 %7, %7\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
      } else if (MODE == 4) {   // v_sub_f32 with SGPR + v_fmac (the distance pattern)
        asm volatile("v_subrev_f32 %0, %8, %1\n v_fmac_f32 %2, %0, %0\n v_subrev_f32 %3, %8, %4\n v_fmac_f32 %5, %3, %3\n"
                     "v_subrev_f32 %0, %8, %6\n v_fmac_f32 %2, %0, %0\n v_subrev_f32 %3, %8, %7\n v_fmac_f32 %5, %3, %3\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "s"(sv));
      } else if (MODE == 5) {   // v_pk_add_f32 + v_pk_fma_f32 (packed distance pattern), SGPR pair operand
        asm volatile("v_pk_add_f32 %0, %1, %4 neg_lo:[0,1] neg_hi:[0,1]\n v_pk_fma_f32 %2, %0, %0, %2\n"
                     "v_pk_add_f32 %0, %3, %4 neg_lo:[0,1] neg_hi:[0,1]\n v_pk_fma_f32 %2, %0, %0, %2\n"
                     "v_pk_add_f32 %0, %1, %4 neg_lo:[0,1] neg_hi:[0,1]\n v_pk_fma_f32 %2, %0, %0, %2\n"
                     "v_pk_add_f32 %0, %3, %4 neg_lo:[0,1] neg_hi:[0,1]\n v_pk_fma_f32 %2, %0, %0, %2\n"
                     : "+v"(*(double*)&a0), "+v"(*(double*)&a2), "+v"(*(double*)&a4), "+v"(*(double*)&a6) : "s"(*(double*)&sv));
      } else if (MODE == 7) {   // v_fmac_f32_e32 VOP2, VGPR only
        asm volatile("v_fmac_f32_e32 %0, %8, %8\n v_fmac_f32_e32 %1, %8, %8\n v_fmac_f32_e32 %2, %8, %8\n v_fmac_f32_e32 %3, %8, %8\n"
                     "v_fmac_f32_e32 %4, %8, %8\n v_fmac_f32_e32 %5, %8, %8\n v_fmac_f32_e32 %6, %8, %8\n v_fmac_f32_e32 %7, %8, %8\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
      } else if (MODE == 8) {   // v_fmac_f32_e32 VOP2, SGPR src0 (same SGPR)
        asm volatile("v_fmac_f32_e32 %0, %9, %8\n v_fmac_f32_e32 %1, %9, %8\n v_fmac_f32_e32 %2, %9, %8\n v_fmac_f32_e32 %3, %9, %8\n"
                     "v_fmac_f32_e32 %4, %9, %8\n v_fmac_f32_e32 %5, %9, %8\n v_fmac_f32_e32 %6, %9, %8\n v_fmac_f32_e32 %7, %9, %8\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "s"(sv));
      } else if (MODE == 9) {   // v_fmac_f32_e32 VOP2, 4 different SGPRs
        asm volatile("v_fmac_f32_e32 %0, %9, %8\n v_fmac_f32_e32 %1, %10, %8\n v_fmac_f32_e32 %2, %11, %8\n v_fmac_f32_e32 %3, %12, %8\n"
                     "v_fmac_f32_e32 %4, %9, %8\n v_fmac_f32_e32 %5, %10, %8\n v_fmac_f32_e32 %6, %11, %8\n v_fmac_f32_e32 %7, %12, %8\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "s"(sv), "s"(sv*2), "s"(sv*3), "s"(sv*4));
      } else if (MODE == 10) {   // v_subrev_f32_e32 VOP2 with SGPR
        asm volatile("v_subrev_f32_e32 %0, %8, %0\n v_subrev_f32_e32 %1, %8, %1\n v_subrev_f32_e32 %2, %8, %2\n v_subrev_f32_e32 %3, %8, %3\n"
                     "v_subrev_f32_e32 %4, %8, %4\n v_subrev_f32_e32 %5, %8, %5\n v_subrev_f32_e32 %6, %8, %6\n v_subrev_f32_e32 %7, %8, %7\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "s"(sv));
      } else if (MODE == 11) {   // v_add_f32_e32 VOP2 VGPR only
        asm volatile("v_add_f32_e32 %0, %8, %0\n v_add_f32_e32 %1, %8, %1\n v_add_f32_e32 %2, %8, %2\n v_add_f32_e32 %3, %8, %3\n"
                     "v_add_f32_e32 %4, %8, %4\n v_add_f32_e32 %5, %8, %5\n v_add_f32_e32 %6, %8, %6\n v_add_f32_e32 %7, %8, %7\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
      } else if (MODE == 12) {   // v_pk_fma_f32 with SGPR pair broadcast operand
        asm volatile("v_pk_fma_f32 %0, %5, %4, %0 op_sel_hi:[0,1,1]\n v_pk_fma_f32 %1, %5, %4, %1 op_sel_hi:[0,1,1]\n v_pk_fma_f32 %2, %5, %4, %2 op_sel_hi:[0,1,1]\n v_pk_fma_f32 %3, %5, %4, %3 op_sel_hi:[0,1,1]\n"
                     "v_pk_fma_f32 %0, %5, %4, %0 op_sel_hi:[0,1,1]\n v_pk_fma_f32 %1, %5, %4, %1 op_sel_hi:[0,1,1]\n v_pk_fma_f32 %2, %5, %4, %2 op_sel_hi:[0,1,1]\n v_pk_fma_f32 %3, %5, %4, %3 op_sel_hi:[0,1,1]\n"
                     : "+v"(*(double*)&a0), "+v"(*(double*)&a2), "+v"(*(double*)&a4), "+v"(*(double*)&a6) : "s"(*(double*)&sv), "v"(*(double*)&b));
      } else if (MODE == 13) {   // v_mul_f32 + v_exp_f32 + 2 fmac mix
        asm volatile("v_mul_f32_e32 %0, %8, %0\n v_exp_f32_e32 %1, %0\n v_fmac_f32_e32 %2, %1, %1\n v_fmac_f32_e32 %3, %1, %1\n"
                     "v_mul_f32_e32 %4, %8, %4\n v_exp_f32_e32 %5, %4\n v_fmac_f32_e32 %6, %5, %5\n v_fmac_f32_e32 %7, %5, %5\n"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
      } else if (MODE == 6) {   // v_pk_mul_f32
        asm volatile("v_pk_mul_f32 %0, %0, %4\n v_pk_mul_f32 %1, %1, %4\n v_pk_mul_f32 %2, %2, %4\n v_pk_mul_f32 %3, %3, %4\n"
                     "v_pk_mul_f32 %0, %0, %4\n v_pk_mul_f32 %1, %1, %4\n v_pk_mul_f32 %2, %2, %4\n v_pk_mul_f32 %3, %3, %4\n"
                     : "+v"(*(double*)&a0), "+v"(*(double*)&a2), "+v"(*(double*)&a4), "+v"(*(double*)&a6) : "v"(*(double*)&b));
      }
    }
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
  if (threadIdx.x == 0) { cyc[blockIdx.x] = t1 - t0; cyc[4096 + blockIdx.x] = r1 - r0; }
}

template <int MODE>
void run(const char* name, int lanes_per_instr_ops) {
  float* out;
  unsigned long long* cyc;
  hipMalloc(&out, 256 * 8 * 1024 * sizeof(float) * 4);
  hipMalloc(&cyc, 8192 * sizeof(unsigned long long));
  for (int wps : {1, 2, 4, 8}) {   // waves per SIMD: block = 256*wps threads, 1 block per CU
    int threads = 256 * wps;
    if (threads > 1024) { threads = 1024; }
    int blocks = 256 * (256 * wps / threads);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(threads), 0, 0, out, 1.0001f, cyc);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(threads), 0, 0, out, 1.0001f, cyc);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h(8192);
    hipMemcpy(h.data(), cyc, 8192 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    double avg = 0, rt = 0; for (int i = 0; i < blocks; ++i) { avg += h[i]; rt += h[4096 + i]; } avg /= blocks; rt /= blocks;
    double mhz = avg / (rt / 100.0);   // memrealtime = 100 MHz
    double instr_per_wave = (double)ITERS * REP;
    // memtime ticks at 100 MHz constant? report both ticks per instr and wall-derived cycles at 2.4 GHz
    double waves_per_simd = wps;
    double wall_cycles = ms * 1e-3 * 2.4e9;
    printf("%-30s wps=%d wall %.3f ms  %.2f cyc@2.4/instr/SIMD  memtime/instr/wave %.2f  clk(memtime/realtime) %.0f MHz\n", name, wps, ms,
           wall_cycles / (instr_per_wave * waves_per_simd), avg / instr_per_wave, mhz);
  }
  hipFree(out); hipFree(cyc);
}

// ---- the 2^11 gain of K1g's operand split (rbf_forward_gram.h, split_pair_mix), per value PAIR ------------------------------
// ARM 1: v_lshl_add_u64 on a VGPR pair, the constant in an SGPR pair; 2: the constant in a VGPR pair; 3: two v_mul_f32 by 2048
// (alternating with 2^-11, so the values stay finite); 4 / 5: the split's two v_fma_mix_f32 with the multiplier in an SGPR / as
// the inline constant -1.0; 0: nothing (MIX only: the frame on its own).
// MIX = false: 8 pairs' worth of the arm per block, alone.  MIX = true: the same 8 pairs' worth spread over a frame of K1g's
// step -- 18 v_mfma_f32_16x16x32_f16 (six accumulators in turn) and 57 plain v_fma_f32 -- so the add arms run at K1g's
// 18 MFMA : 65 VALU; (block - frame) / 8 is what the gain of one pair costs beside the matrix cores.
typedef _Float16 ub_h8 __attribute__((ext_vector_type(8)));
typedef float ub_f4 __attribute__((ext_vector_type(4)));
#define SPLIT_ITERS 20000
#define UB_MF(a) "v_mfma_f32_16x16x32_f16 %" #a ", %6, %7, %" #a "\n"
#define UB_F(k) "v_fma_f32 %" #k ", %" #k ", %16, %" #k "\n"
#define UB_G(a, f0, f1, f2, X) UB_MF(a) UB_F(f0) UB_F(f1) UB_F(f2) X
// 18 groups of (MFMA, 3 v_fma, arm piece) + 3 v_fma; X0..X15: the arm's pieces (the add arms use the even ones)
#define UB_FRAME(X0, X1, X2, X3, X4, X5, X6, X7, X8, X9, X10, X11, X12, X13, X14, X15)                                             \
  UB_G(0, 8, 9, 10, X0) UB_G(1, 11, 12, 13, X1) UB_G(2, 14, 15, 8, X2) UB_G(3, 9, 10, 11, X3) UB_G(4, 12, 13, 14, X4)             \
  UB_G(5, 15, 8, 9, X5) UB_G(0, 10, 11, 12, X6) UB_G(1, 13, 14, 15, X7) UB_G(2, 8, 9, 10, X8) UB_G(3, 11, 12, 13, X9)             \
  UB_G(4, 14, 15, 8, X10) UB_G(5, 9, 10, 11, X11) UB_G(0, 12, 13, 14, X12) UB_G(1, 15, 8, 9, X13) UB_G(2, 10, 11, 12, X14)        \
  UB_G(3, 13, 14, 15, X15) UB_G(4, 8, 9, 10, "") UB_G(5, 11, 12, 13, "") UB_F(14) UB_F(15) UB_F(8)
#define UB_ACC "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5)
#define UB_FIL "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+v"(b)   // %8..%15, %16
#define UB_ADD(p) "v_lshl_add_u64 %" #p ", %" #p ", 0, %21\n"
#define UB_MUL(m, c) "v_mul_f32_e32 %" #m ", " c ", %" #m "\n"
#define UB_MIXS(d, sel) "v_fma_mix_f32 %" #d ", %25, %26, %" #d " op_sel:[" #sel ",0,0] op_sel_hi:[1,0,0]\n"
#define UB_MIXI(d, sel) "v_fma_mix_f32 %" #d ", %25, -1.0, %" #d " op_sel:[" #sel ",0,0] op_sel_hi:[1,0,0]\n"

template <int ARM, bool MIX>
__global__ void ksplit(float* out, unsigned long long gain, float sv, unsigned long long* cyc) {
  float a0 = threadIdx.x * 1e-3f, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  float m0 = a0 + 1, m1 = a0 + 2, m2 = a0 + 3, m3 = a0 + 4, m4 = a0 + 5, m5 = a0 + 6, m6 = a0 + 7, m7 = a0 + 8;
  float n0 = m0, n1 = m1, n2 = m2, n3 = m3, n4 = m4, n5 = m5, n6 = m6, n7 = m7;
  float b = 1.0001f;
  unsigned long long p0 = threadIdx.x, p1 = p0 + 1, p2 = p0 + 2, p3 = p0 + 3, p4 = p0 + 4, p5 = p0 + 5, p6 = p0 + 6, p7 = p0 + 7;
  unsigned long long gv = gain + threadIdx.x;                // the constant in a VGPR pair
  asm volatile("" : "+v"(gv));
  ub_f4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0;
  ub_h8 A, B;
  for (int j = 0; j < 8; ++j) { A[j] = (_Float16)(a0 * 1e-2f + j); B[j] = (_Float16)(1.0f / (j + 1)); }
  unsigned hsrc = threadIdx.x * 0x00010001u + 0x3c003c00u;   // two f16 numbers for the mixes
  unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < SPLIT_ITERS; ++it) {
    if constexpr (!MIX) {
      if constexpr (ARM == 1 || ARM == 2) {
#define UB_A1(p) "v_lshl_add_u64 %" #p ", %" #p ", 0, %8\n"
        if constexpr (ARM == 1)
          asm volatile(UB_A1(0) UB_A1(1) UB_A1(2) UB_A1(3) UB_A1(4) UB_A1(5) UB_A1(6) UB_A1(7)
                       : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "s"(gain));
        else
          asm volatile(UB_A1(0) UB_A1(1) UB_A1(2) UB_A1(3) UB_A1(4) UB_A1(5) UB_A1(6) UB_A1(7)
                       : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(gv));
      } else if constexpr (ARM == 3) {
        asm volatile(UB_MUL(0, "0x45000000") UB_MUL(1, "0x45000000") UB_MUL(2, "0x45000000") UB_MUL(3, "0x45000000")
                     UB_MUL(4, "0x45000000") UB_MUL(5, "0x45000000") UB_MUL(6, "0x45000000") UB_MUL(7, "0x45000000")
                     UB_MUL(0, "0x3a000000") UB_MUL(1, "0x3a000000") UB_MUL(2, "0x3a000000") UB_MUL(3, "0x3a000000")
                     UB_MUL(4, "0x3a000000") UB_MUL(5, "0x3a000000") UB_MUL(6, "0x3a000000") UB_MUL(7, "0x3a000000")
                     : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7));
      } else {
#define UB_X1S(d, sel) "v_fma_mix_f32 %" #d ", %16, %17, %" #d " op_sel:[" #sel ",0,0] op_sel_hi:[1,0,0]\n"
#define UB_X1I(d, sel) "v_fma_mix_f32 %" #d ", %16, -1.0, %" #d " op_sel:[" #sel ",0,0] op_sel_hi:[1,0,0]\n"
        if constexpr (ARM == 4)
          asm volatile(UB_X1S(0, 0) UB_X1S(1, 1) UB_X1S(2, 0) UB_X1S(3, 1) UB_X1S(4, 0) UB_X1S(5, 1) UB_X1S(6, 0) UB_X1S(7, 1)
                       UB_X1S(8, 0) UB_X1S(9, 1) UB_X1S(10, 0) UB_X1S(11, 1) UB_X1S(12, 0) UB_X1S(13, 1) UB_X1S(14, 0) UB_X1S(15, 1)
                       : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7), "+v"(n0), "+v"(n1), "+v"(n2),
                         "+v"(n3), "+v"(n4), "+v"(n5), "+v"(n6), "+v"(n7) : "v"(hsrc), "s"(sv));
        else
          asm volatile(UB_X1I(0, 0) UB_X1I(1, 1) UB_X1I(2, 0) UB_X1I(3, 1) UB_X1I(4, 0) UB_X1I(5, 1) UB_X1I(6, 0) UB_X1I(7, 1)
                       UB_X1I(8, 0) UB_X1I(9, 1) UB_X1I(10, 0) UB_X1I(11, 1) UB_X1I(12, 0) UB_X1I(13, 1) UB_X1I(14, 0) UB_X1I(15, 1)
                       : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7), "+v"(n0), "+v"(n1), "+v"(n2),
                         "+v"(n3), "+v"(n4), "+v"(n5), "+v"(n6), "+v"(n7) : "v"(hsrc), "s"(sv));
      }
    } else if constexpr (ARM == 0) {
      asm volatile(UB_FRAME("", "", "", "", "", "", "", "", "", "", "", "", "", "", "", "") : UB_ACC, "+v"(A), "+v"(B), UB_FIL);
    } else if constexpr (ARM == 1) {
      asm volatile(UB_FRAME(UB_ADD(17), "", UB_ADD(18), "", UB_ADD(19), "", UB_ADD(20), "", UB_ADD(17), "", UB_ADD(18), "", UB_ADD(19), "", UB_ADD(20), "")
                   : UB_ACC, "+v"(A), "+v"(B), UB_FIL, "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3) : "s"(gain));
    } else if constexpr (ARM == 2) {
      asm volatile(UB_FRAME(UB_ADD(17), "", UB_ADD(18), "", UB_ADD(19), "", UB_ADD(20), "", UB_ADD(17), "", UB_ADD(18), "", UB_ADD(19), "", UB_ADD(20), "")
                   : UB_ACC, "+v"(A), "+v"(B), UB_FIL, "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3) : "v"(gv));
    } else if constexpr (ARM == 3) {
      asm volatile(UB_FRAME(UB_MUL(17, "0x45000000"), UB_MUL(18, "0x45000000"), UB_MUL(19, "0x45000000"), UB_MUL(20, "0x45000000"),
                            UB_MUL(21, "0x45000000"), UB_MUL(22, "0x45000000"), UB_MUL(23, "0x45000000"), UB_MUL(24, "0x45000000"),
                            UB_MUL(17, "0x3a000000"), UB_MUL(18, "0x3a000000"), UB_MUL(19, "0x3a000000"), UB_MUL(20, "0x3a000000"),
                            UB_MUL(21, "0x3a000000"), UB_MUL(22, "0x3a000000"), UB_MUL(23, "0x3a000000"), UB_MUL(24, "0x3a000000"))
                   : UB_ACC, "+v"(A), "+v"(B), UB_FIL, "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7));
    } else if constexpr (ARM == 4) {
      asm volatile(UB_FRAME(UB_MIXS(17, 0), UB_MIXS(18, 1), UB_MIXS(19, 0), UB_MIXS(20, 1), UB_MIXS(21, 0), UB_MIXS(22, 1), UB_MIXS(23, 0), UB_MIXS(24, 1),
                            UB_MIXS(17, 0), UB_MIXS(18, 1), UB_MIXS(19, 0), UB_MIXS(20, 1), UB_MIXS(21, 0), UB_MIXS(22, 1), UB_MIXS(23, 0), UB_MIXS(24, 1))
                   : UB_ACC, "+v"(A), "+v"(B), UB_FIL, "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7)
                   : "v"(hsrc), "s"(sv));
    } else {
      asm volatile(UB_FRAME(UB_MIXI(17, 0), UB_MIXI(18, 1), UB_MIXI(19, 0), UB_MIXI(20, 1), UB_MIXI(21, 0), UB_MIXI(22, 1), UB_MIXI(23, 0), UB_MIXI(24, 1),
                            UB_MIXI(17, 0), UB_MIXI(18, 1), UB_MIXI(19, 0), UB_MIXI(20, 1), UB_MIXI(21, 0), UB_MIXI(22, 1), UB_MIXI(23, 0), UB_MIXI(24, 1))
                   : UB_ACC, "+v"(A), "+v"(B), UB_FIL, "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5), "+v"(m6), "+v"(m7)
                   : "v"(hsrc));
    }
  }
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + m0 + m1 + m2 + m3 + m4 + m5 + m6 + m7 + n0 + n1 + n2 + n3 +
                                               n4 + n5 + n6 + n7 + c0[0] + c1[1] + c2[2] + c3[3] + c4[0] + c5[1] +
                                               (float)(p0 ^ p1 ^ p2 ^ p3 ^ p4 ^ p5 ^ p6 ^ p7);
  if (threadIdx.x == 0) { cyc[blockIdx.x] = t1 - t0; cyc[4096 + blockIdx.x] = r1 - r0; }
}

// cycles (at 2.4 GHz, from the wall time) per block per SIMD; a block holds the gain of 8 value pairs
template <int ARM, bool MIX>
void run_split(const char* name, double (&blk)[3]) {
  float* out;
  unsigned long long* cyc;
  hipMalloc(&out, 256 * 1024 * sizeof(float));
  hipMalloc(&cyc, 8192 * sizeof(unsigned long long));
  int row = 0;
  for (int wps : {1, 2, 4}) {                                // waves per SIMD: one block of 256 * wps threads per CU
    const int threads = 256 * wps, blocks = 256;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    float ms = 1e30f;                                        // the fastest of five launches behind two untimed ones (the clock ramps up)
    for (int rep = 0; rep < 7; ++rep) {
      hipEventRecord(e0);
      hipLaunchKernelGGL((ksplit<ARM, MIX>), dim3(blocks), dim3(threads), 0, 0, out, 0x0580000005800000ull, -1.0f, cyc);
      hipEventRecord(e1);
      hipEventSynchronize(e1);
      float m; hipEventElapsedTime(&m, e0, e1);
      if (rep >= 2 && m < ms) ms = m;
    }
    std::vector<unsigned long long> h(8192);
    hipMemcpy(h.data(), cyc, 8192 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    double avg = 0, rt = 0; for (int i = 0; i < blocks; ++i) { avg += h[i]; rt += h[4096 + i]; } avg /= blocks; rt /= blocks;
    blk[row] = ms * 1e-3 * 2.4e9 / ((double)SPLIT_ITERS * wps);
    printf("%-34s %-5s wps=%d wall %.3f ms  %.2f cyc@2.4/block/SIMD  %.2f /pair  clk(memtime/realtime) %.0f MHz\n", name, MIX ? "mixed" : "alone",
           wps, ms, blk[row], blk[row] / 8.0, avg / (rt / 100.0));
    ++row;
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  hipFree(out); hipFree(cyc);
}

// The two forms of the split on the device, bit for bit, over every float exponent up to 2^14 of both signs (the mantissas: 0,
// all ones, one bit at either end and pseudo-random ones), +-0 and the subnormals.  Says what the instructions do -- the
// inline constant of the mix, the sign of a zero out of the round-toward-zero conversion -- where the host test
// (tests/test_split_gain_cpu.py) says what the arithmetic does.
__global__ void ksplit_check(unsigned* res) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned e = tid >> 7, s = (tid >> 6) & 1, k = tid & 63;       // e <= 127 + 14
  unsigned man = k == 0 ? 0u : (k == 1 ? 0x7fffffu : (k == 2 ? 1u : (k == 3 ? 0x400000u : (k == 4 ? 0x001000u : (k == 5 ? 0x000fffu : (tid * 2654435761u) >> 9)))));
  if (e == 127 + 14) man = 0;                                // 2^14 exactly
  const unsigned man1 = e == 127 + 14 ? 0u : (man * 40503u + 12345u) & 0x7fffffu;
  const unsigned bits0 = (s << 31) | (e << 23) | man, bits1 = (s << 31) | (e << 23) | man1;
  const float p0 = __builtin_bit_cast(float, bits0), p1 = __builtin_bit_cast(float, bits1);
  const unsigned hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(p0, p1));
  // the form with the two multiplies
  const float q0 = p0 * 2048.0f, q1 = p1 * 2048.0f, ng = -2048.0f;
  float d0, d1;
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(hi), "s"(ng), "v"(q0));
  asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d1) : "v"(hi), "s"(ng), "v"(q1));
  const unsigned lo_old = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(d0, d1));
  // the form with the 64-bit add
  float f0, f1;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(f0) : "v"(hi), "v"(p0));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(f1) : "v"(hi), "v"(p1));
  unsigned long long dd = (unsigned long long)__builtin_bit_cast(unsigned, f0) | ((unsigned long long)__builtin_bit_cast(unsigned, f1) << 32);
  asm("v_lshl_add_u64 %0, %0, 0, %1" : "+v"(dd) : "s"(0x0580000005800000ull));
  const unsigned lo_new = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(__builtin_bit_cast(float, (unsigned)dd), __builtin_bit_cast(float, (unsigned)(dd >> 32))));
  if (lo_old != lo_new) {
    if (atomicAdd(&res[0], 1u) == 0) { res[1] = bits0; res[2] = bits1; res[3] = lo_old; res[4] = lo_new; res[5] = hi; }
  }
  if (lo_old != 0) atomicAdd(&res[6], 1u);                   // the sweep is not all zeros
}

void run_split_check() {
  unsigned* res;
  hipMalloc(&res, 8 * sizeof(unsigned));
  hipMemset(res, 0, 8 * sizeof(unsigned));
  const int n = (127 + 14 + 1) * 128;
  hipLaunchKernelGGL(ksplit_check, dim3(n / 128), dim3(128), 0, 0, res);
  unsigned h[8];
  hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost);
  printf("split check: %d pairs, %u with a non-zero lo, %u mismatches old / new", n, h[6], h[0]);
  if (h[0]) printf(" (first: p = %08x %08x hi %08x lo old %08x new %08x)", h[1], h[2], h[5], h[3], h[4]);
  printf("\n");
  hipFree(res);
}

void run_split_gain() {
  run_split_check();
  double fr[3], r[3];
  run_split<1, false>("v_lshl_add_u64 sgpr-pair const x8", r);
  run_split<2, false>("v_lshl_add_u64 vgpr-pair const x8", r);
  run_split<3, false>("v_mul_f32 2048 x16", r);
  run_split<4, false>("v_fma_mix_f32 sgpr mult x16", r);
  run_split<5, false>("v_fma_mix_f32 inline -1.0 x16", r);
  run_split<0, true>("frame 18 mfma + 57 v_fma", fr);
  auto delta = [&](const char* name) {
    printf("%-34s (block - frame) / 8 pairs: wps=1 %.2f  wps=2 %.2f  wps=4 %.2f cyc@2.4/pair/SIMD\n", name, (r[0] - fr[0]) / 8, (r[1] - fr[1]) / 8,
           (r[2] - fr[2]) / 8);
  };
  run_split<1, true>("frame + 8 v_lshl_add_u64 sgpr", r); delta("  add sgpr");
  run_split<2, true>("frame + 8 v_lshl_add_u64 vgpr", r); delta("  add vgpr");
  run_split<3, true>("frame + 16 v_mul_f32", r); delta("  two muls");
  run_split<4, true>("frame + 16 v_fma_mix_f32 sgpr", r); delta("  two mixes, sgpr mult");
  run_split<5, true>("frame + 16 v_fma_mix_f32 inline", r); delta("  two mixes, inline mult");
  run_split<0, true>("frame again", fr);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "split")) { run_split_gain(); return 0; }   // the rows of profiles/k1g_split_gain.txt
  run<0>("v_fma_f32 vgpr", 1);
  run<1>("v_fma_f32 sgpr-operand", 1);
  run<2>("v_pk_fma_f32", 2);
  run<6>("v_pk_mul_f32", 2);
  run<3>("v_exp_f32", 1);
  run<4>("v_subrev(sgpr)+v_fmac", 1);
  run<5>("v_pk_add(sgpr)+v_pk_fma", 2);
  run<7>("v_fmac_e32 vgpr", 1);
  run<8>("v_fmac_e32 sgpr src0 (same)", 1);
  run<9>("v_fmac_e32 sgpr src0 (4 diff)", 1);
  run<10>("v_subrev_e32 sgpr", 1);
  run<11>("v_add_e32 vgpr", 1);
  run<12>("v_pk_fma sgprpair bcast", 2);
  run<13>("mul+exp+2fmac mix", 1);
  return 0;
}
