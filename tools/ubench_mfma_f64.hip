// What does one v_mfma_f64_16x16x4_f64 cost on gfx950?  Back to back, NA independent accumulators (1 = a dependent chain),
// one and two waves per SIMD, then with the v_cvt_f64_f32 + ds_read_b32 operand traffic of K8 (syrk_f64.hip) between them.
// Also checks the C/D lane map with exact integer data: D[i][j] = sum_k A[i][k] B[k][j], row = (lane >> 4) + 4 reg.
//   hipcc --offload-arch=gfx950 -O3 -o tools/_bin/ubench_mfma_f64 tools/ubench_mfma_f64.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef double d4_t __attribute__((ext_vector_type(4)));
#define ITERS 2000
#define UNROLL 8

template <int NA, bool CVT>
__global__ __launch_bounds__(512) void k(double* out, const float* src) {
  __shared__ float zs[1024];
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) zs[i] = src[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  d4_t acc[NA];
  for (int a = 0; a < NA; ++a) acc[a] = d4_t{0, 0, 0, 0};
  double av = (double)zs[lane], bv = (double)zs[64 + lane];
  for (int it = 0; it < ITERS; ++it) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if constexpr (CVT) {       // one operand refreshed per MFMA: K8's ratio at a 32 x 32 patch per wave
        const float f = zs[(lane + 64 * ((it * UNROLL + u) & 15)) & 1023];
        if (u & 1) av = (double)f; else bv = (double)f;
      }
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[a], 0, 0, 0);
    }
  }
  double r = 0;
  for (int a = 0; a < NA; ++a) r += acc[a][0] + acc[a][1] + acc[a][2] + acc[a][3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

template <int NA, bool CVT>
void run(const char* name, double* out, const float* src, int threads) {
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int blocks = 256;                                   // one block per CU: threads / 256 waves per SIMD
  k<NA, CVT><<<blocks, threads>>>(out, src); (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0); k<NA, CVT><<<blocks, threads>>>(out, src); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1);
  const double wps = threads / 256.0, n = (double)ITERS * UNROLL * NA * wps;      // MFMAs per SIMD
  const double cyc = ms * 1e-3 * 2.4e9 / n;
  printf("%-44s wps=%1.0f %8.3f ms  %6.1f cyc@2.4 per MFMA per SIMD  %6.1f TFLOP/s over 1024 SIMDs\n", name, wps, ms, cyc,
         2048.0 * n * 1024 / (ms * 1e-3) * 1e-12);
}

__global__ void lane_map(const double* A, const double* B, double* D) {     // A [16][4], B [4][16], D [16][16]
  const int l = threadIdx.x;
  d4_t c = {0, 0, 0, 0};
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], c, 0, 0, 0);
  for (int r = 0; r < 4; ++r) D[((l >> 4) + 4 * r) * 16 + (l & 15)] = c[r];
}

int main() {
  double *out, *dA, *dB, *dD; float* src;
  (void)hipMalloc(&out, 256 * 512 * 8); (void)hipMalloc(&src, 4096); (void)hipMemset(src, 0, 4096);
  double hA[64], hB[64], hD[256];
  for (int i = 0; i < 64; ++i) { hA[i] = 1 + (i * 7) % 13; hB[i] = 2 + (i * 5) % 11; }
  (void)hipMalloc(&dA, sizeof(hA)); (void)hipMalloc(&dB, sizeof(hB)); (void)hipMalloc(&dD, sizeof(hD));
  (void)hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice); (void)hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
  lane_map<<<1, 64>>>(dA, dB, dD);
  (void)hipMemcpy(hD, dD, sizeof(hD), hipMemcpyDeviceToHost);
  int bad = 0;
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      double s = 0;
      for (int kk = 0; kk < 4; ++kk) s += hA[i * 4 + kk] * hB[kk * 16 + j];
      bad += s != hD[i * 16 + j];
    }
  printf("lane map A[l&15][l>>4], B[l>>4][l&15], D row (l>>4)+4*reg, col l&15: %d of 256 entries differ\n", bad);
  for (int threads : {256, 512}) {
    run<1, false>("1 accumulator (dependent chain)", out, src, threads);
    run<2, false>("2 independent accumulators", out, src, threads);
    run<4, false>("4 independent accumulators", out, src, threads);
    run<8, false>("8 independent accumulators", out, src, threads);
    run<4, true>("4 accumulators + ds_read_b32 + cvt per 4", out, src, threads);
    run<1, true>("1 accumulator + ds_read_b32 + cvt per MFMA", out, src, threads);
  }
  return bad != 0;
}
