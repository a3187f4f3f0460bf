// How does v_mfma_f32_16x16x32_f16 accumulate its 32 products?  (hipcc --offload-arch=gfx950 -O2 -o /tmp/probe tools/probe_mfma_accum.hip)
// Row 0 of A carries +big at slot i, -big at slot j and `small` at slot k, B is all ones (exact products): the exact sum is
// `small`.  An adder tree that keeps W bits below the largest product returns small rounded to 2^-W big.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <math.h>
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef float f4_t __attribute__((ext_vector_type(4)));

__global__ void probe(const _Float16* A, const _Float16* Bm, const float* Cin, float* out) {
  const int l = threadIdx.x, g = l >> 4, n = l & 15;
  h8_t a, b;
  for (int j = 0; j < 8; ++j) { a[j] = A[n * 32 + 8 * g + j]; b[j] = Bm[(8 * g + j) * 16 + n]; }
  f4_t c;
  for (int r = 0; r < 4; ++r) c[r] = Cin[(4 * g + r) * 16 + n];
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  for (int r = 0; r < 4; ++r) out[(4 * g + r) * 16 + n] = c[r];
}

// `fold` mode: may the fixed-point heads of a distance tile share one 16x16x32 MFMA with tails?  (probe fold [draws] [seed])
// Block d multiplies draw d's A[16][32] by B[32][16] three ways:
//   out[0]  heads (k 0-15) alone, C = 0                              -> must be the exact integer sum
//   out[1]  heads and tails (k 16-31) in the one MFMA, C = 0         -> the folded form
//   out[2]  16x16x16 of the heads, then the 16x16x32 with the heads' slots zero accumulating onto it -> today's form
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
__global__ void probe_fold(const _Float16* A, const _Float16* Bm, float* out) {
  const int l = threadIdx.x, g = l >> 4, n = l & 15;
  A += (size_t)blockIdx.x * 512; Bm += (size_t)blockIdx.x * 512; out += (size_t)blockIdx.x * 768;
  h8_t a, b, ah, bh, at;
  for (int j = 0; j < 8; ++j) {
    a[j] = A[n * 32 + 8 * g + j]; b[j] = Bm[(8 * g + j) * 16 + n];
    ah[j] = g < 2 ? a[j] : (_Float16)0; bh[j] = g < 2 ? b[j] : (_Float16)0; at[j] = g < 2 ? (_Float16)0 : a[j];
  }
  h4_t a4, b4;
  for (int j = 0; j < 4; ++j) { a4[j] = A[n * 32 + 4 * g + j]; b4[j] = Bm[(4 * g + j) * 16 + n]; }
  const f4_t z = {0.f, 0.f, 0.f, 0.f};
  const f4_t r0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, z, 0, 0, 0);
  const f4_t r1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, z, 0, 0, 0);
  f4_t r2 = __builtin_amdgcn_mfma_f32_16x16x16f16(a4, b4, z, 0, 0, 0);
  r2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(at, b, r2, 0, 0, 0);
  for (int r = 0; r < 4; ++r) {
    out[(4 * g + r) * 16 + n] = r0[r]; out[256 + (4 * g + r) * 16 + n] = r1[r]; out[512 + (4 * g + r) * 16 + n] = r2[r];
  }
}

#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
static uint64_t fold_rng;
static uint32_t rnd() { fold_rng = fold_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(fold_rng >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }   // inclusive
static double ulp_of(double v) { int e; frexp(v, &e); return ldexp(1.0, e - 24); }           // f32 unit in the last place of |v|

// One draw.  Heads: the 16 slots are paired at random (within a lane group or across the two); a pair carries
// +(a + da[row]) (b + db[col]) and -(a + da'[row]) (b + db'[col]) with da, db in {-1, 0, 1}, so every one of the 256 sums
// nearly cancels.  Six pairs share the 2^24-unit budget about evenly, two are up to 2^10 smaller.  a, b are integers
// below 2^11 (exact in f16) times 2^ea, 2^eb: every product is a multiple of the grid 2^(ea+eb).
// Tails: full 11-bit mantissas, products below 2^10 grid units = 2^-10 of a 2^20-unit head product, down to 2^-2.
static void fold_draw(_Float16* A, _Float16* B, int64_t* headsum, double* tailsum, double* tailmax, double* magmax, int* ea_eb) {
  const int ea = rnd_in(-12, 4), eb = rnd_in(-12, 4);
  *ea_eb = ea + eb;
  int perm[16];
  for (int i = 0; i < 16; ++i) perm[i] = i;
  for (int i = 15; i > 0; --i) { const int j = rnd_in(0, i), t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
  double f[8], fs = 0;
  for (int p = 0; p < 8; ++p) { f[p] = p < 6 ? 1.0 + rnd() / 2147483648.0 : ldexp(1.0, -rnd_in(0, 10)); fs += f[p]; }
  int iA[16][32] = {}, iB[32][16] = {};
  const double budget = ldexp(1.0, 24) - ldexp(1.0, 17);          // the +-1 terms add at most 16 x 2 x 2047 + 16 < 2^17
  for (int p = 0; p < 8; ++p) {
    const double w = budget * f[p] / fs / 2;                       // one slot's share, at most 2^24 / 6
    const int a = p < 6 ? rnd_in(1400, 2046) : rnd_in(2, 2046);
    int b = (int)(w / a); b = b < 2 ? 2 : b > 2046 ? 2046 : b;
    const int s = rnd() & 1 ? 1 : -1, t = rnd() & 1 ? 1 : -1, k1 = perm[2 * p], k2 = perm[2 * p + 1];
    for (int m = 0; m < 16; ++m) { iA[m][k1] = s * (a + rnd_in(-1, 1)); iA[m][k2] = -s * (a + rnd_in(-1, 1)); }
    for (int n = 0; n < 16; ++n) { iB[k1][n] = t * (b + rnd_in(-1, 1)); iB[k2][n] = t * (b + rnd_in(-1, 1)); }
  }
  for (int m = 0; m < 16; ++m) for (int k = 0; k < 16; ++k) A[m * 32 + k] = (_Float16)ldexpf((float)iA[m][k], ea);
  for (int k = 0; k < 16; ++k) for (int n = 0; n < 16; ++n) B[k * 16 + n] = (_Float16)ldexpf((float)iB[k][n], eb);
  for (int k = 16; k < 32; ++k) {
    const int qa = rnd_in(-2, 4), qb = rnd_in(-2, 8 - qa > 4 ? 4 : 8 - qa);
    for (int m = 0; m < 16; ++m) A[m * 32 + k] = (_Float16)ldexpf((float)(rnd_in(1024, 2047) * (rnd() & 1 ? 1 : -1)), ea + qa - 10);
    for (int n = 0; n < 16; ++n) B[k * 16 + n] = (_Float16)ldexpf((float)(rnd_in(1024, 2047) * (rnd() & 1 ? 1 : -1)), eb + qb - 10);
  }
  for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) {
    int64_t hs = 0, mag = 0;
    for (int k = 0; k < 16; ++k) { const int64_t p = (int64_t)iA[m][k] * iB[k][n]; hs += p; mag += p < 0 ? -p : p; }
    double ts = 0, tm = 0;
    for (int k = 16; k < 32; ++k) { const double p = (double)(float)A[m * 32 + k] * (double)(float)B[k * 16 + n]; ts += p; tm = fmax(tm, fabs(p)); }
    headsum[m * 16 + n] = hs; tailsum[m * 16 + n] = ts; tailmax[m * 16 + n] = tm; magmax[m * 16 + n] = (double)mag;
  }
}

static int fold_main(int draws, uint64_t seed) {
  fold_rng = seed;
  std::vector<_Float16> hA((size_t)draws * 512), hB((size_t)draws * 512);
  std::vector<int64_t> hs((size_t)draws * 256);
  std::vector<double> ts((size_t)draws * 256), tm((size_t)draws * 256), mg((size_t)draws * 256);
  std::vector<int> ee(draws);
  std::vector<float> hO((size_t)draws * 768);
  for (int d = 0; d < draws; ++d)
    fold_draw(&hA[(size_t)d * 512], &hB[(size_t)d * 512], &hs[(size_t)d * 256], &ts[(size_t)d * 256], &tm[(size_t)d * 256], &mg[(size_t)d * 256], &ee[d]);
  _Float16 *dA, *dB; float* dO;
  if (hipMalloc(&dA, hA.size() * 2) || hipMalloc(&dB, hB.size() * 2) || hipMalloc(&dO, hO.size() * 4)) { printf("hipMalloc failed\n"); return 2; }
  hipMemcpy(dA, hA.data(), hA.size() * 2, hipMemcpyHostToDevice); hipMemcpy(dB, hB.data(), hB.size() * 2, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe_fold, dim3(draws), dim3(64), 0, 0, dA, dB, dO);
  if (hipMemcpy(hO.data(), dO, hO.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel or copy failed\n"); return 2; }
  long a_bad = 0, b_diff = 0, b_bad = 0;
  double mag_lo = 1e300, mag_hi = 0, sum_hi = 0, b_worst = 0, f64_fold = 0, f64_parent = 0;
  for (int d = 0; d < draws; ++d) for (int e = 0; e < 256; ++e) {
    const size_t i = (size_t)d * 256 + e;
    const double grid = ldexp(1.0, ee[d]), exact_h = (double)hs[i] * grid, exact = exact_h + ts[i];
    const float r0 = hO[(size_t)d * 768 + e], r1 = hO[(size_t)d * 768 + 256 + e], r2 = hO[(size_t)d * 768 + 512 + e];
    mag_lo = fmin(mag_lo, mg[i]); mag_hi = fmax(mag_hi, mg[i]); sum_hi = fmax(sum_hi, fabs((double)hs[i]));
    if ((double)r0 != exact_h) { if (a_bad++ < 8) printf("  (a) draw %d row %d col %d: got %.9g exact %.9g (%lld grid units of 2^%d)\n", d, e >> 4, e & 15, r0, exact_h, (long long)hs[i], ee[d]); }
    const double unit = ulp_of(fmax(fabs((double)r2), tm[i]));
    const double db = fabs((double)r1 - (double)r2) / unit;
    if (db != 0) ++b_diff;
    if (db > 1.0) { if (b_bad++ < 8) printf("  (b) draw %d row %d col %d: folded %.9g parent %.9g f64 %.12g, %.3g units\n", d, e >> 4, e & 15, r1, r2, exact, db); }
    b_worst = fmax(b_worst, db);
    f64_fold = fmax(f64_fold, fabs((double)r1 - exact) / unit); f64_parent = fmax(f64_parent, fabs((double)r2 - exact) / unit);
  }
  printf("fold mode: %d draws x 256 elements, seed %llu\n", draws, (unsigned long long)seed);
  printf("heads: sum of |products| between %.6f and %.6f of 2^24 grid units; largest |true head sum| %.0f units (2^%.1f)\n",
         mag_lo / 16777216.0, mag_hi / 16777216.0, sum_hi, log2(sum_hi > 1 ? sum_hi : 1));
  printf("(a) heads alone, C = 0: %ld of %ld elements differ from the exact integer sum -> %s\n", a_bad, (long)draws * 256, a_bad ? "FAIL" : "pass");
  printf("(b) heads + tails in one MFMA against 16x16x16 heads then 16x16x32 tails: %ld elements differ, largest %.3g units in the last place of max(|u|, largest tail product); %ld above one unit -> %s\n",
         b_diff, b_worst, b_bad, b_bad ? "FAIL" : "pass");
  printf("    against the float64 sum, same unit: folded %.3g, parent %.3g\n", f64_fold, f64_parent);
  return (a_bad || b_bad) ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "fold"))
    return fold_main(argc > 2 ? atoi(argv[2]) : 4096, argc > 3 ? strtoull(argv[3], nullptr, 10) : 20240611ull);
  _Float16 hA[16 * 32], hB[32 * 16]; float hC[256], hO[256];
  _Float16 *dA, *dB; float *dC, *dO;
  hipMalloc(&dA, sizeof(hA)); hipMalloc(&dB, sizeof(hB)); hipMalloc(&dC, sizeof(hC)); hipMalloc(&dO, sizeof(hO));
  auto run = [&](int i, int j, int k, float big, float smallA, float smallB, float cin) {
    for (auto& v : hA) v = 0; for (auto& v : hB) v = 0; for (auto& v : hC) v = 0;
    for (int s = 0; s < 32; ++s) hB[s * 16 + 0] = (_Float16)1.0f;
    hA[i] = (_Float16)big; hA[j] = (_Float16)(-big); hA[k] = (_Float16)smallA; hB[k * 16 + 0] = (_Float16)smallB;
    hB[i * 16] = (_Float16)big; hB[j * 16] = (_Float16)big;
    hC[0] = cin;
    hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
    hipMemcpy(dC, hC, sizeof(hC), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dC, dO);
    hipMemcpy(hO, dO, sizeof(hO), hipMemcpyDeviceToHost);
    return hO[0];
  };
  const float sA = 1.0f + ldexpf(1.0f, -10), sB = 1.0f + ldexpf(1.0f, -10);       // product 1 + 2^-9 + 2^-20
  const double exact = (double)sA * sB;
  printf("exact small product %.10f\n", exact);
  const int pos[][3] = {{0, 1, 2}, {0, 2, 1}, {0, 4, 8}, {0, 8, 16}, {0, 16, 31}, {1, 30, 15}, {0, 31, 16}, {2, 3, 0}};
  for (auto& p : pos) {
    printf("slots +big %2d  -big %2d  small %2d :", p[0], p[1], p[2]);
    for (int e = 0; e <= 15; e += 1) {
      const float r = run(p[0], p[1], p[2], ldexpf(1.0f, e), sA, sB, 0.0f);         // products +-2^(2e)
      printf(" %d:%.3g", 2 * e, (r - exact));
    }
    printf("\n");
  }
  // C input: big in C, -big as a product, small as a product
  printf("C = +big, product -big, small product (slots 0, 5):");
  for (int e = 0; e <= 15; ++e) {
    for (auto& v : hA) v = 0; for (auto& v : hB) v = 0; for (auto& v : hC) v = 0;
    hA[0] = (_Float16)(-ldexpf(1.0f, e)); hB[0] = (_Float16)ldexpf(1.0f, e); hA[5] = (_Float16)sA; hB[5 * 16] = (_Float16)sB;
    hC[0] = ldexpf(1.0f, 2 * e);
    hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
    hipMemcpy(dC, hC, sizeof(hC), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dC, dO);
    hipMemcpy(hO, dO, sizeof(hO), hipMemcpyDeviceToHost);
    printf(" %d:%.3g", 2 * e, hO[0] - exact);
  }
  printf("\n");
  // rounding of the final sum: 32 products of (1 + 2^-10)^2 each -> exact 32 (1 + 2^-9 + 2^-20) = 32 + 2^-4 + 2^-15
  {
    for (auto& v : hA) v = 0; for (auto& v : hB) v = 0; for (auto& v : hC) v = 0;
    for (int s = 0; s < 32; ++s) { hA[s] = (_Float16)sA; hB[s * 16] = (_Float16)sB; }
    hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
    hipMemcpy(dC, hC, sizeof(hC), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dC, dO);
    hipMemcpy(hO, dO, sizeof(hO), hipMemcpyDeviceToHost);
    printf("32 equal products: got %.10f exact %.10f\n", hO[0], 32.0 * exact);
  }
  // subnormal f16 inputs honoured?
  {
    const float r = run(0, 1, 2, 1.0f, ldexpf(1.0f, -20), 1.0f, 0.0f);
    printf("subnormal f16 input 2^-20 x 1: got %.6g (2^-20 = %.6g)\n", r, ldexp(1.0, -20));
  }
  return 0;
}
