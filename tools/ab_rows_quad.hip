// Which block geometry should K11 (irbfn_amd/csrc/rows_quad_f64.hip) run?  Times rows_quad_f64_kernel<RT, MINW> -- 64 RT rows and
// 4 RT waves per block, MINW waves per SIMD asked of the register allocator -- at rows = 65 536, nd = 10, m = 1001 and 4097:
// ROUNDS interleaved rounds of INNER launches between two device events in one process, median [min .. max], and checks that
// every geometry gives the bits of the first (a row's sums do not depend on the geometry).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I irbfn_amd/csrc -o tools/_bin/ab_rows_quad tools/ab_rows_quad.hip
#include "../irbfn_amd/csrc/rows_quad_f64.hip"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace irbfn { thread_local int g_last_hip_error = 0; }

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("HIP error %d at line %d\n", (int)r_, __LINE__); return 1; } } while (0)

typedef int (*launch_t)(const float*, int64_t, int64_t, int, const double*, int64_t, int, double*, double*, hipStream_t);
struct Variant { const char* name; launch_t fn; };

int main() {
  const Variant vs[] = {{"RT=1 MINW=2 ( 64 rows, 4 waves)", launch_rows_quad<1, 2>}, {"RT=1 MINW=4 ( 64 rows, 4 waves)", launch_rows_quad<1, 4>},
                        {"RT=2 MINW=2 (128 rows, 8 waves)", launch_rows_quad<2, 2>}, {"RT=2 MINW=4 (128 rows, 8 waves)", launch_rows_quad<2, 4>}};
  const int NV = sizeof(vs) / sizeof(vs[0]), ROUNDS = 7, INNER = 3, nd = 10;
  const int64_t rows = 65536;
  for (int m : {1001, 4097}) {
    const int64_t ld = m + nd;
    std::vector<float> z((size_t)rows * ld);
    std::vector<double> p((size_t)m * ld);
    uint64_t s = 12345;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)((int64_t)(s >> 11) % 2001 - 1000) / 1000.0; };
    for (auto& e : z) e = (float)rnd();
    for (auto& e : p) e = rnd() / 32.0;
    float* zd; double *pd, *qd, *vd;
    CK(hipMalloc(&zd, z.size() * 4)); CK(hipMalloc(&pd, p.size() * 8)); CK(hipMalloc(&qd, rows * 8)); CK(hipMalloc(&vd, rows * nd * 8));
    CK(hipMemcpy(zd, z.data(), z.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(pd, p.data(), p.size() * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<double> q0(rows), v0(rows * nd), q(rows), v(rows * nd);
    std::vector<std::vector<float>> t(NV);
    for (int i = 0; i < NV; ++i) {                       // warm-up and the bitwise check
      CK(hipMemset(qd, 0xFF, rows * 8)); CK(hipMemset(vd, 0xFF, rows * nd * 8));
      if (vs[i].fn(zd, ld, rows, m, pd, ld, nd, qd, vd, 0) != IRBFN_OK) { printf("launch failed\n"); return 1; }
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(q.data(), qd, rows * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(v.data(), vd, rows * nd * 8, hipMemcpyDeviceToHost));
      if (i == 0) { q0 = q; v0 = v; }
      const bool same = !memcmp(q.data(), q0.data(), rows * 8) && !memcmp(v.data(), v0.data(), rows * nd * 8);
      printf("m = %4d  %s  %s\n", m, vs[i].name, i == 0 ? "the reference bits" : same ? "bit-identical to the first" : "DIFFERS from the first");
    }
    for (int r = 0; r < ROUNDS; ++r)
      for (int i = 0; i < NV; ++i) {
        CK(hipEventRecord(e0));
        for (int k = 0; k < INNER; ++k) vs[i].fn(zd, ld, rows, m, pd, ld, nd, qd, vd, 0);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        t[i].push_back(ms / INNER * 1e3f);
      }
    for (int i = 0; i < NV; ++i) {
      std::sort(t[i].begin(), t[i].end());
      printf("m = %4d  %s  %10.1f us  [%.1f .. %.1f]\n", m, vs[i].name, t[i][ROUNDS / 2], t[i].front(), t[i].back());
    }
    CK(hipFree(zd)); CK(hipFree(pd)); CK(hipFree(qd)); CK(hipFree(vd));
  }
  return 0;
}
