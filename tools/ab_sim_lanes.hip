// How many lanes should share a car in K12 (irbfn_amd/csrc/sim_advance.hip)?  Times sim_advance_kernel<G, SELECT> for G = 8, 16, 64
// at B = 1024 and 65 536 on a closed line of 1000 way-points, for the default window (8 back, 55 ahead) and the whole line:
// ROUNDS interleaved rounds of INNER launches between two device events in one process, median [min .. max], and checks that
// every layout gives the bits of the first (a car's result does not depend on the layout).  Every launch includes a plant
// step with dt = 1e-4 s, so that the cars stay where they are and none is frozen during the timed launches.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I include -I irbfn_amd/csrc -o tools/_bin/ab_sim_lanes tools/ab_sim_lanes.hip
#include "../irbfn_amd/csrc/sim_advance.hip"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace irbfn { thread_local int g_last_hip_error = 0; }

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("HIP error %d at line %d\n", (int)r_, __LINE__); return 1; } } while (0)

typedef int (*launch_t)(const SimArgs&, bool, hipStream_t);
struct Variant { const char* name; launch_t fn; };

int main() {
  const Variant vs[] = {{"16 lanes per car", launch_sim<16>}, {" 8 lanes per car", launch_sim<8>}, {"64 lanes per car", launch_sim<64>}};
  const int NV = sizeof(vs) / sizeof(vs[0]), ROUNDS = 7, INNER = 200, N = 1000, T = 5;
  // the line: an ellipse, way-points about 0.4 m apart, and its arc-length tables
  std::vector<double> wp(4 * N), cum(N - 1), len(N - 1);
  const double r = 0.08 * N, two_pi = 6.283185307179586;
  for (int i = 0; i < N; ++i) {
    const double th = two_pi * i / N;
    wp[4 * i] = r * cos(th); wp[4 * i + 1] = 0.6 * r * sin(th); wp[4 * i + 2] = th + 1.5707963267948966; wp[4 * i + 3] = 2.5 + cos(2 * th);
  }
  double total = 0.0;
  for (int i = 0; i + 1 < N; ++i) {
    len[i] = hypot(wp[4 * i + 4] - wp[4 * i], wp[4 * i + 5] - wp[4 * i + 1]);
    cum[i] = total;
    total += len[i];
  }
  total += hypot(wp[0] - wp[4 * (N - 1)], wp[1] - wp[4 * (N - 1) + 1]);
  double *wpd, *cumd, *lend;
  CK(hipMalloc(&wpd, wp.size() * 8)); CK(hipMalloc(&cumd, cum.size() * 8)); CK(hipMalloc(&lend, len.size() * 8));
  CK(hipMemcpy(wpd, wp.data(), wp.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(cumd, cum.data(), cum.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(lend, len.data(), len.size() * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (long B : {1024L, 65536L}) {
    // cars within 0.2 m of the line (per axis) at 1 .. 5 m/s, each on the segment its seg word names
    std::vector<float> st(7 * B, 0.0f), ctrl(2 * T * B, 0.0f);
    std::vector<int> seg(B);
    uint64_t s = 12345 + B;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
    for (long b = 0; b < B; ++b) {
      const int j = (int)(rnd() * (N - 1));
      seg[b] = j;
      st[7 * b] = (float)(wp[4 * j] + 0.4 * (rnd() - 0.5)); st[7 * b + 1] = (float)(wp[4 * j + 1] + 0.4 * (rnd() - 0.5));
      st[7 * b + 3] = (float)(1.0 + 4.0 * rnd()); st[7 * b + 4] = (float)(wp[4 * j + 2] + 0.4 * (rnd() - 0.5));
      ctrl[2 * T * b] = 0.2f;
    }
    float *std_, *ctrld, *xd; int *segd, *statd, *mird; double* recd;
    CK(hipMalloc(&std_, st.size() * 4)); CK(hipMalloc(&ctrld, ctrl.size() * 4)); CK(hipMalloc(&xd, 7 * B * 4));
    CK(hipMalloc(&segd, B * 4)); CK(hipMalloc(&statd, B * 4)); CK(hipMalloc(&mird, B * 4)); CK(hipMalloc(&recd, kSimRecord * B * 8));
    CK(hipMemcpy(ctrld, ctrl.data(), ctrl.size() * 4, hipMemcpyHostToDevice));
    for (int whole = 0; whole < 2; ++whole) {
      SimArgs a;
      memset(&a, 0, sizeof(a));
      a.tr = irbfn_sim_track{wpd, cumd, lend, total, 1.5, 4.0, 0.0, N, 1, whole ? -1 : 8, whole ? -1 : 55};
      const float dyn[13] = {1.0f, 1.0489f, 0.04712f, 0.15875f, 0.17145f, 5.0f, 5.0f, 0.074f, 1e-4f, 3.2f, 9.51f, 0.4189f, 7.0f};
      for (int i = 0; i < 13; ++i) a.dp.p[i] = dyn[i];
      a.controls = ctrld; a.T = T; a.n_sub = 1; a.tick = 1;
      a.state = std_; a.seg = segd; a.status = statd; a.record = recd; a.x = xd; a.mirror = mird; a.B = B;
      auto reset = [&]() -> int {
        CK(hipMemcpy(std_, st.data(), st.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(segd, seg.data(), B * 4, hipMemcpyHostToDevice));
        CK(hipMemset(statd, 0, B * 4)); CK(hipMemset(recd, 0, kSimRecord * B * 8)); CK(hipMemset(xd, 0xFF, 7 * B * 4));
        return 0;
      };
      const char* wname = whole ? "whole line   " : "window (8,55)";
      std::vector<float> x0(7 * B), x(7 * B);
      std::vector<int> stat(B);
      std::vector<std::vector<float>> t(NV);
      for (int i = 0; i < NV; ++i) {                     // warm-up and the bitwise check on one launch from the same states
        if (reset()) return 1;
        if (vs[i].fn(a, true, 0) != IRBFN_OK) { printf("launch failed\n"); return 1; }
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(x.data(), xd, 7 * B * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(stat.data(), statd, B * 4, hipMemcpyDeviceToHost));
        if (i == 0) x0 = x;
        long live = 0;
        for (long b = 0; b < B; ++b) live += stat[b] == 0;
        printf("B = %6ld  %s  %s  %s, %ld cars driving\n", B, wname, vs[i].name,
               i == 0 ? "the reference bits" : !memcmp(x.data(), x0.data(), 7 * B * 4) ? "bit-identical to the first" : "DIFFERS from the first", live);
      }
      for (int rd = 0; rd < ROUNDS; ++rd)
        for (int i = 0; i < NV; ++i) {
          if (reset()) return 1;
          CK(hipEventRecord(e0));
          for (int k = 0; k < INNER; ++k) vs[i].fn(a, true, 0);
          CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
          float ms; CK(hipEventElapsedTime(&ms, e0, e1));
          t[i].push_back(ms / INNER * 1e3f);
        }
      CK(hipMemcpy(stat.data(), statd, B * 4, hipMemcpyDeviceToHost));
      long live = 0;
      for (long b = 0; b < B; ++b) live += stat[b] == 0;
      for (int i = 0; i < NV; ++i) {
        std::sort(t[i].begin(), t[i].end());
        printf("B = %6ld  %s  %s  %10.1f us  [%.1f .. %.1f]\n", B, wname, vs[i].name, t[i][ROUNDS / 2], t[i].front(), t[i].back());
      }
      printf("B = %6ld  %s  cars still driving after the last round: %ld\n\n", B, wname, live);
    }
    CK(hipFree(std_)); CK(hipFree(ctrld)); CK(hipFree(xd)); CK(hipFree(segd)); CK(hipFree(statd)); CK(hipFree(mird)); CK(hipFree(recd));
  }
  return 0;
}
