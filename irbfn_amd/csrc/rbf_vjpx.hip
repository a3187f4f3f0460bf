// x-VJP: kernel selection (plan_vjp_x) and launchers of K5 (rbf_vjpx_kernels.hip) and K5m (rbf_vjpx_mfma.hip).
// Design notes: rbf_vjpx.h.
#include <stdio.h>
#include <string.h>

#include "rbf_vjpx.h"

namespace irbfn {

static int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

// K5: waves per workgroup and LDS.  One query per lane, 64 queries per workgroup; as K1, enough waves to cover the chip
// (1024 SIMDs) several times while a wave keeps >= 32 centres (whole regions when it owns q[b,r] for dgamma)
static VjpxPlan plan_qlane_x(const irbfn_net* net, int64_t B, bool ext, bool region_split) {
  VjpxPlan p;
  const long tiles = (B + kWave - 1) / kWave;
  const int max_threads = net->OP > 48 ? 512 : 1024;
  long want = (16384 + tiles - 1) / tiles;
  int nw = want < 1 ? 1 : (want > 16 ? 16 : (int)want);
  nw = pow2_floor(nw);
  while (nw > 1 && net->N / nw < 32) nw /= 2;
  while (nw > 1 && net->N / nw < 128 && tiles * (nw / 2) >= 8192) nw /= 2;
  while (nw * kWave > max_threads) nw /= 2;
  if (region_split) {
    while (nw > 1 && nw > net->R) nw /= 2;
  }
  const size_t E = ext ? 0 : (size_t)net->nsplit * net->max_ranges;
  const size_t stage = (size_t)kWave * net->D + (size_t)kWave * (net->O | 1);
  const size_t red = (size_t)nw * net->DC * (kWave + 1);
  const size_t lds = (2 * E * kWave + (stage > red ? stage : red)) * sizeof(float);
  if (lds > 160 * 1024) return p;
  p.kind = VX_K5; p.status = IRBFN_OK;
  p.nw = nw; p.lds = lds; p.grid = tiles; p.block = nw * kWave;
  return p;
}

// the x-VJP's kernel for B > 0 queries.  K5m takes one region (the net's own gate), the three fast basis classes, d = 2..8 and
// O <= 128; IRBFN_VJPX_AUTO selects it for O > 16, where it was measured ahead (vjpxm_preferred), else K5
static VjpxPlan plan_vjp_x(const irbfn_net* net, int64_t B, bool ext, bool want_dgamma) {
  const int forced = net->opt[IRBFN_OPT_VJPX_KERNEL];
  if (forced == IRBFN_VJPX_K5M || (forced == IRBFN_VJPX_AUTO && vjpxm_preferred(net, B, ext))) {
    VjpxPlan p;
    if (ext || !vjpxm_eligible(net)) return p;   // forced but ineligible: IRBFN_ERR_UNSUPPORTED
    return plan_vjpx_mfma(net, B);
  }
  return plan_qlane_x(net, B, ext, want_dgamma);
}

static void record_vjpx(irbfn_net* net, const VjpxPlan& p, bool ext) {
  if (p.kind == VX_K5M)
    snprintf(net->last_name, sizeof(net->last_name), "rbf_vjpx_mfma<D=%d,OW=%d,BC=%d>", net->D, vjpxm_width(net), net->bclass);
  else
    snprintf(net->last_name, sizeof(net->last_name), "rbf_vjpx_qlane<D=%d,OP=%d,BC=%d,EXT=%d>", net->DC, net->OP, net->bclass, (int)ext);
  net->last_grid = (int)p.grid;
  net->last_block = p.block;
}

int launch_vjp_x(irbfn_net* net, const float* x, const float* gamma, const float* gout, float* gx, float* dgamma, int64_t B,
                 hipStream_t s) {
  if (B == 0) return IRBFN_OK;
  const bool ext = gamma != nullptr;
  const VjpxPlan p = plan_vjp_x(net, B, ext, dgamma != nullptr);
  if (p.kind == VX_NONE) return p.status;
  int rc;
  if (p.kind == VX_K5M) {
    rc = launch_vjpx_mfma(net, p, x, gout, gx, B, s);
  } else {
    VjpxArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.g = gout; a.rec = net->rec; a.gamma_ext = gamma; a.gx = gx; a.dgamma = dgamma;
    a.gate = net->gate();
    a.B = (long)B;
    a.Dreal = net->D; a.O = net->O; a.N = net->N; a.K = net->K; a.R = net->R; a.S = net->S; a.basis = net->basis;
    a.region_split = dgamma != nullptr;
    switch (net->DC) {
      case 3: rc = launch_vjpx_d3(a, net->OP, net->bclass, p.nw, p.lds, s); break;
      case 4: rc = launch_vjpx_d4(a, net->OP, net->bclass, p.nw, p.lds, s); break;
      case 7: rc = launch_vjpx_d7(a, net->OP, net->bclass, p.nw, p.lds, s); break;
      case 8: rc = launch_vjpx_d8(a, net->OP, net->bclass, p.nw, p.lds, s); break;
      default: rc = IRBFN_ERR_UNSUPPORTED; break;
    }
  }
  if (rc == IRBFN_OK) record_vjpx(net, p, ext);
  return rc;
}

}  // namespace irbfn
