// k_wvlcty.hip -- true vertical velocity w at rho points on the device:
// wvlcty_tile (wvlcty.F:18-192), for history files (wrt_W), averages files
// (wrt_avg_W) and the host.  Three parts, all of one column:
//   Wrk(0) = 0;  Wrk(k) = Wrk(k-1) - pm*pn*(FlxU(i+1)-FlxU(i)+FlxV(j+1)-FlxV(j))
//   (no grid-motion term, unlike omega: Wrk(N) /= 0), interpolated to rho levels
//   with the four-point weights 0.5625 / -0.0625 and the one-sided ends;
//   + 0.25*(Wxi(i)+Wxi(i+1)+Weta(j)+Weta(j+1)), the motion along s-surfaces,
//   Wxi(i) = u(i,nstp)*(z_r(i)-z_r(i-1))*(pm(i)+pm(i-1)), Weta alike in j;
//   gradient copies onto the physical edges and corners.  No mask multiply.
// The computed range is istr..iend x jstr..jend, one row wider on both sides in
// a periodic direction only (wvlcty.F:46-59).
//
// MI355X design: one lane per column, 64 consecutive i per wavefront, four rows
// per block, the levels walked upwards.  Wrk lives in a rolling window of four
// registers: level k-1 is emitted as soon as Wrk(k) exists, with the slope term
// of level k-1 carried one level in a register, so Wrk, Wxi and Weta never touch
// memory.  pm, pn of the column and its four neighbours stay in registers, and
// while the stored grid is set_depth's own the five z_r columns are formed from
// the kept free surface (VGrid) instead of streamed.  Per level a lane loads
// FlxU(i), FlxU(i+1), FlxV(j), FlxV(j+1), u(i), u(i+1), v(j), v(j+1): the
// neighbours' values come from the lines the wavefront and the block's other
// rows fetch anyway.  The lane that owns an edge column also writes the copy
// next to it, the corner lane the corner.  No LDS, no atomics.  Two sinks of the
// same body: a store into the work array, or the running mean
// avg = avg*(1-coef) + w*coef of the averages (at coef == 1 without the load).
// The reference's operand order, no contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/roms_gpu.h"
#include "roms_dev.h"
#include "shim_state.h"

namespace roms {
namespace {

// R: the computed range imin..imax x jmin..jmax; off: (nstp-1)*n3; out: element IJ = 0 of level 1
template <int SINK, bool VG>
__global__ void __launch_bounds__(256) k_wvlcty(Dev d, Range R, long off, double* __restrict__ out, double coef,
                                                 double cm1) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const int N = b.N;
  const long ij = IJ(b, i, j), n2 = b.n2, nx = b.nx2;
  // gradient copies (wvlcty.F:138-191): physical edges only, none in a periodic direction
  const bool cw = b.west_edge && i == R.i0, ce = b.east_edge && i == R.i1;
  const bool cs = b.south_edge && j == R.j0, cn = b.north_edge && j == R.j1;
  // old: the lane's own old mean of level k, loaded a level ahead with the level's other loads (kMean);
  // the copies next to an edge column update theirs in place
  auto emit = [&](int k, double w, double old) {
    double* __restrict__ o = out + ij + (long)(k - 1) * n2;
    if (SINK == kMean) *o = old * cm1 + w * coef;
    else sink_put<SINK>(o, w, coef, cm1);
    if (cw) sink_put<SINK>(o - 1, w, coef, cm1);
    if (ce) sink_put<SINK>(o + 1, w, coef, cm1);
    if (cs) {
      sink_put<SINK>(o - nx, w, coef, cm1);
      if (cw) sink_put<SINK>(o - nx - 1, w, coef, cm1);
      if (ce) sink_put<SINK>(o - nx + 1, w, coef, cm1);
    }
    if (cn) {
      sink_put<SINK>(o + nx, w, coef, cm1);
      if (cw) sink_put<SINK>(o + nx - 1, w, coef, cm1);
      if (ce) sink_put<SINK>(o + nx + 1, w, coef, cm1);
    }
  };
  const double pm0 = F.pm[ij], pn0 = F.pn[ij];
  const double mn = pm0 * pn0;
  const double pmw = pm0 + F.pm[ij - 1], pme = F.pm[ij + 1] + pm0;     // pm(i)+pm(i-1) of Wxi(i), Wxi(i+1)
  const double pns = pn0 + F.pn[ij - nx], pnn = F.pn[ij + nx] + pn0;   // pn(j)+pn(j-1) of Weta(j), Weta(j+1)
  VGrid g0, gw, ge, gs, gn;
  if constexpr (VG) {
    g0 = vg_column(d, ij); gw = vg_column(d, ij - 1); ge = vg_column(d, ij + 1);
    gs = vg_column(d, ij - nx); gn = vg_column(d, ij + nx);
  }
  const double* __restrict__ FU = F.FlxU + ij;
  const double* __restrict__ FV = F.FlxV + ij;
  const double* __restrict__ U = F.u + off + ij;
  const double* __restrict__ V = F.v + off + ij;
  const double* __restrict__ ZR = F.z_r + ij;
  double wm1 = 0.0, wm2 = 0.0, wm3 = 0.0;   // Wrk(k-1), Wrk(k-2), Wrk(k-3); Wrk(0) = 0
  double sl1 = 0.0;                          // the slope term of level k-1
  double oldtop = 0.0;                       // the old mean of level N (kMean)
#pragma unroll 2
  for (int k = 1; k <= N; k++) {
    const long o = (long)(k - 1) * n2;
    double old = 0.0, oldN = 0.0;
    if (SINK == kMean) {
      if (k >= 2) old = out[ij + o - n2];
      if (k == N) oldN = out[ij + o];
    }
    const double w = wm1 - mn * (FU[o + 1] - FU[o] + FV[o + nx] - FV[o]);
    double z0, zw, ze, zs, zn;
    if constexpr (VG) {
      const double csr = F.Cs_r[k];
      z0 = g0.zr(k, csr); zw = gw.zr(k, csr); ze = ge.zr(k, csr); zs = gs.zr(k, csr); zn = gn.zr(k, csr);
    } else {
      z0 = ZR[o]; zw = ZR[o - 1]; ze = ZR[o + 1]; zs = ZR[o - nx]; zn = ZR[o + nx];
    }
    const double wx0 = U[o] * (z0 - zw) * pmw, wx1 = U[o + 1] * (ze - z0) * pme;
    const double we0 = V[o] * (z0 - zs) * pns, we1 = V[o + nx] * (zn - z0) * pnn;
    const double sl = 0.25 * (wx0 + wx1 + we0 + we1);
    if (k == 2) emit(1, (-0.125 * w + 0.75 * wm1 + 0.375 * wm2) + sl1, old);
    else if (k > 2) emit(k - 1, (0.5625 * (wm1 + wm2) - 0.0625 * (w + wm3)) + sl1, old);
    wm3 = wm2; wm2 = wm1; wm1 = w; sl1 = sl; oldtop = oldN;
  }
  emit(N, (0.375 * wm1 + 0.75 * wm2 - 0.125 * wm3) + sl1, oldtop);
}

struct WvlCtx {
  double* base = nullptr;   // the allocation
  double* p = nullptr;      // element IJ = 0 of level 1, aligned like u
  bool have = false;        // a store launch filled it
};
thread_local WvlCtx Wv;

bool tlev_ok(const roms_tlev* t) { return t && t->nstp >= 1 && t->nstp <= 3; }

}  // namespace

double* wvl_alloc_like_u(const Dev& d, hipStream_t s, double** base) {
  const long n = d.b.n3;
  *base = nullptr;
  if (hipMalloc(base, (size_t)(n + kRowAlign) * sizeof(double)) != hipSuccess) return nullptr;
  // cells no launch writes (level planes outside the computed range and its copies) read as zero
  if (hipMemsetAsync(*base, 0, (size_t)(n + kRowAlign) * sizeof(double), s) != hipSuccess) {
    (void)hipFree(*base);
    *base = nullptr;
    return nullptr;
  }
  return *base + ((uintptr_t)d.f.u / sizeof(double)) % kRowAlign;
}

int wvl_launch(const ShimState& S, int nstp, double* out, int sink, double coef, double cm1) {
  const Dev& d = *S.d;
  const Bounds& b = d.b;
  if (b.N < 2) {
    *S.err = "wvlcty: N < 2 has no defined formula (the top level needs Wrk(N-2))";
    return -1;
  }
  // wvlcty.F:46-59: one more row on each side in a periodic direction only
  // (every rank of a periodic direction has istr = iwest, iend = ieast)
  Range R{b.istr, b.iend, b.jstr, b.jend};
  if (b.ew_periodic) { R.i0 = b.istr - 1 > b.istrE ? b.istr - 1 : b.istrE; R.i1 = b.iend + 1 < b.iendE ? b.iend + 1 : b.iendE; }
  if (b.ns_periodic) { R.j0 = b.jstr - 1 > b.jstrE ? b.jstr - 1 : b.jstrE; R.j1 = b.jend + 1 < b.jendE ? b.jend + 1 : b.jendE; }
  const long off = (long)(nstp - 1) * b.n3;
  const dim3 grid = grid_of(R), blk(kBX, kBY);
  const bool vg = shim_vgrid_valid();
#define ROMS_WVL_GO(SINK)                                                                                   \
  do {                                                                                                      \
    if (vg) hipLaunchKernelGGL((k_wvlcty<SINK, true>), grid, blk, 0, S.s, d, R, off, out, coef, cm1);      \
    else hipLaunchKernelGGL((k_wvlcty<SINK, false>), grid, blk, 0, S.s, d, R, off, out, coef, cm1);        \
  } while (0)
  ROMS_SINKS(sink, ROMS_WVL_GO);
#undef ROMS_WVL_GO
  if (hipGetLastError() != hipSuccess) { *S.err = "wvlcty: launch failed"; return -3; }
  return 0;
}

const double* wvl_compute(const ShimState& S, int nstp, int* rc) {
  *rc = 0;
  if (S.d->b.N < 2) { *rc = wvl_launch(S, nstp, nullptr, kStore, 1.0, 0.0); return nullptr; }
  if (!Wv.p) {
    Wv.p = wvl_alloc_like_u(*S.d, S.s, &Wv.base);
    if (!Wv.p) { *S.err = "wvlcty: allocation of the work array failed"; *rc = -2; return nullptr; }
  }
  if ((*rc = wvl_launch(S, nstp, Wv.p, kStore, 1.0, 0.0))) return nullptr;
  Wv.have = true;
  return Wv.p;
}

void wvl_free() {
  if (Wv.base) (void)hipFree(Wv.base);
  Wv = WvlCtx{};
}

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_wvlcty(const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!tlev_ok(t)) { *S.err = "roms_gpu_wvlcty: bad time levels"; return -1; }
  (void)wvl_compute(S, t->nstp, &r);
  return r;
}

int roms_gpu_wvlcty_copy_out(double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Wv.have || !dst) { *S.err = "roms_gpu_wvlcty_copy_out: nothing was computed (roms_gpu_wvlcty)"; return -4; }
  const Bounds& b = S.d->b;
  const long rows = (long)b.N * (b.Mm + 4);
  if (count != rows * (b.Lm + 4)) { *S.err = "roms_gpu_wvlcty_copy_out: count is not N*(Mm+4)*(Lm+4)"; return -1; }
  if (shim_rows_d2h(dst, Wv.p, rows) != hipSuccess) { *S.err = "roms_gpu_wvlcty_copy_out: copy failed"; return -2; }
  return 0;
}

// n launches of each sink between two events on the library stream
// (tools/wvlcty_cost.py): ms[0] the store into the work array, ms[1] the
// running-mean sink with the old mean read, into the armed window's mean of w
// (0 when ROMS_WRT_W is not armed).  The mean goes on from the open window with
// coef = 1/2: re-arm before the averages are used
int roms_gpu_time_wvlcty(int n, const roms_tlev* t, double* ms) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!tlev_ok(t) || n < 1 || !ms) { *S.err = "roms_gpu_time_wvlcty: bad arguments"; return -1; }
  (void)wvl_compute(S, t->nstp, &r);   // allocates; an untimed first launch
  if (r) return r;
  double* mean = avg_view().wvl;
  ms[0] = time_rounds(S.s, n, false, [&]() { return wvl_launch(S, t->nstp, Wv.p, kStore, 1.0, 0.0); });
  ms[1] = mean && ms[0] >= 0 ? time_rounds(S.s, n, false, [&]() { return wvl_launch(S, t->nstp, mean, kMean, 0.5, 0.5); }) : 0.0;
  if (ms[0] < 0 || ms[1] < 0) {
    *S.err = "roms_gpu_time_wvlcty: launch or timing failed";
    return (int)(ms[0] < 0 ? ms[0] : ms[1]);
  }
  return 0;
}

}  // extern "C"
