// k_uvdiag.hip -- the term-by-term momentum budget of the corrector on the device:
// DIAGNOSTICS with diag_uv (diagnostics.F and its hooks in prsgrd.F, compute_horiz_rhs_uv_terms.h, step3d_uv1.F,
// visc3d_S.F, step3d_uv2.F), the IMPLICIT_BOTTOM_DRAG branch.  Seven terms per component, m2/s2, N planes each in
// the layout of u (of v); the u terms at i = istrU..iend, j = jstr..jend, the v terms at i = istr..iend,
// j = jstrV..jend, 0 elsewhere (include/roms_gpu.h, ABI 31).  With dxdyi_u = 0.25*(pn(i-1,j)+pn(i,j))*
// (pm(i-1,j)+pm(i,j)) (diagnostics.F:211-214) and the v forms the mirror image in eta:
//   pgr = ru*dxdyi_u*umask, ru as the corrector's prsgrd leaves it (prsgrd.F:462)
//   cor = 0.5*(UFx(i,j)+UFx(i-1,j))*dxdyi_u, v: -0.5*(VFe(i,j)+VFe(i,j-1))*dxdyi_v, UFx, VFe the Coriolis /
//     curvilinear products over u, v(nrhs) (compute_horiz_rhs_uv_terms.h:4-14, 32-33)
//   adv = -dxdyi_u*(FX4(i)-FX4(i-1)+FY4(j+1)-FY4(j)) - dxdyi_u*(FZ4(k)-FZ4(k-1)) (diagnostics.F:238-439): centred
//     fourth-order fluxes inv24*(flux pair)*(-q + 7q - q + 7q) of u, v(nrhs) with the corrector's FlxU, FlxV, We+Wi;
//     the second-order form 0.25*(flux pair)*(q + q) at the first and last flux of a physical, non-periodic edge
//     of the whole grid (the reference tests *_msg_exch: the same thing on a closed single-rank grid; on a
//     periodic side or a rank boundary the form stays fourth order, so a decomposed run is bitwise the single
//     domain) and at k = 1, N-1; FZ4(0) = FZ4(N) = 0
//   dis = ru*dxdyi_u*umask - pgr - cor - adv, ru the final right-hand side of step3d_uv1 (step3d_uv1.F:211-214)
//   vmx = (u(nnew) - u_prev)/dt - ru*dxdyi_u, u_prev the u(nnew) step3d_uv1 was given, u(nnew) the Hz*u its implicit
//     solve leaves (:141-144, 215-216)
//   hmx = 0.5*dxdyi_u*((pn(i-1,j)+pn(i,j))*(UFx(i,j)-UFx(i-1,j)) + (pm(i-1,j)+pm(i,j))*(UFe(i,j+1)-UFe(i,j))), the
//     stresses of visc3d over u, v(nstp) (visc3d_S.F:55-91, 122-127); 0 without UV_VIS2
//   cpl = -DC(i,0)*umask*0.5*(Hz(i,j,k)+Hz(i-1,j,k))/dt, DC(i,0) the mismatch step3d_uv2 removes (step3d_uv2.F:
//     244-278), summed in k_uv2_couple's order
//   means (calc_diag_avg, :709-732): navg += 1; coef = 1/navg; X_avg = X_avg*(1-coef) + X*coef, one sample per
//     corrector
//
// MI355X design.  The snapshots are streaming kernels, one lane per point and level.  k_uvdiag_rhs: one lane per
// (u point, v point) pair at (i,j), 64 consecutive i per wavefront, four rows per block, the levels walked upwards
// with the four u(nrhs) and v(nrhs) levels of FZ4 in a rolling register window and the metric factors, masks and
// edge tests formed once per lane; the horizontal stencils are read from global memory directly (the neighbours'
// lines are the ones the wavefront and the block's other rows fetch anyway).  k_uvdiag_hmx: one lane per pair and
// level, the six stresses around it from visc_rho / visc_psi's expressions.  k_uvdiag_cpl: one column per lane and
// direction.  Each takes its sink as a template parameter like k_tdiag: store, or the running mean, which at
// coef == 1 does not load the old mean.  The reference's operand order, no contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "k_common.h"
#include "shim_state.h"

namespace roms {
namespace {

// the device arrays: [0..6] the u terms ROMS_UVD_PGR..CPL, [7..13] the v terms, then the four snapshots
constexpr int kUvTerms = 7, kUvRuPgr = 14, kUvRvPgr = 15, kUvUPrev = 16, kUvVPrev = 17, kUvArr = 18;
struct UvArrs {
  double* p[kUvArr];   // element IJ = 0 of level 1
};

__device__ __forceinline__ double uv_dxdyi(const Fields& F, long ij, long s) {
  return 0.25 * (F.pn[ij - s] + F.pn[ij]) * (F.pm[ij - s] + F.pm[ij]);
}

// ru_pgr = ru*dxdyi_u*umask, rv_pgr alike, after the corrector's prsgrd
__global__ void __launch_bounds__(256) k_uvdiag_snap_r(Dev d, Range R, UvArrs A) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const long ij = IJ(b, i, j), o = ij + (long)bI.z * b.n2;
  if (i >= b.istrU) A.p[kUvRuPgr][o] = F.ru[o] * uv_dxdyi(F, ij, 1) * F.umask[ij];
  if (j >= b.jstrV) A.p[kUvRvPgr][o] = F.rv[o] * uv_dxdyi(F, ij, b.nx2) * F.vmask[ij];
}

// u_prev = u(nnew), v_prev = v(nnew) on entry to step3d_uv1
__global__ void __launch_bounds__(256) k_uvdiag_snap_q(Dev d, Range R, int nnew, UvArrs A) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const long o = IJ(b, i, j) + (long)bI.z * b.n2, l = (long)(nnew - 1) * b.n3;
  if (i >= b.istrU) A.p[kUvUPrev][o] = d.f.u[o + l];
  if (j >= b.jstrV) A.p[kUvVPrev][o] = d.f.v[o + l];
}

__device__ __forceinline__ double uv_f4(double a, double b, double c, double e) { return -a + 7.0 * b - c + 7.0 * e; }

// pgr, cor, adv, dis, vmx after step3d_uv1 and before visc3d.  R: istr..iend x jstr..jend
template <int SINK>
__global__ void __launch_bounds__(256) k_uvdiag_rhs(Dev d, Range R, int nnew, int nrhs, UvArrs A, double coef,
                                                    double cm1) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const bool du = i >= b.istrU, dv = j >= b.jstrV;
  if (!du && !dv) return;
  const int N = b.N;
  const long ij = IJ(b, i, j), n2 = b.n2, nx = b.nx2;
  const double inv24 = 1.0 / 24.0, dt = d.p.dt;
  const double dxu = uv_dxdyi(F, ij, 1), dxv = uv_dxdyi(F, ij, nx);
  const double um = F.umask[ij], vm = F.vmask[ij];
  // the second-order faces: the first and last flux of a physical, non-periodic edge of the whole grid
  const bool W = b.west_edge, E = b.east_edge, S = b.south_edge, Nn = b.north_edge;
  const bool ux0 = (W && i == b.istr) || (E && i == b.iend), uxm = W && i - 1 == b.istr;   // FX4(i), FX4(i-1) of u
  const bool uy1 = Nn && j == b.jend, uy0 = S && j == b.jstr;                                // FY4(j+1), FY4(j) of u
  const bool vx1 = E && i == b.iend, vx0 = W && i == b.istr;                                 // FX4(i+1), FX4(i) of v
  const bool vy0 = (S && j == b.jstr) || (Nn && j == b.jend), vym = S && j - 1 == b.jstr;   // FY4(j), FY4(j-1) of v
  const bool ucor = d.p.uv_cor, curv = d.p.curvgrid, corb = ucor || curv;
  const double* __restrict__ Ur = F.u + (long)(nrhs - 1) * b.n3;
  const double* __restrict__ Vr = F.v + (long)(nrhs - 1) * b.n3;
  const double* __restrict__ Un = F.u + (long)(nnew - 1) * b.n3;
  const double* __restrict__ Vn = F.v + (long)(nnew - 1) * b.n3;
  auto lev = [&](int k) { return (long)(min(max(k, 1), N) - 1) * n2; };
  // the rolling windows of FZ4: q(k-1), q(k), q(k+1), q(k+2)
  double ua = 0.0, ub = du ? Ur[ij] : 0.0, uc = du ? Ur[ij + lev(2)] : 0.0, ud = du ? Ur[ij + lev(3)] : 0.0;
  double va = 0.0, vb = dv ? Vr[ij] : 0.0, vc = dv ? Vr[ij + lev(2)] : 0.0, vd = dv ? Vr[ij + lev(3)] : 0.0;
  double fzu = 0.0, fzv = 0.0;   // FZ4(k-1)
  for (int k = 1; k <= N; k++) {
    const long kk = (long)(k - 1) * n2, o = ij + kk, w = ij + (long)k * n2;
    const double* __restrict__ U = Ur + kk;
    const double* __restrict__ V = Vr + kk;
    const double* __restrict__ FU = F.FlxU + kk;
    const double* __restrict__ FV = F.FlxV + kk;
    const bool face = k < N, second = k == 1 || k == N - 1;
    auto cff = [&](long mn) {   // compute_horiz_rhs_uv_terms.h:4-12 at the rho point mn
      if (curv) {
        const double ct = 0.5 * ((V[mn] + V[mn + nx]) * F.dndx[mn] - (U[mn] + U[mn + 1]) * F.dmde[mn]);
        return 0.5 * F.Hz[mn + kk] * (ucor ? F.fomn[mn] + ct : ct);
      }
      return 0.5 * F.Hz[mn + kk] * (F.fomn[mn]);
    };
    if (du) {
      auto FX = [&](long p, bool two) {   // the Uu flux east of u(p)
        const double fu = FU[p] + FU[p + 1];
        return two ? 0.25 * fu * (U[p] + U[p + 1]) : inv24 * fu * uv_f4(U[p - 1], U[p], U[p + 2], U[p + 1]);
      };
      auto FY = [&](long p, bool two) {   // the Vu flux south of u(p)
        const double fv = FV[p - 1] + FV[p];
        return two ? 0.25 * fv * (U[p] + U[p - nx]) : inv24 * fv * uv_f4(U[p - 2 * nx], U[p - nx], U[p + nx], U[p]);
      };
      double adv = -dxu * (FX(ij, ux0) - FX(ij - 1, uxm) + FY(ij + nx, uy1) - FY(ij, uy0));
      double fz = 0.0;
      if (face) {
        const double wk = F.We[w - 1] + F.We[w] + F.Wi[w - 1] + F.Wi[w];
        fz = second ? 0.25 * wk * (ub + uc) : inv24 * wk * uv_f4(ua, ub, ud, uc);
      }
      adv = adv - dxu * (fz - fzu);
      fzu = fz;
      double cr = 0.0;
      if (corb) {
        const double U0 = cff(ij) * (V[ij] + V[ij + nx]), U1 = cff(ij - 1) * (V[ij - 1] + V[ij - 1 + nx]);
        cr = 0.5 * (U0 + U1) * dxu;
      }
      const double pg = A.p[kUvRuPgr][o], rf = F.ru[o];
      const double ds = rf * dxu * um - pg - cr - adv;
      const double vx = (Un[o] - A.p[kUvUPrev][o]) / dt - rf * dxu;
      sink_put<SINK>(A.p[0] + o, pg, coef, cm1);
      sink_put<SINK>(A.p[1] + o, cr, coef, cm1);
      sink_put<SINK>(A.p[2] + o, adv, coef, cm1);
      sink_put<SINK>(A.p[3] + o, ds, coef, cm1);
      sink_put<SINK>(A.p[5] + o, vx, coef, cm1);
      ua = ub; ub = uc; uc = ud; ud = Ur[ij + lev(k + 3)];
    }
    if (dv) {
      auto FX = [&](long p, bool two) {   // the Uv flux west of v(p)
        const double fu = FU[p - nx] + FU[p];
        return two ? 0.25 * fu * (V[p - 1] + V[p]) : inv24 * fu * uv_f4(V[p - 2], V[p - 1], V[p + 1], V[p]);
      };
      auto FY = [&](long p, bool two) {   // the Vv flux north of v(p)
        const double fv = FV[p] + FV[p + nx];
        return two ? 0.25 * fv * (V[p] + V[p + nx]) : inv24 * fv * uv_f4(V[p - nx], V[p], V[p + 2 * nx], V[p + nx]);
      };
      double adv = -dxv * (FX(ij + 1, vx1) - FX(ij, vx0) + FY(ij, vy0) - FY(ij - nx, vym));
      double fz = 0.0;
      if (face) {
        const double wk = F.We[w - nx] + F.Wi[w - nx] + F.We[w] + F.Wi[w];
        fz = second ? 0.25 * wk * (vb + vc) : inv24 * wk * uv_f4(va, vb, vd, vc);
      }
      adv = adv - dxv * (fz - fzv);
      fzv = fz;
      double cr = 0.0;
      if (corb) {
        const double V0 = cff(ij) * (U[ij] + U[ij + 1]), V1 = cff(ij - nx) * (U[ij - nx] + U[ij - nx + 1]);
        cr = -0.5 * (V0 + V1) * dxv;
      }
      const double pg = A.p[kUvRvPgr][o], rf = F.rv[o];
      const double ds = rf * dxv * vm - pg - cr - adv;
      const double vx = (Vn[o] - A.p[kUvVPrev][o]) / dt - rf * dxv;
      sink_put<SINK>(A.p[7] + o, pg, coef, cm1);
      sink_put<SINK>(A.p[8] + o, cr, coef, cm1);
      sink_put<SINK>(A.p[9] + o, adv, coef, cm1);
      sink_put<SINK>(A.p[10] + o, ds, coef, cm1);
      sink_put<SINK>(A.p[12] + o, vx, coef, cm1);
      va = vb; vb = vc; vc = vd; vd = Vr[ij + lev(k + 3)];
    }
  }
}

// visc_rho / visc_psi's expressions (k_step3d_uv.hip, visc3d_S.F:58-89) at the 2-D offset ij of level offset kk
__device__ __forceinline__ void uvd_rho(const Dev& d, long ij, long kk, long l, double& UFx, double& VFe) {
  const Fields& F = d.f;
  const double* pm = F.pm;
  const double* pn = F.pn;
  const long sj = d.b.nx2, o = ij + kk;
  const double cff = 0.5 * F.Hz[o] * F.visc2_r[ij] *
                     (F.dn_r[ij] * pm[ij] * ((pn[ij] + pn[ij + 1]) * F.u[o + 1 + l] - (pn[ij - 1] + pn[ij]) * F.u[o + l]) -
                      F.dm_r[ij] * pn[ij] * ((pm[ij] + pm[ij + sj]) * F.v[o + sj + l] - (pm[ij - sj] + pm[ij]) * F.v[o + l]));
  UFx = cff * F.dn_r[ij] * F.dn_r[ij];
  VFe = -cff * F.dm_r[ij] * F.dm_r[ij];
}
__device__ __forceinline__ void uvd_psi(const Dev& d, long ij, long kk, long l, double& UFe, double& VFx) {
  const Fields& F = d.f;
  const double* pm = F.pm;
  const double* pn = F.pn;
  const long sj = d.b.nx2, o = ij + kk;
  const double cff =
      0.125 * (F.Hz[o - 1] + F.Hz[o] + F.Hz[o - 1 - sj] + F.Hz[o - sj]) * F.visc2_p[ij] *
      (0.25 * (pm[ij - 1] + pm[ij] + pm[ij - 1 - sj] + pm[ij - sj]) * F.dn_p[ij] *
           ((pn[ij - sj] + pn[ij]) * F.v[o + l] - (pn[ij - 1 - sj] + pn[ij - 1]) * F.v[o - 1 + l]) +
       0.25 * (pn[ij - 1] + pn[ij] + pn[ij - 1 - sj] + pn[ij - sj]) * F.dm_p[ij] *
           ((pm[ij - 1] + pm[ij]) * F.u[o + l] - (pm[ij - 1 - sj] + pm[ij - sj]) * F.u[o - sj + l])) *
      F.pmask[ij];
  UFe = cff * F.dm_p[ij] * F.dm_p[ij];
  VFx = cff * F.dn_p[ij] * F.dn_p[ij];
}

// hmx beside visc3d (u, v(nstp) and Hz are inputs it leaves alone).  R: istr..iend x jstr..jend, grid z = level
template <int SINK>
__global__ void __launch_bounds__(256) k_uvdiag_hmx(Dev d, Range R, int nstp, UvArrs A, double coef, double cm1) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const bool du = i >= b.istrU, dv = j >= b.jstrV;
  if (!du && !dv) return;
  const long ij = IJ(b, i, j), sj = b.nx2, kk = (long)bI.z * b.n2, l = (long)(nstp - 1) * b.n3, o = ij + kk;
  const double* pm = F.pm;
  const double* pn = F.pn;
  double UFx0, VFe0, UFe0, VFx0, t0, t1;
  uvd_rho(d, ij, kk, l, UFx0, VFe0);
  uvd_psi(d, ij, kk, l, UFe0, VFx0);
  if (du) {
    double UFxm, UFe1;
    uvd_rho(d, ij - 1, kk, l, UFxm, t0);
    uvd_psi(d, ij + sj, kk, l, UFe1, t1);
    const double h = 0.5 * uv_dxdyi(F, ij, 1) *
                     ((pn[ij - 1] + pn[ij]) * (UFx0 - UFxm) + (pm[ij - 1] + pm[ij]) * (UFe1 - UFe0));
    sink_put<SINK>(A.p[4] + o, h, coef, cm1);
  }
  if (dv) {
    double VFx1, VFem;
    uvd_psi(d, ij + 1, kk, l, t0, VFx1);
    uvd_rho(d, ij - sj, kk, l, t1, VFem);
    const double h = 0.5 * uv_dxdyi(F, ij, sj) *
                     ((pn[ij - sj] + pn[ij]) * (VFx1 - VFx0) + (pm[ij - sj] + pm[ij]) * (VFe0 - VFem));
    sink_put<SINK>(A.p[11] + o, h, coef, cm1);
  }
}

// cpl on entry to step3d_uv2: k_uv2_couple's sums in its order.  R: istr..iend x jstr..jend, grid z = direction
template <int SINK>
__global__ void __launch_bounds__(256) k_uvdiag_cpl(Dev d, Range R, int nnew, UvArrs A, double coef, double cm1) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const int N = b.N, dir = (int)bI.z;
  if (dir == 0 ? i < b.istrU : j < b.jstrV) return;
  const long ij = IJ(b, i, j), n2 = b.n2, s = dir == 0 ? 1 : b.nx2;
  const double* __restrict__ Un = (dir == 0 ? F.u : F.v) + (long)(nnew - 1) * b.n3 + ij;
  const double* __restrict__ Hz = F.Hz + ij;
  const double dn = dir == 0 ? F.dn_u[ij] : F.dm_v[ij];
  const double avg1 = dir == 0 ? F.DU_avg1[ij] : F.DV_avg1[ij];
  const double msk = dir == 0 ? F.umask[ij] : F.vmask[ij];
  const double dt = d.p.dt;
  long o = (long)(N - 1) * n2;
  double CF0 = 0.5 * (Hz[o] + Hz[o - s]);
  double DC0 = Un[o];
#pragma unroll 8
  for (int k = N - 1; k >= 1; k--) {
    o = (long)(k - 1) * n2;
    CF0 = CF0 + 0.5 * (Hz[o] + Hz[o - s]);
    DC0 = DC0 + Un[o];
  }
  DC0 = (DC0 * dn - avg1) / (CF0 * dn);
  double* __restrict__ out = A.p[dir == 0 ? 6 : 13] + ij;
#pragma unroll 4
  for (int k = 1; k <= N; k++) {
    o = (long)(k - 1) * n2;
    sink_put<SINK>(out + o, -DC0 * msk * 0.5 * (Hz[o] + Hz[o - s]) / dt, coef, cm1);
  }
}

struct UvCtx {
  double* base[kUvArr] = {};
  UvArrs A = {};
  bool armed = false, sampling = false;
  bool open = false;        // step3d_uv1 opened a sample that step3d_uv2 has not closed
  bool hmx_done = false, cpl_done = false;
  MeanWindow w;             // coef, cm1 of the open sample
  bool have = false;        // a complete sample since begin (avg: since the last record); w.have is set a sample early
};
thread_local UvCtx Uv;

void uv_release() {
  for (double* q : Uv.base)
    if (q) (void)hipFree(q);
  Uv = UvCtx{};
}

Range uv_range(const Bounds& b) { return Range{b.istr, b.iend, b.jstr, b.jend}; }

void launch_snap_r(const Dev& d, hipStream_t s) {
  const Range R = uv_range(d.b);
  hipLaunchKernelGGL(k_uvdiag_snap_r, grid3_of(R, d.b.N), dim3(kBX, kBY), 0, s, d, R, Uv.A);
}
void launch_snap_q(const Dev& d, hipStream_t s, int nnew) {
  const Range R = uv_range(d.b);
  hipLaunchKernelGGL(k_uvdiag_snap_q, grid3_of(R, d.b.N), dim3(kBX, kBY), 0, s, d, R, nnew, Uv.A);
}
void launch_rhs(const Dev& d, hipStream_t s, int nnew, int nrhs, int sink, double coef, double cm1) {
  const Range R = uv_range(d.b);
#define ROMS_UV_RHS(SINK) \
  hipLaunchKernelGGL((k_uvdiag_rhs<SINK>), grid_of(R), dim3(kBX, kBY), 0, s, d, R, nnew, nrhs, Uv.A, coef, cm1)
  ROMS_SINKS(sink, ROMS_UV_RHS);
#undef ROMS_UV_RHS
}
void launch_hmx(const Dev& d, hipStream_t s, int nstp, int sink, double coef, double cm1) {
  const Range R = uv_range(d.b);
#define ROMS_UV_HMX(SINK) \
  hipLaunchKernelGGL((k_uvdiag_hmx<SINK>), grid3_of(R, d.b.N), dim3(kBX, kBY), 0, s, d, R, nstp, Uv.A, coef, cm1)
  ROMS_SINKS(sink, ROMS_UV_HMX);
#undef ROMS_UV_HMX
}
void launch_cpl(const Dev& d, hipStream_t s, int nnew, int sink, double coef, double cm1) {
  const Range R = uv_range(d.b);
#define ROMS_UV_CPL(SINK) \
  hipLaunchKernelGGL((k_uvdiag_cpl<SINK>), grid3_of(R, 2), dim3(kBX, kBY), 0, s, d, R, nnew, Uv.A, coef, cm1)
  ROMS_SINKS(sink, ROMS_UV_CPL);
#undef ROMS_UV_CPL
}

// the momentum variables of a diagnostics record (create_diagvars, diagnostics.F:812-889; wrt_diag_uv :923-962):
// u_pgr .. u_cpl at u points, v_pgr .. v_cpl at v points, N levels
std::vector<OutVar> uvdiag_vars(const ShimState& S) {
  static const char* sfx[7] = {"_pgr", "_cor", "_adv", "_dis", "_hmx", "_vmx", "_cpl"};
  static const char* lnm[7] = {"Hydrostatic Presssure Gradient", "Coriolis and Curvilinear", "Advection (Hor. and Vert.",
                               "Numerical dissipation", "Horizontal mixing", "Vertical mixing", "2D/3D coupling"};
  std::vector<OutVar> v;
  for (int c = 0; c < 2; c++)
    for (int a = 0; a < kUvTerms; a++)
      v.push_back(out_var(S, std::string(c == 0 ? "u" : "v") + sfx[a], lnm[a], "m^2/s^2", c == 0 ? 'u' : 'v', S.d->b.N, 0,
                          Uv.A.p[c * kUvTerms + a], S.d->b.n2));
  return v;
}

}  // namespace

bool uvdiag_sampling() { return Uv.sampling; }

void uvdiag_prsgrd(const Dev& d, hipStream_t s) { launch_snap_r(d, s); }

void uvdiag_uv1_begin(const Dev& d, hipStream_t s, const Tlev& t) {
  Uv.w.open();
  Uv.open = true;
  Uv.hmx_done = Uv.cpl_done = false;
  launch_snap_q(d, s, t.nnew);
}
void uvdiag_uv1_end(const Dev& d, hipStream_t s, const Tlev& t) {
  launch_rhs(d, s, t.nnew, t.nrhs, Uv.w.sink(), Uv.w.coef, Uv.w.cm1);
}
void uvdiag_visc3d(const Dev& d, hipStream_t s, const Tlev& t) {
  if (!Uv.open || Uv.hmx_done) return;
  Uv.hmx_done = true;
  launch_hmx(d, s, t.nstp, Uv.w.sink(), Uv.w.coef, Uv.w.cm1);
}
void uvdiag_uv2(const Dev& d, hipStream_t s, const Tlev& t) {
  if (!Uv.open || Uv.cpl_done) return;
  Uv.cpl_done = true;
  Uv.have = true;
  launch_cpl(d, s, t.nnew, Uv.w.sink(), Uv.w.coef, Uv.w.cm1);
}

void uvdiag_free() { uv_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_uvdiag_begin(int on, int do_avg) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (hipStreamSynchronize(S.s) != hipSuccess) { *S.err = "roms_gpu_uvdiag_begin: stream"; return -2; }
  if (!on) { uv_release(); return 0; }
  // allocate the new set first: a refused call leaves an earlier arming as it was
  double *base[kUvArr] = {}, *p[kUvArr] = {};
  for (int a = 0; a < kUvArr; a++) {
    p[a] = wvl_alloc_like_u(*S.d, S.s, &base[a]);
    if (!p[a]) {
      for (double* q : base)
        if (q) (void)hipFree(q);
      *S.err = "roms_gpu_uvdiag_begin: allocation of the 14 term arrays and 4 snapshots failed";
      return -2;
    }
  }
  if (hipStreamSynchronize(S.s) != hipSuccess) {
    for (double* q : base) (void)hipFree(q);
    *S.err = "roms_gpu_uvdiag_begin: zero fill failed";
    return -2;
  }
  uv_release();
  for (int a = 0; a < kUvArr; a++) { Uv.base[a] = base[a]; Uv.A.p[a] = p[a]; }
  Uv.armed = true;
  Uv.w.avg = do_avg != 0;
  Uv.sampling = true;
  return 0;
}

int roms_gpu_uvdiag_sample(int on) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Uv.armed) { *S.err = "roms_gpu_uvdiag_sample: not armed (roms_gpu_uvdiag_begin)"; return -4; }
  Uv.sampling = on != 0;
  return 0;
}

int roms_gpu_uvdiag_state(int* armed, int* do_avg, int* navg, int* sampling) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (armed) *armed = Uv.armed ? 1 : 0;
  if (do_avg) *do_avg = Uv.w.avg ? 1 : 0;
  if (navg) *navg = Uv.w.reported();
  if (sampling) *sampling = Uv.sampling ? 1 : 0;
  return 0;
}

int roms_gpu_uvdiag_copy_out(int comp, int term, double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Uv.armed) { *S.err = "roms_gpu_uvdiag_copy_out: not armed (roms_gpu_uvdiag_begin)"; return -4; }
  if (comp != ROMS_UVD_U && comp != ROMS_UVD_V) { *S.err = "roms_gpu_uvdiag_copy_out: comp is neither ROMS_UVD_U nor ROMS_UVD_V"; return -1; }
  if (term < ROMS_UVD_PGR || term > ROMS_UVD_PREV || !dst) { *S.err = "roms_gpu_uvdiag_copy_out: term outside 1..8"; return -1; }
  const Bounds& b = S.d->b;
  const long rows = (long)b.N * (b.Mm + 4);
  if (count != rows * (b.Lm + 4)) { *S.err = "roms_gpu_uvdiag_copy_out: count is not N*(Mm+4)*(Lm+4)"; return -1; }
  const double* src = term == ROMS_UVD_PREV ? Uv.A.p[kUvUPrev + comp] : Uv.A.p[comp * kUvTerms + term - 1];
  if (shim_rows_d2h(dst, src, rows) != hipSuccess) { *S.err = "roms_gpu_uvdiag_copy_out: copy failed"; return -2; }
  return 0;
}

int roms_gpu_wrt_diag(const char* path, int rec, int total_rec, double time, double period, const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Uv.armed) { *S.err = "roms_gpu_wrt_diag: not armed (roms_gpu_uvdiag_begin)"; return -4; }
  if (!Uv.have) { *S.err = "roms_gpu_wrt_diag: no complete sample to write (no corrector reached step3d_uv2 while sampling)"; return -4; }
  RecordSpec spec;
  spec.vars = uvdiag_vars(S);   // create_diagvars' order: the momentum variables, then the tracers'
  bool tavg, thave;
  const bool trc = tdiag_record(S, spec.vars, &tavg, &thave);
  if (trc && tavg != Uv.w.avg) { *S.err = "roms_gpu_wrt_diag: the momentum and the tracer terms disagree on do_avg"; return -1; }
  if (trc && !thave) { *S.err = "roms_gpu_wrt_diag: the armed tracers have no sample to write"; return -4; }
  spec.type = "ROMS diagnostics file";   // create_diagnostics_file (diagnostics.F:1006-1010)
  // init_diagnostics (:231-234): what is in the file
  spec.gatts.push_back({"diagnostic_options", std::string("Chosen Diagnostics = Momentum") + (trc ? ", Tracers" : "")});
  if (Uv.w.avg) spec.gatts.push_back({"diag_avg_time", seconds_att(period)});   // :754-755
  spec.time = time;
  if ((r = write_record(S, path, rec, total_rec, t, spec))) return r;
  if (trc) tdiag_window_written();   // diagnostics.F:778
  if (Uv.w.avg) {
    Uv.w.written();
    Uv.have = false;
    Uv.open = false;
  }
  return 0;
}

// n launches of each kernel group over the whole interior between two events on the library stream
// (tools/uvdiag_cost.py): ms[0] the two snapshots, ms[1] k_uvdiag_rhs, ms[2] k_uvdiag_hmx, ms[3] k_uvdiag_cpl.  With
// do_avg the mean sink at coef = 1/2 goes on from the open window: re-arm before the means are used
int roms_gpu_time_uvdiag(int n, roms_tlev* t, double ms[4]) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Uv.armed) { *S.err = "roms_gpu_time_uvdiag: not armed (roms_gpu_uvdiag_begin)"; return -4; }
  if (!t || !ms || n < 1 || t->nnew < 1 || t->nnew > 3 || t->nrhs < 1 || t->nrhs > 3 || t->nstp < 1 || t->nstp > 2) {
    *S.err = "roms_gpu_time_uvdiag: bad arguments";
    return -1;
  }
  const Dev& d = *S.d;
  const int sink = Uv.w.avg ? kMean : kStore;
  for (int which = 0; which < 4; which++) {
    ms[which] = time_rounds(S.s, n, true, [&]() {   // an untimed first launch
      if (which == 0) { launch_snap_r(d, S.s); launch_snap_q(d, S.s, t->nnew); }
      else if (which == 1) launch_rhs(d, S.s, t->nnew, t->nrhs, sink, 0.5, 0.5);
      else if (which == 2) launch_hmx(d, S.s, t->nstp, sink, 0.5, 0.5);
      else launch_cpl(d, S.s, t->nnew, sink, 0.5, 0.5);
      return 0;
    });
    if (ms[which] < 0) { *S.err = "roms_gpu_time_uvdiag: launch or timing failed"; return (int)ms[which]; }
  }
  return 0;
}

}  // extern "C"
