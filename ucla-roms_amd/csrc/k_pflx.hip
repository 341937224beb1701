// k_pflx.hip -- baroclinic pressure fluxes on the device: calc_pressure_flux
// (calc_pflx_mod.F:81-171) on the hydrostatic pressure P the corrector's prsgrd
// hands it (prsgrd.F:160-226, 466-468).  Per corrector, while armed:
//   p_slow = beta*p_slow + alpha*P,  p_fast = P - p_slow           (0..nx x 0..ny)
//   Uflx = sum_k FlxU (k = 1..N in turn), divided into a velocity; Vflx alike
//   u_slow = beta*u_slow + alpha*(u(nrhs) - Uflx)                  (1..nx+1 x 1..ny)
//   v_slow = beta*v_slow + alpha*(v(nrhs) - Vflx)                  (1..nx x 1..ny+1)
//   up = sum_k u_fast*0.25*(p_fast(i-1)+p_fast(i))*(Hz(i-1)+Hz(i)) (1..nx x 1..ny), vp alike in j
// alpha = dt/timescale, beta = 1 - alpha.  dzt, which the reference forms and
// nothing reads, is left out.  Nothing is masked.
// One deviation, at a physical western edge: prsgrd writes P for i = istrU-1 =
// 1.. only there and calc_pressure_flux reads the unwritten P(0,j,k) into
// p_slow(0,j,:) and up(1,j); every input of P exists at i = 0, so P(0,j,:) is
// formed by the same expressions.
//
// MI355X design: two streaming launches, no LDS, no atomics.
// k_pflx_p: one rho column per lane, 64 consecutive i per wavefront, four rows per
// block, walking k = N..1 (P is a top-down recurrence) with k_prsgrd_P's rolling
// register window over z_r, rho1, qp1 (or rho), the elementary differences and
// their harmonic means.  While the stored grid is set_depth's own, z_r and
// z_w(N) are formed from the kept free surface (VGrid) instead of streamed.  Per
// level it reads p_slow, writes p_slow and p_fast: rho1, qp1 (z_r) in, three
// passes of its own.
// k_pflx_uv: one lane per (i,j) over 1..nx+1 x 1..ny+1.  The barotropic sums first
// (k = 1..N in turn: the order is part of the bits), then the walk k = 1..N with
// up, vp accumulated in registers in the reference's expression order and stored
// once.  The neighbours' p_fast and Hz come from the lines the wavefront and the
// block's other rows fetch anyway.
// The reference's operand order, no contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/roms_gpu.h"
#include "roms_dev.h"
#include "shim_state.h"

namespace roms {
namespace {

struct PfArrs {
  double *p_slow, *u_slow, *v_slow, *p_fast;   // N planes each, element IJ = 0 of level 1
  double *up, *vp;                             // one plane each
};

// R: 0..Lm x 0..Mm
template <bool VG>
__global__ void __launch_bounds__(256) k_pflx_p(Dev d, Range R, int split, int tides, PfArrs A, double alpha,
                                                 double beta) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const int N = b.N;
  const double g = d.p.g, rho0 = d.p.rho0, qp2 = d.p.qp2;
  const double OneFifth = 0.2, OneTwelfth = 1.0 / 12.0;
  const double grho = g / rho0, HalfGRho = 0.5 * grho;
  const long ij = IJ(b, i, j), n2 = b.n2;
  const double* __restrict__ zr = F.z_r + ij;
  const double* __restrict__ R1 = (split ? F.rho1 : F.rho) + ij;
  const double* __restrict__ qp1 = F.qp1 + ij;
  double* __restrict__ ps = A.p_slow + ij;
  double* __restrict__ pf = A.p_fast + ij;
  VGrid vg;
  if constexpr (VG) vg = vg_column(d, ij);
  auto rhov = [&](double r1, double q1, double z) {  // in-situ density at a rho level (prsgrd.F:198-200)
    if (split) {
      const double dpth = -z;
      return r1 + q1 * dpth * (1.0 - qp2 * dpth);
    }
    return r1;
  };
  auto eRof = [&](double ru, double rl, double qu, double ql, double zu, double zl) {  // levels l+1 (u), l (:166-172)
    if (split) {
      const double dpth = -0.5 * (zu + zl);
      return ru - rl + (qu - ql) * dpth * (1.0 - qp2 * dpth);
    }
    return ru - rl;
  };
  auto ldz = [&](int k) {
    if constexpr (VG) return vg.zr(k, F.Cs_r[k]);
    else return zr[(long)(k - 1) * n2];
  };
  auto ldr = [&](int k) { return R1[(long)(k - 1) * n2]; };
  auto ldq = [&](int k) { return split ? qp1[(long)(k - 1) * n2] : 0.0; };
  double zC = ldz(N), rC = ldr(N), qC = ldq(N);              // level k
  double zM = ldz(N - 1), rM = ldr(N - 1), qM = ldq(N - 1);  // level k-1
  double eZk = zC - zM, eRk = eRof(rC, rM, qC, qM, zC, zM);  // d(N) = d(N-1)
  double dZ1 = 0.0, dR1 = 0.0, P1 = 0.0;                     // values at k+1
  double z1 = 0.0, v1 = 0.0;                                 // z_r, in-situ rho at k+1
  double so = ps[(long)(N - 1) * n2];                        // p_slow of level k, loaded a level ahead
#pragma unroll 2
  for (int k = N; k >= 1; k--) {
    double eZm, eRm;
    if (k >= 2) { eZm = zC - zM; eRm = eRof(rC, rM, qC, qM, zC, zM); }
    else { eZm = eZk; eRm = eRk; }                           // d(0) = d(1)
    const double cff = 2.0 * eZk * eZm;
    const double dZk = cff / (eZk + eZm);
    const double cfr = 2.0 * eRk * eRm;
    double dRk = cfr > 0.0 ? cfr / (eRk + eRm) : 0.0;        // epsil = 0.
    const long o = (long)(k - 1) * n2;
    const double v0 = rhov(rC, qC, zC);
    if (split) {
      const double dpth = -zC;
      dRk = dRk - qC * dZk * (1.0 - 2.0 * qp2 * dpth);
    }
    double Pk;
    if (k == N) {
      double zw;
      if constexpr (VG) zw = vg.zw1(N, F.Cs_w[N]);
      else zw = F.z_w[ij + (long)N * n2];
      const double rNm = rhov(rM, qM, zM);
      Pk = g * zw + grho * (v0 + 0.5 * (v0 - rNm) * (zw - zC) / (zC - zM)) * (zw - zC);
      if (tides) Pk = Pk - g * F.ptide[ij];   // pot_tides (prsgrd.F:209-211)
    } else {
      Pk = P1 + HalfGRho * ((v1 + v0) * (z1 - zC) -
                            OneFifth * ((dR1 - dRk) * (z1 - zC - OneTwelfth * (dZ1 + dZk)) -
                                        (dZ1 - dZk) * (v1 - v0 - OneTwelfth * (dR1 + dRk))));
    }
    const double sn = beta * so + alpha * Pk;   // calc_pflx_mod.F:139-140
    if (k >= 2) so = ps[o - n2];
    ps[o] = sn;
    pf[o] = Pk - sn;
    P1 = Pk;
    dZ1 = dZk; dR1 = dRk;
    eZk = eZm; eRk = eRm;
    z1 = zC; v1 = v0;
    zC = zM; rC = rM; qC = qM;
    if (k >= 3) { zM = ldz(k - 2); rM = ldr(k - 2); qM = ldq(k - 2); }
  }
}

// R: 1..Lm+1 x 1..Mm+1; off: (nrhs-1)*n3
__global__ void __launch_bounds__(256) k_pflx_uv(Dev d, Range R, long off, PfArrs A, double alpha, double beta) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const int N = b.N;
  const bool du = j <= b.Mm, dv = i <= b.Lm;   // u_slow 1..nx+1 x 1..ny, v_slow 1..nx x 1..ny+1
  if (!du && !dv) return;
  const bool dp = du && dv;                    // up, vp 1..nx x 1..ny
  const long ij = IJ(b, i, j), n2 = b.n2, nx = b.nx2;
  const double* __restrict__ FU = F.FlxU + ij;
  const double* __restrict__ FV = F.FlxV + ij;
  const double* __restrict__ U = F.u + off + ij;
  const double* __restrict__ V = F.v + off + ij;
  const double* __restrict__ Hz = F.Hz + ij;
  const double* __restrict__ pf = A.p_fast + ij;
  double* __restrict__ us = A.u_slow + ij;
  double* __restrict__ vs = A.v_slow + ij;
  // the barotropic fluxes (calc_pflx_mod.F:111-112), k = 1..N in turn
  double Uflx = 0.0, Vflx = 0.0;
  if (du) {
#pragma unroll 4
    for (int k = 1; k <= N; k++) Uflx = Uflx + FU[(long)(k - 1) * n2];
  }
  if (dv) {
#pragma unroll 4
    for (int k = 1; k <= N; k++) Vflx = Vflx + FV[(long)(k - 1) * n2];
  }
  // divided into velocities (:120-131)
  const long oN = ij + (long)N * n2;
  const double zN = F.z_w[oN], z0 = F.z_w[ij];
  if (du) Uflx = Uflx * (F.pn[ij] + F.pn[ij - 1]) / (zN - z0 + F.z_w[oN - 1] - F.z_w[ij - 1]);
  if (dv) Vflx = Vflx * (F.pm[ij] + F.pm[ij - nx]) / (zN - z0 + F.z_w[oN - nx] - F.z_w[ij - nx]);
  double up = 0.0, vp = 0.0;
#pragma unroll 2
  for (int k = 1; k <= N; k++) {
    const long o = (long)(k - 1) * n2;
    double uf = 0.0, vf = 0.0;
    if (du) {
      const double ub = U[o] - Uflx;
      const double s = beta * us[o] + alpha * ub;   // :146-148
      us[o] = s;
      uf = ub - s;
    }
    if (dv) {
      const double vb = V[o] - Vflx;
      const double s = beta * vs[o] + alpha * vb;   // :154-156
      vs[o] = s;
      vf = vb - s;
    }
    if (dp) {                                       // :162-165
      const double p0 = pf[o], h0 = Hz[o];
      up = up + uf * 0.25 * (pf[o - 1] + p0) * (Hz[o - 1] + h0);
      vp = vp + vf * 0.25 * (pf[o - nx] + p0) * (Hz[o - nx] + h0);
    }
  }
  if (dp) {
    A.up[ij] = up;
    A.vp[ij] = vp;
  }
}

constexpr int kPfArr = 6;
struct PfCtx {
  double* base[kPfArr] = {};
  PfArrs A = {};
  bool armed = false;
  double alpha = 0.0, beta = 0.0;
  long nsamples = 0;
  long formed = 0, streamed = 0;   // k_pflx_p launches of each form since arming
};
thread_local PfCtx Pf;

void pf_release() {
  for (double* q : Pf.base)
    if (q) (void)hipFree(q);
  Pf = PfCtx{};
}

double** pf_slot(PfArrs& A, int a) {
  double** s[kPfArr] = {&A.p_slow, &A.u_slow, &A.v_slow, &A.p_fast, &A.up, &A.vp};
  return s[a];
}

// `planes` zeroed planes in the layout and alignment of u; *base is the allocation to free
double* pf_alloc(const Dev& d, hipStream_t s, long planes, double** base) {
  const size_t n = (size_t)(planes * d.b.n2 + kRowAlign) * sizeof(double);
  *base = nullptr;
  if (hipMalloc(base, n) != hipSuccess) return nullptr;
  if (hipMemsetAsync(*base, 0, n, s) != hipSuccess) {
    (void)hipFree(*base);
    *base = nullptr;
    return nullptr;
  }
  return *base + ((uintptr_t)d.f.u / sizeof(double)) % kRowAlign;
}

void launch_p(const Dev& d, hipStream_t s) {
  const Range R{0, d.b.Lm, 0, d.b.Mm};
  const dim3 grid = grid_of(R), blk(kBX, kBY);
  // ROMS_GPU_VGRID=0: the streaming form throughout
  const bool vg = shim_vgrid_valid() && d.p.vgrid;
  (vg ? Pf.formed : Pf.streamed)++;
  if (vg)
    hipLaunchKernelGGL((k_pflx_p<true>), grid, blk, 0, s, d, R, d.p.nonlin_eos, d.p.tides, Pf.A, Pf.alpha, Pf.beta);
  else
    hipLaunchKernelGGL((k_pflx_p<false>), grid, blk, 0, s, d, R, d.p.nonlin_eos, d.p.tides, Pf.A, Pf.alpha, Pf.beta);
}
void launch_uv(const Dev& d, hipStream_t s, int nrhs) {
  const Range R{1, d.b.Lm + 1, 1, d.b.Mm + 1};
  hipLaunchKernelGGL(k_pflx_uv, grid_of(R), dim3(kBX, kBY), 0, s, d, R, (long)(nrhs - 1) * d.b.n3, Pf.A, Pf.alpha,
                     Pf.beta);
}

// the device array and its planes of a ROMS_PFLX_* id (nullptr: no such id)
double* pf_array(int which, int N, long* planes) {
  *planes = which == ROMS_PFLX_UP || which == ROMS_PFLX_VP ? 1 : N;
  switch (which) {
    case ROMS_PFLX_UP: return Pf.A.up;
    case ROMS_PFLX_VP: return Pf.A.vp;
    case ROMS_PFLX_U_SLOW: return Pf.A.u_slow;
    case ROMS_PFLX_V_SLOW: return Pf.A.v_slow;
    case ROMS_PFLX_P_SLOW: return Pf.A.p_slow;
  }
  return nullptr;
}

}  // namespace

bool pflx_armed() { return Pf.armed; }

void pflx_corrector(const Dev& d, hipStream_t s, const Tlev& t) {
  launch_p(d, s);
  launch_uv(d, s, t.nrhs);
  Pf.nsamples++;
}

PflxView pflx_view() {
  PflxView v;
  if (Pf.armed) { v.armed = true; v.u_slow = Pf.A.u_slow; v.v_slow = Pf.A.v_slow; v.p_slow = Pf.A.p_slow; v.up = Pf.A.up; v.vp = Pf.A.vp; }
  return v;
}

void pflx_free() { pf_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_pflx_begin(double timescale, int on) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (hipStreamSynchronize(S.s) != hipSuccess) { *S.err = "roms_gpu_pflx_begin: stream"; return -2; }
  if (!on) { pf_release(); return 0; }
  const Bounds& b = S.d->b;
  if (b.N < 2) { *S.err = "roms_gpu_pflx_begin: N < 2 (prsgrd's P needs two levels)"; return -1; }
  // allocate the new set first: a refused call leaves an earlier arming as it was
  double* base[kPfArr] = {};
  PfArrs A = {};
  for (int a = 0; a < kPfArr; a++) {
    *pf_slot(A, a) = pf_alloc(*S.d, S.s, a < 4 ? b.N : 1, &base[a]);
    if (!*pf_slot(A, a)) {
      for (double* q : base)
        if (q) (void)hipFree(q);
      *S.err = "roms_gpu_pflx_begin: allocation of the three filter states, the work array, up and vp failed";
      return -2;
    }
  }
  if (hipStreamSynchronize(S.s) != hipSuccess) {
    for (double* q : base) (void)hipFree(q);
    *S.err = "roms_gpu_pflx_begin: zero fill failed";
    return -2;
  }
  pf_release();
  for (int a = 0; a < kPfArr; a++) Pf.base[a] = base[a];
  Pf.A = A;
  Pf.armed = true;
  Pf.alpha = S.d->p.dt / (timescale > 0.0 ? timescale : 86400.0);   // calc_pflx.opt: timescale = 24*3600
  Pf.beta = 1 - Pf.alpha;
  return 0;
}

int roms_gpu_pflx_state(int* armed, double* alpha, long* nsamples) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (armed) *armed = Pf.armed ? 1 : 0;
  if (alpha) *alpha = Pf.alpha;
  if (nsamples) *nsamples = Pf.nsamples;
  return 0;
}

int roms_gpu_pflx_path(long* formed, long* streamed) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (formed) *formed = Pf.formed;
  if (streamed) *streamed = Pf.streamed;
  return 0;
}

int roms_gpu_pflx_copy_out(int which, double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Pf.armed) { *S.err = "roms_gpu_pflx_copy_out: not armed (roms_gpu_pflx_begin)"; return -4; }
  const Bounds& b = S.d->b;
  long planes;
  const double* src = pf_array(which, b.N, &planes);
  if (!src || !dst) { *S.err = "roms_gpu_pflx_copy_out: which is no ROMS_PFLX_* id"; return -1; }
  const long rows = planes * (b.Mm + 4);
  if (count != rows * (b.Lm + 4)) { *S.err = "roms_gpu_pflx_copy_out: count is not [N*](Mm+4)*(Lm+4)"; return -1; }
  if (shim_rows_d2h(dst, src, rows) != hipSuccess) { *S.err = "roms_gpu_pflx_copy_out: copy failed"; return -2; }
  return 0;
}

int roms_gpu_pflx_copy_in(int which, const double* src, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Pf.armed) { *S.err = "roms_gpu_pflx_copy_in: not armed (roms_gpu_pflx_begin)"; return -4; }
  const Bounds& b = S.d->b;
  if (which != ROMS_PFLX_U_SLOW && which != ROMS_PFLX_V_SLOW && which != ROMS_PFLX_P_SLOW) {
    *S.err = "roms_gpu_pflx_copy_in: which is none of ROMS_PFLX_U_SLOW, V_SLOW, P_SLOW (up and vp are results)";
    return -1;
  }
  long planes;
  double* dst = pf_array(which, b.N, &planes);
  const long rows = planes * (b.Mm + 4);
  if (!src || count != rows * (b.Lm + 4)) { *S.err = "roms_gpu_pflx_copy_in: count is not N*(Mm+4)*(Lm+4)"; return -1; }
  if (shim_rows_h2d(dst, src, rows) != hipSuccess) { *S.err = "roms_gpu_pflx_copy_in: copy failed"; return -2; }
  return 0;
}

// n launches of each kernel between two events on the library stream (tools/pflx_cost.py): ms[0] k_pflx_p,
// ms[1] k_pflx_uv over slot 3.  The filters go on from their state: re-arm before they are used
int roms_gpu_time_pflx(int n, double ms[2]) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Pf.armed) { *S.err = "roms_gpu_time_pflx: not armed (roms_gpu_pflx_begin)"; return -4; }
  if (n < 1 || !ms) { *S.err = "roms_gpu_time_pflx: bad arguments"; return -1; }
  const Dev& d = *S.d;
  for (int which = 0; which < 2; which++) {
    ms[which] = time_rounds(S.s, n, true, [&]() {   // an untimed first launch
      if (which == 0) launch_p(d, S.s);
      else launch_uv(d, S.s, 3);
      return 0;
    });
    if (ms[which] < 0) { *S.err = "roms_gpu_time_pflx: launch or timing failed"; return (int)ms[which]; }
  }
  return 0;
}

}  // extern "C"
