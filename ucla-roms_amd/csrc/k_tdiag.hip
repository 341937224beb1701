// k_tdiag.hip -- the term-by-term tracer budget of the corrector on the device:
// DIAGNOSTICS with diag_trc (diagnostics.F, hooks in step3d_t_ISO.F), the
// non-isoneutral build.  Per armed tracer six terms, C m^3/s, on N planes in a
// rho field's layout, 0 outside the ranges named (include/roms_gpu.h, ABI 30):
//   advx(i,j,k), i = 1..Lm+1, j = 1..Mm (diagnostics.F:620-639):
//     grd(i) = (t(i)-t(i-1))*umask(i,j);  g2(i) = grd(i+1)+grd(i)
//     advx = 0.5*( t(i)+t(i-1) - 0.1666666666666667*(g2(i)-g2(i-1)) )*FlxU(i,j,k)
//   advy(i,j,k), i = 1..Lm, j = 1..Mm+1: the same in eta with vmask, FlxV (:640-659)
//     The elementary differences one face outside a physical, non-periodic edge
//     of the whole grid are copies of the first one inside
//     (compute_horiz_tracer_fluxes.h:50-84, 131-165: tracer_fx's index clamp);
//     on a periodic side or a rank boundary nothing is copied.  As written,
//     diag_t_adv_hc4 assigns a slice of length nx to one of length ny (:627-628)
//     and tests the north flag for the south copy and vice versa (:645-646); on
//     a square single-rank grid both forms coincide.
//   mixx = FX - advx, mixy = FE - advy (step3d_t_ISO.F:236-248), FX, FE the
//     UPSTREAM_TS fluxes the corrector applied (tracer_fx / tracer_fe's
//     expressions), river faces overridden (river_tracer_flux)
//   advz(k) = FC(k), the corrector's spline flux, FC(N) = 0 (step3d_t_ISO.F:911-913)
//   mixz(k) = ZFlx(k) - advz(k) (step3d_t_ISO.F:914, 1104-1132), with S the
//     content of t(nnew) between the horizontal and the vertical update:
//     D(k) = (S(k) - Hz(k)*t_new(k))/dt;  ZFlx(1) = D(1)/(pm*pn);
//     ZFlx(k) = D(k)/(pm*pn) + ZFlx(k-1)
//   means (calc_diag_avg, :709-732): navg += 1; coef = 1/navg;
//     X_avg = X_avg*(1-coef) + X*coef, one sample per corrector
//
// MI355X design.  k_tdiag_snap: one lane per cell and level, a copy of t(nnew)
// over the range launch_step3d_t's run() was given.  k_tdiag_h: one lane per
// face pair (the u face and the v face at (i,j)), 64 consecutive i per
// wavefront, four rows per block, the levels walked upwards; masks, the clamped
// stencil offsets and the river tests once per lane; per level the lane loads
// its seven t(nrhs) values, FlxU and FlxV -- the neighbours' come from lines
// the wavefront and the block's other rows fetch anyway -- and writes four
// terms.  The range is one face wider than the cells in each direction.
// k_tdiag_v: one column per lane, the spline phase of k_step3d_t_v
// (tracer_spline_lds) on the same ColLds / ColGlb storage and switch, then a
// bottom-up walk.  Both take their sink as a template parameter like k_wvlcty:
// store, or the running mean, which at coef == 1 does not load the old mean.
// The reference's operand order, no contraction (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "k_common.h"
#include "shim_state.h"

namespace roms {
namespace {

// Tn, snap: element IJ = 0 of level 1 of the tracer's t(nnew) slot / its snapshot
__global__ void __launch_bounds__(256) k_tdiag_snap(Dev d, Range R, const double* __restrict__ Tn,
                                                    double* __restrict__ snap) {
  ROMS_IJ_OR_RETURN(R)
  const long o = IJ(d.b, i, j) + (long)bI.z * d.b.n2;
  snap[o] = Tn[o];
}

// R: the cells istr..iend x jstr..jend; lanes cover istr..iend+1 x jstr..jend+1.
// Tr: element IJ = 0 of level 1 of the tracer's t(nrhs) slot
template <int SINK>
__global__ void __launch_bounds__(256) k_tdiag_h(Dev d, Range R, int itrc, const double* __restrict__ Tr,
                                                 double* __restrict__ advx, double* __restrict__ advy,
                                                 double* __restrict__ mixx, double* __restrict__ mixy, double coef,
                                                 double cm1) {
  const Range RF{R.i0, R.i1 + 1, R.j0, R.j1 + 1};
  ROMS_IJ_OR_RETURN(RF)
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const bool fx = j <= R.j1, fe = i <= R.i1;   // the lane has a u face / a v face
  if (!fx && !fe) return;
  const int N = b.N;
  const long ij = IJ(b, i, j), n2 = b.n2, nx = b.nx2;
  // the clamp of tracer_fx / tracer_fe: faces m-1, m, m+1 of the three elementary differences
  const int ilo = b.west_edge ? b.istr : -1000000, ihi = b.east_edge ? b.iend + 1 : 1000000;
  const int jlo = b.south_edge ? b.jstr : -1000000, jhi = b.north_edge ? b.jend + 1 : 1000000;
  long px[3], pe[3];
  double um[3], vm[3];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    px[q] = IJ(b, iclamp(i - 1 + q, ilo, ihi), j);
    pe[q] = IJ(b, i, iclamp(j - 1 + q, jlo, jhi));
    um[q] = fx ? F.umask[px[q]] : 0.0;
    vm[q] = fe ? F.vmask[pe[q]] : 0.0;
  }
  // river inflow faces (river_tracer_flux's own test, once)
  const bool rx = d.p.nriv > 0 && fx && fabs(F.riv_uflx[ij]) > 1e-3;
  const bool re = d.p.nriv > 0 && fe && fabs(F.riv_vflx[ij]) > 1e-3;
#pragma unroll 2
  for (int k = 1; k <= N; k++) {
    const long kk = (long)(k - 1) * n2;
    const double* __restrict__ T = Tr + kk;
    if (fx) {
      double el[3];
#pragma unroll
      for (int q = 0; q < 3; q++) el[q] = (T[px[q]] - T[px[q] - 1]) * um[q];
      const double Fl = F.FlxU[ij + kk], t0 = T[ij], t1 = T[ij - 1];
      const double cm = el[1] - el[0], c0 = el[2] - el[1];   // curv(m-1), curv(m) of tracer_fx
      double FX = 0.5 * (t0 + t1) * Fl - 0.1666666666666666 * (cm * fmax0(Fl) + c0 * fmin0(Fl));
      if (rx) river_tracer_flux(d, 0, i, j, k, itrc, FX);
      const double g0 = el[2] + el[1], gm = el[1] + el[0];   // g2(i), g2(i-1)
      const double adv = 0.5 * (t0 + t1 - 0.1666666666666667 * (g0 - gm)) * Fl;
      sink_put<SINK>(advx + ij + kk, adv, coef, cm1);
      sink_put<SINK>(mixx + ij + kk, FX - adv, coef, cm1);
    }
    if (fe) {
      double el[3];
#pragma unroll
      for (int q = 0; q < 3; q++) el[q] = (T[pe[q]] - T[pe[q] - nx]) * vm[q];
      const double Fl = F.FlxV[ij + kk], t0 = T[ij], t1 = T[ij - nx];
      const double cm = el[1] - el[0], c0 = el[2] - el[1];
      double FE = 0.5 * (t0 + t1) * Fl - 0.1666666666666666 * (cm * fmax0(Fl) + c0 * fmin0(Fl));
      if (re) river_tracer_flux(d, 1, i, j, k, itrc, FE);
      const double g0 = el[2] + el[1], gm = el[1] + el[0];
      const double adv = 0.5 * (t0 + t1 - 0.1666666666666667 * (g0 - gm)) * Fl;
      sink_put<SINK>(advy + ij + kk, adv, coef, cm1);
      sink_put<SINK>(mixy + ij + kk, FE - adv, coef, cm1);
    }
  }
}

// The spline phase of k_step3d_t_v (slots A: FC, B: CF), then ZFlx bottom-up.
// Tr, Tn, snap: element IJ = 0 of level 1 of t(nrhs), t(nnew), the snapshot
template <class C, int SINK>
__global__ void __launch_bounds__(64) k_tdiag_v(Dev d, Range R, const double* __restrict__ Tr,
                                                const double* __restrict__ Tn, const double* __restrict__ snap,
                                                double* __restrict__ advz, double* __restrict__ mixz, double coef,
                                                double cm1) {
  ROMS_IJC_OR_RETURN(R)
  col_lds_poison<C>(2, d.b.N);
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const int N = b.N;
  const long n2 = b.n2, ij = IJ(b, i, j);
  const double* __restrict__ Hz = F.Hz + ij;
  const C A = ColMake<C>::at(d, 0, 0, ij), B = ColMake<C>::at(d, 1, 0, ij);
  tracer_spline_lds(N, n2, Hz, Tr + ij, F.We + ij, A, B);   // A[k] = FC(k)*We(k), A[0] = A[N] = 0
  const double dt = d.p.dt, pmn = F.pm[ij] * F.pn[ij];
  double zf = 0.0;
#pragma unroll 2
  for (int k = 1; k <= N; k++) {
    const long o = (long)(k - 1) * n2;
    const double D = (snap[ij + o] - Hz[o] * Tn[ij + o]) / dt;
    zf = k == 1 ? D / pmn : D / pmn + zf;
    const double adv = A[k];
    sink_put<SINK>(advz + ij + o, adv, coef, cm1);
    sink_put<SINK>(mixz + ij + o, zf - adv, coef, cm1);
  }
}

constexpr int kTdArr = 7;   // ROMS_TDIA_ADVX..MIXZ, ROMS_TDIA_SNAP at [term - 1]
struct TdTrc {
  int itrc = 0;
  double* base[kTdArr] = {};
  double* p[kTdArr] = {};   // element IJ = 0 of level 1, aligned like u
};
struct TdCtx {
  std::vector<TdTrc> trc;
  bool sampling = false;
  MeanWindow w;   // w.have: a sample since begin (avg: since the last record); coef, cm1 of the corrector under way
};
thread_local TdCtx Td;

void td_release() {
  for (TdTrc& t : Td.trc)
    for (double* q : t.base)
      if (q) (void)hipFree(q);
  Td = TdCtx{};
}

const double* slot_of(const Dev& d, int tlev, int itrc) {
  return d.f.t + (long)(tlev - 1) * d.b.n3 + (long)(itrc - 1) * 3 * d.b.n3;
}

void launch_snap(const Dev& d, hipStream_t s, const Range& r, int nnew) {
  for (const TdTrc& t : Td.trc)
    hipLaunchKernelGGL(k_tdiag_snap, grid3_of(r, d.b.N), dim3(kBX, kBY), 0, s, d, r, slot_of(d, nnew, t.itrc),
                       t.p[ROMS_TDIA_SNAP - 1]);
}

void launch_h(const Dev& d, hipStream_t s, const Range& R, int nrhs, int sink, double coef, double cm1) {
  const Range RF{R.i0, R.i1 + 1, R.j0, R.j1 + 1};
  const dim3 g = grid_of(RF), blk(kBX, kBY);
  for (const TdTrc& t : Td.trc) {
    double *ax = t.p[ROMS_TDIA_ADVX - 1], *ay = t.p[ROMS_TDIA_ADVY - 1], *mx = t.p[ROMS_TDIA_MIXX - 1],
           *my = t.p[ROMS_TDIA_MIXY - 1];
    const double* Tr = slot_of(d, nrhs, t.itrc);
#define ROMS_TD_H(SINK) hipLaunchKernelGGL((k_tdiag_h<SINK>), g, blk, 0, s, d, R, t.itrc, Tr, ax, ay, mx, my, coef, cm1)
    ROMS_SINKS(sink, ROMS_TD_H);
#undef ROMS_TD_H
  }
}

void launch_v(const Dev& d, hipStream_t s, const Range& r, int nnew, int nrhs, int sink, double coef, double cm1) {
  const dim3 g = gridc_of(r);
  for (const TdTrc& t : Td.trc) {
    const double *Tr = slot_of(d, nrhs, t.itrc), *Tn = slot_of(d, nnew, t.itrc), *sn = t.p[ROMS_TDIA_SNAP - 1];
    double *az = t.p[ROMS_TDIA_ADVZ - 1], *mz = t.p[ROMS_TDIA_MIXZ - 1];
#define ROMS_TD_V(SINK)                                                                                           \
  do {                                                                                                            \
    if (d.f.colscr) hipLaunchKernelGGL((k_tdiag_v<ColGlb, SINK>), g, dim3(kCX), 0, s, d, r, Tr, Tn, sn, az, mz,   \
                                       coef, cm1);                                                                \
    else hipLaunchKernelGGL((k_tdiag_v<ColLds, SINK>), g, dim3(kCX), col_lds_bytes(2, d.b.N), s, d, r, Tr, Tn,    \
                            sn, az, mz, coef, cm1);                                                               \
  } while (0)
    ROMS_SINKS(sink, ROMS_TD_V);
#undef ROMS_TD_V
  }
}

void set_lds_limit(int N) {
  const int bytes = (int)col_lds_bytes(2, N);
  (void)hipFuncSetAttribute((const void*)k_tdiag_v<ColLds, kStore>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)hipFuncSetAttribute((const void*)k_tdiag_v<ColLds, kMean>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)hipFuncSetAttribute((const void*)k_tdiag_v<ColLds, kMeanFirst>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            bytes);
}

}  // namespace

bool tdiag_sampling() { return Td.sampling; }

void tdiag_corrector(const Dev& d, hipStream_t s, const Range& R, const Tlev& t) {
  Td.w.open();
  launch_h(d, s, R, t.nrhs, Td.w.sink(), Td.w.coef, Td.w.cm1);
}
void tdiag_snap(const Dev& d, hipStream_t s, const Range& r, const Tlev& t) { launch_snap(d, s, r, t.nnew); }
void tdiag_vert(const Dev& d, hipStream_t s, const Range& r, const Tlev& t) {
  launch_v(d, s, r, t.nnew, t.nrhs, Td.w.sink(), Td.w.coef, Td.w.cm1);
}

// the variable list of a diagnostics record (create_diagvars, diagnostics.F:891-921; wrt_diag_trc :964-991): per
// armed tracer <name>_advx, _advy, _advz, _mixx, _mixy, _mixz, N levels at rho points
bool tdiag_record(const ShimState& S, std::vector<OutVar>& vars, bool* do_avg, bool* have) {
  static const char* sfx[6] = {"_advx", "_advy", "_advz", "_mixx", "_mixy", "_mixz"};
  static const char* lnm[6] = {"x-advective flux", "y-advective flux", "z-advective flux", "mixing x-flux", "mixing y-flux",
                               "mixing z-flux"};
  *do_avg = Td.w.avg;
  *have = Td.w.have;
  std::vector<std::string> nm, un, ln;
  io_tracer_meta(S, nm, un, ln);
  for (const TdTrc& t : Td.trc)
    for (int a = 0; a < 6; a++)
      vars.push_back(out_var(S, nm[t.itrc - 1] + sfx[a], lnm[a], "C m^3/s", 'r', S.d->b.N, 0, t.p[a], S.d->b.n2));
  return !Td.trc.empty();
}
void tdiag_window_written() { Td.w.written(); }   // diagnostics.F:778
void tdiag_free() { td_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_tdiag_begin(int ntd, const int* itrc, int do_avg) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const Bounds& b = S.d->b;
  // every refusal comes before the release: a refused call leaves an earlier arming as it was
  if (ntd != 0) {
    if (S.d->p.iso) {
      *S.err = "roms_gpu_tdiag_begin: adv_isoneutral defines other terms (step3d_t_ISO.F:222-234, 825-843); not built";
      return -1;
    }
    if (ntd < 0 || !itrc) { *S.err = "roms_gpu_tdiag_begin: bad arguments"; return -1; }
    for (int q = 0; q < ntd; q++) {
      if (itrc[q] < 1 || itrc[q] > b.NT) { *S.err = "roms_gpu_tdiag_begin: tracer index outside 1..NT"; return -1; }
      for (int p = 0; p < q; p++)
        if (itrc[p] == itrc[q]) { *S.err = "roms_gpu_tdiag_begin: tracer index repeated"; return -1; }
    }
  }
  if (hipStreamSynchronize(S.s) != hipSuccess) { *S.err = "roms_gpu_tdiag_begin: stream"; return -2; }
  td_release();
  if (ntd == 0) return 0;
  for (int q = 0; q < ntd; q++) {
    TdTrc t;
    t.itrc = itrc[q];
    Td.trc.push_back(t);
    for (int a = 0; a < kTdArr; a++) {
      TdTrc& T = Td.trc.back();
      T.p[a] = wvl_alloc_like_u(*S.d, S.s, &T.base[a]);
      if (!T.p[a]) {
        td_release();
        *S.err = "roms_gpu_tdiag_begin: allocation of 7 arrays per armed tracer failed";
        return -2;
      }
    }
  }
  if (!S.d->f.colscr) set_lds_limit(b.N);
  Td.w.avg = do_avg != 0;
  Td.sampling = true;
  if (hipStreamSynchronize(S.s) != hipSuccess) { td_release(); *S.err = "roms_gpu_tdiag_begin: zero fill failed"; return -2; }
  return 0;
}

int roms_gpu_tdiag_sample(int on) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (Td.trc.empty()) { *S.err = "roms_gpu_tdiag_sample: not armed (roms_gpu_tdiag_begin)"; return -4; }
  Td.sampling = on != 0;
  return 0;
}

int roms_gpu_tdiag_state(int* ntd, int* do_avg, int* navg, int* sampling) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (ntd) *ntd = (int)Td.trc.size();
  if (do_avg) *do_avg = Td.w.avg ? 1 : 0;
  if (navg) *navg = Td.w.reported();
  if (sampling) *sampling = Td.sampling ? 1 : 0;
  return 0;
}

int roms_gpu_tdiag_copy_out(int itrc, int term, double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const TdTrc* T = nullptr;
  for (const TdTrc& t : Td.trc)
    if (t.itrc == itrc) T = &t;
  if (!T) { *S.err = "roms_gpu_tdiag_copy_out: tracer is not armed (roms_gpu_tdiag_begin)"; return -1; }
  if (term < ROMS_TDIA_ADVX || term > ROMS_TDIA_SNAP || !dst) { *S.err = "roms_gpu_tdiag_copy_out: term outside 1..7"; return -1; }
  const Bounds& b = S.d->b;
  const long rows = (long)b.N * (b.Mm + 4);
  if (count != rows * (b.Lm + 4)) { *S.err = "roms_gpu_tdiag_copy_out: count is not N*(Mm+4)*(Lm+4)"; return -1; }
  if (shim_rows_d2h(dst, T->p[term - 1], rows) != hipSuccess) { *S.err = "roms_gpu_tdiag_copy_out: copy failed"; return -2; }
  return 0;
}

int roms_gpu_wrt_tdiag(const char* path, int rec, int total_rec, double time, double period, const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (Td.trc.empty()) { *S.err = "roms_gpu_wrt_tdiag: not armed (roms_gpu_tdiag_begin)"; return -4; }
  if (!Td.w.have) { *S.err = "roms_gpu_wrt_tdiag: no sample to write (no corrector ran while sampling)"; return -4; }
  RecordSpec spec;
  bool avg, have;
  (void)tdiag_record(S, spec.vars, &avg, &have);
  spec.type = "ROMS diagnostics file";   // create_diagnostics_file (diagnostics.F:1006-1010)
  // init_diagnostics (:231-234) names what is in the file: no momentum terms ahead of the comma here
  spec.gatts.push_back({"diagnostic_options", "Chosen Diagnostics = , Tracers"});
  if (avg) spec.gatts.push_back({"diag_avg_time", seconds_att(period)});   // :754-755
  spec.time = time;
  if ((r = write_record(S, path, rec, total_rec, t, spec))) return r;
  tdiag_window_written();
  return 0;
}

// n launches of each kernel over the whole interior, every armed tracer, between two events on the library stream
// (tools/tdiag_cost.py): ms[0] the snapshot, ms[1] k_tdiag_h, ms[2] k_tdiag_v.  With do_avg the mean sink at
// coef = 1/2 goes on from the open window: re-arm before the means are used
int roms_gpu_time_tdiag(int n, roms_tlev* t, double ms[3]) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (Td.trc.empty()) { *S.err = "roms_gpu_time_tdiag: not armed (roms_gpu_tdiag_begin)"; return -4; }
  if (!t || !ms || n < 1 || t->nnew < 1 || t->nnew > 3 || t->nrhs < 1 || t->nrhs > 3) {
    *S.err = "roms_gpu_time_tdiag: bad arguments";
    return -1;
  }
  const Dev& d = *S.d;
  const Bounds& b = d.b;
  const Range R{b.istr, b.iend, b.jstr, b.jend};
  const int sink = Td.w.avg ? kMean : kStore;
  for (int which = 0; which < 3; which++) {
    ms[which] = time_rounds(S.s, n, true, [&]() {   // an untimed first launch
      if (which == 0) launch_snap(d, S.s, R, t->nnew);
      else if (which == 1) launch_h(d, S.s, R, t->nrhs, sink, 0.5, 0.5);
      else launch_v(d, S.s, R, t->nnew, t->nrhs, sink, 0.5, 0.5);
      return 0;
    });
    if (ms[which] < 0) { *S.err = "roms_gpu_time_tdiag: launch or timing failed"; return (int)ms[which]; }
  }
  return 0;
}

}  // extern "C"
