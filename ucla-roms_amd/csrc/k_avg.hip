// k_avg.hip -- time-averaged output on the device: calc_avg_ocean_vars
// (basic_output.F:1036-1118, tracers.F:252-269).  Once per step, after the
// closing rho_eos(nnew), the running means of the selected fields advance by
//   navg = navg + 1;  coef = 1/navg;  X_avg = X_avg*(1-coef) + X*coef
// with X = zeta/ubar/vbar(knew), u/v/t(nstp) -- slot nstp, which holds time n
// after the step, as the reference samples it -- rho1 - qp1*z_r (SPLIT_EOS) or
// rho, We + Wi, Akv, Akt(itemp), Akt(isalt), hbls, hbbl; the true vertical
// velocity w (ROMS_WRT_W) is sampled by k_wvlcty.hip's running-mean sink.
//
// MI355X design: a pure stream.  The average of a field has the device layout
// of one slot of that field (same row pitch, same plane stride, same
// alignment), so a sample is one flat sweep over whole planes, halos and pad
// columns included (the reference's ranges i0:i1 / 1:i1 lie inside; what is
// outside is never written to a file or compared).  One launch serves every
// selected field: a table of field descriptors built when averaging is armed,
// blockIdx.y picks the field, the per-sample slot offsets and coef, 1-coef
// come as kernel arguments.  16 bytes per lane where every pointer of a field
// is 16-byte aligned (the padded pitch: slot offsets are multiples of 128 B),
// an 8-byte sweep otherwise (ROMS_GPU_PITCH=0 with an odd plane size puts the
// nstp = 2 slot on an odd double).  No a*b+c contraction (-ffp-contract=off):
// two multiplies and an add, the reference's operations in its order.  At
// coef == 1 (the first sample of a window) the old average is not loaded, so
// the result does not depend on what the buffer held.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/roms_gpu.h"
#include "roms_dev.h"
#include "shim_state.h"

namespace roms {
namespace {

enum AvgKind : int { kAvgCopy = 0, kAvgSum = 1, kAvgSplitRho = 2 };   // x = a | a + b | a - b*c
enum AvgSlot : int { kSlotNone = 0, kSlotKnew = 1, kSlotNstp = 2 };   // which per-sample offset the source takes

struct AvgField {
  const double *a, *b, *c;   // sources (slot 1 of a time-levelled field); b, c by kind
  double* avg;
  long n;                    // elements of one slot
  int kind, slot;
};

template <int KIND>
__device__ __forceinline__ double avg_x(const double* a, const double* b, const double* c, long q) {
  if (KIND == kAvgSum) return a[q] + b[q];
  if (KIND == kAvgSplitRho) return a[q] - b[q] * c[q];
  return a[q];
}
template <int KIND>
__device__ __forceinline__ double2 avg_x2(const double* a, const double* b, const double* c, long q) {
  const double2 va = *reinterpret_cast<const double2*>(a + q);
  if (KIND == kAvgCopy) return va;
  const double2 vb = *reinterpret_cast<const double2*>(b + q);
  if (KIND == kAvgSum) return make_double2(va.x + vb.x, va.y + vb.y);
  const double2 vc = *reinterpret_cast<const double2*>(c + q);
  return make_double2(va.x - vb.x * vc.x, va.y - vb.y * vc.y);
}

// one field's sweep; FIRST: coef == 1, the old average is not read
template <int KIND, bool FIRST>
__device__ __forceinline__ void avg_sweep(const double* a, const double* b, const double* c, double* avg, long n,
                                          bool vec, double coef, double cm1) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  if (vec) {
    const long n2v = n >> 1;
    for (long p = tid; p < n2v; p += nth) {
      const long q = 2 * p;
      const double2 x = avg_x2<KIND>(a, b, c, q);
      double2 r;
      if (FIRST) {
        r = make_double2(x.x * coef, x.y * coef);
      } else {
        const double2 o = *reinterpret_cast<const double2*>(avg + q);
        r = make_double2(o.x * cm1 + x.x * coef, o.y * cm1 + x.y * coef);
      }
      *reinterpret_cast<double2*>(avg + q) = r;
    }
    if ((n & 1) && tid == 0) {
      const long q = n - 1;
      const double x = avg_x<KIND>(a, b, c, q);
      avg[q] = FIRST ? x * coef : avg[q] * cm1 + x * coef;
    }
  } else {
    for (long q = tid; q < n; q += nth) {
      const double x = avg_x<KIND>(a, b, c, q);
      avg[q] = FIRST ? x * coef : avg[q] * cm1 + x * coef;
    }
  }
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// off_knew = (knew-1)*n2, off_nstp = (nstp-1)*n3: the sampled slots of this step
template <bool FIRST>
__global__ void __launch_bounds__(256) k_calc_avg(const AvgField* __restrict__ tab, long off_knew, long off_nstp,
                                                  double coef, double cm1) {
  const AvgField f = tab[blockIdx.y];
  const long n = f.n;   // blocks past a small field's work fall through their loops (2-D fields next to 3-D ones)
  const long off = f.slot == kSlotKnew ? off_knew : f.slot == kSlotNstp ? off_nstp : 0;
  const double* a = f.a + off;
  const bool vec = al16(a) && al16(f.avg) && (f.kind == kAvgCopy || al16(f.b)) && (f.kind != kAvgSplitRho || al16(f.c));
  if (f.kind == kAvgCopy) avg_sweep<kAvgCopy, FIRST>(a, nullptr, nullptr, f.avg, n, vec, coef, cm1);
  else if (f.kind == kAvgSum) avg_sweep<kAvgSum, FIRST>(a, f.b, nullptr, f.avg, n, vec, coef, cm1);
  else avg_sweep<kAvgSplitRho, FIRST>(a, f.b, f.c, f.avg, n, vec, coef, cm1);
}

struct AvgBuf {
  double* base = nullptr;   // the allocation
  double* p = nullptr;      // element IJ = 0, aligned like the field it mirrors
  long n = 0;
};

struct AvgCtx {
  AvgView v;                       // what rst_io.hip's averages record reads
  MeanWindow w;                    // w.avg is set while armed
  double t_avg = 0.0;              // the mean time of the window's samples
  std::vector<AvgBuf> bufs;
  std::vector<AvgField> fields;    // host copy of the table
  AvgField* d_tab = nullptr;
  long nmax = 0;                   // largest field of the table
};
thread_local AvgCtx A;

void avg_release() {
  for (AvgBuf& b : A.bufs)
    if (b.base) (void)hipFree(b.base);
  if (A.d_tab) (void)hipFree(A.d_tab);
  A = AvgCtx{};
}

// one average of n doubles with the 128-byte phase of `like` (a field's slot 1)
double* avg_alloc(const double* like, long n) {
  AvgBuf b;
  if (hipMalloc(&b.base, (size_t)(n + kRowAlign) * sizeof(double)) != hipSuccess) return nullptr;
  b.p = b.base + ((uintptr_t)like / sizeof(double)) % kRowAlign;
  b.n = n;
  A.bufs.push_back(b);
  return b.p;
}

// blocks per field: 16 B per lane, at most kAvgBlocks and grid strides beyond.
// At C3 (105 M doubles per 3-D field) 32768 blocks measured 5-6 % faster than
// 2048 on both masks in each of three alternations, 16384 no faster than 2048
// (profiles/avg_cost.txt)
constexpr long kAvgBlocks = 32768;
unsigned avg_blocks(long nmax) {
  const long b = (nmax / 2 + 1 + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > kAvgBlocks ? kAvgBlocks : b);
}

// one sample of the window A.w has just opened
int avg_launch(const ShimState& S, const roms_tlev& t) {
  const double coef = A.w.coef, cm1 = A.w.cm1;
  const Bounds& b = S.d->b;
  const long ok = (long)(t.knew - 1) * b.n2, on = (long)(t.nstp - 1) * b.n3;
  const dim3 grid(avg_blocks(A.nmax), (unsigned)(A.fields.empty() ? 1 : A.fields.size()));
  // AKs samples Akt(isalt), which whole steps may leave unformed (shim_akt_sync)
  if ((A.v.mask & ROMS_WRT_AKS) && shim_akt_sync() != hipSuccess) return -3;
  if (!A.fields.empty()) {
    if (A.w.sink() == kMeanFirst) hipLaunchKernelGGL(k_calc_avg<true>, grid, dim3(256), 0, S.s, A.d_tab, ok, on, coef, cm1);
    else hipLaunchKernelGGL(k_calc_avg<false>, grid, dim3(256), 0, S.s, A.d_tab, ok, on, coef, cm1);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  // w (wvlcty.F) is a launch of its own: k_wvlcty with the running mean as its sink, over the cells it
  // computes or copies (k_wvlcty.hip)
  if (A.v.wvl) return wvl_launch(S, t.nstp, A.v.wvl, A.w.sink(), coef, cm1);
  return 0;
}

bool tlev_ok(const roms_tlev* t) { return t && t->knew >= 1 && t->knew <= 4 && t->nstp >= 1 && t->nstp <= 3; }

}  // namespace

const AvgView& avg_view() { return A.v; }
const MeanWindow& avg_window(double* t_avg) {
  *t_avg = A.t_avg;
  return A.w;
}
void avg_window_written() { A.w.written(); }
void avg_free() { avg_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_avg_begin(int wrt_mask) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (hipStreamSynchronize(S.s) != hipSuccess) { *S.err = "roms_gpu_avg_begin: stream synchronisation failed"; return -2; }
  avg_release();
  const Bounds& b = S.d->b;
  const Fields& F = S.d->f;
  const int all = ROMS_WRT_Z | ROMS_WRT_UB | ROMS_WRT_VB | ROMS_WRT_U | ROMS_WRT_V | ROMS_WRT_T | ROMS_WRT_R | ROMS_WRT_O |
                  ROMS_WRT_AKV | ROMS_WRT_AKT | ROMS_WRT_AKS | ROMS_WRT_HBLS | ROMS_WRT_HBBL | ROMS_WRT_W;
  int mask = wrt_mask & all;
  if (!S.cfg->salinity) mask &= ~ROMS_WRT_AKS;
  if (!S.cfg->lmd_mixing) mask &= ~(ROMS_WRT_HBLS | ROMS_WRT_HBBL);
  if (!mask) { wvl_free(); return 0; }   // disarmed
  if ((mask & ROMS_WRT_W) && b.N < 2) {
    *S.err = "roms_gpu_avg_begin: ROMS_WRT_W needs N >= 2 (wvlcty.F has no formula below)";
    return -1;
  }
  bool oom = false;
  auto add = [&](double*& dst, const double* a, long n, int kind, int slot, const double* bb = nullptr,
                 const double* cc = nullptr) {
    dst = avg_alloc(a, n);
    if (!dst) { oom = true; return; }
    A.fields.push_back(AvgField{a, bb, cc, dst, n, kind, slot});
    A.nmax = n > A.nmax ? n : A.nmax;
  };
  AvgView& V = A.v;
  if (mask & ROMS_WRT_Z) add(V.zeta, F.zeta, b.n2, kAvgCopy, kSlotKnew);
  if (mask & ROMS_WRT_UB) add(V.ubar, F.ubar, b.n2, kAvgCopy, kSlotKnew);
  if (mask & ROMS_WRT_VB) add(V.vbar, F.vbar, b.n2, kAvgCopy, kSlotKnew);
  if (mask & ROMS_WRT_U) add(V.u, F.u, b.n3, kAvgCopy, kSlotNstp);
  if (mask & ROMS_WRT_V) add(V.v, F.v, b.n3, kAvgCopy, kSlotNstp);
  if (mask & ROMS_WRT_T) {
    V.t.assign(b.NT, nullptr);
    for (int q = 0; q < b.NT && !oom; q++) add(V.t[q], F.t + (long)q * 3 * b.n3, b.n3, kAvgCopy, kSlotNstp);
  }
  if (!oom && (mask & ROMS_WRT_R)) {
    if (S.cfg->nonlin_eos) add(V.rho, F.rho1, b.n3, kAvgSplitRho, kSlotNone, F.qp1, F.z_r);
    else add(V.rho, F.rho, b.n3, kAvgCopy, kSlotNone);
  }
  if (!oom && (mask & ROMS_WRT_O)) add(V.w, F.We, b.n3w, kAvgSum, kSlotNone, F.Wi);
  if (!oom && (mask & ROMS_WRT_AKV)) add(V.akv, F.Akv, b.n3w, kAvgCopy, kSlotNone);
  if (!oom && (mask & ROMS_WRT_AKT)) add(V.akt, F.Akt, b.n3w, kAvgCopy, kSlotNone);
  if (!oom && (mask & ROMS_WRT_AKS)) add(V.aks, F.Akt + b.n3w, b.n3w, kAvgCopy, kSlotNone);
  if (!oom && (mask & ROMS_WRT_HBLS)) add(V.hbls, F.hbls, b.n2, kAvgCopy, kSlotNone);
  if (!oom && (mask & ROMS_WRT_HBBL)) add(V.hbbl, F.hbbl, b.n2, kAvgCopy, kSlotNone);
  if (!oom && (mask & ROMS_WRT_W)) {   // not in the table: sampled by k_wvlcty itself
    AvgBuf wb;
    V.wvl = wvl_alloc_like_u(*S.d, S.s, &wb.base);
    wb.p = V.wvl;
    wb.n = b.n3;
    if (V.wvl) A.bufs.push_back(wb);
    else oom = true;
  }
  if (!oom && !A.fields.empty()) {
    const size_t bytes = A.fields.size() * sizeof(AvgField);
    oom = hipMalloc(&A.d_tab, bytes) != hipSuccess ||
          copy_on(A.d_tab, A.fields.data(), bytes, hipMemcpyHostToDevice, S.s) != hipSuccess;
  }
  if (oom) {
    avg_release();
    *S.err = "roms_gpu_avg_begin: allocation of the average buffers failed";
    return -2;
  }
  V.mask = mask;
  A.w.avg = true;
  return 0;
}

int roms_gpu_calc_avg(const roms_tlev* t, double time) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!A.v.mask) { *S.err = "roms_gpu_calc_avg: averaging is not armed (roms_gpu_avg_begin)"; return -4; }
  if (!tlev_ok(t)) { *S.err = "roms_gpu_calc_avg: bad time levels"; return -1; }
  const MeanWindow before = A.w;
  A.w.open();
  if ((r = avg_launch(S, *t))) { A.w = before; *S.err = "roms_gpu_calc_avg: launch failed"; return r; }
  A.t_avg = A.t_avg * A.w.cm1 + time * A.w.coef;
  return 0;
}

int roms_gpu_avg_state(int* navg, double* t_avg, int* mask) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (navg) *navg = A.w.reported();
  if (t_avg) *t_avg = A.t_avg;
  if (mask) *mask = A.v.mask;
  return 0;
}

int roms_gpu_avg_copy_out(int wrt_bit, int itrc, double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const AvgView& V = A.v;
  if (!(V.mask & wrt_bit) || !dst) { *S.err = "roms_gpu_avg_copy_out: that field is not being averaged"; return -4; }
  const double* p = nullptr;
  int levels = 1;
  const int N = S.d->b.N;
  switch (wrt_bit) {
    case ROMS_WRT_Z: p = V.zeta; break;
    case ROMS_WRT_UB: p = V.ubar; break;
    case ROMS_WRT_VB: p = V.vbar; break;
    case ROMS_WRT_U: p = V.u; levels = N; break;
    case ROMS_WRT_V: p = V.v; levels = N; break;
    case ROMS_WRT_T:
      if (itrc < 1 || itrc > (int)V.t.size()) { *S.err = "roms_gpu_avg_copy_out: no such tracer"; return -1; }
      p = V.t[itrc - 1]; levels = N; break;
    case ROMS_WRT_R: p = V.rho; levels = N; break;
    case ROMS_WRT_O: p = V.w; levels = N + 1; break;
    case ROMS_WRT_AKV: p = V.akv; levels = N + 1; break;
    case ROMS_WRT_AKT: p = V.akt; levels = N + 1; break;
    case ROMS_WRT_AKS: p = V.aks; levels = N + 1; break;
    case ROMS_WRT_HBLS: p = V.hbls; break;
    case ROMS_WRT_HBBL: p = V.hbbl; break;
    case ROMS_WRT_W: p = V.wvl; levels = N; break;
    default: *S.err = "roms_gpu_avg_copy_out: wrt_bit must be one ROMS_WRT_* bit"; return -1;
  }
  const long rows = (long)levels * (S.d->b.Mm + 4), hcount = rows * (S.d->b.Lm + 4);
  if (count != hcount) { *S.err = "roms_gpu_avg_copy_out: count is not the field's one-slot size"; return -1; }
  if (shim_rows_d2h(dst, p, rows) != hipSuccess) { *S.err = "roms_gpu_avg_copy_out: copy failed"; return -2; }
  return 0;
}

// n samples between two events on the library stream (tools/avg_cost.py).
// They go on from the open window (navg += n), so after one roms_gpu_calc_avg
// every timed sample is a full one (old mean read); t_avg is left as it was:
// re-arm before the averages are used
int roms_gpu_time_calc_avg(int n, const roms_tlev* t, double* ms) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!A.v.mask) { *S.err = "roms_gpu_time_calc_avg: averaging is not armed (roms_gpu_avg_begin)"; return -4; }
  if (!tlev_ok(t) || n < 1 || !ms) { *S.err = "roms_gpu_time_calc_avg: bad arguments"; return -1; }
  const double f = time_rounds(S.s, n, false, [&]() {
    A.w.open();
    return avg_launch(S, *t);
  });
  if (f < 0) { *S.err = "roms_gpu_time_calc_avg: launch or timing failed"; return (int)f; }
  *ms = f;
  return 0;
}

}  // extern "C"
