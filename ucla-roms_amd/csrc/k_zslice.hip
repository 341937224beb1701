// k_zslice.hip -- z-level slices on the device: calc_zslice / sigma_to_z /
// calc_average of zslice_output.F:100-282.  u, v and chosen tracers (slot
// nnew) are interpolated from the terrain-following levels to fixed depths
// below the free surface, as a snapshot or as a running mean sampled by every
// call (do_avg).  For a column and a depth zlev, with zz(0..N+1) the column's
// z relative to its free surface (u, v points: the mean of the two rho
// columns), the first test that holds classifies the cell:
//   rmask(i,j) < 0.5 masked | above surface | top half-layer | below bottom |
//   bottom half-layer | else the first k = N-1..1 with
//   (zz(k+1)-zlev)*(zlev-zz(k)) >= 0
// and the value is 0, the half-layer extrapolations or the linear
// interpolation of the reference, its expressions in its order, IEEE division,
// no contraction: bitwise reproducible from numpy.
//
// MI355X design: search, then gather.  The class and the bracket of a depth
// depend on the column's z only, and while the grid's validity flag holds
// z_r, z_w come from VGrid (z_sd, h, hinv, the Cs tables; for u, v also the
// neighbour column's), so the search is ALU work without memory traffic: one
// descending pass forms zz(k) once, kZslAhead levels per trip, tests up to
// kZslChunk depths held in registers against it, keeps the bracket's index
// only, and ends when every lane of the wave has its brackets.  That
// arithmetic, not memory, is what a sample costs (the same time
// with the field loads taken out).  A field then costs two level reads per depth in place of N
// (neighbouring lanes mostly share k: whole 128-B lines), shared by every
// tracer of the rho grid and by the averaging update.  One launch serves
// every selected field and depth: blockIdx.z picks the grid type (rho, u, v),
// lanes run along i, every output plane has the 2-D device layout and is
// written coalesced.  Without VGrid validity the same code streams the stored
// z_r / z_w (bitwise equal by the VGrid guarantee).  Cells outside 1..Lm x
// 1..Mm are never written: they keep the 0 of the allocation, which is what
// the file holds there.  The reference's exchange of Uz, Vz is left out: it
// only ever writes 1:nx, 1:ny.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/roms_gpu.h"
#include "roms_dev.h"
#include "shim_state.h"

namespace roms {
namespace {

constexpr int kZslChunk = 8;   // depths whose brackets one pass of the search holds in registers
constexpr int kZslAhead = 4;   // levels of the search formed per trip (C3: 2 measured 3 % slower, profiles/zslice_cost.txt)
enum ZslClass : int { kZslZero = 0, kZslTop = 1, kZslBottom = 2, kZslInterior = 3 };

struct ZslField {
  const double* src;   // slot 1, level 1 of the field
  double *out, *avg;   // ndep planes each (avg: nullptr without do_avg)
};
struct ZslArgs {
  const ZslField* tab;      // the rho-point fields (tracers) first, then u, then v
  int first[3], count[3];   // per grid type 0 rho, 1 u, 2 v: its entries of tab
  int types[3];             // grid type of blockIdx.z
  int ndep;
  long slot_off;            // (nnew-1)*n3: the sampled slot of u, v, t
  double coef, cm1;
  double dep[ROMS_ZSL_MAXDEP];
};

// z_r(1..N), z_w(0..N) of one column: formed (VG) or streamed
template <bool VG>
struct ZslCol {
  VGrid g;
  const double *zr_, *zw_;
  long n2;
  __device__ __forceinline__ double r(int k) const { return VG ? g.zr(k) : zr_[(long)(k - 1) * n2]; }
  __device__ __forceinline__ double w(int k) const { return VG ? vg_zw(g, k) : zw_[(long)k * n2]; }
};
template <bool VG>
__device__ __forceinline__ ZslCol<VG> zsl_col(const Dev& d, long ij) {
  ZslCol<VG> c;
  if (VG) c.g = vg_column(d, ij);
  c.zr_ = d.f.z_r + ij;
  c.zw_ = d.f.z_w + ij;
  c.n2 = d.b.n2;
  return c;
}

// FIRST: coef == 1, the old mean is not read
template <bool VG, bool FIRST>
__global__ void __launch_bounds__(256) k_zslice(Dev d, Range R, ZslArgs a) {
  ROMS_IJ_OR_RETURN(R)
  const Bounds& b = d.b;
  const int N = b.N, gt = a.types[bI.z];
  const long ij = IJ(b, i, j), n2 = b.n2;
  const bool two = gt != 0;
  const long ijn = gt == 1 ? IJ(b, i - 1, j) : gt == 2 ? IJ(b, i, j - 1) : ij;   // the neighbour column of a u, v point
  const ZslCol<VG> c0 = zsl_col<VG>(d, ij), c1 = zsl_col<VG>(d, ijn);
  // zz(k) = z_r(k) - z_w(N), at u, v points 0.5*(a + a') of both terms (IEEE addition commutes: the
  // reference's operand orders, (i-1) first in the u surface term, give the same bits)
  const double wn0 = c0.w(N), wn1 = c1.w(N), wb0 = c0.w(0), wb1 = c1.w(0);
  const double surf = two ? 0.5 * (wn0 + wn1) : wn0;
  auto zzr = [&](int k) { return (two ? 0.5 * (c0.r(k) + c1.r(k)) : c0.r(k)) - surf; };
  const double zs = surf - surf, zb = (two ? 0.5 * (wb0 + wb1) : wb0) - surf;   // zz(N+1), zz(0)
  const double z1 = zzr(1), zn = zzr(N);
  const double dpth = zs - zb;
  const bool masked = d.f.rmask[ij] < 0.5;   // rmask(i,j) at u and v points too, as the reference tests it
  const ZslField* tab = a.tab + a.first[gt];
  const int nf = a.count[gt];

  for (int m0 = 0; m0 < a.ndep; m0 += kZslChunk) {
    const int nq = a.ndep - m0 < kZslChunk ? a.ndep - m0 : kZslChunk;   // the chunk's depths: uniform, dead slots cost a scalar branch
    int cls[kZslChunk], kk[kZslChunk];   // kk: the bracket's lower level; 0 while an interior depth still searches
    double zl[kZslChunk];
    int npend = 0;
#pragma unroll
    for (int q = 0; q < kZslChunk; q++) {
      cls[q] = kZslZero; kk[q] = 1; zl[q] = 0.0;
      if (q >= nq) continue;
      const double zlev = zl[q] = a.dep[m0 + q];
      if (masked) continue;
      if (dpth * (zlev - zs) > 0.0) continue;                                  // above surface
      if (dpth * (zlev - zn) > 0.0) { cls[q] = kZslTop; kk[q] = N - 1; continue; }
      if (dpth * (zb - zlev) > 0.0) continue;                                  // below bottom
      if (dpth * (z1 - zlev) > 0.0) { cls[q] = kZslBottom; continue; }
      cls[q] = kZslInterior;
      kk[q] = 0;
      npend++;
    }
    // kZslAhead levels per trip: their Cs_r (or streamed z_r) loads are issued together and waited on once.
    // The walk keeps kk only: one select per depth and level; the bracket's two zz are formed again below
    double zhi = zn;
    for (int k0 = N - 1; k0 >= 1; k0 -= kZslAhead) {
      if (!__any(npend != 0)) break;
      double zk[kZslAhead];
#pragma unroll
      for (int u = 0; u < kZslAhead; u++) zk[u] = zzr(k0 - u > 1 ? k0 - u : 1);
#pragma unroll
      for (int u = 0; u < kZslAhead; u++) {
        const int k = k0 - u;
        if (k < 1) break;
        const double zlo = zk[u];
#pragma unroll
        for (int q = 0; q < kZslChunk; q++) {
          if (q >= nq) break;
          const bool hit = kk[q] == 0 && (zhi - zl[q]) * (zl[q] - zlo) >= 0.0;
          kk[q] = hit ? k : kk[q];
          npend -= hit ? 1 : 0;
        }
        zhi = zlo;
      }
    }
    double za[kZslChunk], zc[kZslChunk];   // zz(kk), zz(kk+1)
#pragma unroll
    for (int q = 0; q < kZslChunk; q++) {
      za[q] = zc[q] = 0.0;
      if (q >= nq) break;
      // a depth no bracket took (a non-monotonic stored z_r): the reference then reads var(km = -1); here 0
      if (kk[q] == 0) { cls[q] = kZslZero; kk[q] = 1; }
      za[q] = zzr(kk[q]);
      zc[q] = zzr(kk[q] + 1);
    }

    for (int f = 0; f < nf; f++) {
      const ZslField fd = tab[f];
      const double* src = fd.src + a.slot_off + ij;
      double va[kZslChunk], vb[kZslChunk];
#pragma unroll
      for (int q = 0; q < kZslChunk; q++) {   // every load of the chunk in flight before the first division
        const bool on = q < nq && cls[q] != kZslZero;
        va[q] = on ? src[(long)(kk[q] - 1) * n2] : 0.0;
        vb[q] = on ? src[(long)kk[q] * n2] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < kZslChunk; q++) {
        if (q >= nq) break;
        const double zlev = zl[q];
        double x = 0.0;
        if (cls[q] != kZslZero) {
          const double dv = vb[q] - va[q];
          const double num = cls[q] == kZslInterior ? va[q] * (zc[q] - zlev) + vb[q] * (zlev - za[q])
                             : cls[q] == kZslTop    ? (zlev - zc[q]) * dv
                                                    : (za[q] - zlev) * dv;
          const double quo = num / (zc[q] - za[q]);
          x = cls[q] == kZslInterior ? quo : cls[q] == kZslTop ? vb[q] + quo : va[q] - quo;
        }
        const long o = (long)(m0 + q) * n2 + ij;
        fd.out[o] = x;
        if (fd.avg) fd.avg[o] = FIRST ? x * a.coef : fd.avg[o] * a.cm1 + x * a.coef;
      }
    }
  }
}

struct ZslBuf {
  double* base = nullptr;   // the allocation
  double* p = nullptr;      // element IJ = 0 of plane 1, aligned like a 2-D field
};

struct ZslCtx {
  // ndep planes per sliced field in the 2-D device layout, zero outside cells 1..Lm x 1..Mm
  int what = 0;                   // ROMS_ZSL_* bits armed (0: slicing off)
  int ndep = 0;
  MeanWindow w;                   // w.avg: the means are kept (do_avg)
  std::vector<double> vecdep;
  std::vector<int> trc;           // tracer index (1..NT) of each sliced tracer
  std::vector<double*> t, t_avg;  // one per sliced tracer
  double *u = nullptr, *v = nullptr, *u_avg = nullptr, *v_avg = nullptr;
  std::vector<ZslBuf> bufs;
  std::vector<ZslField> fields;   // host copy of the table
  ZslField* d_tab = nullptr;
  int first[3] = {0, 0, 0}, count[3] = {0, 0, 0};
};
thread_local ZslCtx Z;

void zsl_release() {
  for (ZslBuf& b : Z.bufs)
    if (b.base) (void)hipFree(b.base);
  if (Z.d_tab) (void)hipFree(Z.d_tab);
  Z = ZslCtx{};
}

// ndep zeroed planes with the 128-byte phase of `like` (a 2-D field)
double* zsl_alloc(const double* like, long n, hipStream_t s) {
  ZslBuf b;
  const size_t bytes = (size_t)(n + kRowAlign) * sizeof(double);
  if (hipMalloc(&b.base, bytes) != hipSuccess) return nullptr;
  b.p = b.base + ((uintptr_t)like / sizeof(double)) % kRowAlign;
  Z.bufs.push_back(b);
  if (hipMemsetAsync(b.base, 0, bytes, s) != hipSuccess) return nullptr;
  return b.p;
}

int zsl_launch(const ShimState& S, const roms_tlev& t) {
  const Bounds& b = S.d->b;
  ZslArgs a{};
  a.tab = Z.d_tab;
  int nz = 0;
  for (int g = 0; g < 3; g++) {
    a.first[g] = Z.first[g];
    a.count[g] = Z.count[g];
    if (Z.count[g]) a.types[nz++] = g;
  }
  a.ndep = Z.ndep;
  a.slot_off = (long)(t.nnew - 1) * b.n3;
  a.coef = Z.w.coef;
  a.cm1 = Z.w.cm1;
  for (int m = 0; m < Z.ndep; m++) a.dep[m] = Z.vecdep[m];
  const Range R{1, b.Lm, 1, b.Mm};
  const dim3 grid = grid3_of(R, nz), blk(kBX, kBY);
  const bool vg = shim_vgrid_valid(), first = Z.w.sink() != kMean;
  if (vg && first) hipLaunchKernelGGL((k_zslice<true, true>), grid, blk, 0, S.s, *S.d, R, a);
  else if (vg) hipLaunchKernelGGL((k_zslice<true, false>), grid, blk, 0, S.s, *S.d, R, a);
  else if (first) hipLaunchKernelGGL((k_zslice<false, true>), grid, blk, 0, S.s, *S.d, R, a);
  else hipLaunchKernelGGL((k_zslice<false, false>), grid, blk, 0, S.s, *S.d, R, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// one sample: the slices, and with do_avg the means' next step
int zsl_sample(const ShimState& S, const roms_tlev& t) {
  const MeanWindow before = Z.w;
  Z.w.open();
  const int r = zsl_launch(S, t);
  if (r) Z.w = before;
  return r;
}

// the variable list of a slices record (def_vars_zslice): each sliced tracer
// under its name, u, v, ndep planes each (the means with do_avg).  The reference writes 'averaged'
// straight ahead of a tracer's long name and 'averaged ' ahead of u's and v's
std::vector<OutVar> zslice_vars(const ShimState& S) {
  const bool avg = Z.w.avg;
  const long n2 = S.d->b.n2;
  std::vector<OutVar> v;
  if (Z.what & ROMS_ZSL_T) {
    std::vector<std::string> nm, un, ln;
    io_tracer_meta(S, nm, un, ln);
    for (size_t q = 0; q < Z.trc.size(); q++) {
      const int it = Z.trc[q] - 1;
      v.push_back(out_var(S, nm[it], avg ? "averaged" + ln[it] : ln[it], un[it], 'r', 0, Z.ndep, avg ? Z.t_avg[q] : Z.t[q], n2));
    }
  }
  const std::string av = avg ? "averaged " : "";
  if (Z.what & ROMS_ZSL_U)
    v.push_back(out_var(S, "u", av + "u-momentum component", "meter second-1", 'u', 0, Z.ndep, avg ? Z.u_avg : Z.u, n2));
  if (Z.what & ROMS_ZSL_V)
    v.push_back(out_var(S, "v", av + "v-momentum component", "meter second-1", 'v', 0, Z.ndep, avg ? Z.v_avg : Z.v, n2));
  return v;
}

bool zsl_tlev_ok(const roms_tlev* t) { return t && t->nnew >= 1 && t->nnew <= 3; }

}  // namespace

void zslice_free() { zsl_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_zslice_begin(int what, int ndep, const double* vecdep, int nt_z, const int* trc2zsc, int do_avg) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (hipStreamSynchronize(S.s) != hipSuccess) { *S.err = "roms_gpu_zslice_begin: stream synchronisation failed"; return -2; }
  const Bounds& b = S.d->b;
  const Fields& F = S.d->f;
  what &= ROMS_ZSL_T | ROMS_ZSL_U | ROMS_ZSL_V;
  if (!what) { zsl_release(); return 0; }   // disarmed
  if (ndep < 1 || ndep > ROMS_ZSL_MAXDEP || !vecdep) {
    *S.err = "roms_gpu_zslice_begin: ndep must be 1.." + std::to_string(ROMS_ZSL_MAXDEP);
    return -1;
  }
  if (b.N < 2) { *S.err = "roms_gpu_zslice_begin: N < 2 (the half-layer formulas read two levels)"; return -1; }
  if (what & ROMS_ZSL_T) {
    if (nt_z < 1 || !trc2zsc) { *S.err = "roms_gpu_zslice_begin: ROMS_ZSL_T needs nt_z >= 1 tracers"; return -1; }
    for (int q = 0; q < nt_z; q++)
      if (trc2zsc[q] < 1 || trc2zsc[q] > b.NT) {
        *S.err = "roms_gpu_zslice_begin: tracer index " + std::to_string(trc2zsc[q]) + " outside 1.." + std::to_string(b.NT);
        return -1;
      }
  }
  zsl_release();
  ZslCtx& V = Z;
  const long n = (long)ndep * b.n2;
  bool oom = false;
  auto add = [&](const double* src, double*& out, double*& avg) {
    out = zsl_alloc(F.zeta, n, S.s);
    avg = do_avg && out ? zsl_alloc(F.zeta, n, S.s) : nullptr;
    if (!out || (do_avg && !avg)) oom = true;
    Z.fields.push_back(ZslField{src, out, avg});
  };
  if (what & ROMS_ZSL_T) {
    Z.first[0] = 0;
    Z.count[0] = nt_z;
    V.t.assign(nt_z, nullptr);
    V.t_avg.assign(nt_z, nullptr);
    for (int q = 0; q < nt_z && !oom; q++) {
      V.trc.push_back(trc2zsc[q]);
      add(F.t + (long)(trc2zsc[q] - 1) * 3 * b.n3, V.t[q], V.t_avg[q]);
    }
  }
  if (!oom && (what & ROMS_ZSL_U)) { Z.first[1] = (int)Z.fields.size(); Z.count[1] = 1; add(F.u, V.u, V.u_avg); }
  if (!oom && (what & ROMS_ZSL_V)) { Z.first[2] = (int)Z.fields.size(); Z.count[2] = 1; add(F.v, V.v, V.v_avg); }
  if (!oom) {
    const size_t bytes = Z.fields.size() * sizeof(ZslField);
    oom = hipMalloc(&Z.d_tab, bytes) != hipSuccess ||
          copy_on(Z.d_tab, Z.fields.data(), bytes, hipMemcpyHostToDevice, S.s) != hipSuccess;
  }
  if (oom) {
    (void)hipStreamSynchronize(S.s);
    zsl_release();
    *S.err = "roms_gpu_zslice_begin: allocation of the slice planes failed";
    return -2;
  }
  V.what = what;
  V.ndep = ndep;
  V.w.avg = do_avg != 0;
  V.vecdep.assign(vecdep, vecdep + ndep);
  return 0;
}

int roms_gpu_calc_zslice(const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Z.what) { *S.err = "roms_gpu_calc_zslice: slicing is not armed (roms_gpu_zslice_begin)"; return -4; }
  if (!zsl_tlev_ok(t)) { *S.err = "roms_gpu_calc_zslice: bad time levels"; return -1; }
  if ((r = zsl_sample(S, *t))) { *S.err = "roms_gpu_calc_zslice: launch failed"; return r; }
  return 0;
}

int roms_gpu_wrt_zslice(const char* path, int rec, int total_rec, double time, const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Z.what) { *S.err = "roms_gpu_wrt_zslice: slicing is not armed (roms_gpu_zslice_begin)"; return -4; }
  if (!path || rec < 1 || !zsl_tlev_ok(t)) { *S.err = "roms_gpu_wrt_zslice: bad path/record/time levels"; return -1; }
  if (Z.w.avg && !Z.w.have) { *S.err = "roms_gpu_wrt_zslice: no sample in the window (roms_gpu_calc_zslice)"; return -4; }
  if (!Z.w.avg && (r = zsl_sample(S, *t))) { *S.err = "roms_gpu_wrt_zslice: launch failed"; return r; }
  RecordSpec spec;
  spec.type = "ROMS zslice file";
  spec.time = time;
  spec.depths = Z.vecdep;
  spec.vars = zslice_vars(S);
  if ((r = write_record(S, path, rec, total_rec, t, spec))) return r;
  Z.w.written();   // the next sample starts a fresh window (zslice_output.F:406)
  return 0;
}

int roms_gpu_zslice_state(int* navg, int* what, int* ndep, int* do_avg) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (navg) *navg = Z.w.reported();
  if (what) *what = Z.what;
  if (ndep) *ndep = Z.ndep;
  if (do_avg) *do_avg = Z.w.avg ? 1 : 0;
  return 0;
}

int roms_gpu_zslice_copy_out(int what_bit, int q, double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const ZslCtx& V = Z;
  const bool do_avg = V.w.avg;
  if (what_bit != ROMS_ZSL_T && what_bit != ROMS_ZSL_U && what_bit != ROMS_ZSL_V) {
    *S.err = "roms_gpu_zslice_copy_out: what_bit must be one ROMS_ZSL_* bit";
    return -1;
  }
  if (!(V.what & what_bit) || !dst) { *S.err = "roms_gpu_zslice_copy_out: that field is not being sliced"; return -4; }
  const double* p = nullptr;
  if (what_bit == ROMS_ZSL_T) {
    if (q < 1 || q > (int)V.t.size()) { *S.err = "roms_gpu_zslice_copy_out: no such sliced tracer"; return -1; }
    p = do_avg ? V.t_avg[q - 1] : V.t[q - 1];
  } else if (what_bit == ROMS_ZSL_U) {
    p = do_avg ? V.u_avg : V.u;
  } else {
    p = do_avg ? V.v_avg : V.v;
  }
  const long rows = (long)V.ndep * (S.d->b.Mm + 4);
  if (count != rows * (S.d->b.Lm + 4)) { *S.err = "roms_gpu_zslice_copy_out: count is not ndep*(Mm+4)*(Lm+4)"; return -1; }
  if (shim_rows_d2h(dst, p, rows) != hipSuccess) { *S.err = "roms_gpu_zslice_copy_out: copy failed"; return -2; }
  return 0;
}

// n samples between two events on the library stream (tools/zslice_cost.py).
// With do_avg they go on from the open window (navg += n): after one
// roms_gpu_calc_zslice every timed sample reads the old mean
int roms_gpu_time_calc_zslice(int n, const roms_tlev* t, double* ms) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!Z.what) { *S.err = "roms_gpu_time_calc_zslice: slicing is not armed (roms_gpu_zslice_begin)"; return -4; }
  if (!zsl_tlev_ok(t) || n < 1 || !ms) { *S.err = "roms_gpu_time_calc_zslice: bad arguments"; return -1; }
  const double f = time_rounds(S.s, n, false, [&]() { return zsl_sample(S, *t); });
  if (f < 0) { *S.err = "roms_gpu_time_calc_zslice: launch or timing failed"; return (int)f; }
  *ms = f;
  return 0;
}

}  // extern "C"
