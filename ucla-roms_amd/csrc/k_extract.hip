// k_extract.hip -- child-boundary extraction on the device: do_extract_data of
// extract_data.F with the vertical remap of vertical_remapping.F.  Objects are
// lines of fractional positions (a child grid's boundary, a mooring); every
// sample interpolates zeta, ubar, vbar (slot knew) and u, v, temp, salt (slot
// nstp) to them with mask-weighted bilinear coefficients, rotates the vectors
// to each point's angle and, when the child's vertical grid differs from the
// parent's, remaps every profile conservatively onto the child's N_chd layers
// (piecewise parabolas, White and Adcroft 2008).
//
// Host part (arm time): read_extraction_objects, find_local_points,
// init_extract_data, compute_coef, set_chd_scoord restated; the quirks kept
// are listed in DESIGN.md 3d (first contiguous run only, findstr flags, NaN
// coefficients of a point with four masked corners).
//
// MI355X design: the points of all objects form one list; lanes run along it.
// k_ext_interp (one launch, blockIdx.y = 2-D / rho 3-D / u,v 3-D work) walks
// the levels with the four corner loads of kExtAhead levels in flight and
// writes (level, point) staging, point-fastest, so the per-column work arrays
// of the remap are coalesced across lanes.  k_ext_remap (one launch) runs
// blocks of 64 points x 4 variables: first the lanes y < 3 form, per point and
// grid type, the child thicknesses and the search (tgt_index_end,
// tgt_frac_end), which depend on the thicknesses only; after the barrier one
// lane per (point, variable) forms the interface values, the parabola
// coefficients and the integrals with its type's search.  The column work
// arrays (length N+1) live in global scratch.  Integer powers are products:
// x**2 = x*x, x**3 = (x*x)*x, x**4 = (x*x)*(x*x); no contraction
// (-ffp-contract=off), IEEE division.  The source-index search is clamped to
// N_src, so no data (NaN included) indexes past the column.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/roms_gpu.h"
#include "ncio.h"
#include "roms_dev.h"
#include "shim_state.h"

namespace roms {
namespace {

constexpr int kExtAhead = 4;   // levels whose corner loads one trip of a walk has in flight
constexpr int kExtSupported = ROMS_EXT_ZETA | ROMS_EXT_UBAR | ROMS_EXT_VBAR | ROMS_EXT_U | ROMS_EXT_V | ROMS_EXT_TEMP | ROMS_EXT_SALT;
constexpr int kExtPflx = ROMS_EXT_UP | ROMS_EXT_VP;   // produced for objects added while the pressure fluxes are armed (k_pflx.hip)
constexpr int kExtVector = ROMS_EXT_UBAR | ROMS_EXT_VBAR | ROMS_EXT_U | ROMS_EXT_V | kExtPflx;
constexpr int kExt3d = ROMS_EXT_U | ROMS_EXT_V | ROMS_EXT_TEMP | ROMS_EXT_SALT;
// 3-D variable slots: 0 u, 1 v, 2 temp, 3 salt; their grid types 1 u, 2 v, 0 rho
__host__ __device__ constexpr int ext_bit3(int v) { return v == 0 ? ROMS_EXT_U : v == 1 ? ROMS_EXT_V : v == 2 ? ROMS_EXT_TEMP : ROMS_EXT_SALT; }
__host__ __device__ constexpr int ext_type3(int v) { return v == 0 ? 1 : v == 1 ? 2 : 0; }

struct ExtArgs {
  int NP, N, Nc, mismatch, nx2;
  long n2;
  const int* ij[3];        // per grid type (rho, u, v): IJ of the lower left corner
  const double* cf[3];     // (4, NP) coefficients
  const double *cosa, *sina;
  const int* vars;         // the armed ROMS_EXT_* bits of the point's object
  const double *zeta, *ubar, *vbar;   // slot knew
  const double *u, *v, *temp, *salt;  // slot nstp (salt: nullptr without salinity)
  const double *Hz, *Hz_u, *Hz_v;
  double* o2[3];           // zeta, ubar, vbar (NP)
  double* prof[4];         // u, v, temp, salt: (N, NP) interpolated, rotated
  double* hzp[3];          // parent thickness at rho, u, v points (N, NP)
  double* outc[4];         // remapped (Nc, NP)
  double* wk[4];           // per variable: iv, cp -> a1, dp -> a2, (N+1, NP) each
  double* hzc[3];          // child thickness (Nc, NP)
  double* fend[3];         // tgt_frac_end (Nc, NP)
  int* iend[3];            // tgt_index_end (Nc, NP)
  const double* csw;       // Cs_w_chd(0:Nc)
  double hc_chd;
};

// interpolate_2D / interpolate_3D: the four products summed left to right
__device__ __forceinline__ double ext_at(const double* __restrict__ f, int nx2, double c0, double c1, double c2, double c3) {
  return f[0] * c0 + f[1] * c1 + f[nx2] * c2 + f[nx2 + 1] * c3;
}
__device__ __forceinline__ void ext_walk(const double* __restrict__ src, int nx2, long n2, int N, const double c[4],
                                         double* __restrict__ dst, int NP) {
  for (int k0 = 0; k0 < N; k0 += kExtAhead) {
    double a[kExtAhead][4];
#pragma unroll
    for (int q = 0; q < kExtAhead; q++) {
      const double* s = src + (long)(k0 + q < N ? k0 + q : N - 1) * n2;
      a[q][0] = s[0]; a[q][1] = s[1]; a[q][2] = s[nx2]; a[q][3] = s[nx2 + 1];
    }
#pragma unroll
    for (int q = 0; q < kExtAhead; q++)
      if (k0 + q < N) dst[(long)(k0 + q) * NP] = a[q][0] * c[0] + a[q][1] * c[1] + a[q][2] * c[2] + a[q][3] * c[3];
  }
}

__global__ void __launch_bounds__(64) k_ext_interp(ExtArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.NP) return;
  const int vars = a.vars[p], NP = a.NP, N = a.N, nx2 = a.nx2;
  const long n2 = a.n2;
  double c[3][4];
  long o[3];
#pragma unroll
  for (int g = 0; g < 3; g++) {
    o[g] = a.ij[g][p];
#pragma unroll
    for (int q = 0; q < 4; q++) c[g][q] = a.cf[g][(long)q * NP + p];
  }
  const double cs = a.cosa[p], sn = a.sina[p];
  if (blockIdx.y == 0) {   // the 2-D variables
    if (vars & ROMS_EXT_ZETA) a.o2[0][p] = ext_at(a.zeta + o[0], nx2, c[0][0], c[0][1], c[0][2], c[0][3]);
    if (vars & (ROMS_EXT_UBAR | ROMS_EXT_VBAR)) {
      const double ui = ext_at(a.ubar + o[1], nx2, c[1][0], c[1][1], c[1][2], c[1][3]);
      const double vi = ext_at(a.vbar + o[2], nx2, c[2][0], c[2][1], c[2][2], c[2][3]);
      if (vars & ROMS_EXT_UBAR) a.o2[1][p] = cs * ui - sn * vi;
      if (vars & ROMS_EXT_VBAR) a.o2[2][p] = sn * ui + cs * vi;
    }
  } else if (blockIdx.y == 1) {   // rho points: temp, salt and the parent's Hz
    if (!(vars & (ROMS_EXT_TEMP | ROMS_EXT_SALT))) return;
    if (vars & ROMS_EXT_TEMP) ext_walk(a.temp + o[0], nx2, n2, N, c[0], a.prof[2] + p, NP);
    if (vars & ROMS_EXT_SALT) ext_walk(a.salt + o[0], nx2, n2, N, c[0], a.prof[3] + p, NP);
    if (a.mismatch) ext_walk(a.Hz + o[0], nx2, n2, N, c[0], a.hzp[0] + p, NP);
  } else {   // u and v, both interpolated for the rotation, and Hz_u / Hz_v
    if (!(vars & (ROMS_EXT_U | ROMS_EXT_V))) return;
    const double* __restrict__ us = a.u + o[1];
    const double* __restrict__ vs = a.v + o[2];
    for (int k0 = 0; k0 < N; k0 += kExtAhead) {
      double x[kExtAhead][4], y[kExtAhead][4];
#pragma unroll
      for (int q = 0; q < kExtAhead; q++) {
        const long ok = (long)(k0 + q < N ? k0 + q : N - 1) * n2;
        x[q][0] = us[ok]; x[q][1] = us[ok + 1]; x[q][2] = us[ok + nx2]; x[q][3] = us[ok + nx2 + 1];
        y[q][0] = vs[ok]; y[q][1] = vs[ok + 1]; y[q][2] = vs[ok + nx2]; y[q][3] = vs[ok + nx2 + 1];
      }
#pragma unroll
      for (int q = 0; q < kExtAhead; q++) {
        if (k0 + q >= N) break;
        const double ui = x[q][0] * c[1][0] + x[q][1] * c[1][1] + x[q][2] * c[1][2] + x[q][3] * c[1][3];
        const double vi = y[q][0] * c[2][0] + y[q][1] * c[2][1] + y[q][2] * c[2][2] + y[q][3] * c[2][3];
        const long od = (long)(k0 + q) * NP + p;
        if (vars & ROMS_EXT_U) a.prof[0][od] = cs * ui - sn * vi;
        if (vars & ROMS_EXT_V) a.prof[1][od] = sn * ui + cs * vi;
      }
    }
    if (a.mismatch && (vars & ROMS_EXT_U)) ext_walk(a.Hz_u + o[1], nx2, n2, N, c[1], a.hzp[1] + p, NP);
    if (a.mismatch && (vars & ROMS_EXT_V)) ext_walk(a.Hz_v + o[2], nx2, n2, N, c[2], a.hzp[2] + p, NP);
  }
}

// up, vp (extract_data.F:764-770, 815-821): upe, vpe interpolated with the u and the v coefficients, rotated.  A
// launch of its own beside k_ext_interp, taken only while an object asks for them
struct ExtPfArgs {
  int NP, nx2;
  const int *iju, *ijv, *vars;
  const double *cfu, *cfv, *cosa, *sina;
  const double *upe, *vpe;   // up, vp inside 1..nx x 1..ny, 0 elsewhere, halos exchanged
  double *oup, *ovp;         // (NP)
};
__global__ void __launch_bounds__(64) k_ext_pflx(ExtPfArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.NP) return;
  const int vars = a.vars[p], NP = a.NP;
  if (!(vars & kExtPflx)) return;
  const double ui = ext_at(a.upe + a.iju[p], a.nx2, a.cfu[p], a.cfu[(long)NP + p], a.cfu[(long)2 * NP + p], a.cfu[(long)3 * NP + p]);
  const double vi = ext_at(a.vpe + a.ijv[p], a.nx2, a.cfv[p], a.cfv[(long)NP + p], a.cfv[(long)2 * NP + p], a.cfv[(long)3 * NP + p]);
  const double cs = a.cosa[p], sn = a.sina[p];
  if (vars & ROMS_EXT_UP) a.oup[p] = cs * ui - sn * vi;
  if (vars & ROMS_EXT_VP) a.ovp[p] = sn * ui + cs * vi;
}

// x**n of the reference, n = 1..4, as products
__device__ __forceinline__ double ext_pow(double x, int n) {
  return n == 1 ? x : n == 2 ? x * x : n == 3 ? (x * x) * x : (x * x) * (x * x);
}
// gauss (vertical_remapping.F:265-296): first element of the solution
__device__ __forceinline__ double ext_gauss(double M[4][4], double b[4]) {
#pragma unroll
  for (int i = 3; i >= 1; i--) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (j >= i) continue;
      const double ratio = M[j][i] / M[i][i];
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (k <= i) M[j][k] = M[j][k] - ratio * M[i][k];
      b[j] = b[j] - ratio * b[i];
    }
  }
  return b[0] / M[0][0];
}
// the boundary extrapolations of calc_interface_values: up = false from the
// bottom (cells 1..5), up = true from the top (cells N..N-4)
__device__ __forceinline__ double ext_edge(const double* __restrict__ H, const double* __restrict__ A, int N, int NP, bool top) {
  double M[4][4], B[4];
  auto at = [&](const double* f, int k) { return f[(long)((top ? N + 1 - k : k) - 1) * NP]; };   // k = 1..5 from the edge
  double h_b = 0.0, h_t = at(H, 1);
  double iH = 1.0 / (h_t - h_b);
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int kk = 0; kk < 4; kk++) M[k][kk] = (1.0 / (double)(kk + 1)) * iH * (ext_pow(h_t, kk + 1) - ext_pow(h_b, kk + 1));
    h_b = h_b + at(H, k + 1);
    h_t = h_t + at(H, k + 2);
    iH = 1.0 / (h_t - h_b);
    B[k] = at(A, k + 1);
  }
  return ext_gauss(M, B);
}
// integrate (vertical_remapping.F:182-193); one_third as the reference writes it
__device__ __forceinline__ double ext_integ(double a0, double a1, double a2, double z0, double z1) {
  const double one_third = 0.3333333333;
  return a0 * (z1 - z0) + 0.5 * a1 * (z1 * z1 - z0 * z0) + one_third * a2 * ((z1 * z1) * z1 - (z0 * z0) * z0);
}

__global__ void __launch_bounds__(256) k_ext_remap(ExtArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x, y = threadIdx.y;
  const int NP = a.NP, N = a.N, Nc = a.Nc;
  const int vars = p < NP ? a.vars[p] : 0;
  // ---- per point and grid type: child thickness and the search ----
  const int need_t = y == 0 ? (ROMS_EXT_TEMP | ROMS_EXT_SALT) : y == 1 ? ROMS_EXT_U : y == 2 ? ROMS_EXT_V : 0;
  if (vars & need_t) {
    const double* __restrict__ H = a.hzp[y] + p;
    double* __restrict__ hzc = a.hzc[y] + p;
    double* __restrict__ fend = a.fend[y] + p;
    int* __restrict__ iend = a.iend[y] + p;
    double h = 0.0;   // h_par, and total_depth_src: the same sum
    for (int k = 0; k < N; k++) h = h + H[(long)k * NP];
    // get_child_thickness
    const double ds = 1.0 / (double)Nc, hc = a.hc_chd;
    const double hinv = 1.0 / (h + hc);
    double zprev = -h, tdt = 0.0;
    for (int k = 1; k <= Nc; k++) {
      const double cff_w = hc * ds * (double)(k - Nc);
      const double z = h * (cff_w + a.csw[k] * h) * hinv;
      const double hz = z - zprev;
      hzc[(long)(k - 1) * NP] = hz;
      tdt = tdt + hz;
      zprev = z;
    }
    // H_orig: the source thicknesses rescaled to the target depth, the rest on the top layer
    const double scale = tdt / h;
    double hst = 0.0;
    for (int k = 0; k < N; k++) hst = hst + H[(long)k * NP] * scale;
    auto horig = [&](int idx) {
      const double x = H[(long)(idx - 1) * NP] * scale;
      return idx == N ? x + tdt - hst : x;
    };
    double cth = hzc[0], csh = horig(1), zlo = 0.0;   // zlo: z_orig_interfaces(idx)
    int idx = 1;
    for (int kn = 1; kn < Nc; kn++) {
      while (cth > csh && idx < N) {   // idx < N: the clamp the reference lacks
        zlo = zlo + horig(idx);
        idx++;
        csh = csh + horig(idx);
      }
      iend[(long)(kn - 1) * NP] = idx;
      fend[(long)(kn - 1) * NP] = (cth - zlo) / horig(idx);
      cth = cth + hzc[(long)kn * NP];
    }
    iend[(long)(Nc - 1) * NP] = N;
    fend[(long)(Nc - 1) * NP] = 1.0;
  }
  __syncthreads();
  // ---- per point and variable ----
  if (!(vars & ext_bit3(y))) return;
  const int g = ext_type3(y);
  const double* __restrict__ H = a.hzp[g] + p;
  const double* __restrict__ A = a.prof[y] + p;
  const double* __restrict__ Ht = a.hzc[g] + p;
  const double* __restrict__ fend = a.fend[g] + p;
  const int* __restrict__ iend = a.iend[g] + p;
  double* __restrict__ out = a.outc[y] + p;
  const long nw = (long)(N + 1) * NP;
  double* __restrict__ iv = a.wk[y] + p;   // interface values (1..N+1), then a0
  double* __restrict__ cp = iv + nw;       // cp of thomas_PPM, then a1
  double* __restrict__ dp = cp + nw;       // dp, then a2
  const double Ts_bot = ext_edge(H, A, N, NP, false), Ts_top = ext_edge(H, A, N, NP, true);
  // thomas_PPM: b = 1, a = alpha, c = beta; cp(1) = 0/1, dp(1) = Ts_bot/1
  double cpk = 0.0 / 1.0, dpk = Ts_bot / 1.0;
  cp[0] = cpk;
  dp[0] = dpk;
  double h0 = H[0], t0 = A[0];
  double tts = 0.0 + t0 * h0;   // total_t_src
  for (int k = 2; k <= N; k++) {
    const double h1 = H[(long)(k - 1) * NP], t1 = A[(long)(k - 1) * NP];
    const double s = h0 + h1, s2 = s * s, s4 = (s * s) * (s * s);
    const double alpha = (h1 * h1) / s2, beta = (h0 * h0) / s2;
    const double d1 = 2 * (h1 * h1) * (h1 * h1 + 2 * (h0 * h0) + 3 * h0 * h1) / s4;
    const double d2 = 2 * (h0 * h0) * (h0 * h0 + 2 * (h1 * h1) + 3 * h0 * h1) / s4;
    const double d = d1 * t0 + d2 * t1;
    const double den = 1.0 - alpha * cpk;
    cpk = beta / den;
    dpk = (d - alpha * dpk) / den;
    cp[(long)(k - 1) * NP] = cpk;
    dp[(long)(k - 1) * NP] = dpk;
    tts = tts + t1 * h1;
    h0 = h1;
    t0 = t1;
  }
  double ivn = Ts_top;   // int_vals(k+1)
  iv[(long)N * NP] = ivn;
  for (int k = N; k >= 1; k--) {
    const long ok = (long)(k - 1) * NP;
    const double ivk = dp[ok] - cp[ok] * ivn, t = A[ok];
    iv[ok] = ivk;                                // a0
    cp[ok] = 6 * t - 4 * ivk - 2 * ivn;          // a1
    dp[ok] = 3 * (ivk + ivn - 2 * t);            // a2
    ivn = ivk;
  }
  // the integrals over each target cell
  double tt = 0.0, fs = 0.0;
  int is = 1;
  for (int k = 1; k <= Nc; k++) {
    const long okc = (long)(k - 1) * NP;
    const int ie = iend[okc];
    const double fe = fend[okc], ht = Ht[okc];
    double di = 0.0;
    for (int idx = is; idx <= ie; idx++) {
      const long ok = (long)(idx - 1) * NP;
      const double a0 = iv[ok], a1 = cp[ok], a2 = dp[ok], hs = H[ok];
      if (is == ie) di = ext_integ(a0, a1, a2, fs, fe) * hs;
      else if (idx == is) di = ext_integ(a0, a1, a2, fs, 1.0) * hs;
      else if (idx < ie) di = di + ext_integ(a0, a1, a2, 0.0, 1.0) * hs;
      else di = di + ext_integ(a0, a1, a2, 0.0, fe) * hs;
    }
    const double tmp = di / ht;
    out[okc] = tmp;
    tt = tt + tmp * ht;
    is = ie;
    fs = fe;
  }
  // the mass correction, spread by each cell's share
  const double diff = tt - tts;
  for (int k = 0; k < Nc; k++) {
    const double tmp = out[(long)k * NP];
    out[(long)k * NP] = tt != 0.0 ? tmp - diff * (tmp / tt) : 0.0;
  }
}

struct ExtObject {
  std::string name, dname, set, bnd;
  int dsize = 0, np = 0, start_idx = 0, vars = 0, unsupported = 0, p0 = 0;
  bool scalar = true;
  std::vector<double> ang;            // the local points' angles (vector objects)
  std::vector<int> ip[3], jp[3];
  std::vector<double> cf[3];          // (4, np)
  std::vector<double> cosa, sina;
};

struct ExtCtx {
  bool begun = false, mismatch = false, built = false, sampled = false;
  int Nc = 0;
  double theta_s = 0.0, theta_b = 0.0, hc = 0.0;
  std::vector<double> csw;                      // Cs_w_chd(0:Nc)
  std::vector<ExtObject> obj;
  std::vector<double> rmask, umask, vmask, angler;   // host copies, rows of Lm+4
  bool have_masks = false;
  int NP = 0;
  std::vector<void*> dev;                       // every device allocation
  ExtArgs a{};
  double *oup = nullptr, *ovp = nullptr;        // up, vp of every point (NP; among dev)
  double *upe_base = nullptr, *vpe_base = nullptr, *upe = nullptr, *vpe = nullptr;   // extract_data.F's upe, vpe: one plane each
  double* pack = nullptr;
  size_t pack_n = 0;
};
thread_local ExtCtx E;

void ext_release_device() {
  for (void* q : E.dev)
    if (q) (void)hipFree(q);
  E.dev.clear();
  if (E.pack) (void)hipFree(E.pack);
  E.pack = nullptr;
  E.pack_n = 0;
  E.a = ExtArgs{};
  E.oup = E.ovp = nullptr;
  E.built = E.sampled = false;
}
void ext_release() {
  ext_release_device();
  if (E.upe_base) (void)hipFree(E.upe_base);
  if (E.vpe_base) (void)hipFree(E.vpe_base);
  E = ExtCtx{};
  shim_extract_huv(false);
}

int ext_union() {
  int u = 0;
  for (const ExtObject& o : E.obj) u |= o.vars;
  return u;
}
bool ext_need_huv() { return E.mismatch && (ext_union() & (ROMS_EXT_U | ROMS_EXT_V)); }

// findstr of roms_read_write.F: is `sub` a substring of `s`
bool ext_find(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }

// find_local_points (extract_data.F:421-473): the first contiguous run inside the subdomain
void ext_locate(int nx, int ny, int isw, int jsw, long npg, const double* ipos, const double* jpos, int* start_idx, int* np) {
  auto in = [&](long q) {
    const double x = ipos[q] - (double)isw, y = jpos[q] - (double)jsw;
    return x >= 0 && x < nx && y >= 0 && y < ny;
  };
  long s = -1;
  for (long q = 0; q < npg; q++)
    if (in(q)) { s = q; break; }
  if (s < 0) { *start_idx = 0; *np = 0; return; }
  long e = npg - 1;
  for (long q = s; q < npg; q++)
    if (!in(q)) { e = q - 1; break; }
  *start_idx = (int)(s + 1);
  *np = (int)(e - s + 1);
}

// compute_coef (extract_data.F:475-503); mask in the host layout, rows of w
void ext_coef(const std::vector<double>& ipos, const std::vector<double>& jpos, const std::vector<double>& mask, int w,
              std::vector<int>& ip, std::vector<int>& jp, std::vector<double>& cf) {
  const size_t np = ipos.size();
  ip.resize(np); jp.resize(np); cf.resize(4 * np);
  auto M = [&](int i, int j) { return mask[(size_t)(j + 1) * w + (i + 1)]; };
  for (size_t q = 0; q < np; q++) {
    const int i = (int)std::floor(ipos[q]), j = (int)std::floor(jpos[q]);
    const double cfx = ipos[q] - (double)i, cfy = jpos[q] - (double)j;
    const double c0 = (1 - cfx) * (1 - cfy) * M(i, j), c1 = cfx * (1 - cfy) * M(i + 1, j);
    const double c2 = (1 - cfx) * cfy * M(i, j + 1), c3 = cfx * cfy * M(i + 1, j + 1);
    const double sum = c0 + c1 + c2 + c3;   // 0 when all four corners are masked: NaN coefficients, as the reference
    ip[q] = i; jp[q] = j;
    cf[q] = c0 / sum; cf[np + q] = c1 / sum; cf[2 * np + q] = c2 / sum; cf[3 * np + q] = c3 / sum;
  }
}

// calc_cs / set_chd_scoord (extract_data.F:962-998)
double ext_calc_cs(double sc, double theta_s, double theta_b) {
  double csrf;
  if (theta_s > 0.0) csrf = (1.0 - std::cosh(theta_s * sc)) / (std::cosh(theta_s) - 1.0);
  else csrf = -(sc * sc);
  if (theta_b > 0.0) return (std::exp(theta_b * csrf) - 1.0) / (1.0 - std::exp(-theta_b));
  return csrf;
}

template <class T>
T* ext_alloc(size_t n, hipStream_t s, bool& oom) {
  if (oom) return nullptr;
  void* q = nullptr;
  const size_t bytes = (n < 1 ? 1 : n) * sizeof(T);
  if (hipMalloc(&q, bytes) != hipSuccess || hipMemsetAsync(q, 0, bytes, s) != hipSuccess) { oom = true; return nullptr; }
  E.dev.push_back(q);
  return (T*)q;
}

int ext_masks(const ShimState& S) {
  if (E.have_masks) return 0;
  const Bounds& b = S.d->b;
  const size_t n = (size_t)(b.Mm + 4) * (b.Lm + 4);
  E.rmask.resize(n); E.umask.resize(n); E.vmask.resize(n);
  if (shim_rows_d2h(E.rmask.data(), S.d->f.rmask, b.Mm + 4) != hipSuccess ||
      shim_rows_d2h(E.umask.data(), S.d->f.umask, b.Mm + 4) != hipSuccess ||
      shim_rows_d2h(E.vmask.data(), S.d->f.vmask, b.Mm + 4) != hipSuccess)
    return -2;
  if (E.angler.size() != n) E.angler.assign(n, 0.0);
  E.have_masks = true;
  return 0;
}

// the device tables and buffers of the armed objects
int ext_build(const ShimState& S) {
  if (E.built) return 0;
  ext_release_device();
  const Bounds& b = S.d->b;
  int NP = 0;
  for (ExtObject& o : E.obj) { o.p0 = NP; NP += o.np; }
  E.NP = NP;
  if (NP == 0) { E.built = true; return 0; }
  const int N = b.N, Nc = E.Nc, un = ext_union();
  std::vector<int> hij[3], hvars(NP, 0);
  std::vector<double> hcf[3], hcs(NP, 1.0), hsn(NP, 0.0);
  for (int g = 0; g < 3; g++) { hij[g].assign(NP, (int)IJ(b, 0, 0)); hcf[g].assign((size_t)4 * NP, 0.0); }
  for (const ExtObject& o : E.obj) {
    for (int q = 0; q < o.np; q++) {
      const int p = o.p0 + q;
      hvars[p] = o.vars;
      for (int g = 0; g < (o.scalar ? 1 : 3); g++) {
        hij[g][p] = (int)IJ(b, o.ip[g][q], o.jp[g][q]);
        for (int c = 0; c < 4; c++) hcf[g][(size_t)c * NP + p] = o.cf[g][(size_t)c * o.np + q];
      }
      if (!o.scalar) { hcs[p] = o.cosa[q]; hsn[p] = o.sina[q]; }
    }
  }
  bool oom = false;
  ExtArgs a{};
  a.NP = NP; a.N = N; a.Nc = Nc; a.mismatch = E.mismatch ? 1 : 0; a.nx2 = b.nx2; a.n2 = b.n2;
  a.hc_chd = E.hc;
  auto up = [&](const void* h, size_t bytes, void* d) {
    if (!oom && hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, S.s) != hipSuccess) oom = true;
  };
  for (int g = 0; g < 3; g++) {
    int* dij = ext_alloc<int>(NP, S.s, oom);
    double* dcf = ext_alloc<double>((size_t)4 * NP, S.s, oom);
    up(hij[g].data(), (size_t)NP * sizeof(int), dij);
    up(hcf[g].data(), (size_t)4 * NP * sizeof(double), dcf);
    a.ij[g] = dij; a.cf[g] = dcf;
  }
  double *dcs = ext_alloc<double>(NP, S.s, oom), *dsn = ext_alloc<double>(NP, S.s, oom);
  int* dv = ext_alloc<int>(NP, S.s, oom);
  up(hcs.data(), (size_t)NP * sizeof(double), dcs);
  up(hsn.data(), (size_t)NP * sizeof(double), dsn);
  up(hvars.data(), (size_t)NP * sizeof(int), dv);
  a.cosa = dcs; a.sina = dsn; a.vars = dv;
  for (int q = 0; q < 3; q++) a.o2[q] = ext_alloc<double>(NP, S.s, oom);
  if (un & kExtPflx) { E.oup = ext_alloc<double>(NP, S.s, oom); E.ovp = ext_alloc<double>(NP, S.s, oom); }
  for (int v = 0; v < 4; v++) {
    if (!(un & ext_bit3(v))) continue;
    a.prof[v] = ext_alloc<double>((size_t)N * NP, S.s, oom);
    if (!E.mismatch) continue;
    a.outc[v] = ext_alloc<double>((size_t)Nc * NP, S.s, oom);
    a.wk[v] = ext_alloc<double>((size_t)3 * (N + 1) * NP, S.s, oom);
  }
  if (E.mismatch) {
    for (int g = 0; g < 3; g++) {
      const int bits = g == 0 ? (ROMS_EXT_TEMP | ROMS_EXT_SALT) : g == 1 ? ROMS_EXT_U : ROMS_EXT_V;
      if (!(un & bits)) continue;
      a.hzp[g] = ext_alloc<double>((size_t)N * NP, S.s, oom);
      a.hzc[g] = ext_alloc<double>((size_t)Nc * NP, S.s, oom);
      a.fend[g] = ext_alloc<double>((size_t)Nc * NP, S.s, oom);
      a.iend[g] = ext_alloc<int>((size_t)Nc * NP, S.s, oom);
    }
    double* dcsw = ext_alloc<double>(Nc + 1, S.s, oom);
    up(E.csw.data(), (size_t)(Nc + 1) * sizeof(double), dcsw);
    a.csw = dcsw;
  }
  if (oom || hipStreamSynchronize(S.s) != hipSuccess) {   // the uploads read host vectors of this scope
    (void)hipStreamSynchronize(S.s);
    ext_release_device();
    return -2;
  }
  E.a = a;
  E.built = true;
  return 0;
}

bool ext_tlev_ok(const roms_tlev* t) { return t && t->knew >= 1 && t->knew <= 4 && t->nstp >= 1 && t->nstp <= 3; }

void ext_slots(const ShimState& S, const roms_tlev& t) {
  const Bounds& b = S.d->b;
  const Fields& F = S.d->f;
  ExtArgs& a = E.a;
  a.zeta = F.zeta + (long)(t.knew - 1) * b.n2;
  a.ubar = F.ubar + (long)(t.knew - 1) * b.n2;
  a.vbar = F.vbar + (long)(t.knew - 1) * b.n2;
  a.u = F.u + (long)(t.nstp - 1) * b.n3;
  a.v = F.v + (long)(t.nstp - 1) * b.n3;
  a.temp = F.t + (long)(t.nstp - 1) * b.n3;
  a.salt = b.NT >= 2 ? F.t + (long)(t.nstp - 1) * b.n3 + (long)3 * b.n3 : nullptr;
  a.Hz = F.Hz; a.Hz_u = F.Hz_u; a.Hz_v = F.Hz_v;
}
void ext_launch_interp(const ShimState& S) {
  hipLaunchKernelGGL(k_ext_interp, dim3((E.NP + 63) / 64, 3), dim3(64), 0, S.s, E.a);
}
void ext_launch_pflx(const ShimState& S) {
  const ExtArgs& a = E.a;
  const ExtPfArgs q{a.NP, a.nx2, a.ij[1], a.ij[2], a.vars, a.cf[1], a.cf[2], a.cosa, a.sina, E.upe, E.vpe, E.oup, E.ovp};
  hipLaunchKernelGGL(k_ext_pflx, dim3((E.NP + 63) / 64), dim3(64), 0, S.s, q);
}
// upe(1:nx,1:ny) = up, vpe alike, and their halos (extract_data.F:598-604): every rank of a decomposed run takes part
int ext_pflx_planes(const ShimState& S, const char* who) {
  const PflxView pf = pflx_view();
  if (!pf.armed) {
    *S.err = std::string(who) + ": an object asks for up, vp but the pressure fluxes were disarmed since it was added "
                                "(roms_gpu_pflx_begin)";
    return -4;
  }
  const Bounds& b = S.d->b;
  const size_t n = (size_t)(b.n2 + kRowAlign) * sizeof(double);
  const long lead = ((uintptr_t)S.d->f.u / sizeof(double)) % kRowAlign;   // the alignment of the model's fields
  if (!E.upe_base) {
    if (hipMalloc(&E.upe_base, n) != hipSuccess || hipMalloc(&E.vpe_base, n) != hipSuccess ||
        hipMemsetAsync(E.upe_base, 0, n, S.s) != hipSuccess || hipMemsetAsync(E.vpe_base, 0, n, S.s) != hipSuccess) {
      *S.err = std::string(who) + ": allocation of upe, vpe failed";
      return -2;
    }
    E.upe = E.upe_base + lead;
    E.vpe = E.vpe_base + lead;
  }
  if (hipMemcpyAsync(E.upe, pf.up, (size_t)b.n2 * sizeof(double), hipMemcpyDeviceToDevice, S.s) != hipSuccess ||
      hipMemcpyAsync(E.vpe, pf.vp, (size_t)b.n2 * sizeof(double), hipMemcpyDeviceToDevice, S.s) != hipSuccess) {
    *S.err = std::string(who) + ": copy of up, vp failed";
    return -2;
  }
  launch_exchange_list(*S.d, S.s, ExchList{{E.upe, E.vpe}, {1, 1}, 2});
  return 0;
}
void ext_launch_remap(const ShimState& S) {
  hipLaunchKernelGGL(k_ext_remap, dim3((E.NP + 63) / 64), dim3(64, 4), 0, S.s, E.a);
}

// the checks of a sample, the tables, and the halo of Hz_u / Hz_v: set_HUV
// stores them on its own range only, the points next to a rank's edge read
// one cell further.  Every rank of a decomposed run takes part.
int ext_prepare(const ShimState& S, const roms_tlev* t, const char* who) {
  if (!E.begun || E.obj.empty()) { *S.err = std::string(who) + ": extraction is not armed (roms_gpu_extract_begin, _add_object)"; return -4; }
  if (!ext_tlev_ok(t)) { *S.err = std::string(who) + ": bad time levels"; return -1; }
  if (ext_need_huv() && !shim_hzuv_valid()) {
    *S.err = std::string(who) + ": Hz_u/Hz_v are stale: armed after a whole step that did not store them; take a step "
                                "or call roms_gpu_set_huv first";
    return -4;
  }
  if (ext_build(S)) { *S.err = std::string(who) + ": allocation of the extraction buffers failed"; return -2; }
  ext_slots(S, *t);
  if (ext_need_huv()) launch_exchange_list(*S.d, S.s, ExchList{{S.d->f.Hz_u, S.d->f.Hz_v}, {S.d->b.N, S.d->b.N}, 2});
  if (ext_union() & kExtPflx) return ext_pflx_planes(S, who);
  return 0;
}
int ext_sample(const ShimState& S) {
  if (E.NP > 0) {
    ext_launch_interp(S);
    if (ext_union() & kExtPflx) ext_launch_pflx(S);
    if (E.mismatch && (ext_union() & kExt3d)) ext_launch_remap(S);
  }
  E.sampled = true;
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

struct ExtOut { const double* p; int rows; };
// where variable `bit` of an object lies after a sample: rows of np at pitch NP
ExtOut ext_out(const ExtObject& o, int bit) {
  const ExtArgs& a = E.a;
  if (bit == ROMS_EXT_ZETA) return {a.o2[0] + o.p0, 1};
  if (bit == ROMS_EXT_UBAR) return {a.o2[1] + o.p0, 1};
  if (bit == ROMS_EXT_VBAR) return {a.o2[2] + o.p0, 1};
  if (bit == ROMS_EXT_UP) return {E.oup + o.p0, 1};
  if (bit == ROMS_EXT_VP) return {E.ovp + o.p0, 1};
  const int v = bit == ROMS_EXT_U ? 0 : bit == ROMS_EXT_V ? 1 : bit == ROMS_EXT_TEMP ? 2 : 3;
  if (E.mismatch) return {a.outc[v] + o.p0, E.Nc};
  return {a.prof[v] + o.p0, a.N};
}

const int kExtOrder[9] = {ROMS_EXT_ZETA, ROMS_EXT_UBAR, ROMS_EXT_VBAR, ROMS_EXT_TEMP, ROMS_EXT_SALT, ROMS_EXT_U, ROMS_EXT_V,
                          ROMS_EXT_UP, ROMS_EXT_VP};   // create_edata_vars
const char* ext_vname(int bit) {
  switch (bit) {
    case ROMS_EXT_ZETA: return "zeta"; case ROMS_EXT_UBAR: return "ubar"; case ROMS_EXT_VBAR: return "vbar";
    case ROMS_EXT_U: return "u"; case ROMS_EXT_V: return "v"; case ROMS_EXT_TEMP: return "temp";
    case ROMS_EXT_UP: return "up"; case ROMS_EXT_VP: return "vp"; default: return "salt";
  }
}
void ext_meta(int bit, std::string& ln, std::string& un) {   // the history table's long_name and units
  switch (bit) {
    case ROMS_EXT_ZETA: ln = "free-surface elevation"; un = "meter"; break;
    case ROMS_EXT_UBAR: ln = "vertically averaged u-momentum component"; un = "meter second-1"; break;
    case ROMS_EXT_VBAR: ln = "vertically averaged v-momentum component"; un = "meter second-1"; break;
    case ROMS_EXT_U: ln = "u-momentum component"; un = "meter second-1"; break;
    case ROMS_EXT_V: ln = "v-momentum component"; un = "meter second-1"; break;
    case ROMS_EXT_TEMP: ln = "potential temperature"; un = "Celsius"; break;
    case ROMS_EXT_UP: case ROMS_EXT_VP: ln = "pressure flux"; un = "W/m^2"; break;   // create_var without an index (:954-957)
    default: ln = "salinity"; un = "PSU"; break;
  }
}

std::string ext_unsupported_names(int m) {
  std::string s;
  const char* nm[4] = {"up", "vp", "w", "bgc"};
  const int bit[4] = {ROMS_EXT_UP, ROMS_EXT_VP, ROMS_EXT_W, ROMS_EXT_BGC};
  for (int q = 0; q < 4; q++)
    if (m & bit[q]) s += std::string(s.empty() ? "" : ", ") + nm[q];
  return s;
}

// one object: the checks, the local range, the coefficients.  Nothing is
// changed when it refuses.
int ext_add(const ShimState& S, const char* name, const char* dname, long npg, const double* ipos, const double* jpos,
            const double* ang, const char* output_vars) {
  const Bounds& b = S.d->b;
  if (!E.begun) { *S.err = "roms_gpu_extract_add_object: call roms_gpu_extract_begin first"; return -4; }
  if (!name || !*name || !ipos || !jpos || !output_vars || npg < 1 || npg > 2147483647L) {
    *S.err = "roms_gpu_extract_add_object: bad name/positions/output_vars";
    return -1;
  }
  ExtObject o;
  o.name = name;
  o.dname = dname ? dname : "";
  o.dsize = (int)npg;
  o.scalar = ang == nullptr;
  // set, bnd: 'grid1_west_r' -> 'grid1', '_west'
  const size_t u1 = o.name.find('_');
  if (u1 == std::string::npos) o.set = o.name;
  else {
    o.set = o.name.substr(0, u1);
    const size_t u2 = o.name.find('_', u1 + 1);
    o.bnd = u2 == std::string::npos ? "" : o.name.substr(u1, u2 - u1);
  }
  const std::string ov(output_vars);
  int f = 0;
  if (ext_find(ov, "zeta")) f |= ROMS_EXT_ZETA;
  if (ext_find(ov, "temp")) f |= ROMS_EXT_TEMP;
  if (ext_find(ov, "salt")) f |= ROMS_EXT_SALT;
  if (ext_find(ov, "ubar")) f |= ROMS_EXT_UBAR;
  if (ext_find(ov, "vbar")) f |= ROMS_EXT_VBAR;
  if (ext_find(ov, "u")) f |= ROMS_EXT_U;      // also inside 'ubar' and 'up', as findstr finds it
  if (ext_find(ov, "v")) f |= ROMS_EXT_V;
  if (ext_find(ov, "w")) f |= ROMS_EXT_W;
  if (ext_find(ov, "up")) f |= ROMS_EXT_UP;
  if (ext_find(ov, "vp")) f |= ROMS_EXT_VP;
  if (ext_find(ov, "bgc")) f |= ROMS_EXT_BGC;
  if (!S.cfg->salinity || b.NT < 2) f &= ~ROMS_EXT_SALT;   // #ifdef SALINITY
  // up, vp are produced for an object added while the pressure fluxes are armed (roms_gpu_pflx_begin); otherwise
  // they stay unsupported, as the reference refuses them without calc_pflx
  const int can = kExtSupported | (pflx_view().armed ? kExtPflx : 0);
  o.vars = f & can;
  o.unsupported = f & ~can;
  if (o.scalar && (o.vars & kExtVector)) {
    *S.err = "roms_gpu_extract_add_object: " + o.name + " asks for a vector variable (ubar, vbar, u, v, up, vp) but is a scalar "
             "object (no angle column)";
    return -1;
  }
  if (E.mismatch && (o.vars & kExt3d) && b.N < 5) {
    *S.err = "roms_gpu_extract_add_object: the vertical remap needs N >= 5 (calc_interface_values reads five layers)";
    return -1;
  }
  if (ext_masks(S)) { *S.err = "roms_gpu_extract_add_object: download of the masks failed"; return -2; }
  const int nx = b.Lm, ny = b.Mm, isw = S.dims->iSW_corn, jsw = S.dims->jSW_corn, w = b.Lm + 4;
  ext_locate(nx, ny, isw, jsw, npg, ipos, jpos, &o.start_idx, &o.np);
  if (o.np > 0) {
    std::vector<double> ip(o.np), jp(o.np);
    for (int q = 0; q < o.np; q++) {
      ip[q] = (ipos[o.start_idx - 1 + q] - (double)isw) + 0.5;   // absolute index -> rho index
      jp[q] = (jpos[o.start_idx - 1 + q] - (double)jsw) + 0.5;
    }
    ext_coef(ip, jp, E.rmask, w, o.ip[0], o.jp[0], o.cf[0]);
    if (!o.scalar) {
      o.ang.assign(ang + (o.start_idx - 1), ang + (o.start_idx - 1) + o.np);
      o.cosa.resize(o.np); o.sina.resize(o.np);
      for (int q = 0; q < o.np; q++) {
        const size_t c = (size_t)(o.jp[0][q] + 1) * w + (o.ip[0][q] + 1);
        const double angp = E.angler[c] * o.cf[0][q] + E.angler[c + 1] * o.cf[0][o.np + q] +
                            E.angler[c + w] * o.cf[0][2 * o.np + q] + E.angler[c + w + 1] * o.cf[0][3 * o.np + q];
        o.cosa[q] = std::cos(angp - o.ang[q]);
        o.sina[q] = std::sin(angp - o.ang[q]);
      }
      for (int q = 0; q < o.np; q++) ip[q] = ip[q] + 0.5;   // rho index -> u index
      ext_coef(ip, jp, E.umask, w, o.ip[1], o.jp[1], o.cf[1]);
      for (int q = 0; q < o.np; q++) { ip[q] = ip[q] - 0.5; jp[q] = jp[q] + 0.5; }   // u index -> v index
      ext_coef(ip, jp, E.vmask, w, o.ip[2], o.jp[2], o.cf[2]);
    }
  }
  E.obj.push_back(std::move(o));
  E.built = E.sampled = false;
  shim_extract_huv(ext_need_huv());
  const ExtObject& added = E.obj.back();
  if (added.unsupported)   // reported, not fatal: the reference's sample script asks for up, vp by default
    shim_set_error("roms_gpu_extract_add_object: " + added.name + ": not produced here: " + ext_unsupported_names(added.unsupported));
  return 0;
}

ExtObject* ext_obj(int iobj) { return iobj >= 1 && iobj <= (int)E.obj.size() ? &E.obj[iobj - 1] : nullptr; }

}  // namespace

void extract_free() { ext_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_extract_locate(int nx, int ny, int iSW_corn, int jSW_corn, long npg, const double* ipos, const double* jpos,
                            int* start_idx, int* np) {
  if (nx < 1 || ny < 1 || npg < 0 || (npg && (!ipos || !jpos)) || !start_idx || !np) return -1;
  ext_locate(nx, ny, iSW_corn, jSW_corn, npg, ipos, jpos, start_idx, np);
  return 0;
}

int roms_gpu_extract_begin(int N_chd, double theta_s_chd, double theta_b_chd, double hc_chd) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (hipStreamSynchronize(S.s) != hipSuccess) { *S.err = "roms_gpu_extract_begin: stream synchronisation failed"; return -2; }
  if (N_chd < 1 || !(theta_s_chd == theta_s_chd) || !(theta_b_chd == theta_b_chd) || !(hc_chd == hc_chd)) {
    *S.err = "roms_gpu_extract_begin: N_chd must be >= 1 and the child's S-coordinate parameters numbers";
    return -1;
  }
  std::string err;
  if ((r = io_writer_join(err))) { *S.err = err; return r; }
  ext_release();
  E.begun = true;
  E.Nc = N_chd;
  E.theta_s = theta_s_chd; E.theta_b = theta_b_chd; E.hc = hc_chd;
  const roms_cfg& C = *S.cfg;
  E.mismatch = !(S.d->b.N == N_chd && C.theta_s == theta_s_chd && C.theta_b == theta_b_chd && C.hc == hc_chd);
  // set_chd_scoord
  E.csw.assign(N_chd + 1, 0.0);
  const double ds = 1.0 / (double)N_chd;
  for (int k = N_chd - 1; k >= 1; k--) E.csw[k] = ext_calc_cs(ds * (double)(k - N_chd), theta_s_chd, theta_b_chd);
  E.csw[0] = -1.0;
  return 0;
}

int roms_gpu_extract_angler(const double* angler, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!E.begun) { *S.err = "roms_gpu_extract_angler: call roms_gpu_extract_begin first"; return -4; }
  const long n = (long)(S.d->b.Mm + 4) * (S.d->b.Lm + 4);
  if (!angler || count != n) { *S.err = "roms_gpu_extract_angler: count is not (Mm+4)*(Lm+4)"; return -1; }
  if (!E.obj.empty()) { *S.err = "roms_gpu_extract_angler: set the angle before the first object"; return -4; }
  E.angler.assign(angler, angler + n);
  return 0;
}

int roms_gpu_extract_add_object(const char* name, const char* dname, long np_global, const double* ipos, const double* jpos,
                                const double* ang, const char* output_vars) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  return ext_add(S, name, dname, np_global, ipos, jpos, ang, output_vars);
}

int roms_gpu_extract_objects_file(const char* path) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!E.begun) { *S.err = "roms_gpu_extract_objects_file: call roms_gpu_extract_begin first"; return -4; }
  if (!path) { *S.err = "roms_gpu_extract_objects_file: no path"; return -1; }
  struct Rd { std::string name, dname, ov; long n1; int n2; std::vector<double> data; };
  std::vector<Rd> all;
  try {
    nc::File f;
    f.open(path, false);
    for (size_t q = 0; q < f.vars.size(); q++) {
      const nc::Var& v = f.vars[q];
      if (v.dims.size() != 2 || v.type != nc::NC_DOUBLE || v.is_rec) throw std::runtime_error("object " + v.name + " is not a fixed double (2|3, np) variable");
      Rd o;
      o.name = v.name;
      o.n2 = (int)f.dims[v.dims[0]].len;
      o.n1 = (long)f.dims[v.dims[1]].len;   // the fastest dimension: the points
      o.dname = f.dims[v.dims[1]].name;
      if ((o.n2 != 2 && o.n2 != 3) || o.n1 < 1) throw std::runtime_error("object " + v.name + " must have 2 or 3 columns");
      bool have = false;
      for (const nc::Att& at : v.atts)
        if (at.name == "output_vars" && at.type == nc::NC_CHAR) { o.ov = at.text; have = true; }
      if (!have) throw std::runtime_error("object " + v.name + " has no output_vars attribute");
      o.data.resize((size_t)o.n1 * o.n2);
      f.get_double((int)q, 0, o.data.data());
      all.push_back(std::move(o));
    }
    f.close();
  } catch (const std::exception& e) {
    *S.err = std::string("roms_gpu_extract_objects_file: ") + path + ": " + e.what();
    return -7;
  }
  // all objects or none: a refused one takes back those added before it
  const size_t n0 = E.obj.size();
  for (const Rd& o : all) {
    r = ext_add(S, o.name.c_str(), o.dname.c_str(), o.n1, o.data.data(), o.data.data() + o.n1,
                o.n2 == 3 ? o.data.data() + 2 * o.n1 : nullptr, o.ov.c_str());
    if (r) {
      E.obj.resize(n0);
      E.built = E.sampled = false;
      shim_extract_huv(ext_need_huv());
      return r;
    }
  }
  std::string skipped;   // every object's variables that are asked for and not produced, in one message
  for (size_t q = n0; q < E.obj.size(); q++)
    if (E.obj[q].unsupported)
      skipped += std::string(skipped.empty() ? "" : "; ") + E.obj[q].name + ": " + ext_unsupported_names(E.obj[q].unsupported);
  if (!skipped.empty()) *S.err = "roms_gpu_extract_objects_file: not produced here: " + skipped;
  return 0;
}

int roms_gpu_calc_extract(const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if ((r = ext_prepare(S, t, "roms_gpu_calc_extract"))) return r;
  if ((r = ext_sample(S))) { *S.err = "roms_gpu_calc_extract: launch failed"; return r; }
  return 0;
}

int roms_gpu_wrt_extract(const char* path, int rec, int total_rec, double time, const roms_tlev* t) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  (void)total_rec;   // the reference's extraction file has no time_step variable
  if (!E.begun || E.obj.empty()) { *S.err = "roms_gpu_wrt_extract: extraction is not armed (roms_gpu_extract_begin, _add_object)"; return -4; }
  if (!path || rec < 1) { *S.err = "roms_gpu_wrt_extract: bad path/record"; return -1; }
  std::string err;
  if ((r = io_writer_join(err))) { *S.err = err; return r; }   // the packed buffer is the writer's until it has landed
  if ((r = ext_prepare(S, t, "roms_gpu_wrt_extract"))) return r;
  if ((r = ext_sample(S))) { *S.err = "roms_gpu_wrt_extract: launch failed"; return r; }
  ExtRecord R;
  R.time_dim = "time_" + E.obj[0].set;
  R.s_rho = 0;
  size_t n = 0;
  std::vector<ExtOut> src;
  std::vector<int> np_of;
  for (size_t q = 0; q < E.obj.size(); q++) {
    const ExtObject& o = E.obj[q];
    if (o.np <= 0) continue;
    char lab[16];
    snprintf(lab, sizeof lab, "np%03d", (int)q + 1);
    R.dims.push_back({lab, o.np});
    const std::string tv = o.set + "_time";
    bool seen = false;
    for (const std::string& s : R.time_vars) seen = seen || s == tv;
    if (!seen) R.time_vars.push_back(tv);
    for (int bit : kExtOrder) {
      if (!(o.vars & bit)) continue;
      const ExtOut x = ext_out(o, bit);
      ExtFileVar v;
      v.name = o.set + "_" + ext_vname(bit) + o.bnd;
      v.dim_np = (int)R.dims.size() - 1;
      v.levels = (bit & kExt3d) != 0;
      if (v.levels) R.s_rho = E.Nc;   // N_chd; equal to N without a mismatch
      v.start = o.start_idx; v.count = o.np; v.dsize = o.dsize; v.dname = o.dname;
      ext_meta(bit, v.lname, v.units);
      v.off = (long)n; v.n = (long)x.rows * o.np;
      n += (size_t)v.n;
      R.vars.push_back(v);
      src.push_back(x);
      np_of.push_back(o.np);
    }
  }
  if (E.pack_n < n) {
    if (E.pack) (void)hipFree(E.pack);
    E.pack = nullptr;
    E.pack_n = 0;
    if (hipMalloc(&E.pack, n * sizeof(double)) != hipSuccess) { *S.err = "roms_gpu_wrt_extract: staging allocation failed"; return -2; }
    E.pack_n = n;
  }
  for (size_t q = 0; q < src.size(); q++) {
    const size_t wb = (size_t)np_of[q] * sizeof(double);
    if (hipMemcpy2DAsync(E.pack + R.vars[q].off, wb, src[q].p, (size_t)E.NP * sizeof(double), wb, (size_t)src[q].rows,
                         hipMemcpyDeviceToDevice, S.s) != hipSuccess) {
      *S.err = "roms_gpu_wrt_extract: packing failed";
      return -2;
    }
  }
  R.dev = E.pack;
  R.n = n;
  return extract_write(path, rec, time, R);
}

int roms_gpu_extract_state(int* nobj, int* mismatch, int* N_chd, int* np_total, int* need_huv) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  int np = 0;
  for (const ExtObject& o : E.obj) np += o.np;
  if (nobj) *nobj = (int)E.obj.size();
  if (mismatch) *mismatch = E.begun && E.mismatch ? 1 : 0;
  if (N_chd) *N_chd = E.Nc;
  if (np_total) *np_total = np;
  if (need_huv) *need_huv = ext_need_huv() ? 1 : 0;
  return 0;
}

int roms_gpu_extract_object_info(int iobj, int* np, int* start_idx, int* vars, int* unsupported, int* scalar) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const ExtObject* o = ext_obj(iobj);
  if (!o) { *S.err = "roms_gpu_extract_object_info: no such object"; return -1; }
  if (np) *np = o->np;
  if (start_idx) *start_idx = o->start_idx;
  if (vars) *vars = o->vars;
  if (unsupported) *unsupported = o->unsupported;
  if (scalar) *scalar = o->scalar ? 1 : 0;
  return 0;
}

int roms_gpu_extract_object_coef(int iobj, int grid, int* ip, int* jp, double* coef, double* cosa, double* sina) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const ExtObject* o = ext_obj(iobj);
  if (!o || grid < 0 || grid > 2) { *S.err = "roms_gpu_extract_object_coef: no such object or grid type (0 rho, 1 u, 2 v)"; return -1; }
  if (grid > 0 && o->scalar) { *S.err = "roms_gpu_extract_object_coef: a scalar object has rho coefficients only"; return -1; }
  for (int q = 0; q < o->np; q++) {
    if (ip) ip[q] = o->ip[grid][q];
    if (jp) jp[q] = o->jp[grid][q];
    if (cosa) cosa[q] = o->scalar ? 1.0 : o->cosa[q];
    if (sina) sina[q] = o->scalar ? 0.0 : o->sina[q];
  }
  if (coef)
    for (size_t q = 0; q < o->cf[grid].size(); q++) coef[q] = o->cf[grid][q];
  return 0;
}

int roms_gpu_extract_child_cs(double* cs_w) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (!E.begun || !cs_w) { *S.err = "roms_gpu_extract_child_cs: call roms_gpu_extract_begin first"; return -4; }
  for (int k = 0; k <= E.Nc; k++) cs_w[k] = E.csw[k];
  return 0;
}

int roms_gpu_extract_copy_out(int iobj, int var_bit, double* dst, long count) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const ExtObject* o = ext_obj(iobj);
  if (!o) { *S.err = "roms_gpu_extract_copy_out: no such object"; return -1; }
  if (!(var_bit & (kExtSupported | kExtPflx)) || (var_bit & (var_bit - 1))) { *S.err = "roms_gpu_extract_copy_out: var_bit must be one ROMS_EXT_* bit"; return -1; }
  if (!(o->vars & var_bit) || !dst) { *S.err = "roms_gpu_extract_copy_out: that variable is not extracted for this object"; return -4; }
  if (!E.sampled || !E.built) { *S.err = "roms_gpu_extract_copy_out: no sample yet (roms_gpu_calc_extract)"; return -4; }
  const int rows = (var_bit & kExt3d) ? (E.mismatch ? E.Nc : S.d->b.N) : 1;
  if (count != (long)rows * o->np) { *S.err = "roms_gpu_extract_copy_out: count is not levels*np"; return -1; }
  if (o->np == 0) return 0;
  const ExtOut x = ext_out(*o, var_bit);
  const size_t wb = (size_t)o->np * sizeof(double);
  if (hipMemcpy2DAsync(dst, wb, x.p, (size_t)E.NP * sizeof(double), wb, (size_t)rows, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
      hipStreamSynchronize(S.s) != hipSuccess) {
    *S.err = "roms_gpu_extract_copy_out: copy failed";
    return -2;
  }
  return 0;
}

// n launches of the interpolation, then n of the remap, each between two
// events of its own on the library stream: ms[0], ms[1] their totals (tools/extract_cost.py)
int roms_gpu_time_calc_extract(int n, const roms_tlev* t, double* ms) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  if (n < 1 || !ms) { *S.err = "roms_gpu_time_calc_extract: bad arguments"; return -1; }
  if ((r = ext_prepare(S, t, "roms_gpu_time_calc_extract"))) return r;
  if ((r = ext_sample(S))) { *S.err = "roms_gpu_time_calc_extract: launch failed"; return r; }
  const bool remap = E.NP > 0 && E.mismatch && (ext_union() & kExt3d);
  ms[0] = time_rounds(S.s, n, false, [&]() { if (E.NP > 0) ext_launch_interp(S); return 0; });
  ms[1] = ms[0] < 0 ? 0.0 : time_rounds(S.s, n, false, [&]() { if (remap) ext_launch_remap(S); return 0; });
  if (ms[0] < 0 || ms[1] < 0) {
    *S.err = "roms_gpu_time_calc_extract: launch or timing failed";
    return (int)(ms[0] < 0 ? ms[0] : ms[1]);
  }
  return 0;
}

}  // extern "C"
