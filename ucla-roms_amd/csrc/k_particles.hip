// k_particles.hip -- Lagrangian particles on the device: do_particles of
// particles.F (rhs_particles :475-573, advance_particles :213-267,
// exchange_particles :661-840, sort_particles :902-931) and the _part file
// (wrt_particles / create_particles_file :389-473).
//
// Particles live in the rank's index space [0,nx] x [0,ny] x [0,nz]; the list
// is the reference's part(npmx, npv = 13), column-major, so the 13 words of
// neighbouring particles lie in 13 coalesced columns.  One call is
//   k_part_rhs_adv    one lane per particle: trilinear u, v(nnew), Wp, Hz and
//                     bilinear pm, pn at the particle, the increments, the AB2
//                     advance and the bottom / surface clamp.  All indices are
//                     formed once, the 48 loads are issued ahead of the
//                     arithmetic, and every expression keeps the reference's
//                     order (interp_2D / interp_3D: weights left to right, the
//                     sum in array-element order; -ffp-contract=off).
//   k_part_classify   a destination code per particle (stay, one of eight
//                     neighbours, lost) in exchange_particles' branch order,
//                     and each block's count of every code.
//   k_part_scan       exclusive prefix sums of the block counts, one block per
//                     code; writes the message headers and the counters.
//   k_part_scatter    stable compaction: survivors into the other list buffer
//                     in list order, leavers into their message in list order
//                     (rank within the block from wavefront ballots: no atomic
//                     hands out a slot), nx / ny subtracted going east / north.
//   transport         the rank's Halo (halo_exchange_messages), or nothing on
//                     one rank, where a periodic direction reads its own
//                     message: the wrap.
//   k_part_append     arrivals behind the survivors in the order sw, s, se, w,
//                     e, nw, n, ne, nx / ny added coming from the east / north.
//   with ROMS_PART_SORT: k_part_keys, rocPRIM's stable radix sort of (cell key,
//                     index) pairs, k_part_permute.
// One deviation from the reference: Wp, which rhs_particles interpolates but
// nothing fills (its lines :499-502 are commented out), is formed in the lane
// as ((We + Wi) * pm) * pn from the gathered corners -- what those lines say.
// Where the reference stops (a particle more than half a cell outside, a full
// send buffer) the device counts (n_range, n_overflow), reads nothing out of
// range, and the next call fails with a message.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <string>
#include <vector>

#include "../../include/roms_gpu.h"
#include "halo.h"
#include "roms_dev.h"
#include "shim_state.h"

namespace roms {
namespace {

constexpr int kNpv = 13;         // particles.F:61
constexpr int kPB = 256;         // lanes per block of the per-particle kernels
constexpr int kCodes = 10;       // 0 stay, 1 + HaloDir the eight neighbours, 9 lost
constexpr int kLost = 9;
constexpr double kBigNumber = 10000000.0;   // particles.F:81
// arrivals in the order of exchange_particles :746-838: sw, s, se, w, e, nw, n, ne
__device__ __constant__ int kArrive[8] = {kSW, kS, kSE, kW, kE, kNW, kN, kNE};
constexpr int kOppDir[8] = {kE, kW, kN, kS, kNE, kNW, kSE, kSW};
// counters on the device, read back once per call
enum { cNp = 0, cSur, cBot, cLost, cMoved, cRange, cOver, cStay, cN = 16 };

struct PGeom {
  int nx, ny, nz;
  long npmx;
  int ex[4];      // west, east, south, north_msg_exch (a periodic direction is its own neighbour, mpi_setup.F:65-67)
  int act[8];     // a neighbour exists in HaloDir d
  long cap[8];    // particles a message to / from d holds (init_arrays_mpi_roms :1164-1182)
  long off[8];    // its first word in the send / receive allocation; word 0 is the count
};
struct Msgs {
  double* p[8];
};

__device__ __forceinline__ double interp3(const double f[8], double x, double y, double z) {   // interp_3D :639-659
  const double w0 = (1 - x) * (1 - y) * (1 - z), w1 = x * (1 - y) * (1 - z), w2 = (1 - x) * y * (1 - z), w3 = x * y * (1 - z);
  const double w4 = (1 - x) * (1 - y) * z, w5 = x * (1 - y) * z, w6 = (1 - x) * y * z, w7 = x * y * z;
  return f[0] * w0 + f[1] * w1 + f[2] * w2 + f[3] * w3 + f[4] * w4 + f[5] * w5 + f[6] * w6 + f[7] * w7;
}
__device__ __forceinline__ double interp2(const double f[4], double x, double y) {   // interp_2D :621-637
  const double w0 = (1 - x) * (1 - y), w1 = x * (1 - y), w2 = (1 - x) * y, w3 = x * y;
  return f[0] * w0 + f[1] * w1 + f[2] * w2 + f[3] * w3;
}

// uoff: (nnew-1)*n3; first: the run's first call, dm = d for every particle (:241-246)
__global__ void __launch_bounds__(kPB) k_part_rhs_adv(Dev d, double* __restrict__ part, long npmx, long np, long uoff,
                                                       double dt, int first, unsigned long long* __restrict__ cnt) {
  const long ip = (long)blockIdx.x * kPB + threadIdx.x;
  if (ip >= np) return;
  const Bounds& b = d.b;
  const Fields& F = d.f;
  const int nx = b.Lm, ny = b.Mm, nz = b.N;
  double* __restrict__ P = part + ip;
  double px = P[1 * npmx], py = P[2 * npmx], pz = P[3 * npmx];
  double dxm = P[10 * npmx], dym = P[11 * npmx], dzm = P[12 * npmx];
  double prx = 0.0, pry = 0.0, prz = 0.0;
  if (pz < 2 * nz) {
    // where the reference stops (:524-535) nothing is read: zero increments, counted
    const bool in = px >= -0.5 && px <= nx + 0.5 && py >= -0.5 && py <= ny + 0.5 && pz >= 0.0 && pz <= nz;
    if (!in) {
      atomicAdd(cnt + cRange, 1ull);
    } else {
      const int i = (int)floor(px + 0.5), j = (int)floor(py + 0.5);
      const int k = iclamp((int)floor(pz + 0.5), 1, nz - 1);
      const int iu = (int)floor(px + 1.0), jv = (int)floor(py + 1.0);
      int kw = (int)floor(pz);
      kw = kw > nz - 1 ? nz - 1 : kw;   // pz == nz: Wp(kw+1) would lie outside (0:nz); zw is then 1
      const double x = px - i + 0.5, y = py - j + 0.5, z = pz - k + 0.5;
      const double xu = px - iu + 1.0, yv = py - jv + 1.0, zw = pz - kw;
      const long n2 = b.n2, nxp = b.nx2;
      const long r = IJ(b, i, j), c3 = r + (long)(k - 1) * n2, cw = r + (long)kw * n2;
      const long cu = IJ(b, iu, j) + (long)(k - 1) * n2 + uoff, cv = IJ(b, i, jv) + (long)(k - 1) * n2 + uoff;
      double fu[8], fv[8], fh[8], fe[8], fi[8], fm[4], fn[4];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const long o = (q & 1) + ((q >> 1) & 1) * nxp + (q >> 2) * n2;
        fu[q] = F.u[cu + o];
        fv[q] = F.v[cv + o];
        fh[q] = F.Hz[c3 + o];
        fe[q] = F.We[cw + o];
        fi[q] = F.Wi[cw + o];
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const long o = (q & 1) + (q >> 1) * nxp;
        fm[q] = F.pm[r + o];
        fn[q] = F.pn[r + o];
      }
      double fw[8];
#pragma unroll
      for (int q = 0; q < 8; q++) fw[q] = ((fe[q] + fi[q]) * fm[q & 3]) * fn[q & 3];
      const double pu = interp3(fu, xu, y, z), pv = interp3(fv, x, yv, z), pw = interp3(fw, x, y, zw);
      const double pdxi = interp2(fm, x, y), pdyi = interp2(fn, x, y), pdz = interp3(fh, x, y, z);
      prx = dt * pu * pdxi;
      pry = dt * pv * pdyi;
      prz = dt * pw / pdz;
      P[4 * npmx] = pu; P[5 * npmx] = pv; P[6 * npmx] = pw;
    }
  }
  if (first) { dxm = prx; dym = pry; dzm = prz; }
  px = px + 1.5 * prx - 0.5 * dxm;
  py = py + 1.5 * pry - 0.5 * dym;
  pz = pz + 1.5 * prz - 0.5 * dzm;
  if (pz < 0) { pz = 0.02; atomicAdd(cnt + cBot, 1ull); }
  if (pz > nz) { pz = nz - 0.02; atomicAdd(cnt + cSur, 1ull); }
  P[1 * npmx] = px; P[2 * npmx] = py; P[3 * npmx] = pz;
  P[7 * npmx] = prx; P[8 * npmx] = pry; P[9 * npmx] = prz;
  P[10 * npmx] = prx; P[11 * npmx] = pry; P[12 * npmx] = prz;
}

// exchange_particles :684-732, branch for branch: east before west before north before south; the east branch
// asks for the corner's second neighbour, the west branch does not -- a particle it puts into a corner message
// that is never sent (no such neighbour) is lost, as in the reference
__device__ __forceinline__ int part_code(const PGeom& g, double px, double py, double pz) {
  if (!(pz < g.nz)) return 0;
  int c = 0;
  if (px > g.nx) {
    if (!g.ex[1]) return kLost;
    c = (py > g.ny && g.ex[3]) ? kNE : (py < 0 && g.ex[2]) ? kSE : kE;
  } else if (px < 0.0) {
    if (!g.ex[0]) return kLost;
    c = py > g.ny ? kNW : py < 0 ? kSW : kW;
  } else if (py > g.ny) {
    if (!g.ex[3]) return kLost;
    c = kN;
  } else if (py < 0.0) {
    if (!g.ex[2]) return kLost;
    c = kS;
  } else {
    return 0;
  }
  return g.act[c] ? 1 + c : kLost;
}

__global__ void __launch_bounds__(kPB) k_part_classify(PGeom g, const double* __restrict__ part, long np,
                                                        unsigned char* __restrict__ code, int* __restrict__ bcnt) {
  __shared__ int cnt[kCodes];
  if (threadIdx.x < kCodes) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long ip = (long)blockIdx.x * kPB + threadIdx.x;
  if (ip < np) {
    const int c = part_code(g, part[ip + 1 * g.npmx], part[ip + 2 * g.npmx], part[ip + 3 * g.npmx]);
    code[ip] = (unsigned char)c;
    atomicAdd(&cnt[c], 1);   // a count, not a slot: the order of the adds does not matter
  }
  __syncthreads();
  if (threadIdx.x < kCodes) bcnt[(long)blockIdx.x * kCodes + threadIdx.x] = cnt[threadIdx.x];
}

// one block per code: boff = exclusive prefix sum of bcnt over the blocks; then the code's total into the message
// header and the counters
__global__ void __launch_bounds__(1024) k_part_scan(PGeom g, const int* __restrict__ bcnt, long* __restrict__ boff, long nblk,
                                                     Msgs sb, unsigned long long* __restrict__ cnt) {
  __shared__ long sh[1024];
  const int c = blockIdx.x, t = threadIdx.x;
  long run = 0;
  for (long base = 0; base < nblk; base += 1024) {
    const long q = base + t;
    const long v = q < nblk ? bcnt[q * kCodes + c] : 0;
    sh[t] = v;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
      const long a = t >= s ? sh[t - s] : 0;
      __syncthreads();
      sh[t] += a;
      __syncthreads();
    }
    if (q < nblk) boff[q * kCodes + c] = run + sh[t] - v;
    run += sh[1023];
    __syncthreads();
  }
  if (t == 0) {
    if (c == 0) {
      cnt[cStay] = (unsigned long long)run;
    } else if (c == kLost) {
      cnt[cLost] += (unsigned long long)run;
    } else {
      const int d = c - 1;
      const long kept = run < g.cap[d] ? run : g.cap[d];   // an overflowing message keeps what fits
      sb.p[d][0] = (double)kept;
      atomicAdd(cnt + cMoved, (unsigned long long)kept);   // eight blocks add to these two
      atomicAdd(cnt + cOver, (unsigned long long)(run - kept));
    }
  }
}

__global__ void __launch_bounds__(kPB) k_part_scatter(PGeom g, const double* __restrict__ part, double* __restrict__ out,
                                                       long np, const unsigned char* __restrict__ code,
                                                       const long* __restrict__ boff, Msgs sb) {
  __shared__ int wcnt[kPB / 64][kCodes];
  const long ip = (long)blockIdx.x * kPB + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = ip < np ? (int)code[ip] : -1;
  int rank = 0;
  for (int q = 0; q < kCodes; q++) {
    const unsigned long long m = __ballot(c == q);
    if (c == q) rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w][q] = __popcll(m);
  }
  __syncthreads();
  if (c < 0 || c == kLost) return;
  for (int v = 0; v < w; v++) rank += wcnt[v][c];
  const long dst = boff[(long)blockIdx.x * kCodes + c] + rank;
  const double* __restrict__ P = part + ip;
  if (c == 0) {
#pragma unroll
    for (int v = 0; v < kNpv; v++) out[dst + v * g.npmx] = P[v * g.npmx];
    return;
  }
  const int d = c - 1;
  if (dst >= g.cap[d]) return;   // counted by k_part_scan
  double* __restrict__ m = sb.p[d] + 1 + dst * kNpv;
  const bool east = d == kE || d == kSE || d == kNE, north = d == kN || d == kNW || d == kNE;
#pragma unroll
  for (int v = 0; v < kNpv; v++) {
    double a = P[v * g.npmx];
    if (v == 1 && east) a = a - g.nx;
    if (v == 2 && north) a = a - g.ny;
    m[v] = a;
  }
}

// grid (x, 8): y = place in the arrival order.  rb.p[h]: the message that came from direction h (nullptr: none)
__global__ void __launch_bounds__(kPB) k_part_append(PGeom g, double* __restrict__ out, Msgs rb,
                                                      unsigned long long* __restrict__ cnt) {
  const int q = blockIdx.y;
  long base = (long)cnt[cStay], mine = 0;
  for (int a = 0; a < 8; a++) {
    const int h = kArrive[a];
    long n = rb.p[h] ? (long)rb.p[h][0] : 0;
    n = n < 0 ? 0 : (n > g.cap[h] ? g.cap[h] : n);
    if (a < q) base += n;
    if (a == q) mine = n;
  }
  const int h = kArrive[q];
  const long e = (long)blockIdx.x * kPB + threadIdx.x;
  if (q == 7 && e == 0) {   // the last message's first lane knows the new length
    const long all = base + mine;
    cnt[cNp] = (unsigned long long)(all < g.npmx ? all : g.npmx);
    if (all > g.npmx) atomicAdd(cnt + cOver, (unsigned long long)(all - g.npmx));   // a full list keeps what fits
  }
  if (e >= mine || base + e >= g.npmx) return;
  const double* __restrict__ m = rb.p[h] + 1 + e * kNpv;
  const bool east = h == kE || h == kSE || h == kNE, north = h == kN || h == kNW || h == kNE;
#pragma unroll
  for (int v = 0; v < kNpv; v++) {
    double a = m[v];
    if (v == 1 && east) a = a + g.nx;
    if (v == 2 && north) a = a + g.ny;
    out[base + e + v * g.npmx] = a;
  }
}

// sort_particles :913-917: floor(px) + floor(py)*nx + floor(pz)*nx*ny
__global__ void __launch_bounds__(kPB) k_part_keys(PGeom g, const double* __restrict__ part, long np, long long* __restrict__ key,
                                                    unsigned* __restrict__ idx) {
  const long ip = (long)blockIdx.x * kPB + threadIdx.x;
  if (ip >= np) return;
  const long long fx = (long long)floor(part[ip + 1 * g.npmx]), fy = (long long)floor(part[ip + 2 * g.npmx]),
                  fz = (long long)floor(part[ip + 3 * g.npmx]);
  key[ip] = fx + fy * g.nx + fz * g.ny * g.nx;
  idx[ip] = (unsigned)ip;
}
__global__ void __launch_bounds__(kPB) k_part_permute(long npmx, const double* __restrict__ part, double* __restrict__ out,
                                                       long np, const unsigned* __restrict__ idx) {
  const long ip = (long)blockIdx.x * kPB + threadIdx.x;
  if (ip >= np) return;
  const long s = idx[ip];
#pragma unroll
  for (int v = 0; v < kNpv; v++) out[ip + v * npmx] = part[s + v * npmx];
}

// zlev2kidx :1224-1245 for one depth: the first k with z_w(k+1) >= z, then linear inside the level; into [0, nz]
__global__ void __launch_bounds__(kPB) k_part_add(Dev d, PGeom g, double* __restrict__ part, long np, long n,
                                                   const double* __restrict__ in, int zmode, double tag0) {
  const long q = (long)blockIdx.x * kPB + threadIdx.x;
  if (q >= n) return;
  const double px = in[q], py = in[n + q];
  double pz = in[2 * n + q];
  if (zmode) {
    const int i = iclamp((int)floor(px) + 1, 1, g.nx), j = iclamp((int)floor(py) + 1, 1, g.ny);
    const double* __restrict__ zw = d.f.z_w + IJ(d.b, i, j);
    const long n2 = d.b.n2;
    int k = 0;
    while (k < g.nz - 1 && zw[(k + 1) * n2] < pz) k++;
    pz = (pz - zw[k * n2]) / (zw[(k + 1) * n2] - zw[k * n2]) + k;
    pz = pz < 0.0 ? 0.0 : (pz > g.nz ? (double)g.nz : pz);
  }
  double* __restrict__ P = part + np + q;
  P[0] = tag0 + (double)(q + 1);
  P[1 * g.npmx] = px; P[2 * g.npmx] = py; P[3 * g.npmx] = pz;
#pragma unroll
  for (int v = 4; v < kNpv; v++) P[v * g.npmx] = 0.0;
}

// words 1..7 of the live particles as the record particles(npart, seven): px, py global, rows past np zero
__global__ void __launch_bounds__(kPB) k_part_record(long npmx, const double* __restrict__ part, long np, double sx, double sy,
                                                      double* __restrict__ rec) {
  const long ip = (long)blockIdx.x * kPB + threadIdx.x;
  if (ip >= npmx) return;
#pragma unroll
  for (int v = 0; v < 7; v++) {
    double a = 0.0;
    if (ip < np) {
      a = part[ip + v * npmx];
      if (v == 1) a = a + sx;
      if (v == 2) a = a + sy;
    }
    rec[ip + v * npmx] = a;
  }
}

struct PartCtx {
  bool armed = false;
  int flags = 0;
  PGeom g{};
  double* list[2] = {nullptr, nullptr};
  int cur = 0;
  double *sbuf = nullptr, *rbuf = nullptr;   // the eight messages each way
  long msg_n = 0;
  unsigned char* code = nullptr;
  int* bcnt = nullptr;
  long* boff = nullptr;
  unsigned long long* cnt = nullptr;         // device counters
  unsigned long long* hcnt = nullptr;        // pinned mirror
  double* in = nullptr;                      // part_add's upload
  long in_n = 0;
  double* rec = nullptr;                     // the record of wrt_part (7 x npmx)
  long long* key[2] = {nullptr, nullptr};
  unsigned* idx[2] = {nullptr, nullptr};
  void* tmp = nullptr;
  size_t tmp_n = 0;
  long np = 0, ntag = 0;
  bool first = true;
  unsigned long long c[cN] = {};             // the counters as last read back
};
thread_local PartCtx Pt;

unsigned nblocks(long n) { return (unsigned)((n + kPB - 1) / kPB); }

void part_release() {
  for (double*& p : Pt.list) { if (p) (void)hipFree(p); p = nullptr; }
  for (void* p : {(void*)Pt.sbuf, (void*)Pt.rbuf, (void*)Pt.code, (void*)Pt.bcnt, (void*)Pt.boff, (void*)Pt.cnt, (void*)Pt.in,
                  (void*)Pt.rec, (void*)Pt.key[0], (void*)Pt.key[1], (void*)Pt.idx[0], (void*)Pt.idx[1], Pt.tmp})
    if (p) (void)hipFree(p);
  if (Pt.hcnt) (void)hipHostFree(Pt.hcnt);
  Pt = PartCtx{};
}

Msgs msgs_of(double* base, const PGeom& g, bool all) {
  Msgs m;
  for (int d = 0; d < 8; d++) m.p[d] = (all || g.act[d]) ? base + g.off[d] : nullptr;
  return m;
}

bool enter_armed(ShimState& S, const char* who, int* r) {
  *r = shim_enter(S, true);
  if (*r) return false;
  if (!Pt.armed) {
    *S.err = std::string(who) + ": no particle list (roms_gpu_part_begin)";
    *r = -4;
    return false;
  }
  return true;
}
bool failed_before(const ShimState& S, const char* who) {
  if (!Pt.c[cRange] && !Pt.c[cOver]) return false;
  char b[256];
  snprintf(b, sizeof b, "%s: %llu particles left the range the fields cover and %llu did not fit a message or the list "
           "(roms_gpu_part_state); re-arm with roms_gpu_part_begin", who, Pt.c[cRange], Pt.c[cOver]);
  *S.err = b;
  return true;
}

int read_counters(const ShimState& S, const char* who) {
  if (hipMemcpyAsync(Pt.hcnt, Pt.cnt, cN * sizeof(unsigned long long), hipMemcpyDeviceToHost, S.s) != hipSuccess ||
      hipStreamSynchronize(S.s) != hipSuccess) {
    *S.err = std::string(who) + ": counter read-back failed";
    return -2;
  }
  std::memcpy(Pt.c, Pt.hcnt, sizeof Pt.c);
  Pt.np = (long)Pt.c[cNp];
  return 0;
}

// the rhs and advance kernel alone over the current list
int launch_rhs(const ShimState& S, int nnew, bool first) {
  if (Pt.np > 0)
    hipLaunchKernelGGL(k_part_rhs_adv, dim3(nblocks(Pt.np)), dim3(kPB), 0, S.s, *S.d, Pt.list[Pt.cur], Pt.g.npmx, Pt.np,
                       (long)(nnew - 1) * S.d->b.n3, S.cfg->dt, first ? 1 : 0, Pt.cnt);
  return 0;
}

int do_particles(const ShimState& S, int nnew, const char* who) {
  const PGeom& g = Pt.g;
  const long np = Pt.np, nblk = (np + kPB - 1) / kPB;
  double *a = Pt.list[Pt.cur], *b = Pt.list[1 - Pt.cur];
  const Msgs sb = msgs_of(Pt.sbuf, g, true);
  launch_rhs(S, nnew, Pt.first);
  Pt.first = false;
  if (np > 0) hipLaunchKernelGGL(k_part_classify, dim3(nblocks(np)), dim3(kPB), 0, S.s, g, a, np, Pt.code, Pt.bcnt);
  hipLaunchKernelGGL(k_part_scan, dim3(kCodes), dim3(1024), 0, S.s, g, Pt.bcnt, Pt.boff, nblk, sb, Pt.cnt);
  if (np > 0) hipLaunchKernelGGL(k_part_scatter, dim3(nblocks(np)), dim3(kPB), 0, S.s, g, a, b, np, Pt.code, Pt.boff, sb);
  Msgs rb;
  const Halo* H = S.d->halo;
  if (H && H->comm) {
    MsgSet M;
    for (int d = 0; d < 8; d++) {
      M.sb[d] = Pt.sbuf + g.off[d];
      M.rb[d] = Pt.rbuf + g.off[d];
      M.len[d] = g.act[d] ? 1 + g.cap[d] * kNpv : 0;
    }
    const int r = halo_exchange_messages(*H, S.s, M);
    if (r) { *S.err = std::string(who) + ": the particle messages could not be exchanged"; return r; }
    rb = msgs_of(Pt.rbuf, g, false);
  } else {
    // one rank: a periodic direction is its own neighbour, what left to the east arrives from the west
    for (int h = 0; h < 8; h++) rb.p[h] = g.act[h] ? Pt.sbuf + g.off[kOppDir[h]] : nullptr;
  }
  long mx = 1;
  for (int d = 0; d < 8; d++) mx = g.act[d] && g.cap[d] > mx ? g.cap[d] : mx;
  hipLaunchKernelGGL(k_part_append, dim3(nblocks(mx), 8), dim3(kPB), 0, S.s, g, b, rb, Pt.cnt);
  if (hipGetLastError() != hipSuccess) { *S.err = std::string(who) + ": launch failed"; return -3; }
  Pt.cur = 1 - Pt.cur;
  int r = read_counters(S, who);
  if (r) return r;
  if ((Pt.flags & ROMS_PART_SORT) && Pt.np > 1) {
    const long n = Pt.np;
    hipLaunchKernelGGL(k_part_keys, dim3(nblocks(n)), dim3(kPB), 0, S.s, g, Pt.list[Pt.cur], n, Pt.key[0], Pt.idx[0]);
    size_t bytes = Pt.tmp_n;
    if (rocprim::radix_sort_pairs(Pt.tmp, bytes, Pt.key[0], Pt.key[1], Pt.idx[0], Pt.idx[1], (size_t)n, 0, 64, S.s) !=
        hipSuccess) {
      *S.err = std::string(who) + ": sort failed";
      return -3;
    }
    hipLaunchKernelGGL(k_part_permute, dim3(nblocks(n)), dim3(kPB), 0, S.s, g.npmx, Pt.list[Pt.cur], Pt.list[1 - Pt.cur], n,
                       Pt.idx[1]);
    if (hipGetLastError() != hipSuccess) { *S.err = std::string(who) + ": launch failed"; return -3; }
    Pt.cur = 1 - Pt.cur;
  }
  return 0;
}

bool tlev_ok(const roms_tlev* t) { return t && t->nnew >= 1 && t->nnew <= 3; }

}  // namespace

void part_free() { part_release(); }

}  // namespace roms

using namespace roms;

extern "C" {

int roms_gpu_part_begin(long npmx, double fac_x, double fac_y, double fac_c, int flags) {
  ShimState S;
  int r = shim_enter(S, true);
  if (r) return r;
  const Bounds& b = S.d->b;
  if (npmx < 1 || npmx > 2000000000L || fac_x < 0 || fac_y < 0 || fac_c < 0 || fac_x > 1 || fac_y > 1 || fac_c > 1 ||
      (flags & ~ROMS_PART_SORT)) {
    *S.err = "roms_gpu_part_begin: npmx must be 1..2e9, the factors 0..1 and flags 0 or ROMS_PART_SORT";
    return -1;
  }
  if (b.N < 2) { *S.err = "roms_gpu_part_begin: N < 2 leaves no pair of rho levels to interpolate between"; return -1; }
  if ((r = io_writer_join(*S.err))) return r;   // a record of the old list may still be on its way to the host
  (void)hipStreamSynchronize(S.s);
  part_release();
  PGeom& g = Pt.g;
  g.nx = b.Lm; g.ny = b.Mm; g.nz = b.N; g.npmx = npmx;
  g.ex[0] = b.ew_periodic || b.west_exch; g.ex[1] = b.ew_periodic || b.east_exch;
  g.ex[2] = b.ns_periodic || b.south_exch; g.ex[3] = b.ns_periodic || b.north_exch;
  const int act[8] = {g.ex[0], g.ex[1], g.ex[2], g.ex[3], g.ex[2] && g.ex[0], g.ex[2] && g.ex[1], g.ex[3] && g.ex[0],
                      g.ex[3] && g.ex[1]};
  // init_arrays_mpi_roms :1170-1172 with particles.opt's factors for 0
  const double fx = fac_x > 0 ? fac_x : 0.1, fy = fac_y > 0 ? fac_y : 0.1, fc = fac_c > 0 ? fac_c : 0.01;
  const long szx = (long)(fx * (double)npmx * kNpv), szy = (long)(fy * (double)npmx * kNpv), szc = (long)(fc * (double)npmx * kNpv);
  long off = 0;
  for (int d = 0; d < 8; d++) {
    g.act[d] = act[d];
    g.cap[d] = (d < 2 ? szy : d < 4 ? szx : szc) / kNpv;
    g.off[d] = off;
    off += 1 + g.cap[d] * kNpv;
  }
  Pt.msg_n = off;
  Pt.flags = flags;
  const long nblk = (npmx + kPB - 1) / kPB;
  const size_t lb = (size_t)npmx * kNpv * sizeof(double);
  bool ok = hipMalloc(&Pt.list[0], lb) == hipSuccess && hipMalloc(&Pt.list[1], lb) == hipSuccess &&
            hipMalloc(&Pt.sbuf, (size_t)off * sizeof(double)) == hipSuccess &&
            hipMalloc(&Pt.rbuf, (size_t)off * sizeof(double)) == hipSuccess && hipMalloc(&Pt.code, (size_t)npmx) == hipSuccess &&
            hipMalloc(&Pt.bcnt, (size_t)nblk * kCodes * sizeof(int)) == hipSuccess &&
            hipMalloc(&Pt.boff, (size_t)nblk * kCodes * sizeof(long)) == hipSuccess &&
            hipMalloc(&Pt.cnt, cN * sizeof(unsigned long long)) == hipSuccess &&
            hipMalloc(&Pt.rec, (size_t)npmx * 7 * sizeof(double)) == hipSuccess &&
            hipHostMalloc((void**)&Pt.hcnt, cN * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess;
  if (ok && (flags & ROMS_PART_SORT)) {
    for (int q = 0; q < 2 && ok; q++)
      ok = hipMalloc(&Pt.key[q], (size_t)npmx * sizeof(long long)) == hipSuccess &&
           hipMalloc(&Pt.idx[q], (size_t)npmx * sizeof(unsigned)) == hipSuccess;
    size_t bytes = 0;
    ok = ok && rocprim::radix_sort_pairs(nullptr, bytes, Pt.key[0], Pt.key[1], Pt.idx[0], Pt.idx[1], (size_t)npmx, 0, 64,
                                         S.s) == hipSuccess;
    ok = ok && hipMalloc(&Pt.tmp, bytes < 8 ? 8 : bytes) == hipSuccess;
    Pt.tmp_n = bytes;
  }
  ok = ok && hipMemsetAsync(Pt.cnt, 0, cN * sizeof(unsigned long long), S.s) == hipSuccess &&
       hipMemsetAsync(Pt.sbuf, 0, (size_t)off * sizeof(double), S.s) == hipSuccess &&
       hipMemsetAsync(Pt.rbuf, 0, (size_t)off * sizeof(double), S.s) == hipSuccess && hipStreamSynchronize(S.s) == hipSuccess;
  if (!ok) {
    part_release();
    *S.err = "roms_gpu_part_begin: allocation failed";
    return -2;
  }
  Pt.armed = true;
  return 0;
}

int roms_gpu_part_add(long n, const double* px, const double* py, const double* pz, int zmode) {
  ShimState S;
  int r;
  if (!enter_armed(S, "roms_gpu_part_add", &r)) return r;
  const PGeom& g = Pt.g;
  if (n < 0 || (n > 0 && (!px || !py || !pz)) || (zmode != 0 && zmode != 1)) {
    *S.err = "roms_gpu_part_add: bad arguments";
    return -1;
  }
  if (Pt.np + n > g.npmx) { *S.err = "roms_gpu_part_add: the list would exceed npmx"; return -1; }
  for (long q = 0; q < n; q++)
    if (!(px[q] >= 0 && px[q] <= g.nx && py[q] >= 0 && py[q] <= g.ny) || (zmode == 0 && !(pz[q] >= 0 && pz[q] <= g.nz)) ||
        (zmode == 1 && pz[q] != pz[q])) {
      *S.err = "roms_gpu_part_add: a position lies outside [0,nx] x [0,ny] x [0,nz]";
      return -1;
    }
  if (n == 0) return 0;
  if (Pt.in_n < 3 * n) {
    if (Pt.in) { (void)hipStreamSynchronize(S.s); (void)hipFree(Pt.in); }
    Pt.in = nullptr;
    Pt.in_n = 0;
    if (hipMalloc(&Pt.in, (size_t)3 * n * sizeof(double)) != hipSuccess) { *S.err = "roms_gpu_part_add: allocation failed"; return -2; }
    Pt.in_n = 3 * n;
  }
  const size_t nb = (size_t)n * sizeof(double);
  if (copy_on(Pt.in, px, nb, hipMemcpyHostToDevice, S.s) != hipSuccess ||
      copy_on(Pt.in + n, py, nb, hipMemcpyHostToDevice, S.s) != hipSuccess ||
      copy_on(Pt.in + 2 * n, pz, nb, hipMemcpyHostToDevice, S.s) != hipSuccess) {
    *S.err = "roms_gpu_part_add: upload failed";
    return -2;
  }
  // tags ip + big_number*mynode, going on from ntag (:179-185, :347-354)
  const int mynode = S.dims->inode + S.dims->jnode * S.dims->np_xi;
  hipLaunchKernelGGL(k_part_add, dim3(nblocks(n)), dim3(kPB), 0, S.s, *S.d, g, Pt.list[Pt.cur], Pt.np, n, Pt.in, zmode,
                     (double)Pt.ntag + kBigNumber * mynode);
  Pt.np += n;
  Pt.ntag += n;
  Pt.c[cNp] = (unsigned long long)Pt.np;
  const unsigned long long v = (unsigned long long)Pt.np;
  if (hipGetLastError() != hipSuccess || copy_on(Pt.cnt + cNp, &v, sizeof v, hipMemcpyHostToDevice, S.s) != hipSuccess) {
    *S.err = "roms_gpu_part_add: launch failed";
    return -3;
  }
  return 0;
}

int roms_gpu_do_particles(const roms_tlev* t) {
  ShimState S;
  int r;
  if (!enter_armed(S, "roms_gpu_do_particles", &r)) return r;
  if (!tlev_ok(t)) { *S.err = "roms_gpu_do_particles: bad time levels"; return -1; }
  if (failed_before(S, "roms_gpu_do_particles")) return -5;
  return do_particles(S, t->nnew, "roms_gpu_do_particles");
}

int roms_gpu_part_state(long out[8]) {
  ShimState S;
  int r;
  if (!enter_armed(S, "roms_gpu_part_state", &r)) return r;
  if (!out) { *S.err = "roms_gpu_part_state: null argument"; return -1; }
  out[0] = Pt.np; out[1] = Pt.ntag; out[2] = (long)Pt.c[cSur]; out[3] = (long)Pt.c[cBot]; out[4] = (long)Pt.c[cLost];
  out[5] = (long)Pt.c[cMoved]; out[6] = (long)Pt.c[cRange]; out[7] = (long)Pt.c[cOver];
  return 0;
}

int roms_gpu_part_copy_out(double* dst, long count, int global) {
  ShimState S;
  int r;
  if (!enter_armed(S, "roms_gpu_part_copy_out", &r)) return r;
  const long np = Pt.np;
  if (count < np * kNpv || (np > 0 && !dst)) { *S.err = "roms_gpu_part_copy_out: count is less than np*13"; return -1; }
  if (np == 0) return 0;
  if (hipMemcpy2DAsync(dst, (size_t)np * sizeof(double), Pt.list[Pt.cur], (size_t)Pt.g.npmx * sizeof(double),
                       (size_t)np * sizeof(double), kNpv, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
      hipStreamSynchronize(S.s) != hipSuccess) {
    *S.err = "roms_gpu_part_copy_out: copy failed";
    return -2;
  }
  if (global) {   // wrt_particles :416-417
    const double sx = S.dims->iSW_corn + 0.5, sy = S.dims->jSW_corn + 0.5;
    for (long q = 0; q < np; q++) { dst[np + q] = dst[np + q] + sx; dst[2 * np + q] = dst[2 * np + q] + sy; }
  }
  return 0;
}

int roms_gpu_wrt_part(const char* path, int rec, int total_rec, double time) {
  ShimState S;
  int r;
  if (!enter_armed(S, "roms_gpu_wrt_part", &r)) return r;
  if (!path || rec < 1) { *S.err = "roms_gpu_wrt_part: bad path/record"; return -1; }
  if (failed_before(S, "roms_gpu_wrt_part")) return -5;
  // the previous record's copy to the host reads Pt.rec: join it before the record is packed again
  if ((r = io_writer_join(*S.err))) return r;
  hipLaunchKernelGGL(k_part_record, dim3(nblocks(Pt.g.npmx)), dim3(kPB), 0, S.s, Pt.g.npmx, Pt.list[Pt.cur], Pt.np,
                     S.dims->iSW_corn + 0.5, S.dims->jSW_corn + 0.5, Pt.rec);
  if (hipGetLastError() != hipSuccess) { *S.err = "roms_gpu_wrt_part: launch failed"; return -3; }
  return part_write(S, path, rec, time, Pt.rec, Pt.g.npmx, (int)kBigNumber);
}

// n calls on a copy of the list (the particles do not move): ms[0] whole calls, ms[1] the rhs and advance kernel alone
int roms_gpu_time_do_particles(int n, const roms_tlev* t, double ms[2]) {
  ShimState S;
  int r;
  if (!enter_armed(S, "roms_gpu_time_do_particles", &r)) return r;
  if (!tlev_ok(t) || n < 1 || !ms) { *S.err = "roms_gpu_time_do_particles: bad arguments"; return -1; }
  if (failed_before(S, "roms_gpu_time_do_particles")) return -5;
  const size_t lb = (size_t)Pt.g.npmx * kNpv * sizeof(double);
  double* keep = nullptr;
  if (hipMalloc(&keep, lb) != hipSuccess) { *S.err = "roms_gpu_time_do_particles: allocation failed"; return -2; }
  const PartCtx saved = Pt;
  auto restore = [&]() {
    Pt.np = saved.np; Pt.first = saved.first; std::memcpy(Pt.c, saved.c, sizeof Pt.c);
    (void)hipMemcpyAsync(Pt.list[Pt.cur], keep, lb, hipMemcpyDeviceToDevice, S.s);
    (void)hipMemcpyAsync(Pt.cnt, Pt.c, sizeof Pt.c, hipMemcpyHostToDevice, S.s);
    (void)hipStreamSynchronize(S.s);
  };
  if (hipMemcpyAsync(keep, Pt.list[Pt.cur], lb, hipMemcpyDeviceToDevice, S.s) != hipSuccess) r = -2;
  ms[0] = ms[1] = 0.0;
  // every timed call starts from the kept list; the copy back lies outside its two events
  for (int q = -1; q < n && !r; q++) {
    restore();
    const double m = time_rounds(S.s, 1, false, [&]() { return do_particles(S, t->nnew, "roms_gpu_time_do_particles"); });
    if (m < 0) r = (int)m;
    else if (q >= 0) ms[0] += m;
  }
  if (!r) {
    restore();
    ms[1] = time_rounds(S.s, n, true, [&]() { return launch_rhs(S, t->nnew, false); });
    if (ms[1] < 0) r = (int)ms[1];
  }
  restore();
  (void)hipFree(keep);
  if (r) *S.err = "roms_gpu_time_do_particles: launch or timing failed";
  return r;
}

}  // extern "C"
