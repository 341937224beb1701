// roms_dev.h -- device-side state and index helpers of the MI355X ROMS hot path.
//
// Every array keeps the reference's Fortran layout (ocean_vars.F:68-116):
// horizontal extent (-1:Lm+2, -1:Mm+2), i fastest; rho-point 3-D arrays stack
// N levels (1:N), w-point arrays N+1 levels (0:N); u,v add 3 time levels,
// zeta/ubar/vbar 4, t(...,3,NT).  On the device a row j holds nx2 doubles:
// Lm+4 rounded up to kRowAlign (128 B), and every array's base is shifted by
// kAlignOff doubles, so element (i,j) sits at (i+1) + (j+1)*nx2 and i = 1 of
// every row and level starts a 128-B line: a wavefront of 64 consecutive i
// from i = 1 reads exactly four lines (at nx2 = Lm+4 the rows drift 32 B per
// row against the lines and most such runs touch five).  Host copies re-pitch
// the rows (roms_shim.cpp); no transpose anywhere.
//
// Wide fast-time halos (multi-rank, Bounds::gx > 0): every plane also holds
// gx extra ghost rows below j = -1 and above j = Mm+2, and every row gx extra
// ghost columns left of i = -1 and right of i = Lm+2.  The indexing above is
// unchanged: the plane stride n2 covers Mm+4+2gx rows, the base of every
// array sits gx rows into its allocation, and the columns i < -1 of row j are
// the last gx doubles of row j-1's pitch (nx2 >= Lm+4+2gx keeps them apart
// from that row's own columns).  Only the barotropic fast loop reads them
// (launch_step2d: 2+gx-wide exchanges every 1+gx/2 fast steps).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace roms {

constexpr int kMaxFast = 288;  // coupling.F:19, weight(2,288)
constexpr int kRowAlign = 16;  // device row pitch granule: 16 doubles = one 128-B line
constexpr int kAlignOff = 14;  // base shift: element i = 1 (index 2 of a row) on a line start

// Loop bounds of the single tile that covers one rank's subdomain
// (compute_tile_bounds.h, compute_auxiliary_bounds.h, compute_extended_bounds.h).
struct Bounds {
  int Lm, Mm, N, NT, nTS, nx2;   // nx2: device row pitch (>= Lm+4+2gx)
  long n2, n3, n3w;              // n2 = nx2 * (Mm+4+2gx): plane stride
  int gx;                        // extra ghost rows/columns beyond the reference's 2 (wide fast halos)
  int istr, iend, jstr, jend;
  int istrU, istrR, iendR, jstrV, jstrR, jendR;   // auxiliary
  int istrE, iendE, jstrE, jendE;                  // extended
  int west_edge, east_edge, south_edge, north_edge;  // physical (closed) edges
  int ew_periodic, ns_periodic;
  int west_exch, east_exch, south_exch, north_exch;  // message edges (rank neighbours)
};

// Physics switches (cppdefs.opt), kernel-selection switches (ROMS_GPU_*,
// roms_gpu_init) and scalars of the run.
struct Params {
  int nonlin_eos, salinity, lmd, uv_vis2, ts_dif2;
  int lmd_rimix, lmd_convec, lmd_nonlocal;  // LMD_RIMIX, LMD_CONVEC, LMD_NONLOCAL (lmd != 0: MIXING+KPP+BKPP)
  int lmd_ddmix;                            // LMD_DDMIX (needs SALINITY)
  int iso;                                  // ADV_ISONEUTRAL (+SW_TRIADS, STABILIZE): k_iso.hip
  int uv_adv, uv_cor;                       // UV_ADV, UV_COR
  int tides;                                // TIDES pot_tides: ptide in prsgrd
  int bulk_frc;                             // BULK_FRC (k_bulk.hip; u* from sustr_r/svstr_r in lmd_kpp)
  // ---- kernel selection: the form of a routine, never its result ----
  // (the two unnamed ints stand where a retired switch stood, so that no member
  // moves: with them gone and reserved_ grown instead, seg_order .. seg_buf 4-8 B
  // lower, the C3 step, set_HUV and step3d_uv2 measured above the parent,
  // profiles/r11_retire_three_ab.txt)
  int : 32;
  int s2d_split;  // 1: step2d as separate zeta / momentum kernels (ROMS_GPU_S2D_SPLIT=1)
  int colseg;     // 1: segment-partitioned column solvers (k_colseg.h; N > 63, ROMS_GPU_COLSEG=0/1)
  int colreg;     // bit 2: register-resident k_pre_tracer_v_reg where compiled for N (ROMS_GPU_COLREG=0: the LDS form)
  int uv2_fused;  // 1: one-pass step3d_uv2 (k_uv2_fused; ROMS_GPU_UV2_FUSED=0 disables)
  int chain;      // 1: chained 4-lane set_HUV1 (k_chain.h; ROMS_GPU_CHAIN=0 disables)
  int seg_order;  // block order of the segment solvers (seg_tile; ROMS_GPU_SEG_ORDER)
  int seg_xg;     // x-blocks per group of seg_order 3 (ROMS_GPU_SEG_XG)
  int s2d_fold;   // closed-wall edges of the fast step inside k_s2d_fb (ROMS_GPU_S2D_EDGES=1: separate kernels)
  int hoist;        // per-level horizontal kernels with every global load at entry (ROMS_GPU_HOIST=0: per-phase forms)
  int chain_dirz;   // chain kernels (set_HUV1, uv2): one direction per block (ROMS_GPU_CHAIN_DIRZ=0: both in turn)
  int prs_fuse_uv;  // whole steps: horizontal momentum r.h.s. inside prsgrd (ROMS_GPU_PRS_UV=0: separate)
  int : 32;
  int prs_buf;    // k_prsgrd_uv windows through buffer loads (ROMS_GPU_PRS_BUF)
  int prs_strip;  // prsgrd + momentum r.h.s. in j-marching strips (k_prsgrd_strip; ROMS_GPU_PRS_STRIP=0: tiles)
  int t_strip;    // horizontal tracer advection in j-marching strips (k_tracer_strip; ROMS_GPU_T_STRIP=0: tiles)
  int visc_stg;   // visc3d: raw u/v/Hz windows staged in LDS per level (default; ROMS_GPU_VISC_STG=0: per-point loads)
  int t3dmix_stg; // t3dmix (two tracers): Hz/T/S windows staged in LDS per level (default; ROMS_GPU_T3DMIX_STG=0: per-point loads)
  int kpp_ty;     // k_kpp_int: 4 (default) staged Rig windows on 64x4 blocks, 8 on 64x8, 43 64x4 at 3 waves/SIMD, 0 one row per block (ROMS_GPU_KPP_TY)
  int uv1_lds;    // k_uv1_seg: Hz pairs kept in LDS from the spline phase, rufrc chained (ROMS_GPU_UV1_LDS=0: reloads)
  int omega_seg;  // omega: segment form k_omega_seg, one read of each input (ROMS_GPU_OMEGA_SEG=0: two-pass k_omega)
  int omega_cw;   // k_omega_seg columns per block: 64, 32 or 16 (ROMS_GPU_OMEGA_CW)
  int p_in_rho;   // rho_eos's sweep also forms prsgrd's P (ROMS_GPU_P_IN_RHO=0: k_prsgrd_P)
  int omega_hb;   // the predictor's omega forms pre_step3d's Hz_bak/Hz_fwd (ROMS_GPU_OMEGA_HB=0: pre_step3d does)
  int preuv_lds;  // k_pre_uv_seg: u(indx) stored and u(nstp)/u(indx) combined in the spline phase (ROMS_GPU_PREUV_LDS=0: reloads)
  int seg_jrows;  // rows j per block of the momentum segment solvers (1..kSegJMax; ROMS_GPU_SEG_JROWS)
  int seg_buf;    // 1: segment solvers with buffer loads (k_*_segb; ROMS_GPU_SEG_BUF=0: the pointer forms)
  // eight more retired switches stood among the ints above: their room stays, so
  // that every member from here on -- and Fields after Params -- keeps its
  // kernel-argument offset (without it lmd_vmix measured 2-3% slower at C3,
  // its kernels differing in nothing but their scalar-load offsets:
  // profiles/r9_retire_variants_ab.txt)
  // vgrid2 took the first of the eight: further VGrid kernels (ROMS_GPU_VGRID2 bits, 0: the streaming forms):
  // 1 k_omega_seg, 2 k_set_huv1_chain, 4 k_uv2_fused, 8 k_visc3d_stg, 16 k_t3dmix_stg.  In force as bits 8.. of vg.
  int vgrid2;
  // t_pair took the second: tracer segment solvers that carry T and S as two right-hand sides of one block
  // (ROMS_GPU_T_PAIR bits: 1 k_pre_tracer_segb_pair, 2 k_step3d_t_segb_pair).  The bits in force: the configured mask while Akt(isalt) is
  // Akt(itemp) bit for bit (the shim's akt_same flag, set by lmd_vmix, cleared by a host write of Akt), else 0.
  int t_pair;
  // t_hstg took the third: the horizontal tracer kernels of pre_step3d / step3d_t (two tracers) as one block per
  // 64x8 cells walking the levels over staged windows (ROMS_GPU_T_HSTG bits: 1 k_pre_tracer_stg, 2 k_step3d_t_stg,
  // 4 k_pre_tracer_stg forms Hz from VGrid).  The bits in force: bit 4 only while the grid's validity flag holds.
  int t_hstg;
  // kpp_pf took the fourth: levels of k_kpp_ext's descending sweep whose loads are in flight ahead of the level formed
  // (ROMS_GPU_KPP_PF, 1..kKppPfMax; 1: the single level ahead; k_lmd.hip)
  int kpp_pf;
  // lean_st took the first of reserved_: stores of a whole step that nothing in the step reads, left out, bitwise
  // (ROMS_GPU_LEAN_ST bits, default 3, 0: every store): 1 the predictor's u, v(indx) = Hz*u(nstp) (k_pre_uv_segb<false>;
  // k_uv1_segb<true> forms it again), 2 Akt(isalt) where it is Akt(itemp) bit for bit and the step's tracer solvers
  // read one slot (k_kpp_int's one-slot form; the shim's akt_stale flag and akt_sync make the slot current for every
  // other reader).  Whole steps only: the routine entries keep the storing and loading forms.
  int lean_st;
  int reserved_[3];
  // ---- sizes and physics masks ----
  int s2d_k;      // fast steps per zeta/ubar/vbar exchange (multi-rank, wide halos of 2*s2d_k; 1: every step)
  int uv2e_nc, uv2e_nf;   // lengths of Fields::uv2e_couple / uv2e_flux
  int npip;       // pipe_frc.F: number of pipes (0: pipe_source off)
  int nriv, nrivf;  // river_frc.F: number of rivers (0: river_source off), river faces
  int curvgrid;   // CURVGRID && UV_ADV: curvature terms (compute_horiz_rhs_uv_terms.h:8-11)
  int obc;        // open edges: 1 W, 2 E, 4 S, 8 N (Flather / Orlanski + *_FRC_BRY)
  // (four shorts ahead of the doubles)
  short kpp_lean;   // lmd_vmix leaves out work past the boundary layers, bitwise (ROMS_GPU_KPP_LEAN bits, default 7, 0: the full forms):
                    // 1 k_kpp_ext drops Vtsq and its swr_frac loads once the wave has its kbls, 2 k_kpp_ext keeps FC(0:kpp_fckeep) only,
                    // 4 k_kpp_int's kbls scan ends at the first failing level
  short kpp_fckeep; // levels FC(0:keep) of k_kpp_ext's LDS slot, 1..kKppFcKeepMax (ROMS_GPU_KPP_FCKEEP); above them the FC sweep is repeated
  short vgrid;      // kernels that form Hz, z_r, z_w of a column from z_sd, h, hinv (VGrid) instead of streaming the arrays, bitwise
                    // (ROMS_GPU_VGRID bits, default 11, 0: the streaming forms): 1 k_rho_eos_split, 2 k_kpp_ext, 4 k_kpp_int, 8 k_set_huv
  short vg;         // the bits of vgrid, and of vgrid2 << kVg2Shift, in force: both while the stored arrays are set_depth's own (the shim's validity flag), else 0
  double ubind;   // OBC binding velocity
  double dt, dtfast, g, rho0, vonKar, qp2, gamma2, hc;
  double rdrg, Zob, Tcoef, T0, Scoef, S0;
  double Akv_bak, Akt_bak[2];  // scalars.F:83
};
// the kernel-argument offsets the kernels were measured with (reserved_ above)
static_assert(offsetof(Params, s2d_k) == 196 && offsetof(Params, ubind) == 240 && sizeof(Params) == 384,
              "Params: no member from s2d_k on may move");

// Device pointers of the model state (the "module arrays") plus scratch.
struct Fields {
  // grid (grid.F)
  double *h, *hinv, *f, *fomn, *pm, *pn, *dm_r, *dn_r, *dm_u, *dn_u, *dm_v, *dn_v, *dm_p, *dn_p,
      *pmon_u, *pnom_v, *rmask, *pmask, *umask, *vmask;
  double *dndx, *dmde;  // CURVGRID metric derivatives
  double* ptide;        // tides.F surface tidal potential (TIDES)
  // BULK_FRC inputs (rho points) and rho-point stresses (bulk_frc.F, surf_flux.F)
  double *uwnd, *vwnd, *tair, *qair, *prate, *swrad, *lwrad, *sustr_r, *svstr_r;
  double *Cs_w, *Cs_r;  // scoord.F (N+1)
  double* z_sd;         // the free surface the last set_depth formed z_w, z_r, Hz from (VGrid; not an ABI field)
  // ocean vars
  double *zeta, *ubar, *vbar, *u, *v, *t;
  double *FlxU, *FlxV, *We, *Wi, *Hz, *Hz_u, *Hz_v, *z_r, *z_w;
  // coupling.F
  double *rufrc, *rvfrc, *rhoA, *rhoS, *r_D, *Zt_avg1, *DU_avg1, *DV_avg1, *DU_avg2, *DV_avg2,
      *DU_avg_bak, *DV_avg_bak;
  // eos_vars.F / mixing.F
  double *rho, *rho1, *qp1, *bvf, *Akv, *Akt, *visc2_r, *visc2_p, *diff2;
  double *hbls, *hbbl, *ghat, *swr_frac;
  // surf_flux.F
  double *sustr, *svstr, *stflx, *srflx, *swflx;
  // private scratch: A3d(:,1..4) and per-column work arrays
  double *ru, *rv, *P, *rhos;
  double *c0, *c1, *c2, *c3;   // (0:N) column scratch, w-point layout
  double *s0, *s1, *s2, *s3, *s4, *s5, *s6, *s7, *s8, *s9;  // 2-D scratch (step2d, diag)
  // lmd_vmix / lmd_kpp private work arrays: raw Richardson number (0:N) and
  // the 2-D boundary-layer fields carried from the extended-range pass
  double *lmd_rig, *lmd_hbl, *lmd_bbl, *lmd_Bo, *lmd_Bosol, *lmd_ustar;
  // pipe_frc.F: pipe_idx (0: none), pipe_flx, pipe_prf(npip,N), pipe_trc(npip,NT)
  int* pipe_idx;
  double *pipe_flx, *pipe_prf, *pipe_trc;
  // river_frc.F: riv_uflx/riv_vflx (10*iriver + signed fraction on river
  // faces), riv_vol(nriv), riv_trc(nriv,NT); riv_face: (dir, i, j) of every
  // face with |riv_flx| > 1e-3, three ints per face (Params::nrivf of them)
  double *riv_uflx, *riv_vflx, *riv_vol, *riv_trc;
  int* riv_face;
  // step3d_uv2's closed-edge columns (uv2_edge_lists): (dir, i, j) triples of
  // the couple and the flux pass (Params::uv2e_nc / uv2e_nf of them; nullptr: the one-lane edge mode)
  int *uv2e_couple, *uv2e_flux;
  // boundary.F open-boundary data, [0] west, [1] east (index j, 0:Mm+1),
  // [2] south, [3] north (index i, 0:Lm+1); u, v (.,N); t (.,N,NT)
  double *bzeta[4], *bubar[4], *bvbar[4], *bu[4], *bv[4], *bt[4];
  double* ub[4];   // SPONGE_TUNE ub_west/east/south/north (sponge_tune.F; nullptr: ub_tune off)
  // column-solver scratch in global memory, 2*max(NT,2) slots of (0:N) levels
  // (nullptr: the solvers keep their columns in LDS; see ColGlb in k_common.h)
  double* colscr;
  // ADV_ISONEUTRAL (k_iso.hip; nullptr when off): eos_vars.F:28-31 dRdx, dRde
  // (N) and idRz (0:N), mixing.F:24-27 diff3u, diff3v (N), step3d_t's Akz
  // (0:N), and the operator's 3-D work fields dTdz, FSC (0:N), dTdx, dTde, LapT (N)
  double *dRdx, *dRde, *idRz, *diff3u, *diff3v, *Akz;
  double *iso_dTdz, *iso_FSC, *iso_dTdx, *iso_dTde, *iso_LapT;
};

// The fast step's 2-D fields addressed from one buffer window (k_s2d_fb):
// one descriptor plus a 32-bit byte offset per field in place of a 64-bit
// base each -- the fused fast step reads and writes 25 of them, and their
// bases alone held more scalar registers than the kernel has.  roms_gpu_init
// allocates these fields next to each other and fills the window when they
// span less than 2 GiB (base = nullptr: the pointer form).
enum S2dWinField : int {
  kW_zeta, kW_ubar, kW_vbar, kW_h, kW_dn_u, kW_dm_v, kW_pm, kW_pn, kW_swflx, kW_rmask, kW_rhoS, kW_rhoA, kW_umask,
  kW_vmask, kW_rufrc, kW_rvfrc, kW_DU_avg1, kW_DV_avg1, kW_DU_avg2, kW_DV_avg2, kW_Zt_avg1, kW_DU_avg_bak,
  kW_DV_avg_bak, kW_s0, kW_s1, kWinN
};
struct S2dWin {
  const double* base;   // nullptr: no window
  int lead;             // element (i,j) of a field sits (IJ + lead) doubles past its window origin
  unsigned off[kWinN];  // byte offset of each field's origin (its element IJ = -lead) from base
};

struct Halo;  // halo.h: multi-rank exchange state (host object; nullptr = single rank)
struct Dev {
  Bounds b;
  Params p;
  Fields f;
  const Halo* halo;
  S2dWin w2;
};

// ---- index helpers (device + host) ----
__host__ __device__ __forceinline__ long IJ(const Bounds& b, int i, int j) {
  return (long)(i + 1) + (long)(j + 1) * b.nx2;
}
__host__ __device__ __forceinline__ long IJK(const Bounds& b, int i, int j, int k) {  // 1:N
  return IJ(b, i, j) + (long)(k - 1) * b.n2;
}
__host__ __device__ __forceinline__ long IJW(const Bounds& b, int i, int j, int k) {  // 0:N
  return IJ(b, i, j) + (long)k * b.n2;
}
__host__ __device__ __forceinline__ long IJL(const Bounds& b, int i, int j, int l) {  // (:,:,4)
  return IJ(b, i, j) + (long)(l - 1) * b.n2;
}
__host__ __device__ __forceinline__ long IJKL(const Bounds& b, int i, int j, int k, int l) {  // (:,:,N,3)
  return IJ(b, i, j) + (long)(k - 1) * b.n2 + (long)(l - 1) * b.n3;
}
__host__ __device__ __forceinline__ long TIDX(const Bounds& b, int i, int j, int k, int l, int itrc) {
  return IJKL(b, i, j, k, l) + (long)(itrc - 1) * 3 * b.n3;
}

__device__ __forceinline__ double fmax0(double a) { return a > 0.0 ? a : 0.0; }
__device__ __forceinline__ double fmin0(double a) { return a < 0.0 ? a : 0.0; }
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ int iclamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- the vertical grid of one column (set_depth.F:16-186) ----
// z_w, z_r, Hz are functions of the column's free surface z, h, hinv and the
// per-level constants Cs_w, Cs_r, hc, N.  k_set_depth stores them through
// these functions, and the kernels switched by Params::vg form them again from
// z_sd (the z set_depth used), h and hinv instead of streaming the 3-D arrays:
// the same expressions in the same order (-ffp-contract=off), so the same bits.
constexpr int kVgRho = 1, kVgKppExt = 2, kVgKppInt = 4, kVgHuv = 8, kVgAll = 15;   // Params::vgrid bits
constexpr int kVgDefault = kVgRho | kVgKppExt | kVgHuv;   // k_kpp_int measured slower with it (profiles/r8_vgrid_ab.txt)
// Params::vgrid2 bits; in Params::vg they stand kVg2Shift higher
constexpr int kVg2Omega = 1, kVg2Huv1 = 2, kVg2Uv2 = 4, kVg2Visc = 8, kVg2T3dmix = 16, kVg2All = 31, kVg2Shift = 8;
constexpr int kVg2Default = kVg2All;  // profiles/r10_vgrid_rest_ab.txt
// Params::t_pair bits (ROMS_GPU_T_PAIR)
constexpr int kTPairPre = 1, kTPairCor = 2, kTPairAll = 3;
constexpr int kTPairDefault = kTPairAll;
// Params::lean_st bits (ROMS_GPU_LEAN_ST)
constexpr int kLeanUv = 1, kLeanAkt = 2, kLeanAll = 3;
constexpr int kLeanDefault = kLeanAll;
// Params::t_hstg bits (ROMS_GPU_T_HSTG)
constexpr int kTHstgPre = 1, kTHstgCor = 2, kTHstgHz = 4, kTHstgAll = 7;
constexpr int kTHstgDefault = kTHstgAll, kTHstgDefaultCol = kTHstgCor;   // segment path / column solvers (profiles/r13_tracer_stg_ab.txt)
struct VGrid {
  const double *Cs_w, *Cs_r;
  double z, h, hinv, hc, ds;
  int N;
  __device__ __forceinline__ double zw0() const { return -h; }
  // csw = Cs_w[k], csr = Cs_r[k]: a level walk reads them a level ahead (a
  // scalar load per level waited on in place costs the walk its latency)
  __device__ __forceinline__ double zw1(int k, double csw) const {   // z_w(k), k = 1..N
    const double cff_w = hc * ds * (double)(k - N);
    return z + (z + h) * (cff_w + csw * h) * hinv;
  }
  __device__ __forceinline__ double zr(int k, double csr) const {    // z_r(k), k = 1..N
    const double cff_r = hc * ds * ((double)(k - N) - 0.5);
    return z + (z + h) * (cff_r + csr * h) * hinv;
  }
  __device__ __forceinline__ double zw(int k, double csw) const { return k == 0 ? zw0() : zw1(k, csw); }   // k = 0..N
  __device__ __forceinline__ double zw1(int k) const { return zw1(k, Cs_w[k]); }
  __device__ __forceinline__ double zr(int k) const { return zr(k, Cs_r[k]); }
};
__device__ __forceinline__ double vg_zw(const VGrid& g, int k) { return k == 0 ? g.zw0() : g.zw1(k); }   // k = 0..N
__device__ __forceinline__ double vg_zr(const VGrid& g, int k) { return g.zr(k); }
// a level walk carries z_w(k) across levels instead (Hz(k) = z_w(k) - z_w(k-1))
__device__ __forceinline__ double vg_hz(const VGrid& g, int k) { return g.zw1(k) - vg_zw(g, k - 1); }
__device__ __forceinline__ VGrid vg_make(const Dev& d, double z, double h, double hinv) {
  return VGrid{d.f.Cs_w, d.f.Cs_r, z, h, hinv, d.p.hc, 1.0 / (double)d.b.N, d.b.N};
}
// the column's z, h, hinv loaded once; the levels then cost the scalar Cs_w[k] / Cs_r[k] only
__device__ __forceinline__ VGrid vg_column(const Dev& d, long ij) {
  return vg_make(d, d.f.z_sd[ij], d.f.h[ij], d.f.hinv[ij]);
}

// XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs
// (MI355X_MICROARCH.md: blocks b and b+8 share an XCD and its L2), so with
// the plain grid order the four neighbours of a tile live in other XCDs' L2s
// and every halo row is fetched from HBM twice.  xcd_tile() maps the
// physical block id to a logical tile so that each XCD walks one contiguous
// 1/8 of the (x fastest, then y, then z) tile sequence: neighbouring tiles of
// a level are processed by the same XCD at about the same time.
__device__ __forceinline__ uint3 xcd_tile() {
  const unsigned gx = gridDim.x, gy = gridDim.y;
  const unsigned total = gx * gy * gridDim.z;
  const unsigned phys = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const unsigned q = total >> 3, r = total & 7u, x = phys & 7u, slot = phys >> 3;
  const unsigned logical = x * q + (x < r ? x : r) + slot;
  uint3 t;
  t.x = logical % gx;
  t.y = (logical / gx) % gy;
  t.z = logical / (gx * gy);
  return t;
}

// Compiler fence between the levels of a fully unrolled column walk: memory
// operations are not moved across it, so the scheduler cannot hoist the loads
// of all N levels to the top (which would need N x (loads per level)
// registers and spill); a few levels of look-ahead remain within a chunk.
#define ROMS_LEVEL_FENCE() __asm__ volatile("" ::: "memory")
#ifndef ROMS_FENCE_EVERY
#define ROMS_FENCE_EVERY 1000
#endif
#define ROMS_LEVEL_FENCE_AT(k) do { if ((k) % ROMS_FENCE_EVERY == 0) ROMS_LEVEL_FENCE(); } while (0)

// 2-D launch over an inclusive index rectangle [i0,i1]x[j0,j1]: one lane per
// (i,j) column, 64 consecutive i per wavefront (coalesced), 4 rows per block.
struct Range {
  int i0, i1, j0, j1;
};
constexpr int kBX = 64, kBY = 4;
// First tile column of a launch over [i0, i1]: i0 rounded down to a line
// start of the device rows (i = 1 mod kRowAlign, roms_dev.h layout), so the
// wavefront rows of every tile read whole 128-B lines; the lanes left of i0
// in the first tile idle.  (Ranges from istrR/istrE = 0 or -1, istrU = 2 and
// the multi-rank rim strips all start off a line.)
#ifndef ROMS_TILE_ALIGN
#define ROMS_TILE_ALIGN 1   // 0: tiles start at the range's first column (A/B builds, tools/build_variant.sh)
#endif
__host__ __device__ __forceinline__ int tile_i0(int i0) { return ROMS_TILE_ALIGN ? i0 - ((i0 - 1) & (kRowAlign - 1)) : i0; }
inline dim3 grid_of(const Range& r) {
  int ni = r.i1 - tile_i0(r.i0) + 1, nj = r.j1 - r.j0 + 1;
  if (ni < 1) ni = 1;
  if (nj < 1) nj = 1;
  return dim3((ni + kBX - 1) / kBX, (nj + kBY - 1) / kBY, 1);
}
// 3-D launch: same (i,j) tiling with one grid z-slice per level k=1..nk
inline dim3 grid3_of(const Range& r, int nk) {
  dim3 g = grid_of(r);
  g.z = nk;
  return g;
}
// Column launch: one wavefront of 64 consecutive i per block, one row j per
// block row; column scratch lives in LDS (see ColLds in k_common.h).
constexpr int kCX = 64;
// segment-partitioned column solvers (k_colseg.h)
#ifndef ROMS_SEG_ROWS
#define ROMS_SEG_ROWS 13
#endif
#ifndef ROMS_SEG_MAXS
#define ROMS_SEG_MAXS 8
#endif
constexpr int kSegRows = ROMS_SEG_ROWS;   // cells per segment (register arrays of kSegRows + 2)
constexpr int kSegMaxS = ROMS_SEG_MAXS;   // segments per block (kSegCW columns each): N <= kSegRows * kSegMaxS
#ifndef ROMS_SEG_CW
// round 5: 16-column blocks (four segments per wavefront, 128-thread
// blocks, four per CU): against 64 columns pre_step3d 11.1 -> 9.9 ms,
// step3d_uv1 4.55 -> 3.93 ms at C3 (r5_q_seg_cw32_default_ab.txt,
// r5_s_seg_cw16_ab.txt); round 3 had measured 64 ahead of 16
// (r3_l_seg_shape_ab.txt, before the solvers kept their reloads in LDS)
#define ROMS_SEG_CW 16
#endif
constexpr int kSegCW = ROMS_SEG_CW;       // columns per segment-solver block (lanes of one segment)
constexpr int kSegBlock = ((kSegMaxS * kSegCW + 63) / 64) * 64;   // threads of a segment-solver block (max)
// The momentum solvers' blocks may hold several rows j (blockDim.z) of the
// same kSegCW columns, so the v columns' j-1, j-2, j+1 stencil rows are loaded
// by the neighbouring rows' waves of the same block, close together in time.
#ifndef ROMS_SEG_JMAX
#define ROMS_SEG_JMAX 1
#endif
constexpr int kSegJMax = ROMS_SEG_JMAX;
// the fewest rows any segment of a launch may have (k_colseg.h seg_live)
#ifndef ROMS_SEG_NMIN
#define ROMS_SEG_NMIN 11   // 0: every row select kept (the round-4 code; A/B builds)
#endif
constexpr int kSegNMin = ROMS_SEG_NMIN;
// waves per SIMD the buffer-addressed segment solvers are built for (2: one
// 512-thread block per CU at <= 256 VGPRs; 4: two blocks at <= 128)
#ifndef ROMS_SEG_BUF_WAVES
#define ROMS_SEG_BUF_WAVES 2
#endif
#ifndef ROMS_PRE_T_SEG_WAVES   // k_pre_tracer_segb alone (A/B builds)
#define ROMS_PRE_T_SEG_WAVES ROMS_SEG_BUF_WAVES
#endif
#ifndef ROMS_T_SEG_WAVES       // k_step3d_t_segb alone (A/B builds)
#define ROMS_T_SEG_WAVES ROMS_SEG_BUF_WAVES
#endif
// segments of an N-level column (one per wavefront at kSegCW = 64, seg_waves)
// and whether each of them gets at least kSegNMin rows
inline int seg_count(int N) {
  const int per = kCX / kSegCW, S = (N + kSegRows - 1) / kSegRows;
  return (S + per - 1) / per * per;
}
inline bool seg_rows_ok(int N) { return N / seg_count(N) >= kSegNMin; }
inline dim3 gridc_of(const Range& r) {
  int ni = r.i1 - tile_i0(r.i0) + 1, nj = r.j1 - r.j0 + 1;
  if (ni < 1) ni = 1;
  if (nj < 1) nj = 1;
  return dim3((ni + kCX - 1) / kCX, nj, 1);
}
#define ROMS_IJC_OR_RETURN(R)                                       \
  const uint3 bI = xcd_tile();                                      \
  const int i = tile_i0((R).i0) + (int)(bI.x * kCX + threadIdx.x);  \
  const int j = (R).j0 + (int)bI.y;                                 \
  if (i < (R).i0 || i > (R).i1 || j > (R).j1) return;
#define ROMS_IJ_OR_RETURN(R)                                        \
  const uint3 bI = xcd_tile();                                      \
  const int i = tile_i0((R).i0) + (int)(bI.x * kBX + threadIdx.x); \
  const int j = (R).j0 + (int)(bI.y * kBY + threadIdx.y);           \
  if (i < (R).i0 || i > (R).i1 || j > (R).j1) return;

// ---- launcher declarations (one translation unit per routine family) ----
// Each takes the rank's device state and a stream; all enqueue asynchronously.
struct Tlev {
  int iic, ntstart, forw_start, iif, nfast, kstp, knew, nstp, nrhs, nnew;
};

// kernel-level timing hook (roms_gpu_time_routine with a kernel id): HIP
// events on the launch stream opening (end = 0) and closing (end = 1) an
// interval that covers `count` launches of one kernel
constexpr int kTimedS2dFb = 13;   // ROMS_R_K_S2D_FB
constexpr int kTimedPreUvSeg = 14, kTimedUv1Seg = 15, kTimedStep3dTSeg = 16;   // ROMS_R_K_*_SEG
constexpr int kTimedPrsgrdUv = 17;   // ROMS_R_K_PRSGRD_UV
constexpr int kTimedHaloPack = 18, kTimedHaloWait = 19, kTimedHaloUnpack = 20;   // ROMS_R_K_HALO_*
void ktimer_mark(hipStream_t s, int kernel_id, int end, int count = 0);

// The buffer-addressed kernels (BufF64, k_common.h) address one field with
// 32-bit byte offsets that must stay below 2 GiB (kBufOff = 2^31 marks a lane
// whose access the hardware drops): every field -- the largest is a w-point
// field, n2*(N+1) doubles on the padded pitch -- must fit.  roms_gpu_init
// refuses a subdomain that does not (1024^2 x 100 uses 0.85 GiB).
inline bool buffer_span_ok(const Bounds& b) { return b.n3w * 8 < 2147483648L; }

void launch_exchange(const Dev& d, hipStream_t s, double* a, int nlev);
// several arrays in one launch (one reference exchange_xxx(A,B,C,D) call);
// w > 2: a wide exchange (halo w deep, Bounds::gx >= w-2; the fast loop's)
constexpr int kExchMax = 16;
struct ExchList {
  double* p[kExchMax];
  int nlev[kExchMax];
  int n;
  int w = 2;
};
void launch_exchange_list(const Dev& d, hipStream_t s, const ExchList& L);
// ---- rim-first overlap of a producer's trailing exchange (SURVEY.md 8(e);
// mpi_exchanges.F's swaps overlapped with interior compute).  `run(R')`
// launches the producer's kernels on a sub-range.  On a multi-rank run the
// four rim strips (the two rows / columns next to each edge: every cell the
// exchange packs) go first, then `edges()` (kernels that fill ghost cells
// from the rim; they travel with the strips), then the exchange of L is
// forked onto the halo stream while the interior runs on s, and s joins it
// before the next routine.  Single rank / overlap off: run(R), edges(),
// exchange.  Opt-in (ROMS_GPU_OVERLAP3D=1), see halo_setup. ----
bool rim_overlap_on(const Dev& d, const Range& R);
void rim_fork(const Dev& d, hipStream_t s, const ExchList& L);
void rim_join(const Dev& d, hipStream_t s);
template <class Run, class Edges>
void launch_rim_first(const Dev& d, hipStream_t s, const Range& R, const ExchList& L, Run&& run, Edges&& edges) {
  if (!rim_overlap_on(d, R)) {
    run(R);
    edges();
    launch_exchange_list(d, s, L);
    return;
  }
  run(Range{R.i0, R.i0 + 1, R.j0, R.j1});
  run(Range{R.i1 - 1, R.i1, R.j0, R.j1});
  run(Range{R.i0 + 2, R.i1 - 2, R.j0, R.j0 + 1});
  run(Range{R.i0 + 2, R.i1 - 2, R.j1 - 1, R.j1});
  edges();
  rim_fork(d, s, L);
  run(Range{R.i0 + 2, R.i1 - 2, R.j0 + 2, R.j1 - 2});
  rim_join(d, s);
}
// the tracer list t(:,:,:,tlev,1:NT) as one exchange list (false if NT > 8)
bool tracer_exch_list(const Dev& d, int tlev, ExchList& L);
void launch_exchange_tracers(const Dev& d, hipStream_t s, int tlev);  // t(:,:,:,tlev,1:NT)
// Column kernels keep 2 (N+1)-level scratch columns per lane in LDS; opt in to
// the full 160 KB when N needs more than the default 64 KB.  Returns false if
// N is too deep for one wavefront's columns to fit.
bool setup_column_kernels(int N);
void setup_uv1_seg();      // k_uv1_seg's dynamic LDS limit (k_step3d_uv.hip)
void setup_pre_uv_seg();   // k_pre_uv_seg<true>'s dynamic LDS limit (k_pre_step3d.hip)
inline size_t col_smem_bytes(const Dev& d, int nslots) {
  return d.f.colscr ? 0 : (size_t)nslots * (d.b.N + 1) * 64 * sizeof(double);
}
// exchange = false: the caller exchanges z_w, z_r, Hz itself (merged with its own list);
// last: end of the fast loop, zeta(knew) = Zt_avg1 stored first (step2d_FB.F:566)
void launch_set_depth(const Dev& d, hipStream_t s, const Tlev& t, bool exchange = true, bool last = false);
// store_huv: also Hz_u/Hz_v (set_depth.F:220,227), read only by extract_data.F
void launch_set_huv(const Dev& d, hipStream_t s, const Tlev& t, bool store_huv = true);
// cnt (device, 3 counters, zeroed by the caller): mismatches of the stored z_w, z_r, Hz against VGrid
void launch_vgrid_check(const Dev& d, hipStream_t s, unsigned long long* cnt);
void launch_set_huv1(const Dev& d, hipStream_t s, const Tlev& t);
// hcff > 0: the predictor's call also forms pre_step3d's Hz_bak/Hz_fwd (c3/c2) of the
// interior cells with 0.5*dtau = hcff; returns whether it did (k_vertical.hip)
bool launch_omega(const Dev& d, hipStream_t s, const Tlev& t, double hcff = 0.0);
void setup_omega_seg();   // k_omega_seg<true>'s dynamic LDS limit
// The horizontal path decisions, shared by the launchers and
// roms_gpu_horizontal_path: omega's segment form over a range `width` columns
// wide (k_vertical.hip); the fast step's closed-edge mode, 0 none / 1 separate
// k_s2d_edges launches / 2 folded into k_s2d_fb (k_step2d.hip); whether a
// prsgrd call (with_uv: with the momentum r.h.s.) takes the j-marching
// strips, their rows jA..jB and the strips per row (k_prsgrd.hip)
bool omega_takes_seg(const Dev& d, int width);
int s2d_edge_mode(const Dev& d);
// bit m set: a fast step this host thread launched since the last `reset`
// took closed-edge mode m (launch_fast_step, on the bounds a multi-rank fast
// step widens: the mode can differ from one fast step to the next)
int s2d_edge_modes_taken(bool reset = false);
// pair-form tracer solver launches of this host thread since the last reset,
// per Params::t_pair bit (kTPairPre or kTPairCor; add: count `add` launches
// of `bit`); a replayed graph counts the launches of its capture only
long t_pair_launches(int bit, long add = 0, bool reset = false);
// the same for the launches that left a store out, per Params::lean_st bit
// (kLeanUv: k_pre_uv_segb<false>)
long lean_st_launches(int bit, long add = 0, bool reset = false);
// the same for the staged horizontal tracer kernels, per Params::t_hstg bit
// (kTHstgPre: k_pre_tracer_stg, kTHstgCor: k_step3d_t_stg, kTHstgHz: the
// k_pre_tracer_stg launches among them that formed Hz)
long t_hstg_launches(int bit, long add = 0, bool reset = false);
bool prsgrd_takes_strips(const Dev& d, bool with_uv, int& jA, int& jB, int& nstrip);
double pre_step3d_dtau(const Dev& d, const Tlev& t);   // pre_step3d's dtau (k_pre_step3d.hip)
void launch_rho_eos(const Dev& d, hipStream_t s, const Tlev& t, int tidx);
// uv_up >= 0: also add the horizontal momentum r.h.s. (UPSTREAM_UV if 1) of
// the following pre_step3d / step3d_uv1 (prsgrd_can_fuse_uv; the caller then
// passes uv_done to it)
// p_ready: P is current from the last rho_eos (p_in_rho), k_prsgrd_P is skipped
void launch_prsgrd(const Dev& d, hipStream_t s, const Tlev& t, int uv_up = -1, bool p_ready = false);
// k_tracer_strip.hip: rows jA..jB of R's horizontal tracer advection in
// j-marching strips (mode 0 step3d_t, 1 pre_step3d); false: not covered
bool launch_tracer_strip(const Dev& d, hipStream_t s, const Range& R, int mode, bool up, bool hb_done, int nnew,
                         int nrhs, double dtau, double cf_stp, double cf_bak, int nstp, int& jA, int& jB);
bool p_in_rho(const Dev& d);   // every rho_eos also forms prsgrd's P (k_vertical.hip)
bool prsgrd_can_fuse_uv(const Dev& d);
// hb_done: the interior cells' Hz_bak/Hz_fwd are in c3/c2 already (launch_omega)
// lean_uv (whole steps, lean_uv_step): k_pre_uv_segb does not store u, v(indx) and k_uv1_segb forms it again; both
// launches of a step get the same value, and nothing between them may read u, v(indx)
bool lean_uv_step(const Dev& d, const Tlev& t);   // t: the predictor's indices
void launch_pre_step3d(const Dev& d, hipStream_t s, const Tlev& t, bool uv_done = false, bool hb_done = false,
                       bool lean_uv = false);
void launch_step3d_uv1(const Dev& d, hipStream_t s, const Tlev& t, bool uv_done = false, bool lean_uv = false);
void launch_visc3d(const Dev& d, hipStream_t s, const Tlev& t);
void launch_step2d(const Dev& d, hipStream_t s, const Tlev& t, const double* w1, const double* w2);
void launch_step3d_uv2(const Dev& d, hipStream_t s, const Tlev& t);
// exchange = false: skip the closing t(nnew) exchange (whole steps with
// TS_DIF2: t3dmix reads only t(nrhs) and its own cells of t(nnew), and its
// own exchange of t(nnew) follows; the closed-wall ghosts are still set here)
void launch_step3d_t(const Dev& d, hipStream_t s, const Tlev& t, bool exchange = true);
void launch_t3dmix(const Dev& d, hipStream_t s, const Tlev& t);
// Tracer budget terms (k_tdiag.hip; DIAGNOSTICS with diag_trc): launch_step3d_t's hooks while armed and sampling
// (tdiag_sampling, a host flag of the calling thread).  tdiag_corrector, once per corrector ahead of its kernels:
// the sample count and the horizontal terms over the whole interior R (inputs the corrector does not change);
// tdiag_snap(r) between run(r)'s horizontal update and its column solve; tdiag_vert(r) after the solve
bool tdiag_sampling();
void tdiag_corrector(const Dev& d, hipStream_t s, const Range& R, const Tlev& t);
void tdiag_snap(const Dev& d, hipStream_t s, const Range& r, const Tlev& t);
void tdiag_vert(const Dev& d, hipStream_t s, const Range& r, const Tlev& t);
// Momentum budget terms (k_uvdiag.hip; DIAGNOSTICS with diag_uv): the hooks of launch_prsgrd, launch_step3d_uv1,
// launch_visc3d and launch_step3d_uv2 while armed and sampling (uvdiag_sampling, a host flag of the calling thread).
// uvdiag_prsgrd: after the corrector's unfused prsgrd, ru_pgr = ru*dxdyi_u*umask; uvdiag_uv1_begin opens a sample
// (navg, coef) and keeps u, v(nnew); uvdiag_uv1_end forms pgr, cor, adv, dis, vmx from the final ru the solvers
// stored; uvdiag_visc3d and uvdiag_uv2 add hmx and cpl to the open sample, once each
bool uvdiag_sampling();
void uvdiag_prsgrd(const Dev& d, hipStream_t s);
void uvdiag_uv1_begin(const Dev& d, hipStream_t s, const Tlev& t);
void uvdiag_uv1_end(const Dev& d, hipStream_t s, const Tlev& t);
void uvdiag_visc3d(const Dev& d, hipStream_t s, const Tlev& t);
void uvdiag_uv2(const Dev& d, hipStream_t s, const Tlev& t);
// Baroclinic pressure fluxes (k_pflx.hip; calc_pflx): while armed (pflx_armed, a host flag of the calling thread) every
// corrector prsgrd is followed by pflx_corrector -- in whole steps and in the roms_gpu_prsgrd entry with nrhs == 3 --
// which filters P, u, v(nrhs) and forms up, vp: two launches on s
bool pflx_armed();
void pflx_corrector(const Dev& d, hipStream_t s, const Tlev& t);
void launch_u3dbc(const Dev& d, hipStream_t s, const Tlev& t);
// river_frc.F hooks (k_river.hip): ubar/vbar(knew) and DU/DV_avg1 at river
// faces after each fast step; u,v(nnew) at river faces (pred: predictor ranges)
int s2d_exchange_interval(const Dev& d);   // the fast loop's exchange interval in force (k_step2d.hip)
void launch_river_s2d(const Dev& d, hipStream_t s, int knew);
// BULK_FRC: calc_all_bulk_forces (k_bulk.hip)
void launch_bulk_flux(const Dev& d, hipStream_t s, int nrhs);
void launch_river_uv(const Dev& d, hipStream_t s, int nnew, int pred);
void launch_v3dbc(const Dev& d, hipStream_t s, const Tlev& t);
void launch_t3dbc(const Dev& d, hipStream_t s, const Tlev& t, int itrc);
// out (device, 6 doubles): avzeta, KE, KE2b sums, Cu_adv, Cu_w, blow-up flag
void launch_diag(const Dev& d, hipStream_t s, const Tlev& t, double* out);
void launch_swr_frac(const Dev& d, hipStream_t s);
constexpr int kKppFcKeepMax = 16;   // most levels above FC(0) in k_kpp_ext's LDS slot: 17 x 64 x 8 B = 8.7 KB per wave
constexpr int kKppPfMax = 4;        // deepest ring of levels in flight k_kpp_ext is compiled for (Params::kpp_pf)
constexpr int kKppPfDefault = 3;     // C3: k_kpp_ext 1.12 -> 0.79 ms per launch with 2, 3 or 4, profiles/r15_kpp_ring_prs_vg_ab.txt
// one_slot (whole steps; taken only where lmd_vmix_one_slot holds): Akt(isalt), bit for bit Akt(itemp) there, is
// neither formed, stored nor exchanged -- the caller answers for nothing reading it before it is made current again
bool lmd_vmix_one_slot(const Dev& d);
void launch_lmd_vmix(const Dev& d, hipStream_t s, const Tlev& t, int tind, bool one_slot = false);
// ADV_ISONEUTRAL (k_iso.hip): prsgrd's corrector slopes (+ their exchange),
// step3d_uv2's diff3u/diff3v/idRz over its flux-correction ranges and their
// exchange, and step3d_t's rotated biharmonic operator for one tracer
void launch_iso_slopes(const Dev& d, hipStream_t s);
void launch_iso_diff3(const Dev& d, hipStream_t s, const Tlev& t, int iu0, int iu1, int iv0, int iv1, int j0, int j1);
void launch_iso_exch_diff3(const Dev& d, hipStream_t s);
void launch_iso_tracer(const Dev& d, hipStream_t s, const Tlev& t, int itrc);

}  // namespace roms
