/*
 * roms_gpu.h -- C ABI of the MI355X-native UCLA-ROMS split-explicit hot path.
 *
 * Drop-in boundary: the reference's hot-path
 * routines are argument-less / (tile) / (tidx) external Fortran subroutines
 * that read and write module arrays (/root/reference/src/main.F:397-479).
 * Each routine below replaces one of them; all state they touch lives in
 * device memory owned by this library, in the reference's Fortran layout
 * (-1:Lm+2, -1:Mm+2 [,levels] [,time] [,tracer]), i fastest.  Host arrays are
 * borrowed only across roms_gpu_register .. roms_gpu_finalize and are copied
 * explicitly with roms_gpu_upload / roms_gpu_download.
 *
 * One process drives one GPU (one MPI rank / one subdomain, like the
 * reference's one rank per tile).  Every entry returns 0 on success and a
 * negative code on failure; roms_gpu_last_error() gives the message (the
 * reference's error_log%raise_* + abort_check, error_handling_mod.F90:144-365).
 * Routine entries enqueue on the library's HIP stream and return immediately;
 * roms_gpu_sync() waits.
 */
#ifndef ROMS_GPU_H
#define ROMS_GPU_H

#ifdef __cplusplus
extern "C" {
#endif

#define ROMS_GPU_ABI_VERSION 34
#define ROMS_MAX_FAST 288

/* Subdomain geometry of this rank: param.F / dimensions.F / mpi_setup.F:39-210 */
typedef struct roms_dims {
  int Lm, Mm, N, NT;             /* local interior size, levels, tracers   */
  int LLm, MMm;                  /* global interior size                   */
  int np_xi, np_eta, inode, jnode;
  int iSW_corn, jSW_corn;        /* offset of this subdomain (mpi_setup.F) */
  int ew_periodic, ns_periodic;  /* EW_PERIODIC / NS_PERIODIC              */
  int west_exchng, east_exchng, south_exchng, north_exchng; /* message edges */
} roms_dims;

/* LMD switch bits of roms_cfg.lmd_mixing / roms_case.lmd_mixing (cppdefs.opt).
 * Accepted sets are the ones the reference builds and runs correctly:
 *   0 (no LMD_MIXING), or MIXING|KPP|BKPP plus any of RIMIX, NONLOCAL,
 *   CONVEC (CONVEC needs RIMIX) and DDMIX (double diffusion, lmd_vmix.F:279-
 *   360; needs SALINITY for t(..,isalt)).  KPP without BKPP does not compile in the
 *   reference (lmd_kpp.F:178 reads hbbl, imported only under LMD_BKPP,
 *   lmd_kpp.F:37-39); MIXING without KPP/BKPP filters Kv(0), Kv(N) that are
 *   never set (lmd_vmix.F:405-420); CONVEC without RIMIX tests an unset Rig
 *   (lmd_vmix.F:269-274).  The Pipes_ana set is ROMS_LMD_ALL, the Iceland
 *   set (Examples/Iceland/Iceland_parent/cppdefs.opt:41-46) ROMS_LMD_ICELAND. */
#define ROMS_LMD_MIXING   1
#define ROMS_LMD_KPP      2
#define ROMS_LMD_BKPP     4
#define ROMS_LMD_RIMIX    8
#define ROMS_LMD_CONVEC   16
#define ROMS_LMD_NONLOCAL 32
#define ROMS_LMD_ALL      63   /* MIXING..NONLOCAL: the Pipes_ana set (no DDMIX) */
#define ROMS_LMD_ICELAND  47   /* all but LMD_CONVEC */
#define ROMS_LMD_DDMIX    64

/* cppdefs.opt switches and run scalars (scalars.F, read_inp_mod.F, set_weights.F).
 * Switches that need no flag here: MASKING is carried by the mask arrays
 * (all-ones masks reproduce a build without it); IMPLICIT_BOTTOM_DRAG is
 * forced on inside step3d_uv1.F:138 / step3d_uv2.F:82 and its only other use
 * (compute_rd_bott_drag.h:41) is masked by IMPLCT_NO_SLIP_BTTM_BC, always
 * defined (set_global_definitions.h:73). */
typedef struct roms_cfg {
  int nonlin_eos;                /* NONLIN_EOS (+SPLIT_EOS)                */
  int salinity;                  /* SALINITY                               */
  int lmd_mixing;                /* 0 or ROMS_LMD_* bits (see above)       */
  int uv_vis2, ts_dif2;          /* UV_VIS2, TS_DIF2                        */
  double dt;                     /* baroclinic step [s]                    */
  int ndtfast, nfast;            /* mode splitting                         */
  double weight[2][ROMS_MAX_FAST]; /* fast-time averaging weights (C order [2][288]) */
  double g, rho0, rdrg, rdrg2, Zob, gamma2;
  double Akv_bak, Akt_bak[2];
  double Tcoef, T0, Scoef, S0;   /* linear EOS                              */
  double theta_s, theta_b, hc;   /* S-coordinate                            */
  int obc;                       /* open edges (OBC_WEST 1, OBC_EAST 2, OBC_SOUTH 4, OBC_NORTH 8) with
                                    OBC_M2FLATHER, OBC_M3ORLANSKI, OBC_TORLANSKI and Z/M2/M3/T_FRC_BRY;
                                    closed walls elsewhere (zetabc.F, u2dbc_im.F ... t3dbc_im.F)  */
  double ubind;                  /* OBC binding velocity [m/s] (scalars.F, read_inp_mod.F:809)    */
  int curvgrid;                  /* CURVGRID (with UV_ADV): curvature terms in the momentum r.h.s. */
  int uv_adv, uv_cor;            /* UV_ADV (horizontal + vertical momentum advection,
                                    compute_horiz_rhs_uv_terms.h:42-291, compute_vert_rhs_uv_terms.h),
                                    UV_COR (Coriolis, compute_horiz_rhs_uv_terms.h:1-38)              */
  int pot_tides;                 /* TIDES with pot_tides (tides.opt): the surface tidal potential
                                    ptide enters the pressure gradient (prsgrd.F:209-211)             */
  int bulk_frc;                  /* BULK_FRC: the surface fluxes come from roms_gpu_bulk_flux (COARE,
                                    bulk_frc.F:143-913) at both set_forces points of the step, and
                                    lmd_kpp's u* from the rho-point stresses (lmd_kpp.F:173-174)     */
  int adv_isoneutral;            /* ADV_ISONEUTRAL (with SW_TRIADS and STABILIZE, step3d_t_ISO.F:15-18):
                                    corrector prsgrd forms the slopes dRdx/dRde (prsgrd.F:307-338),
                                    step3d_uv2 diff3u/diff3v/idRz (step3d_uv2.F:572-697), step3d_t
                                    centred (not UPSTREAM_TS) fluxes, the rotated biharmonic operator
                                    and Akt+Akz in the implicit diffusion (step3d_t_ISO.F:253-1065)  */
} roms_cfg;

/* Time-step indices (scalars.F:32-36).  The step entry updates them. */
typedef struct roms_tlev {
  int iic, ntstart, forw_start, iif, nfast, kstp, knew, nstp, nrhs, nnew;
} roms_tlev;

/* Field identifiers: the reference's module arrays (names as in the source) */
enum roms_field {
  ROMS_ALL = -1,
  /* grid.F */
  ROMS_h = 0, ROMS_hinv, ROMS_f, ROMS_fomn, ROMS_pm, ROMS_pn, ROMS_dm_r, ROMS_dn_r, ROMS_dm_u, ROMS_dn_u,
  ROMS_dm_v, ROMS_dn_v, ROMS_dm_p, ROMS_dn_p, ROMS_pmon_u, ROMS_pnom_v, ROMS_rmask, ROMS_pmask, ROMS_umask,
  ROMS_vmask,
  /* scoord.F (N+1 each) */
  ROMS_Cs_w, ROMS_Cs_r,
  /* ocean_vars.F, tracers.F */
  ROMS_zeta, ROMS_ubar, ROMS_vbar, ROMS_u, ROMS_v, ROMS_t, ROMS_FlxU, ROMS_FlxV, ROMS_We, ROMS_Wi,
  ROMS_Hz, ROMS_Hz_u, ROMS_Hz_v, ROMS_z_r, ROMS_z_w,
  /* coupling.F */
  ROMS_rufrc, ROMS_rvfrc, ROMS_rhoA, ROMS_rhoS, ROMS_r_D, ROMS_Zt_avg1, ROMS_DU_avg1, ROMS_DV_avg1,
  ROMS_DU_avg2, ROMS_DV_avg2, ROMS_DU_avg_bak, ROMS_DV_avg_bak,
  /* eos_vars.F, mixing.F */
  ROMS_rho, ROMS_rho1, ROMS_qp1, ROMS_bvf, ROMS_Akv, ROMS_Akt, ROMS_visc2_r, ROMS_visc2_p, ROMS_diff2,
  ROMS_hbls, ROMS_hbbl, ROMS_ghat, ROMS_swr_frac,
  /* surf_flux.F */
  ROMS_sustr, ROMS_svstr, ROMS_stflx, ROMS_srflx, ROMS_swflx,
  /* private scratch carried between routines (prsgrd -> pre_step3d/step3d_uv1) */
  ROMS_ru, ROMS_rv,
  /* boundary.F:21-39 open-boundary data: *_west/_east indexed j=0:Mm+1, *_south/_north i=0:Lm+1;
     u,v (.,N); t (.,N,NT) -- column-major like the reference allocations (boundary.F:111-129) */
  ROMS_zeta_west, ROMS_zeta_east, ROMS_zeta_south, ROMS_zeta_north,
  ROMS_ubar_west, ROMS_ubar_east, ROMS_ubar_south, ROMS_ubar_north,
  ROMS_vbar_west, ROMS_vbar_east, ROMS_vbar_south, ROMS_vbar_north,
  ROMS_u_west, ROMS_u_east, ROMS_u_south, ROMS_u_north,
  ROMS_v_west, ROMS_v_east, ROMS_v_south, ROMS_v_north,
  ROMS_t_west, ROMS_t_east, ROMS_t_south, ROMS_t_north,
  /* grid.F CURVGRID metric derivatives d(1/n)/dxi, d(1/m)/deta (setup_grid1.F:89-103) */
  ROMS_dndx, ROMS_dmde,
  /* tides.F:26 surface tidal potential [m] (TIDES, pot_tides) */
  ROMS_ptide,
  /* BULK_FRC inputs at rho points (bulk_frc.F:95-111, surf_flux.F): winds [m/s], air temperature
     [degC], specific humidity Q [kg/kg], precipitation [cm/day], short-wave (the data read into
     srflx) and downward long-wave radiation [W/m2]; and the rho-point stresses sustr_r, svstr_r */
  ROMS_uwnd, ROMS_vwnd, ROMS_tair, ROMS_qair, ROMS_prate, ROMS_swrad, ROMS_lwrad, ROMS_sustr_r, ROMS_svstr_r,
  /* ADV_ISONEUTRAL (eos_vars.F:28-31, mixing.F:24-27): the slopes dRdx, dRde (N) of the corrector prsgrd, the
     limited inverse stratification idRz (0:N) and the roots of the hyperdiffusivities diff3u, diff3v (N) of
     step3d_uv2, and step3d_t's stabilising diffusivity Akz (0:N), a private scratch array of the reference.
     They exist with roms_cfg.adv_isoneutral only: otherwise their size is 0 and every transfer of them fails. */
  ROMS_dRdx, ROMS_dRde, ROMS_idRz, ROMS_diff3u, ROMS_diff3v, ROMS_Akz,
  ROMS_NFIELDS
};

/* ---- lifecycle ---- */
int  roms_gpu_abi_version(void);
/* Allocates device state (the only allocating entry).  device: HIP device
 * ordinal; comm: handle from roms_gpu_comm_create / _create_local for a
 * processor grid np_xi*np_eta > 1 (rank = inode + jnode*np_xi, as
 * mpi_setup.F:60-61), NULL for a single rank, whose periodic halos are
 * wrapped on-device.                                                        */
int  roms_gpu_init(const roms_dims *dims, const roms_cfg *cfg, int device, void *comm);
int  roms_gpu_finalize(void);
const char *roms_gpu_last_error(void);
/* element count of a field in the Fortran layout of this rank */
long roms_gpu_field_size(int field_id);
/* host mirror for upload/download (init_arrays.F; host keeps ownership)     */
int  roms_gpu_register(int field_id, double *host_ptr, long count);
int  roms_gpu_upload(int field_id);      /* host -> device, ROMS_ALL allowed */
int  roms_gpu_download(int field_id);    /* device -> host, ROMS_ALL allowed */
/* direct synchronous copies without registration                            */
int  roms_gpu_copy_in(int field_id, const double *src, long count);
int  roms_gpu_copy_out(int field_id, double *dst, long count);
/* ROMS_Hz_u / ROMS_Hz_v (set_HUV's cell heights, set_depth.F:220,227) are
 * read by no routine of the step, only by extract_data.F:726.  roms_gpu_step
 * stores them only while either is registered for transfer or the
 * environment sets ROMS_GPU_HZ_UV=1 (2 array passes per step saved); after a
 * step that did not, downloading or copying them out returns -5.  The
 * routine roms_gpu_set_huv always stores them. */
int  roms_gpu_sync(void);
void *roms_gpu_stream(void);             /* hipStream_t the routines run on  */

/* ---- hot-path routines (reference entry points they replace) ---- */
int roms_gpu_rho_eos(int tidx, const roms_tlev *t);   /* rho_eos(tidx)   rho_eos.F:6      */
int roms_gpu_set_huv(const roms_tlev *t);             /* set_HUV          set_depth.F:190  */
int roms_gpu_omega(const roms_tlev *t);               /* omega            omega.F:4        */
int roms_gpu_lmd_vmix(int tind, const roms_tlev *t);  /* lmd_vmix(tind)   lmd_vmix.F:5     */
int roms_gpu_prsgrd(const roms_tlev *t);              /* prsgrd           prsgrd.F:4       */
int roms_gpu_pre_step3d(const roms_tlev *t);          /* pre_step3d(tile) pre_step3d4S.F:4 */
int roms_gpu_set_huv1(const roms_tlev *t);           /* set_HUV1(tile)   set_depth.F:239  */
int roms_gpu_step3d_uv1(const roms_tlev *t);          /* step3d_uv1(tile) step3d_uv1.F:5   */
int roms_gpu_visc3d(const roms_tlev *t);              /* visc3d           visc3d_S.F:4     */
int roms_gpu_step2d(const roms_tlev *t);              /* step2d           step2d_FB.F:3    */
int roms_gpu_step3d_uv2(const roms_tlev *t);          /* step3d_uv2(tile) step3d_uv2.F:6   */
int roms_gpu_step3d_t(const roms_tlev *t);            /* step3d_t(tile)   step3d_t_ISO.F:20*/
int roms_gpu_t3dmix(const roms_tlev *t);              /* t3dmix           t3dmix_S.F:4     */
int roms_gpu_swr_frac(const roms_tlev *t);            /* swr_frac(tile)   lmd_swr_frac.F:4 */
/* set_pipe_frc (pipe_frc.F:33-80): the host's pipe_idx (0 = no pipe) and
 * pipe_flx on the (-1:Lm+2,-1:Mm+2) grid, pipe_prf(npip,N) and
 * pipe_trc(npip,NT) column-major.  npip = 0 switches pipe sources off.
 * Call again whenever set_forces updates them; the next step uses them.      */
int roms_gpu_set_pipe_frc(int npip, const int *pipe_idx, const double *pipe_flx, const double *pipe_prf,
                          const double *pipe_trc);
/* set_river_frc (river_frc.F:57-96, init_river_frc :98-222, calc_river_flux
 * :224-282): riv_uflx and riv_vflx as calc_river_flux leaves them on the
 * (-1:Lm+2,-1:Mm+2) grid (10*iriver + the signed flux fraction on every face
 * between a river-mouth cell and a wet neighbour, 0 elsewhere), riv_vol(nriv)
 * [m3/s] and riv_trc(nriv,NT) column-major for the current time.  Passing
 * riv_uflx = riv_vflx = NULL keeps the face arrays of an earlier call and
 * updates only the time-dependent riv_vol/riv_trc.  nriv = 0 switches river
 * sources off.  Returns 0, or -1 on a bad argument. */
int roms_gpu_set_river_frc(int nriv, const double *riv_uflx, const double *riv_vflx, const double *riv_vol,
                           const double *riv_trc);
/* set_bulk_frc -> calc_all_bulk_forces (bulk_frc.F:85-913) on the device:
 * from the uploaded ROMS_uwnd .. ROMS_lwrad fields and the surface t, u, v at
 * t->nrhs, sets srflx, stflx(itemp), swflx, sustr_r, svstr_r, sustr and
 * svstr.  roms_gpu_step calls it itself at both set_forces points when the
 * library was initialised with bulk_frc; the host only uploads the
 * time-interpolated atmospheric fields (set_frc_data) before each step.
 * Returns -4 when the library was initialised without bulk_frc. */
int roms_gpu_bulk_flux(const roms_tlev *t);
/* SPONGE_TUNE with ub_tune (sponge_tune.F, t3dbc_im.F:73-74): the per-edge
 * binding coefficients ub_west(j), ub_east(j) (j = 0..Mm+1) and ub_south(i),
 * ub_north(i) (i = 0..Lm+1) that the host's adjust_orlanski maintains from
 * the parent/child baroclinic pressure fluxes; t3dbc's Orlanski blend then
 * uses cext = max(cext, min(ub(j), 1)).  NULL switches an edge off (the
 * reference default ub_tune = .false., sponge_tune.opt).  Call again after
 * every adjust_orlanski; the next step uses the new values.                 */
int roms_gpu_set_ub_tune(const double *ub_west, const double *ub_east, const double *ub_south, const double *ub_north);
int roms_gpu_set_depth(const roms_tlev *t);           /* set_depth(tile)  set_depth.F:4    */

/* One whole roms_step (main.F:333-520, forcing held fixed): advances t->iic
 * and leaves nstp/nrhs/nnew/kstp/knew as the reference does.  Steady-state
 * steps replay a captured HIP graph.                                        */
int roms_gpu_step(roms_tlev *t);
/* roms_init device sequence after the host uploaded grid + initial state:
 * set_depth, set_HUV, omega, rho_eos(nrhs) (main.F:268-288).                 */
int roms_gpu_init_sequence(roms_tlev *t);

/* ---- analytic cases (host-side ana_grid/ana_init restatements) ---- */
enum roms_case_id { ROMS_CASE_FILAMENT = 0, ROMS_CASE_BASIN = 1, ROMS_CASE_PIPES = 2, ROMS_CASE_RIVERS = 3 };
typedef struct roms_case {
  int case_id, LLm, MMm, N, NT;
  int salinity, nonlin_eos, lmd_mixing;  /* lmd_mixing: 0 or ROMS_LMD_* bits */
  double dt; int ndtfast;
  double sizex, sizey;
  int surf_flux;  /* basin only: analytic cooling, short-wave and salt fluxes (else 0) */
  int obc;        /* basin only: open edges (roms_cfg.obc) with analytic boundary data, ubind 0.1 */
  double v_sponge;/* basin only: SPONGE band viscosity/diffusivity [m2/s] (set_nudgcof.F)      */
  int island;     /* basin only: circular land mask (MASKING)                                   */
  int curvgrid;   /* basin only: non-uniform metrics pm(j), pn(i) and CURVGRID                  */
  int uv_adv, uv_cor;  /* UV_ADV, UV_COR (every reference case defines both: set 1, 1)          */
  int bulk_frc;   /* basin only: BULK_FRC with an analytic atmosphere (westerly jet, cool humid air)
                     uploaded as ROMS_uwnd .. ROMS_lwrad; roms_cfg.bulk_frc                         */
  int adv_isoneutral;  /* ADV_ISONEUTRAL (roms_cfg.adv_isoneutral), any case                            */
} roms_case;
/* Builds the analytic grid/ICs on the host (setup_grid1/2, set_scoord,
 * set_weights, ana_init), initialises the device and runs roms_init.        */
int roms_gpu_init_case(const roms_case *c, int device, roms_tlev *t);
/* Same on this rank's subdomain of an np_xi x np_eta processor grid
 * (mpi_setup.F:39-154 bounds); comm's rank selects inode,jnode.             */
int roms_gpu_init_case_comm(const roms_case *c, int np_xi, int np_eta, void *comm, int device, roms_tlev *t);

/* ---- communicators for the halo exchange (mpi_exchanges.F) ----
 * RCCL: rank 0 calls roms_gpu_comm_unique_id, the 128-byte id is broadcast
 * by the host's own means (MPI_Bcast in a Fortran driver, torch.distributed
 * in the Python one), then every rank calls roms_gpu_comm_create.
 * _create_local: subdomains driven by threads of ONE process (testing).     */
int roms_gpu_comm_unique_id(void *id128);
int roms_gpu_comm_create(const void *id128, int nranks, int rank, int device, void **comm);
int roms_gpu_comm_create_local(int group, int nranks, int rank, void **comm);
/* Host channel: the host supplies its own allgather (every rank calls it
 * with the same nbytes; recv holds nranks * nbytes, rank r's bytes at
 * r * nbytes; returns 0 on success) -- MPI_Allgather(MPI_BYTE) over the
 * reference's communicator (mpi_exchanges.F, mpi_setup.F), a file or socket
 * channel in a test.  It carries only the IPC handles at init and the small
 * diag / area-volume gathers; every halo exchange moves GPU to GPU by IPC
 * peer writes, with RCCL out of the loop.  roms_gpu_init fails if the IPC
 * transport cannot be set up (its self-test reference is a host-staged
 * exchange over the same channel).                                          */
typedef int (*roms_host_allgather_fn)(void *ctx, const void *send, long nbytes, void *recv);
int roms_gpu_comm_create_host(int nranks, int rank, int device, roms_host_allgather_fn allgather, void *ctx,
                              void **comm);
int roms_gpu_comm_destroy(void *comm);
/* Halo transport of this rank after roms_gpu_init: 0 = RCCL send/recv (or
 * single rank / in-process), 1 = IPC peer writes (RCCL communicator: enabled
 * after a start-up self-test against RCCL, ROMS_GPU_HALO_IPC=0 disables;
 * host-channel communicator: always), -1 = IPC with a timed-out arrival wait
 * since init.                                                               */
int roms_gpu_halo_transport(void);
/* Halo exchanges (one reference exchange_xxx call each) in the last whole
 * step this rank enqueued (eager or graph capture; 0 on one rank without a
 * communicator), and the fast-loop exchange interval: the barotropic loop
 * exchanges zeta/ubar/vbar after every *fast_interval-th fast step over
 * 2*fast_interval-deep halos and recomputes the overlap in between (1: every
 * fast step, as step2d_FB.F:572-574; multi-rank runs without open edges
 * default to 4, ROMS_GPU_S2D_K=1..8; K is lowered until 2K+2 fits the
 * smallest subdomain of the mpi_setup.F split, the same on every rank;
 * with rivers or pipes on every fast step exchanges, and 1 is reported).      */
int roms_gpu_halo_exchanges(long *per_step, int *fast_interval);
/* 1 if whole steps defer each producer's 3-D exchange onto the halo stream
 * beside the next routine that reads none of its halo (the default with
 * > 1 rank when every rank drives its own GPU; ROMS_GPU_XOVERLAP=1 forces
 * it on, =0 off), 0 if every exchange runs in place, as the reference's
 * exchange_xxx calls do (mpi_exchanges.F:672-800).                          */
int roms_gpu_halo_overlap(void);
/* 1 if the fused fast step addresses its 2-D fields through one buffer
 * window (the fields allocated side by side within 2 GiB; the default),
 * 0 if through their pointers (ROMS_GPU_S2D_WIN=0, or a subdomain whose
 * 2-D fields span more).  Same results either way.                         */
int roms_gpu_s2d_window(void);
/* Which vertical column solvers this model runs, chosen at init from N:
 * bit 0 (ROMS_COLPATH_SEG): the segment-partitioned solvers (default where
 * the sequential solvers' LDS columns no longer fit and every segment gets
 * its minimum of rows; ROMS_GPU_COLSEG=0/1 forces either where N allows);
 * bit 1 (ROMS_COLPATH_GLOBAL): the sequential solvers' column scratch lives
 * in global memory instead of LDS (default for N >= 64;
 * ROMS_GPU_COL_GLOBAL=0/1).  Negative before init.                        */
#define ROMS_COLPATH_SEG 1
#define ROMS_COLPATH_GLOBAL 2
int roms_gpu_column_path(void);
/* lmd_vmix leaves out work past the boundary layers; the fields are bitwise
 * those of the full forms.  ROMS_GPU_KPP_LEAN (read at init) is a mask of the
 * three parts, default 7, 0 for the full forms:
 *   1  k_kpp_ext forms Vtsq (and loads the swr_frac that feeds it) only
 *      until every column of the wavefront has its surface layer index kbls;
 *   2  k_kpp_ext keeps FC(0:keep) of the bulk Richardson integral in LDS at
 *      every N instead of the whole column FC(0:N) (in global scratch at
 *      N >= 64); keep = ROMS_GPU_KPP_FCKEEP, 1..16, default 16.  A
 *      wavefront with a bottom layer reaching above level keep repeats the
 *      FC sweep for the levels above;
 *   4  k_kpp_int's kbls scan stops at the first level outside the layer.
 * Returns mask + 256 * keep of the live model, negative before init.       */
int roms_gpu_kpp_lean(void);
/* Levels in flight in k_kpp_ext's descending sweep (ABI 24).  The sweep loads
 * the inputs of ROMS_GPU_KPP_PF levels (read at init, 1..4, default 3) ahead
 * of the level it forms; 1 is the single level ahead at three waves per SIMD,
 * 2..4 run at two.  A value outside 1..4 counts as 1.  Same values, same
 * expressions: every field keeps its bits.  Returns the value of the live
 * model, negative before init.                                              */
int roms_gpu_kpp_pf(void);
/* Hz, z_r, z_w formed inside the kernels.  The three arrays are functions of
 * the free surface set_depth used, h, hinv and the Cs tables; the kernels of
 * ROMS_GPU_VGRID (read at init; a mask, default 11, 0 for the streaming forms)
 * form a column's levels from those instead of streaming the arrays, with
 * set_depth's own expressions, so every field keeps its bits:
 *   1  k_rho_eos_split     2  k_kpp_ext     4  k_kpp_int     8  k_set_huv
 * (k_kpp_int measured slower with it and is off by default).
 * They do so only while the stored arrays are set_depth's own: every
 * set_depth (roms_gpu_set_depth, roms_gpu_init_sequence, the last fast step)
 * makes the grid valid; writing Hz, z_r, z_w, h, hinv, Cs_w or Cs_r from the
 * host (roms_gpu_copy_in, roms_gpu_upload) makes it invalid, and every kernel
 * streams the arrays again until the next set_depth -- a host that supplies
 * its own Hz keeps the reference's semantics.
 * roms_gpu_vgrid returns mask + 256 * valid, negative before init.
 * ROMS_GPU_VGRID2 (read at init; a mask, default 31, 0 for the streaming forms) is the same switch, under
 * the same validity, for further kernels that walk a column or stage a level:
 *   1  k_omega_seg   2  k_set_huv1_chain   4  k_uv2_fused   8  k_visc3d_stg
 *   16 k_t3dmix_stg
 * roms_gpu_vgrid2 returns that mask + 256 * valid, negative before init.
 * roms_gpu_vgrid_check compares the stored z_w, z_r, Hz with the values formed
 * from the kept surface as bit patterns, over set_depth's range and the
 * exchanged or wrapped halos; out[0..2] = mismatches of z_w, z_r, Hz (all 0
 * whenever the grid is valid).                                              */
int roms_gpu_vgrid(void);
int roms_gpu_vgrid2(void);
int roms_gpu_vgrid_check(long out[3]);
/* T and S in one block of the tracer segment solvers (ABI 22).
 * Without LMD_DDMIX and with Akt_bak[0], Akt_bak[1] the same bits, lmd_vmix
 * leaves Akt(isalt) bit for bit Akt(itemp), so the two tracers' vertical
 * systems are one matrix with two right-hand sides.  The kernels of
 * ROMS_GPU_T_PAIR (read at init; a mask, default 3, 0 for one block per
 * tracer) then load and factorise it once for both (NT = 2, buffer segment
 * path), every field keeping its bits:
 *   1  k_pre_tracer_segb_pair (pre_step3d)   2  k_step3d_t_segb_pair (step3d_t)
 * They do so only while that equality is known: every lmd_vmix (the routine,
 * or inside a whole step) establishes it under the conditions above; writing
 * Akt from the host (roms_gpu_copy_in, roms_gpu_upload) ends it until the next
 * lmd_vmix, and pre_step3d or step3d_t called on its own after such a write
 * uses the host's Akt(isalt) for S, one block per tracer.
 * roms_gpu_tracer_pair returns mask + 256 * (equality known), negative before
 * init; launches[0], launches[1] (if not NULL) get the pair-form launches of
 * pre_step3d and of step3d_t this host thread enqueued since init (a replayed
 * graph counts those of its capture).                                        */
int roms_gpu_tracer_pair(long launches[2]);
/* Stores of a whole step that nothing in the step reads (ABI 28).
 * ROMS_GPU_LEAN_ST (read at init; a mask, default 3, 0 for every store):
 *   1  pre_step3d's u, v(indx) = Hz*u(nstp): on the buffer segment path
 *      (N = 88..104, UV_ADV) roms_gpu_step's predictor does not store them and
 *      its step3d_uv1, their one reader, forms each value again from the same
 *      Hz and u(nstp) with the same expression, so every field keeps its bits
 *      and after the step u, v(indx) hold what step3d_uv1 left there, as before.
 *      The routine entries roms_gpu_pre_step3d and roms_gpu_step3d_uv1 always
 *      store and load u, v(indx).
 *   2  Akt(isalt): where lmd_vmix leaves it bit for bit Akt(itemp) (no
 *      LMD_DDMIX, equal Akt_bak) and both tracer solvers of the step are the
 *      pair kernels (ROMS_GPU_T_PAIR = 3, NT = 2, buffer segment path, no
 *      ADV_ISONEUTRAL), roms_gpu_step's lmd_vmix neither forms, stores nor
 *      exchanges it.  The library copies Akt(itemp) over it, halos and edge
 *      points included, before anything reads it: roms_gpu_copy_out and
 *      roms_gpu_download of Akt, roms_gpu_calc_avg and roms_gpu_wrt_his with
 *      ROMS_WRT_AKS, roms_gpu_pre_step3d and roms_gpu_step3d_t.  The host sees
 *      Akt as before.  A host write of Akt is kept as written; roms_gpu_lmd_vmix
 *      as a routine always stores both slots.
 * roms_gpu_lean_stores returns the mask, negative before init; launches[0],
 * launches[1] (if not NULL) get the pre_step3d and the lmd_vmix launches this
 * host thread enqueued since init that left their store out (a replayed graph
 * counts those of its capture).                                             */
int roms_gpu_lean_stores(long launches[2]);
/* The horizontal tracer kernels of pre_step3d and step3d_t as level walks
 * (ABI 23).  With two tracers the kernels of ROMS_GPU_T_HSTG (read at init; a
 * mask, default 7 with the segment solvers and 2 with the column solvers of
 * N <= 63, 0 for one block per 64x4 tile and level) run one block per
 * 64x8 cells over all levels: the lane's masks, pm, pn once per block, each
 * level's FlxU, FlxV, T, S windows staged in LDS with the next level's in
 * flight and half the halo rows of the 64x4 tiles, every field keeping its
 * bits:
 *   1  k_pre_tracer_stg (pre_step3d)   2  k_step3d_t_stg (step3d_t)
 *   4  k_pre_tracer_stg forms Hz from the kept free surface instead of
 *      reading it, while the grid is valid (roms_gpu_vgrid)
 * NT = 1 keeps the per-level kernels.
 * roms_gpu_tracer_hstg returns mask + 256 * (grid valid), negative before
 * init; launches[0..2] (if not NULL) get the launches of k_pre_tracer_stg, of
 * k_step3d_t_stg and of the k_pre_tracer_stg that formed Hz which this host
 * thread enqueued since init (a replayed graph counts those of its capture). */
int roms_gpu_tracer_hstg(long launches[3]);
/* Which horizontal paths this rank's model runs, chosen from Lm, Mm, its
 * edges and the ROMS_GPU_* switches by the same host functions the launchers
 * call:
 *   out[0]  the fast step's closed-edge mode: 0 no closed or open edge on
 *           this rank, 1 separate edge launches (k_s2d_edges), 2 the closed
 *           walls folded into the fused fast step;
 *   out[1]  1 if the prsgrd calls of a whole step take the j-marching strips
 *           (k_prsgrd_strip) for some rows, 0 if tiles everywhere;
 *   out[2]  strips per row (each owns 60 columns), 0 without strips;
 *   out[3], out[4]  first and last strip row jA, jB (0, -1 without strips;
 *           the other rows of 1..Mm run in tiles);
 *   out[5]  1 if omega takes the segment form (k_omega_seg: 32 columns or
 *           more and N within the segment solvers' depth), 0: two-pass k_omega;
 *   out[6]  the closed-edge modes the fast steps of the last enqueued whole
 *           step took (eager or graph capture; plus those of any
 *           roms_gpu_step2d call since): bit m set if some fast step ran
 *           mode m of out[0]; 0 before the first step.  out[0] is the mode
 *           on this rank's own bounds.  A multi-rank fast loop with an
 *           exchange interval K > 1 (roms_gpu_halo_exchanges) widens each
 *           fast step's bounds by 2(K-m) cells on every rank boundary and
 *           decides the fold on the widened bounds, so a rank with an east
 *           or a north wall and none opposite can take 1 and 2 in turn;
 *   out[7]  reserved, 0.
 * Negative before init.                                                   */
int roms_gpu_horizontal_path(int out[8]);
/* Self-test of the allocation path: `chunks` arrays of n doubles filled
 * with ones and freed, then allocated again through the library's
 * zero-filling allocator; on the library's stream each is read at once
 * (elements not zero: stale data) and overwritten with ones, and after the
 * device drains the elements not one are counted (writes undone by a late
 * fill).  *bad = both counts (0 unless the null-stream fill races the
 * library's non-blocking stream, the round-2 failure mode).                 */
int roms_gpu_selftest_zero_fill(long n, int chunks, long *bad);
/* Host-only: neighbour ranks (-1 none), per-level message sizes for the 8
 * directions W,E,S,N,SW,SE,NW,NE, and the strip extents {i0,i1,j0,j1}.      */
int roms_gpu_halo_plan(int Lm, int Mm, int np_xi, int np_eta, int inode, int jnode, int ew_periodic,
                       int ns_periodic, int peer[8], long count[8], int strip[4]);
/* Host-only: the (i,j) cells, in message order, that direction dir packs
 * (unpack=0, from this rank's interior) or unpacks into (unpack=1, halo).
 * Returns the per-level count (<= cap) or -1.                               */
long roms_gpu_halo_map(int Lm, int Mm, int np_xi, int np_eta, int inode, int jnode, int ew_periodic,
                       int ns_periodic, int dir, int unpack, int *i, int *j, long cap);
/* Host-only: roms_gpu_halo_map for a `width`-deep exchange (2: the
 * reference's halo, as roms_gpu_halo_map; 2K: the fast loop's swap every K
 * fast steps, roms_gpu_halo_exchanges).  width <= Lm, Mm.                   */
long roms_gpu_halo_map_wide(int Lm, int Mm, int np_xi, int np_eta, int inode, int jnode, int ew_periodic,
                            int ns_periodic, int width, int dir, int unpack, int *i, int *j, long cap);

/* ---- forcing and boundary producers on the device (set_forces.F,
 * set_frc_data roms_read_write.F:303-392, set_bry_all boundary.F:227,
 * set_tides tides.F:86-254) ----
 * roms_gpu_frc_record uploads one record (time rec_time in days, like the
 * reference's forcing times) of a field into record slot 0, 1 or 2 (ABI 13:
 * a third slot); the host uploads a record only when the model time leaves
 * the window of those it holds (as fill_frc_slice does).  At a model time
 * modtime the pair (it1, it2) is the one set_frc_data would hold: the
 * earliest consecutive pair of the loaded records, in time order, whose
 * later time is >= modtime (the reference refreshes to (it2, next record)
 * once times(it2) < modtime, roms_read_write.F:341-350).  A modtime past
 * every loaded record fails with -8 before anything is queued (load the
 * next record first).  roms_gpu_frc_interp forms every field holding two or
 * more records, of the kinds in `kinds` (ROMS_FRC_SURFACE: 2-D
 * surface/atmospheric fields, ROMS_FRC_BRY: the *_west.._north boundary
 * arrays), as cff1*rec(it1) + cff2*rec(it2) at modtime [days], with
 * set_frc_data's out-of-window error (-1).  roms_gpu_set_tide_data hands over
 * the tidal constituents (frequencies ftide [1/s]; potential and boundary
 * elevation/velocity real/imaginary parts, ntides x the field layout,
 * column-major like the reference's (GLOBAL_2D_ARRAY, ntides) arrays; NULL
 * pairs switch that part off); roms_gpu_set_tides(time) then sets ptide
 * (pot_tides) and adds the tides to the open-boundary zeta/ubar/vbar data
 * (bry_tides) at omT = ftide*(time + dt/2), as set_tides_tile does.       */
#define ROMS_FRC_SURFACE 1
#define ROMS_FRC_BRY     2
int roms_gpu_frc_record(int field_id, int slot, double rec_time, const double *data);
int roms_gpu_frc_interp(double modtime, int kinds);
/* In-step forcing: with on = 1, every roms_gpu_step interpolates each field
 * that holds two records at the reference's own points of roms_step, with
 * time = start_time + dt*(iic - ntstart) [s] (main.F:373): surface fields at
 * frc_time 'current' before the first set_forces work (BULK_FRC flux), the
 * open-boundary data at '1/2 fwd' followed by set_tides, surface fields at
 * '1/2 fwd' before the second set_forces, boundary data at 'forward' (from
 * tdays = time + dt/2) followed by set_tides (main.F:384-441,
 * roms_read_write.F:330-336).  The weights are formed on the host per step
 * and read by the step graph from device memory; each of the four points
 * picks its own record pair, so with three records loaded a refresh that
 * falls inside a step (t2 between the '1/2 fwd' and 'forward' points) is
 * reproduced.  A step with any point past a field's last record fails with
 * -8, one outside the window (roms_read_write.F:381-388) with -1, both
 * before anything is queued; with boundary tides on, every open side's
 * zeta/ubar/vbar data must hold two records (set_bry_all re-sets them before
 * each set_tides).  on = 0: the host interpolates (roms_gpu_frc_interp).  */
int roms_gpu_frc_clock(double start_time, int on);
int roms_gpu_set_tide_data(int ntides, const double *ftide, const double *pot_re, const double *pot_im,
                           const double *ztide_re, const double *ztide_im, const double *utide_re,
                           const double *utide_im, const double *vtide_re, const double *vtide_im);
int roms_gpu_set_tides(double time);

/* ---- on-disk formats: partitioned netCDF restart and history files ----
 * One file per rank, as the reference's PARALLEL_FILES build writes them
 * (file name chosen by the host: roms_read_write.F:1389-1447 appends the date
 * and the rank), in the netCDF classic 64-bit-offset format (nf90_open reads
 * it like the reference's own netCDF-4 files), with the reference's
 * dimensions (xi_rho, xi_u, eta_rho, eta_v, s_rho, s_w, time, auxil),
 * variables, attributes and 'partition' global attribute.
 * roms_gpu_wrt_rst replaces wrt_restart_file (basic_output.F:568-682): it
 * writes record rec (1-based; rec 1 creates the file, def_vars_rst_ocean_vars
 * :873-1034) with ocean_time = time, time_step = (t->iic, rec, total_rec, 0,
 * 0, 0), zeta/ubar/vbar(knew), u/v/tracers(nnew), the EXACT_RESTART
 * DU/DV_avg1/avg2/avg_bak, hbls/hbbl (LMD) and riv_umask/riv_vmask.
 * roms_gpu_wrt_his replaces wrt_his_ocean_vars (:273-419) for the fields in
 * wrt_mask (ocean_vars.opt wrt_* switches).  Both snapshot the record on the
 * device, in stream order, and return; the PCIe copy and the file write run
 * behind the next steps.  roms_gpu_io_wait joins the pending write and
 * returns its status.  roms_gpu_get_init replaces get_init (get_init.F): see
 * rst_io.hip for the EXACT_RESTART protocol (call it with tindx 2 on record
 * rec-1, then tindx 1 on rec, then roms_gpu_init_sequence).  With LMD,
 * roms_gpu_swr_frac must have run once at rest (after roms_gpu_set_depth
 * on zeta = 0, main.F:216-220) before get_init; init_sequence fails
 * otherwise.  After a negative return of get_init the fields it had read
 * are already replaced: the model state is invalid until re-initialised.    */
#define ROMS_WRT_Z    1
#define ROMS_WRT_UB   2
#define ROMS_WRT_VB   4
#define ROMS_WRT_U    8
#define ROMS_WRT_V    16
#define ROMS_WRT_T    32     /* all tracers (tracers.opt wrt_t)              */
#define ROMS_WRT_R    64     /* rho1 (SPLIT_EOS) or rho                      */
#define ROMS_WRT_O    128    /* omega = pm*pn*(We+Wi), m/s (basic_output.F:374-384) */
#define ROMS_WRT_AKV  256
#define ROMS_WRT_AKT  512
#define ROMS_WRT_AKS  1024
#define ROMS_WRT_HBLS 2048
#define ROMS_WRT_HBBL 4096
#define ROMS_WRT_W    8192   /* true vertical velocity w at rho points, m/s (wvlcty.F; wrt_W, wrt_avg_W) */
#define ROMS_WRT_DEFAULT 63  /* Z, Ub, Vb, U, V + tracers; the callers choose the rest (ocean_vars.opt also
                                sets wrt_avg_W: an averages file like the reference's default arms ROMS_WRT_W) */
int roms_gpu_wrt_rst(const char *path, int rec, int total_rec, double time, const roms_tlev *t);
int roms_gpu_wrt_his(const char *path, int rec, int total_rec, double time, const roms_tlev *t, int wrt_mask);
int roms_gpu_io_wait(void);
/* ---- time-averaged output on the device (ABI 25): calc_avg_ocean_vars
 * (basic_output.F:1036-1118, tracers.F:252-269) and wrt_avg_ocean_vars
 * (:421-515).  Averaging is off until roms_gpu_avg_begin arms it, and
 * roms_gpu_step never samples by itself: the host owns `time`, so it calls
 * roms_gpu_calc_avg after each step, as main.F:486 does.
 * roms_gpu_avg_begin allocates one running mean per field of wrt_mask
 * (ROMS_WRT_* bits; AKS without salinity and HBLS/HBBL without LMD are dropped
 * silently, as roms_gpu_wrt_his drops them), each the size of one slot of its
 * field, and sets navg = 0, t_avg = 0.  Mask 0 disarms and frees; calling it
 * again re-arms from scratch; roms_gpu_finalize frees.
 * roms_gpu_calc_avg takes one sample on the library stream (one kernel launch
 * whatever the mask and NT): navg += 1, coef = 1/navg,
 *   t_avg = t_avg*(1-coef) + time*coef,  X_avg = X_avg*(1-coef) + X*coef
 * with X = zeta/ubar/vbar(t->knew), u/v/tracers(t->nstp), rho1 - qp1*z_r
 * (SPLIT_EOS) or rho, We + Wi, Akv, Akt(itemp), Akt(isalt), hbls, hbbl, and w
 * (ROMS_WRT_W, ABI 29, below: a second launch).
 * u, v and the tracers are sampled in slot nstp, NOT nnew: after a step nstp
 * holds time n while zeta(knew) and `time` are at n+1 -- the reference's
 * choice, kept for parity of the files.  The state at t = 0 is never sampled.
 * At coef == 1 the old mean is not read.  Returns -4 when not armed.
 * roms_gpu_wrt_avg writes record rec (rec 1 creates the file) through the
 * writer of roms_gpu_wrt_his (device snapshot in stream order, ahead of the
 * next sample; roms_gpu_io_wait joins it): ocean_time = t_avg, the history
 * file's names, units and dimensions, 'averaged ' ahead of every long_name,
 * type 'ROMS averages file', the global attribute averaging_timescale =
 * '<period, one decimal> seconds', omega as (w_avg*pm)*pn.  Then navg = 0:
 * the next sample starts a fresh window.  With no sample in the window (or
 * not armed) it returns -4, writes nothing and resets nothing.
 * roms_gpu_avg_state: a query (any pointer may be NULL).
 * roms_gpu_avg_copy_out: the mean of ONE ROMS_WRT_* bit (itrc 1..NT for
 * ROMS_WRT_T, ignored otherwise) in the host layout of its field, re-pitched
 * as roms_gpu_copy_out does; count must be the field's one-slot size,
 * (Lm+4)*(Mm+4) times 1, N or N+1.  Values outside the reference's write
 * ranges (dimensions.F:40-45) are unspecified.
 * roms_gpu_time_calc_avg: n samples between two events on the library stream,
 * total milliseconds.  They go on from the open window (navg += n; after one
 * roms_gpu_calc_avg every timed sample reads the old mean) and leave t_avg
 * as it was: re-arm before the averages are used.                           */
int roms_gpu_avg_begin(int wrt_mask);
int roms_gpu_calc_avg(const roms_tlev *t, double time);
int roms_gpu_wrt_avg(const char *path, int rec, int total_rec, double period, const roms_tlev *t);
int roms_gpu_avg_state(int *navg, double *t_avg, int *mask);
int roms_gpu_avg_copy_out(int wrt_bit, int itrc, double *dst, long count);
int roms_gpu_time_calc_avg(int n, const roms_tlev *t, double *ms);
/* ---- true vertical velocity on the device (ABI 29): wvlcty_tile of wvlcty.F.
 * w at rho points and rho levels, m/s: Wrk(0) = 0, Wrk(k) = Wrk(k-1) -
 * pm*pn*(FlxU(i+1)-FlxU(i)+FlxV(j+1)-FlxV(j)) (no grid-motion term: Wrk(N) is
 * not 0, unlike omega), interpolated to rho levels with the four-point weights
 * and one-sided ends, plus 0.25*(Wxi(i)+Wxi(i+1)+Weta(j)+Weta(j+1)) with
 * Wxi(i) = u(i,t->nstp)*(z_r(i)-z_r(i-1))*(pm(i)+pm(i-1)) and Weta alike in j
 * -- slot nstp whatever the caller then writes for u itself -- over
 * istr..iend x jstr..jend, one row more on each side in a periodic direction
 * only; gradient copies onto physical edges and corners; no mask multiply.
 * FlxU, FlxV, u and v(nstp) are the arrays as roms_gpu_copy_out returns them
 * (whole steps always store them); z_r is the stored array, or formed from the
 * kept free surface while the stored grid is set_depth's own (the same bits).
 * N < 2 has no formula (the top level needs Wrk(N-2)): every entry that would
 * compute w then returns -1 with a message.
 * roms_gpu_wvlcty fills a device work array of N planes (allocated on first
 * use; freed by roms_gpu_finalize and by roms_gpu_avg_begin with mask 0) on
 * the library stream.  roms_gpu_wvlcty_copy_out returns it as (N, Mm+4, Lm+4)
 * in the host layout of a rho field (count must be that size; cells outside
 * the computed range and its copies hold 0), -4 if nothing was computed.
 * roms_gpu_time_wvlcty: n launches per sink between two events on the library
 * stream, total milliseconds: ms[0] the store into the work array, ms[1] the
 * running-mean sink with the old mean read (0 unless ROMS_WRT_W is armed; the
 * mean it advances is then no average of anything: re-arm before use).
 * roms_gpu_wrt_his with ROMS_WRT_W computes w into the work array ahead of the
 * snapshot and writes variable w ('vertical velocity', meter second-1, on
 * (time, s_rho, eta_rho, xi_rho), levels 1:N over i0:i1, j0:j1) between omega
 * and AKv, where def_vars_ocean_vars defines it.  roms_gpu_avg_begin with
 * ROMS_WRT_W (accepted in every configuration, never dropped) allocates its
 * running mean; every roms_gpu_calc_avg then samples it with one launch of its
 * own (the other fields keep their single launch): the kernel that computes w
 * applies avg = avg*(1-coef) + w*coef in the same lane, over exactly the cells
 * it computes or copies, without the old mean's load at coef == 1.
 * roms_gpu_wrt_avg writes it as w, 'averaged vertical velocity', and
 * roms_gpu_avg_copy_out serves it under ROMS_WRT_W with N levels.
 * Extraction objects still report 'w' as unsupported: the reference hands
 * extract_data a Wvl(..,nz+1) array through a dummy declared (..,0:N) and
 * interpolates levels 0..N-1 of it, level 0 never written, over halo cells no
 * exchange fills (extract_data.F:204, 707-718) -- there is no defined answer
 * to match.                                                                  */
int roms_gpu_wvlcty(const roms_tlev *t);
int roms_gpu_wvlcty_copy_out(double *dst, long count);
int roms_gpu_time_wvlcty(int n, const roms_tlev *t, double *ms);
/* ---- Lagrangian particles on the device (ABI 32): do_particles of particles.F.
 * Particles live in this rank's index space [0,Lm] x [0,Mm] x [0,N]: px = 0 is
 * the western u face i = 1, rho point i sits at px = i - 0.5, rho level k at
 * pz = k - 0.5.  The list is the reference's part(npmx, 13), column-major:
 * tag, px py pz, pu pv pw (m/s), the index-space increments prx pry prz and
 * their previous values.  The step never advances particles by itself.
 * roms_gpu_part_begin allocates the list, its double buffer and the eight send
 * and receive messages of fac_x, fac_y, fac_c * npmx * 13 words (N/S, E/W,
 * corners; init_arrays_mpi_roms; 0: 0.1, 0.1, 0.01) and re-arms from empty;
 * every rank of a run passes the same npmx and factors.  ROMS_PART_SORT: every
 * call ends with sort_particles' ordering by floor(px) + floor(py)*Lm +
 * floor(pz)*Lm*Mm (stable); without it the list keeps arrival order.
 * roms_gpu_part_add appends n particles at (px, py, pz): zmode 0, pz in index
 * space; zmode 1, pz a depth in metres (negative down) converted against z_w
 * of the particle's column by zlev2kidx's formula and clamped into [0, N].
 * Tags are ip + 10000000*mynode and go on from the rank's ntag.  Particles
 * added before the first roms_gpu_do_particles take part in its dm = d start,
 * later ones start from dm = 0 (seed_bry).  It fails and changes nothing if
 * the list would exceed npmx or a position lies outside the index space.
 * roms_gpu_do_particles, called after a step (main.F:501), on the library
 * stream: rhs_particles (trilinear u, v(t->nnew), Wp, Hz, bilinear pm, pn with
 * their halos as the step left them) and advance_particles (AB2, bottom and
 * surface clamps), exchange_particles (eight neighbours through the rank's
 * communicator; a periodic direction of one rank wraps; an edge without a
 * neighbour loses the particle), removal of the dead, arrivals appended in the
 * order sw, s, se, w, e, nw, n, ne, then the ordering if armed.  Compaction and
 * packing are stable, so list and messages are the same from run to run.  Wp,
 * which the reference allocates and never fills, is ((We+Wi)*pm)*pn.  Where
 * the reference stops -- a particle more than half a cell outside the rank, a
 * full message -- the device reads nothing out of range, gives the particle
 * zero increments (n_range) or keeps what fits (n_overflow), and every later
 * roms_gpu_do_particles / roms_gpu_wrt_part returns -5 until re-armed.  Each
 * call reads one block of counters back (one stream synchronisation).
 * roms_gpu_part_state: np, ntag, n_sur, n_bot, n_lost (died at an edge without
 * a neighbour), n_moved (sent or wrapped), n_range, n_overflow.
 * roms_gpu_part_copy_out: the live list as part(np, 13), column-major; count
 * must be at least np*13; global != 0: px, py + iSW_corn + 0.5, jSW_corn + 0.5.
 * roms_gpu_wrt_part: record rec (1 creates the file) of the _part file through
 * the writer thread: particles(time, seven, npart = npmx), double, long_name
 * 'Tag/x/y/z/u/v/w', px and py global, rows past np zero (tags start at 1);
 * ocean_time; global attribute big_number = 10000000.  total_rec is accepted
 * for symmetry with the other writers and not stored.
 * roms_gpu_time_do_particles: n calls on a copy of the list between events on
 * the library stream, total milliseconds: ms[0] whole calls, ms[1] the rhs and
 * advance kernel alone.  The particles do not move.                        */
#define ROMS_PART_SORT 1
int roms_gpu_part_begin(long npmx, double fac_x, double fac_y, double fac_c, int flags);
int roms_gpu_part_add(long n, const double *px, const double *py, const double *pz, int zmode);
int roms_gpu_do_particles(const roms_tlev *t);
int roms_gpu_part_state(long out[8]);
int roms_gpu_part_copy_out(double *dst, long count, int global);
int roms_gpu_wrt_part(const char *path, int rec, int total_rec, double time);
int roms_gpu_time_do_particles(int n, const roms_tlev *t, double ms[2]);
/* ---- tracer budget terms on the device (ABI 30): DIAGNOSTICS with diag_trc,
 * diagnostics.F and its hooks in step3d_t_ISO.F, the non-isoneutral build.
 * For every armed tracer six terms of the corrector step3d_t, each N planes in
 * the layout of a rho field, C m^3/s, 0 outside the ranges named:
 *  ADVX (i = 1..Lm+1, j = 1..Mm): the centred fourth-order flux of t(nrhs)
 *    through the u face (diagnostics.F:620-639), grd(i) = (t(i)-t(i-1))*
 *    umask(i), g2(i) = grd(i+1)+grd(i), advx = 0.5*(t(i)+t(i-1) -
 *    0.1666666666666667*(g2(i)-g2(i-1)))*FlxU(i).  ADVY (i = 1..Lm, j =
 *    1..Mm+1) alike in eta (:640-659).  On a physical, non-periodic edge of the
 *    whole grid the difference one face outside is a copy of the first one
 *    inside (compute_horiz_tracer_fluxes.h:50-84, 131-165); on a periodic side
 *    or a rank boundary nothing is copied, so a decomposed run is bitwise the
 *    single domain.
 *  MIXX = FX - ADVX, MIXY = FE - ADVY (step3d_t_ISO.F:236-248): FX, FE the
 *    UPSTREAM_TS fluxes the corrector applied, river faces overridden.
 *  ADVZ (k = 1..N, i = 1..Lm, j = 1..Mm): the corrector's spline flux FC(k),
 *    FC(N) = 0 (step3d_t_ISO.F:911-913).
 *  MIXZ = ZFlx - ADVZ (step3d_t_ISO.F:914, 1104-1132): with S the content of
 *    t(nnew) after the horizontal and before the vertical update, D(k) =
 *    (S(k) - Hz(k)*t_new(k))/dt, ZFlx(1) = D(1)/(pm*pn), ZFlx(k) =
 *    D(k)/(pm*pn) + ZFlx(k-1); t_new as the implicit solve leaves it, ahead of
 *    t3dbc, the exchange and t3dmix.
 * SNAP is S itself, kept for budget closure.
 * tdiag_begin arms ntd tracers (1-based indices itrc[0..ntd-1]) and allocates
 * seven zeroed arrays per tracer: the six terms (with do_avg their running
 * means instead) and S; ntd = 0 disarms and frees.  It refuses (-1)
 * adv_isoneutral (that branch defines other terms), an index outside 1..NT or
 * repeated; a refused call leaves an earlier arming as it was.  Sampling is
 * on after it; tdiag_sample switches it (the reference's
 * calc_diag).  While armed and sampling every corrector -- the step3d_t entry
 * and the one inside a whole step -- forms the terms: with do_avg navg += 1,
 * coef = 1/navg, X_avg = X_avg*(1-coef) + X*coef (calc_diag_avg,
 * diagnostics.F:709-732) in the lanes that form X, without the old mean's load
 * at coef == 1.  Not armed, or not sampling, the corrector launches and
 * allocates nothing more.  tdiag_state: a query (any pointer may be NULL).
 * tdiag_copy_out: term ROMS_TDIA_* of armed tracer itrc as (N, Mm+4, Lm+4) in
 * the host layout; the mean with do_avg, else the last sample; count must be
 * that size; -1 for a tracer that is not armed.
 * wrt_tdiag writes record rec (rec 1 creates the file) through the writer of
 * the history files: ocean_time, time_step, per armed tracer <name>_advx,
 * _advy, _advz, _mixx, _mixy, _mixz on (time, s_rho, eta_rho, xi_rho) with the
 * reference's long names and units (create_diagvars, diagnostics.F:891-921),
 * the global attribute diagnostic_options and, with do_avg, diag_avg_time =
 * '<period, one decimal> seconds'.  With do_avg it then sets navg = 0.  With no
 * sample since tdiag_begin (or, with do_avg, since the last record) it returns
 * -4 and writes nothing.
 * time_tdiag: n launches of each kernel over the whole interior for every
 * armed tracer between two events, total milliseconds: ms[0] the snapshot,
 * ms[1] the horizontal terms, ms[2] the vertical terms (with do_avg the mean
 * sink at coef = 1/2: re-arm before the means are used).                      */
#define ROMS_TDIA_ADVX 1
#define ROMS_TDIA_ADVY 2
#define ROMS_TDIA_ADVZ 3
#define ROMS_TDIA_MIXX 4
#define ROMS_TDIA_MIXY 5
#define ROMS_TDIA_MIXZ 6
#define ROMS_TDIA_SNAP 7
int roms_gpu_tdiag_begin(int ntd, const int *itrc, int do_avg);
int roms_gpu_tdiag_sample(int on);
int roms_gpu_tdiag_state(int *ntd, int *do_avg, int *navg, int *sampling);
int roms_gpu_tdiag_copy_out(int itrc, int term, double *dst, long count);
int roms_gpu_wrt_tdiag(const char *path, int rec, int total_rec, double time, double period, const roms_tlev *t);
int roms_gpu_time_tdiag(int n, roms_tlev *t, double ms[3]);
/* ---- momentum budget terms on the device (ABI 31): DIAGNOSTICS with diag_uv,
 * diagnostics.F and its hooks in prsgrd.F, compute_horiz_rhs_uv_terms.h,
 * step3d_uv1.F, visc3d_S.F and step3d_uv2.F, the IMPLICIT_BOTTOM_DRAG branch.
 * Seven terms per component, m^2/s^2, each N planes in the layout of u (of v);
 * the u terms at i = istrU..iend, j = jstr..jend, the v terms at i =
 * istr..iend, j = jstrV..jend, 0 elsewhere.  With dxdyi_u = 0.25*(pn(i-1,j)+
 * pn(i,j))*(pm(i-1,j)+pm(i,j)) and the v forms the mirror image in eta:
 *  PGR  ru*dxdyi_u*umask, ru as the corrector's prsgrd leaves it
 *  COR  0.5*(UFx(i,j)+UFx(i-1,j))*dxdyi_u, -0.5*(VFe(i,j)+VFe(i,j-1))*dxdyi_v:
 *       the Coriolis and curvilinear products over u, v(nrhs); 0 with neither
 *  ADV  the centred fourth-order advection of u, v(nrhs) by the corrector's
 *       FlxU, FlxV, We+Wi (set_diags_u_4th_adv, set_diags_v_4th_adv); second
 *       order at the first and last flux of a physical, non-periodic edge of
 *       the whole grid and at k = 1, N-1; fourth order on periodic sides and
 *       rank boundaries, so a decomposed run is bitwise the single domain
 *       (the reference tests *_msg_exch: the same on a closed single rank)
 *  DIS  ru*dxdyi_u*umask - PGR - COR - ADV, ru the final right-hand side
 *  HMX  the stress divergence of visc3d over u, v(nstp); 0 without uv_vis2
 *  VMX  (u(nnew) - u_prev)/dt - ru*dxdyi_u: u_prev the u(nnew) step3d_uv1 is
 *       given, u(nnew) the Hz*u its implicit solve leaves
 *  CPL  -DC0*umask*0.5*(Hz(i,j,k)+Hz(i-1,j,k))/dt, DC0 the mismatch against
 *       DU_avg1 that step3d_uv2 removes, Hz the one step3d_uv2 sees
 * PREV is u_prev itself, kept for budget closure.
 * uvdiag_begin(on = 1) allocates 14 zeroed term arrays (with do_avg their
 * running means instead) and 4 snapshots; on = 0 disarms and frees; a refused
 * call leaves an earlier arming as it was.  Sampling is on after it;
 * uvdiag_sample switches it (the reference's calc_diag).  While armed and
 * sampling the corrector's routines -- the entries roms_gpu_prsgrd,
 * _step3d_uv1, _visc3d, _step3d_uv2 and the ones inside a whole step -- form
 * the terms: prsgrd with nrhs == 3 keeps ru, rv; step3d_uv1 opens a sample
 * (with do_avg navg += 1, coef = 1/navg, X_avg = X_avg*(1-coef) + X*coef,
 * calc_diag_avg) and forms PGR, COR, ADV, DIS, VMX; visc3d and step3d_uv2 add
 * HMX and CPL to the open sample once each; further calls before the next
 * step3d_uv1 leave the terms alone.  A sample is complete after step3d_uv2.
 * A whole step then runs prsgrd without the fused momentum terms, keeps the
 * predictor's u, v(nnew) stored and is enqueued rather than replayed: the
 * model fields are bitwise those of the default.  Not armed, or not sampling,
 * the routines launch and allocate nothing more.
 * uvdiag_state: a query (any pointer may be NULL).  uvdiag_copy_out: term
 * ROMS_UVD_* of component ROMS_UVD_U / ROMS_UVD_V as (N, Mm+4, Lm+4) in the
 * host layout; the mean with do_avg, else the last sample.
 * wrt_diag writes record rec (rec 1 creates the file) through the writer of
 * the history files: ocean_time, time_step, u_pgr, u_cor, u_adv, u_dis, u_hmx,
 * u_vmx, u_cpl on (time, s_rho, eta_rho, xi_u), v_* on (time, s_rho, eta_v,
 * xi_rho) with the reference's long names and units (create_diagvars,
 * diagnostics.F:812-889), then, if tracers are armed too (tdiag_begin), their
 * variables; the global attribute diagnostic_options lists what is in the
 * file and, with do_avg, diag_avg_time = '<period, one decimal> seconds'.
 * With do_avg both windows restart after the record.  -4 with no complete
 * sample; -1 if the two sets disagree on do_avg.
 * time_uvdiag: n launches of each kernel over the whole interior between two
 * events, total milliseconds: ms[0] the snapshots, ms[1] PGR..DIS and VMX,
 * ms[2] HMX, ms[3] CPL (with do_avg the mean sink at coef = 1/2: re-arm before
 * the means are used).                                                      */
#define ROMS_UVD_U 0
#define ROMS_UVD_V 1
#define ROMS_UVD_PGR 1
#define ROMS_UVD_COR 2
#define ROMS_UVD_ADV 3
#define ROMS_UVD_DIS 4
#define ROMS_UVD_HMX 5
#define ROMS_UVD_VMX 6
#define ROMS_UVD_CPL 7
#define ROMS_UVD_PREV 8
int roms_gpu_uvdiag_begin(int on, int do_avg);
int roms_gpu_uvdiag_sample(int on);
int roms_gpu_uvdiag_state(int *armed, int *do_avg, int *navg, int *sampling);
int roms_gpu_uvdiag_copy_out(int comp, int term, double *dst, long count);
int roms_gpu_wrt_diag(const char *path, int rec, int total_rec, double time, double period, const roms_tlev *t);
int roms_gpu_time_uvdiag(int n, roms_tlev *t, double ms[4]);
/* ---- baroclinic pressure fluxes on the device (ABI 34): calc_pressure_flux of
 * calc_pflx_mod.F on the P of the corrector's prsgrd (prsgrd.F:160-226, 466-
 * 468).  Off until roms_gpu_pflx_begin arms it; not armed, no routine launches
 * or allocates anything more and whole steps are the graphs they were.
 * roms_gpu_pflx_begin(timescale, on): on = 1 arms with alpha = dt/timescale,
 * beta = 1 - alpha (timescale <= 0: the reference's 86400 s; calc_pflx.opt has
 * it as a compile-time constant, here it is a run-time argument) and
 * allocates, zeroed, the three filter states u_slow, v_slow, p_slow (N levels),
 * up, vp and an N-level work array for p_fast; on = 0 disarms and frees; a
 * refused call (-1 with N < 2, -2 without memory) leaves an earlier arming as
 * it was.  Arming again starts from zero states.
 * While armed, every corrector prsgrd -- roms_gpu_prsgrd with t->nrhs == 3 and
 * the one inside roms_gpu_step; never the predictor's -- is followed by two
 * launches (whole steps are then enqueued rather than replayed; the model
 * fields are bitwise those of the default):
 *  P over 0..Lm x 0..Mm by prsgrd's expressions (SPLIT_EOS or not, pot_tides),
 *    p_slow = beta*p_slow + alpha*P, p_fast = P - p_slow;
 *  Uflx = FlxU(.,.,1) + .. + FlxU(.,.,N) in that order, then Uflx*(pn(i,j)+
 *    pn(i-1,j))/(z_w(i,j,N)-z_w(i,j,0)+z_w(i-1,j,N)-z_w(i-1,j,0)); Vflx alike
 *    with pm and j-1; for k = 1..N  u_slow = beta*u_slow + alpha*(u(nrhs)-Uflx),
 *    u_fast = u(nrhs)-Uflx-u_slow, up = up + u_fast*0.25*(p_fast(i-1,j)+
 *    p_fast(i,j))*(Hz(i-1,j,k)+Hz(i,j,k)); v_slow, vp alike in j.
 * Ranges (this rank's indices): p_slow 0..Lm x 0..Mm, u_slow 1..Lm+1 x 1..Mm,
 * v_slow 1..Lm x 1..Mm+1, up, vp 1..Lm x 1..Mm; nothing is masked; dzt, which
 * the reference forms and nothing reads, is not formed.  One deviation: at a
 * physical western edge the reference's prsgrd leaves P(0,j,:) unwritten and
 * calc_pressure_flux reads it into p_slow(0,j,:) and up(1,j); here P(0,j,:) is
 * formed like every other column (all its inputs exist).
 * roms_gpu_pflx_state: a query (any pointer may be NULL); nsamples counts the
 * correctors filtered since arming.
 * roms_gpu_pflx_path: launches of the P walk since arming that formed z_r,
 * z_w(N) from the kept free surface, and that streamed them (same bits;
 * roms_gpu_time_pflx's launches count too).
 * roms_gpu_pflx_copy_out(which, dst, count): ROMS_PFLX_UP, VP as (Mm+4, Lm+4),
 * U_SLOW, V_SLOW, P_SLOW as (N, Mm+4, Lm+4) in the host layout of
 * roms_gpu_copy_out, zero outside the ranges above: the up(pos,:) lines a
 * host-side adjust_orlanski (sponge_tune.F:178-198) needs; adjust_orlanski
 * itself and ub_* stay with the host.  roms_gpu_pflx_copy_in: the three filter
 * states only (-1 for up, vp), whole arrays in the same layout.  Both -4 when
 * not armed.
 * Restart: while armed roms_gpu_wrt_rst also writes u_slow (time, s_rho,
 * eta_rho, xi_u), v_slow (.., eta_v, xi_rho), p_slow (.., eta_rho, xi_rho),
 * double, over the write ranges of u, v and a rho field (basic_output.F:977-
 * 990, wrt_rst_diag_slow); not armed the file is byte for byte what it was.
 * roms_gpu_get_init while armed follows get_init_slow per variable: read if
 * present, then 0 where umask / vmask / rmask < 1 (p_slow: its halo exchanged
 * first); if absent u_slow = u(tindx), v_slow = v(tindx) over their write
 * ranges, p_slow = 0, and roms_gpu_last_error holds a WARNING line naming each
 * fallback while the call returns 0.  Arm before roms_gpu_get_init.
 * roms_gpu_time_pflx: n launches of each kernel between two events, total
 * milliseconds: ms[0] the P and p_slow walk, ms[1] the u, v walk (the filters
 * go on from their state: re-arm before they are used).                     */
#define ROMS_PFLX_UP 1
#define ROMS_PFLX_VP 2
#define ROMS_PFLX_U_SLOW 3
#define ROMS_PFLX_V_SLOW 4
#define ROMS_PFLX_P_SLOW 5
int roms_gpu_pflx_begin(double timescale, int on);
int roms_gpu_pflx_state(int *armed, double *alpha, long *nsamples);
int roms_gpu_pflx_path(long *formed, long *streamed);
int roms_gpu_pflx_copy_out(int which, double *dst, long count);
int roms_gpu_pflx_copy_in(int which, const double *src, long count);
int roms_gpu_time_pflx(int n, double ms[2]);
/* ---- z-level slices on the device (ABI 26): calc_zslice / sigma_to_z /
 * calc_average / wrt_zslice of zslice_output.F.  u, v and chosen tracers, slot
 * t->nnew (the slot roms_gpu_wrt_his samples), interpolated from the model
 * levels to fixed depths relative to the free surface (negative: below it),
 * as a snapshot or as a running mean (do_avg).  Slicing is off until
 * roms_gpu_zslice_begin arms it and roms_gpu_step never samples by itself.
 * roms_gpu_zslice_begin(what, ndep, vecdep, nt_z, trc2zsc, do_avg): what is a
 * sum of ROMS_ZSL_* bits; it allocates ndep planes per selected field (one per
 * tracer of trc2zsc, 1-based indices, nt_z of them; both ignored without
 * ROMS_ZSL_T) in the 2-D device layout, and as many again for the means when
 * do_avg, all zero, and sets navg = 0.  what == 0 disarms and frees; calling
 * it again re-arms from scratch; roms_gpu_finalize frees.  It refuses (-1)
 * ndep outside 1..ROMS_ZSL_MAXDEP, a tracer index outside 1..NT, ROMS_ZSL_T
 * with nt_z < 1, and N < 2.  Depths may be unsorted and may repeat.
 * For each cell i = 1..Lm, j = 1..Mm and depth zlev, with zz(k) = z_r(k) -
 * z_w(N) (k = 1..N), zz(0) = z_w(0) - z_w(N), zz(N+1) = 0 (u, v points: the
 * mean of the two rho columns in every term) and dpth = zz(N+1) - zz(0), the
 * first test that holds decides: rmask(i,j) < 0.5 (at u, v points too) -> 0;
 * dpth*(zlev-zz(N+1)) > 0 -> 0; dpth*(zlev-zz(N)) > 0 -> var(N) +
 * (zlev-zz(N))*(var(N)-var(N-1))/(zz(N)-zz(N-1)); dpth*(zz(0)-zlev) > 0 -> 0;
 * dpth*(zz(1)-zlev) > 0 -> var(1) - (zz(1)-zlev)*(var(2)-var(1))/(zz(2)-zz(1));
 * else the first k = N-1..1 with (zz(k+1)-zlev)*(zlev-zz(k)) >= 0 ->
 * (var(k)*(zz(k+1)-zlev) + var(k+1)*(zlev-zz(k)))/(zz(k+1)-zz(k)).
 * roms_gpu_calc_zslice: one sample on the library stream, one kernel launch
 * whatever the fields and depths.  With do_avg the same launch advances the
 * means: navg += 1, coef = 1/navg, X_avg = X_avg*(1-coef) + X*coef; at
 * coef == 1 the old mean is not read.  Returns -4 when not armed.
 * roms_gpu_wrt_zslice writes record rec (rec 1 creates the file) through the
 * writer of roms_gpu_wrt_his (roms_gpu_io_wait joins it): without do_avg it
 * samples first; with do_avg it needs navg > 0 (else -4, nothing written).
 * The file holds the dimension depth, depth(depth) = vecdep, ocean_time =
 * time, time_step as the other files of this writer, every sliced tracer
 * under its roms_gpu_io_tracer_name name on (time, depth, eta_rho, xi_rho), u
 * on (.., eta_rho, xi_u), v on (.., eta_v, xi_rho), the history file's long
 * names and units -- with do_avg 'averaged' straight ahead of a tracer's long
 * name and 'averaged ' ahead of u's and v's, as the reference has them -- and
 * the partition attribute when decomposed.  Points of the partition's write
 * range outside 1..Lm x 1..Mm hold 0.  Afterwards navg = 0.
 * roms_gpu_zslice_state: a query (any pointer may be NULL).
 * roms_gpu_zslice_copy_out: the current slices, or with do_avg the means, of
 * ONE ROMS_ZSL_* bit (q = 1..nt_z picks the tracer for ROMS_ZSL_T, ignored
 * otherwise) as (ndep, Mm+4, Lm+4) in the host layout; count must be that
 * size.
 * roms_gpu_time_calc_zslice: n samples between two events on the library
 * stream, total milliseconds (with do_avg they go on from the open window). */
#define ROMS_ZSL_T 1
#define ROMS_ZSL_U 2
#define ROMS_ZSL_V 4
#define ROMS_ZSL_MAXDEP 32
int roms_gpu_zslice_begin(int what, int ndep, const double *vecdep, int nt_z, const int *trc2zsc, int do_avg);
int roms_gpu_calc_zslice(const roms_tlev *t);
int roms_gpu_wrt_zslice(const char *path, int rec, int total_rec, double time, const roms_tlev *t);
int roms_gpu_zslice_state(int *navg, int *what, int *ndep, int *do_avg);
int roms_gpu_zslice_copy_out(int what_bit, int q, double *dst, long count);
int roms_gpu_time_calc_zslice(int n, const roms_tlev *t, double *ms);
/* ---- child-boundary extraction on the device (ABI 27): do_extract_data of
 * extract_data.F with remap_src_to_grid of vertical_remapping.F.  An object is
 * a line of np_global fractional positions (ipos, jpos) in absolute index
 * space ([0,LLm]x[0,MMm], cell centres at half integers), with an angle per
 * point (a vector object) or without (ang == NULL, a scalar object), and an
 * output_vars string.  Extraction is off until an object is added and
 * roms_gpu_step never samples; extract_period, nrpf_extract and otime stay
 * with the host.
 * roms_gpu_extract_begin(N_chd, theta_s_chd, theta_b_chd, hc_chd) clears every
 * object (disarms) and sets the child's vertical grid: the remap is used
 * unless all four equal the parent's (parent_child_grid_mismatch); Cs_w_chd
 * follows set_chd_scoord.  roms_gpu_extract_angler sets the grid angle
 * (host layout, (Mm+4)*(Lm+4), default 0) ahead of the first object.
 * roms_gpu_extract_add_object: the rank keeps the FIRST contiguous run of
 * points with 0 <= ipos-iSW_corn < Lm and 0 <= jpos-jSW_corn < Mm
 * (find_local_points assumes contiguity: a line that re-enters the subdomain
 * loses its second run) as start_idx (1-based) and np.  set is the name up to
 * its first '_', bnd runs from that '_' up to the next one ('grid1_west_r':
 * 'grid1', '_west'); a variable is called set_var+bnd.  output_vars is
 * searched for substrings as findstr does: 'zeta', 'temp', 'salt', 'ubar',
 * 'vbar', 'u' (also found in 'ubar' and 'up'), 'v', 'w', 'up', 'vp', 'bgc'.
 * ROMS_EXT_UP/VP are produced for an object added while the pressure fluxes
 * are armed (roms_gpu_pflx_begin, ABI 34): up = cosa*ui - sina*vi, vp =
 * sina*ui + cosa*vi with ui, vi the device's up, vp (zero outside 1..Lm x
 * 1..Mm, halos exchanged) interpolated with the u and the v coefficients; 2-D
 * variables <set>_up<bnd>, <set>_vp<bnd> on (time, np), 'pressure flux',
 * 'W/m^2', never remapped; roms_gpu_calc_extract returns -4 if the fluxes were
 * disarmed since.  Added while not armed they are not produced, like
 * ROMS_EXT_W/BGC (no BGC here; w: see ABI 29 above): those
 * are reported in the object's `unsupported` mask and named in
 * roms_gpu_last_error while the call returns 0.  'salt' is ignored without
 * SALINITY.  Refused (-1, nothing armed): a vector variable (up, vp too) on a scalar
 * object; a 3-D variable with the remap when N < 5.  Coefficients follow
 * compute_coef at rho (+0.5,+0.5), u (+0.5 in i) and v (-0.5 in i, +0.5 in j)
 * positions with rmask/umask/vmask and coef/sum(coef): a point whose four
 * corners are masked has NaN coefficients and NaN results, as the reference.
 * cosa, sina = cos, sin(angler interpolated with the rho coefficients - ang).
 * roms_gpu_extract_objects_file reads the reference's objects file (netCDF
 * classic CDF-1/2; each variable one object, (2|3, np) doubles, the point
 * dimension fastest, attribute output_vars); all objects are added or none.
 * roms_gpu_calc_extract: one sample, two launches (interpolation of every
 * object and variable; the remap).  zeta, ubar, vbar from slot t->knew
 * (ubar: cosa*ui - sina*vi, vbar: sina*ui + cosa*vi); u, v, temp, salt from
 * slot t->nstp, u and v rotated level by level.  With the remap the parent's
 * thicknesses are Hz, Hz_u, Hz_v interpolated (Hz_u, Hz_v: set_HUV's of the
 * step just taken, kept by whole steps while an object needs them), the
 * child's come from get_child_thickness of their sums, and every profile goes
 * through remap_src_to_grid onto N_chd layers; otherwise the (N, np) profile
 * is the result.  On a decomposed run every rank calls it (halo of Hz_u, Hz_v).
 * roms_gpu_wrt_extract samples, then writes record rec (rec 1 creates the
 * file; total_rec is unused) through the writer of roms_gpu_wrt_his: one file
 * per rank; per object with np > 0 the dimension np%03d (its 1-based index),
 * <set>_time ('Time since 2000', 'second'), 2-D variables on (time, np), 3-D
 * ones on (time, s_rho = N_chd, np), attributes start, count, dname, dsize,
 * long_name, units, type double.  The one record dimension is
 * time_<set of the first object> for every set.
 * roms_gpu_extract_object_coef: grid 0 rho, 1 u, 2 v; coef is (4, np).
 * roms_gpu_extract_copy_out: one ROMS_EXT_* bit of object iobj (1-based) from
 * the last sample as (levels, np), levels = N_chd with the remap else N, or
 * (np); count must be that size.
 * roms_gpu_time_calc_extract: n interpolation launches, then n remap launches,
 * each between two events: ms[0], ms[1] their total milliseconds.
 * roms_gpu_extract_locate is find_local_points alone, without a device. */
#define ROMS_EXT_ZETA 1
#define ROMS_EXT_UBAR 2
#define ROMS_EXT_VBAR 4
#define ROMS_EXT_U 8
#define ROMS_EXT_V 16
#define ROMS_EXT_TEMP 32
#define ROMS_EXT_SALT 64
#define ROMS_EXT_UP 128
#define ROMS_EXT_VP 256
#define ROMS_EXT_W 512
#define ROMS_EXT_BGC 1024
int roms_gpu_extract_begin(int N_chd, double theta_s_chd, double theta_b_chd, double hc_chd);
int roms_gpu_extract_angler(const double *angler, long count);
int roms_gpu_extract_add_object(const char *name, const char *dname, long np_global, const double *ipos,
                                const double *jpos, const double *ang, const char *output_vars);
int roms_gpu_extract_objects_file(const char *path);
int roms_gpu_calc_extract(const roms_tlev *t);
int roms_gpu_wrt_extract(const char *path, int rec, int total_rec, double time, const roms_tlev *t);
int roms_gpu_extract_state(int *nobj, int *mismatch, int *N_chd, int *np_total, int *need_huv);
int roms_gpu_extract_object_info(int iobj, int *np, int *start_idx, int *vars, int *unsupported, int *scalar);
int roms_gpu_extract_object_coef(int iobj, int grid, int *ip, int *jp, double *coef, double *cosa, double *sina);
int roms_gpu_extract_child_cs(double *cs_w);
int roms_gpu_extract_copy_out(int iobj, int var_bit, double *dst, long count);
int roms_gpu_time_calc_extract(int n, const roms_tlev *t, double *ms);
int roms_gpu_extract_locate(int nx, int ny, int iSW_corn, int jSW_corn, long npg, const double *ipos,
                            const double *jpos, int *start_idx, int *np);
/* t_vname/t_units/t_lname of tracer itrc (tracers.opt); default temp, salt, trcNN */
int roms_gpu_io_tracer_name(int itrc, const char *name, const char *units, const char *long_name);
/* Returns 0 (read), 1 (tindx 2: records not consecutive steps, nothing read),
 * or a negative error.                                                       */
int roms_gpu_get_init(const char *path, int req_rec, int tindx, roms_tlev *t, double *start_time);

/* ---- diagnostics (diag.F code_check norms, device reduction) ----
 * KE, KE2b (barotropic), max advective Courant and the vertical Courant at
 * that point, in the reference's reduction order.  The grid area/volume of
 * setup_grid2.F are formed on first use from the device's h, pm, pn, rmask
 * (per-rank pairwise sums, tree over ranks), so a host that registered its
 * own arrays gets the same norms as roms_gpu_init_case.  Collective.        */
int roms_gpu_diag(const roms_tlev *t, double norms[4]);
/* Host-only: set_weights.F restatement -- the fast-time averaging weights of
 * ndtfast (written into weight, C order [2][288]); returns nfast, or -1.    */
int roms_gpu_set_weights(int ndtfast, double weight[2][ROMS_MAX_FAST]);
/* event-timed replay of n steps on the library stream: total milliseconds  */
int roms_gpu_time_steps(roms_tlev *t, int n, double *ms);
/* Runs nsteps steps eagerly with HIP events on the library stream around
 * every launch of one routine; returns the mean duration of one launch
 * (one call of the routine, incl. its boundary/exchange kernels).            */
enum roms_routine {
  ROMS_R_RHO_EOS = 0, ROMS_R_SET_HUV, ROMS_R_OMEGA, ROMS_R_PRSGRD, ROMS_R_PRE_STEP3D, ROMS_R_SET_HUV1,
  ROMS_R_STEP3D_UV1, ROMS_R_VISC3D, ROMS_R_STEP2D, ROMS_R_STEP3D_UV2, ROMS_R_STEP3D_T, ROMS_R_T3DMIX,
  ROMS_R_LMD_VMIX,
  ROMS_R_K_S2D_FB,  /* kernel level: the fused barotropic kernel k_s2d_fb alone (one fast step) */
  ROMS_R_K_PRE_UV_SEG,     /* kernel level: pre_step3d's momentum segment solver (N > 63) */
  ROMS_R_K_UV1_SEG,        /* kernel level: step3d_uv1's momentum segment solver (N > 63) */
  ROMS_R_K_STEP3D_T_SEG,   /* kernel level: step3d_t's tracer segment solver (N > 63) */
  ROMS_R_K_PRSGRD_UV,      /* kernel level: prsgrd's ru/rv kernel (with the horizontal momentum r.h.s. in whole steps) */
  ROMS_R_K_HALO_PACK,      /* halo path: the pack of every exchange (IPC: straight into the neighbours' buffers) */
  ROMS_R_K_HALO_WAIT,      /* halo path: the transport (IPC: signal + arrival wait; RCCL: the send/recv group) */
  ROMS_R_K_HALO_UNPACK,    /* halo path: the unpack of every exchange */
  ROMS_R_COUNT
};
int roms_gpu_time_routine(int routine, int nsteps, roms_tlev *t, double *avg_ms, long *launches);

#ifdef __cplusplus
}
#endif
#endif /* ROMS_GPU_H */
