! roms_gpu_mod.F90 -- Fortran (iso_c_binding) interface to libromsgpu.so,
! the MI355X hot path of the split-explicit step (include/roms_gpu.h).
!
! A reference build uses it from drop-in replacements of the hot-path
! routines (fortran/dropin/*.F): each keeps the reference's signature
! (src/main.F:397-479 calls) and forwards to roms_gpu_<routine> with the
! time indices of module `scalars` packed into a roms_tlev.
module roms_gpu_mod
  use iso_c_binding
  implicit none

  integer, parameter :: ROMS_MAX_FAST = 288

  type, bind(c) :: roms_dims
    integer(c_int) :: Lm, Mm, N, NT, LLm, MMm
    integer(c_int) :: np_xi, np_eta, inode, jnode, iSW_corn, jSW_corn
    integer(c_int) :: ew_periodic, ns_periodic
    integer(c_int) :: west_exchng, east_exchng, south_exchng, north_exchng
  end type

  type, bind(c) :: roms_cfg
    integer(c_int) :: nonlin_eos, salinity, lmd_mixing, uv_vis2, ts_dif2
    real(c_double) :: dt
    integer(c_int) :: ndtfast, nfast
    real(c_double) :: weight(ROMS_MAX_FAST, 2)   ! C weight[2][288] -> Fortran (288,2)
    real(c_double) :: g, rho0, rdrg, rdrg2, Zob, gamma2
    real(c_double) :: Akv_bak, Akt_bak(2)
    real(c_double) :: Tcoef, T0, Scoef, S0
    real(c_double) :: theta_s, theta_b, hc
    integer(c_int) :: obc                        ! OBC_WEST 1, OBC_EAST 2, OBC_SOUTH 4, OBC_NORTH 8
    real(c_double) :: ubind
    integer(c_int) :: curvgrid                   ! CURVGRID
    integer(c_int) :: uv_adv, uv_cor             ! UV_ADV, UV_COR
    integer(c_int) :: pot_tides                  ! TIDES pot_tides
    integer(c_int) :: bulk_frc                   ! BULK_FRC
    integer(c_int) :: adv_isoneutral             ! ADV_ISONEUTRAL (+SW_TRIADS, STABILIZE)
  end type

  type, bind(c) :: roms_tlev
    integer(c_int) :: iic, ntstart, forw_start, iif, nfast, kstp, knew, nstp, nrhs, nnew
  end type

  type, bind(c) :: roms_case
    integer(c_int) :: case_id, LLm, MMm, N, NT, salinity, nonlin_eos, lmd_mixing
    real(c_double) :: dt
    integer(c_int) :: ndtfast
    real(c_double) :: sizex, sizey
    integer(c_int) :: surf_flux
    integer(c_int) :: obc
    real(c_double) :: v_sponge
    integer(c_int) :: island
    integer(c_int) :: curvgrid
    integer(c_int) :: uv_adv, uv_cor
    integer(c_int) :: bulk_frc
    integer(c_int) :: adv_isoneutral
  end type

  ! LMD switch bits of lmd_mixing (ROMS_LMD_*)
  integer(c_int), parameter :: ROMS_LMD_MIXING = 1, ROMS_LMD_KPP = 2, ROMS_LMD_BKPP = 4, ROMS_LMD_RIMIX = 8, &
                               ROMS_LMD_CONVEC = 16, ROMS_LMD_NONLOCAL = 32, ROMS_LMD_DDMIX = 64
  integer(c_int), parameter :: ROMS_GPU_ABI = 34 ! ROMS_GPU_ABI_VERSION, include/roms_gpu.h
  ! output switches of roms_gpu_wrt_his / roms_gpu_avg_begin (ROMS_WRT_*)
  integer(c_int), parameter :: ROMS_WRT_Z = 1, ROMS_WRT_UB = 2, ROMS_WRT_VB = 4, ROMS_WRT_U = 8, ROMS_WRT_V = 16, &
                               ROMS_WRT_T = 32, ROMS_WRT_R = 64, ROMS_WRT_O = 128, ROMS_WRT_AKV = 256, &
                               ROMS_WRT_AKT = 512, ROMS_WRT_AKS = 1024, ROMS_WRT_HBLS = 2048, ROMS_WRT_HBBL = 4096, &
                               ROMS_WRT_W = 8192, ROMS_WRT_DEFAULT = 63
  ! roms_gpu_part_begin flags (ROMS_PART_*): the cell ordering of sort_particles after every call
  integer(c_int), parameter :: ROMS_PART_SORT = 1
  ! extraction variables (ROMS_EXT_*); UP, VP, W, BGC are parsed and reported, not produced
  integer(c_int), parameter :: ROMS_EXT_ZETA = 1, ROMS_EXT_UBAR = 2, ROMS_EXT_VBAR = 4, ROMS_EXT_U = 8, &
                               ROMS_EXT_V = 16, ROMS_EXT_TEMP = 32, ROMS_EXT_SALT = 64, ROMS_EXT_UP = 128, &
                               ROMS_EXT_VP = 256, ROMS_EXT_W = 512, ROMS_EXT_BGC = 1024
  ! tracer budget terms of roms_gpu_tdiag_copy_out (ROMS_TDIA_*, diagnostics.F:83-88; SNAP: the pre-vertical Hz*t)
  integer(c_int), parameter :: ROMS_TDIA_ADVX = 1, ROMS_TDIA_ADVY = 2, ROMS_TDIA_ADVZ = 3, ROMS_TDIA_MIXX = 4, &
                               ROMS_TDIA_MIXY = 5, ROMS_TDIA_MIXZ = 6, ROMS_TDIA_SNAP = 7
  ! momentum budget terms of roms_gpu_uvdiag_copy_out (ROMS_UVD_*, diagnostics.F:56-63; PREV: u, v(nnew) as step3d_uv1 got them)
  integer(c_int), parameter :: ROMS_UVD_U = 0, ROMS_UVD_V = 1
  integer(c_int), parameter :: ROMS_UVD_PGR = 1, ROMS_UVD_COR = 2, ROMS_UVD_ADV = 3, ROMS_UVD_DIS = 4, &
                               ROMS_UVD_HMX = 5, ROMS_UVD_VMX = 6, ROMS_UVD_CPL = 7, ROMS_UVD_PREV = 8
  ! arrays of roms_gpu_pflx_copy_out / _copy_in (ROMS_PFLX_*, calc_pflx_mod.F:22-27)
  integer(c_int), parameter :: ROMS_PFLX_UP = 1, ROMS_PFLX_VP = 2, ROMS_PFLX_U_SLOW = 3, ROMS_PFLX_V_SLOW = 4, &
                               ROMS_PFLX_P_SLOW = 5
  integer(c_int), parameter :: ROMS_FRC_SURFACE = 1, ROMS_FRC_BRY = 2

  ! field ids (enum roms_field) used by the drivers below
  integer(c_int), parameter :: ROMS_ALL = -1
  integer(c_int), parameter :: ROMS_zeta = 22, ROMS_ubar = 23, ROMS_vbar = 24, ROMS_u = 25, ROMS_v = 26, &
                               ROMS_t = 27, ROMS_Hz = 32, ROMS_z_r = 35, ROMS_NFIELDS = 111
  ! ADV_ISONEUTRAL arrays (size 0 and every transfer refused without the switch)
  integer(c_int), parameter :: ROMS_dRdx = 105, ROMS_dRde = 106, ROMS_idRz = 107, ROMS_diff3u = 108, &
                               ROMS_diff3v = 109, ROMS_Akz = 110

  interface
    integer(c_int) function roms_gpu_abi_version() bind(c)
      import :: c_int
    end function
    integer(c_int) function roms_gpu_init(dims, cfg, device, comm) bind(c)
      import :: c_int, c_ptr, roms_dims, roms_cfg
      type(roms_dims), intent(in) :: dims
      type(roms_cfg), intent(in) :: cfg
      integer(c_int), value :: device
      type(c_ptr), value :: comm
    end function
    integer(c_int) function roms_gpu_finalize() bind(c)
      import :: c_int
    end function
    type(c_ptr) function roms_gpu_last_error() bind(c)
      import :: c_ptr
    end function
    integer(c_long) function roms_gpu_field_size(id) bind(c)
      import :: c_int, c_long
      integer(c_int), value :: id
    end function
    integer(c_int) function roms_gpu_register(id, host, count) bind(c)
      import :: c_int, c_long, c_ptr
      integer(c_int), value :: id
      type(c_ptr), value :: host
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_upload(id) bind(c)
      import :: c_int
      integer(c_int), value :: id
    end function
    integer(c_int) function roms_gpu_download(id) bind(c)
      import :: c_int
      integer(c_int), value :: id
    end function
    integer(c_int) function roms_gpu_copy_out(id, dst, count) bind(c)
      import :: c_int, c_long, c_ptr
      integer(c_int), value :: id
      type(c_ptr), value :: dst
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_sync() bind(c)
      import :: c_int
    end function
    ! out(1:8): closed-edge mode of the fast step, prsgrd strips (taken, count, jA, jB), omega's segment form
    integer(c_int) function roms_gpu_horizontal_path(out) bind(c)
      import :: c_int
      integer(c_int), intent(out) :: out(8)
    end function
    ! ROMS_GPU_VGRID mask + 256 * valid; mismatches of the stored z_w, z_r, Hz against the in-kernel grid
    integer(c_int) function roms_gpu_vgrid() bind(c)
      import :: c_int
    end function
    ! ROMS_GPU_VGRID2 mask + 256 * valid
    integer(c_int) function roms_gpu_vgrid2() bind(c)
      import :: c_int
    end function
    integer(c_int) function roms_gpu_vgrid_check(out) bind(c)
      import :: c_int, c_long
      integer(c_long), intent(out) :: out(3)
    end function
    ! ROMS_GPU_T_PAIR mask + 256 * (Akt(isalt) known equal to Akt(itemp)); pair-form launches of pre_step3d, step3d_t
    integer(c_int) function roms_gpu_tracer_pair(launches) bind(c)
      import :: c_int, c_long
      integer(c_long), intent(out) :: launches(2)
    end function
    ! ROMS_GPU_LEAN_ST mask; pre_step3d launches that left the u, v(indx) store out, lmd_vmix launches that left Akt(isalt) out
    integer(c_int) function roms_gpu_lean_stores(launches) bind(c)
      import :: c_int, c_long
      integer(c_long), intent(out) :: launches(2)
    end function
    ! ROMS_GPU_T_HSTG mask + 256 * valid; launches of k_pre_tracer_stg, k_step3d_t_stg and of the former forming Hz
    integer(c_int) function roms_gpu_tracer_hstg(launches) bind(c)
      import :: c_int, c_long
      integer(c_long), intent(out) :: launches(3)
    end function
    ! ROMS_GPU_KPP_PF: levels of k_kpp_ext's sweep in flight ahead of the one formed
    integer(c_int) function roms_gpu_kpp_pf() bind(c)
      import :: c_int
    end function
    ! hot-path routines (one per reference subroutine)
    integer(c_int) function roms_gpu_rho_eos(tidx, t) bind(c)
      import :: c_int, roms_tlev
      integer(c_int), value :: tidx
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_lmd_vmix(tind, t) bind(c)
      import :: c_int, roms_tlev
      integer(c_int), value :: tind
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_set_huv(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_omega(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_prsgrd(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_pre_step3d(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_set_huv1(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_step3d_uv1(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_visc3d(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_step2d(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_step3d_uv2(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_step3d_t(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_t3dmix(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_set_depth(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_swr_frac(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    ! after set_forces' set_pipe_frc (pipe_frc.F:33): pipe_idx(GLOBAL_2D_ARRAY) integer,
    ! pipe_flx(GLOBAL_2D_ARRAY), pipe_prf(npip,N), pipe_trc(npip,nt)
    integer(c_int) function roms_gpu_set_pipe_frc(npip, pipe_idx, pipe_flx, pipe_prf, pipe_trc) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: npip
      integer(c_int), intent(in) :: pipe_idx(*)
      real(c_double), intent(in) :: pipe_flx(*), pipe_prf(*), pipe_trc(*)
    end function
    ! set_river_frc (river_frc.F:57-282): riv_uflx/riv_vflx as calc_river_flux
    ! leaves them, riv_vol(nriv), riv_trc(nriv,nt)
    integer(c_int) function roms_gpu_set_river_frc(nriv, riv_uflx, riv_vflx, riv_vol, riv_trc) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: nriv
      real(c_double), intent(in) :: riv_uflx(*), riv_vflx(*), riv_vol(*), riv_trc(*)
    end function
    integer(c_int) function roms_gpu_step(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(inout) :: t
    end function
    integer(c_int) function roms_gpu_init_sequence(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(inout) :: t
    end function
    integer(c_int) function roms_gpu_init_case(c, device, t) bind(c)
      import :: c_int, roms_case, roms_tlev
      type(roms_case), intent(in) :: c
      integer(c_int), value :: device
      type(roms_tlev), intent(out) :: t
    end function
    integer(c_int) function roms_gpu_init_case_comm(c, np_xi, np_eta, comm, device, t) bind(c)
      import :: c_int, c_ptr, roms_case, roms_tlev
      type(roms_case), intent(in) :: c
      integer(c_int), value :: np_xi, np_eta, device
      type(c_ptr), value :: comm
      type(roms_tlev), intent(out) :: t
    end function
    integer(c_int) function roms_gpu_set_weights(ndtfast, weight) bind(c)
      import :: c_int, c_double, ROMS_MAX_FAST
      integer(c_int), value :: ndtfast
      real(c_double), intent(out) :: weight(ROMS_MAX_FAST, 2)
    end function
    integer(c_int) function roms_gpu_diag(t, norms) bind(c)
      import :: c_int, c_double, roms_tlev
      type(roms_tlev), intent(in) :: t
      real(c_double), intent(out) :: norms(4)
    end function
    ! partitioned netCDF restart/history files (basic_output.F, get_init.F);
    ! path: a NUL-terminated character(kind=c_char) array
    integer(c_int) function roms_gpu_wrt_rst(path, rec, total_rec, time, t) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: time
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_wrt_his(path, rec, total_rec, time, t, wrt_mask) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec, wrt_mask
      real(c_double), value :: time
      type(roms_tlev), intent(in) :: t
    end function
    ! time-averaged output (k_avg.hip): calc_avg_ocean_vars / wrt_avg_ocean_vars
    integer(c_int) function roms_gpu_avg_begin(wrt_mask) bind(c)
      import :: c_int
      integer(c_int), value :: wrt_mask
    end function
    integer(c_int) function roms_gpu_calc_avg(t, time) bind(c)
      import :: c_int, c_double, roms_tlev
      type(roms_tlev), intent(in) :: t
      real(c_double), value :: time
    end function
    integer(c_int) function roms_gpu_wrt_avg(path, rec, total_rec, period, t) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: period
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_avg_state(navg, t_avg, mask) bind(c)
      import :: c_int, c_double
      integer(c_int), intent(out) :: navg, mask
      real(c_double), intent(out) :: t_avg
    end function
    integer(c_int) function roms_gpu_avg_copy_out(wrt_bit, itrc, dst, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: wrt_bit, itrc
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_time_calc_avg(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(in) :: t
      real(c_double), intent(out) :: ms
    end function
    ! true vertical velocity (k_wvlcty.hip): wvlcty_tile of wvlcty.F
    integer(c_int) function roms_gpu_wvlcty(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_wvlcty_copy_out(dst, count) bind(c)
      import :: c_int, c_long, c_double
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_time_wvlcty(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(in) :: t
      real(c_double), intent(out) :: ms(2)
    end function
    ! Lagrangian particles (k_particles.hip): do_particles of particles.F
    integer(c_int) function roms_gpu_part_begin(npmx, fac_x, fac_y, fac_c, flags) bind(c)
      import :: c_int, c_long, c_double
      integer(c_long), value :: npmx
      real(c_double), value :: fac_x, fac_y, fac_c
      integer(c_int), value :: flags
    end function
    integer(c_int) function roms_gpu_part_add(n, px, py, pz, zmode) bind(c)
      import :: c_int, c_long, c_double
      integer(c_long), value :: n
      real(c_double), intent(in) :: px(*), py(*), pz(*)
      integer(c_int), value :: zmode
    end function
    integer(c_int) function roms_gpu_do_particles(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_part_state(out) bind(c)
      import :: c_int, c_long
      integer(c_long), intent(out) :: out(8)
    end function
    integer(c_int) function roms_gpu_part_copy_out(dst, count, global) bind(c)
      import :: c_int, c_long, c_double
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
      integer(c_int), value :: global
    end function
    integer(c_int) function roms_gpu_wrt_part(path, rec, total_rec, time) bind(c)
      import :: c_int, c_char, c_double
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: time
    end function
    integer(c_int) function roms_gpu_time_do_particles(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(in) :: t
      real(c_double), intent(out) :: ms(2)
    end function
    ! tracer budget terms (k_tdiag.hip): DIAGNOSTICS with diag_trc, diagnostics.F
    integer(c_int) function roms_gpu_tdiag_begin(ntd, itrc, do_avg) bind(c)
      import :: c_int
      integer(c_int), value :: ntd, do_avg
      integer(c_int), intent(in) :: itrc(*)
    end function
    integer(c_int) function roms_gpu_tdiag_sample(on) bind(c)
      import :: c_int
      integer(c_int), value :: on
    end function
    integer(c_int) function roms_gpu_tdiag_state(ntd, do_avg, navg, sampling) bind(c)
      import :: c_int
      integer(c_int), intent(out) :: ntd, do_avg, navg, sampling
    end function
    integer(c_int) function roms_gpu_tdiag_copy_out(itrc, term, dst, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: itrc, term
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_wrt_tdiag(path, rec, total_rec, time, period, t) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: time, period
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_time_tdiag(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(inout) :: t
      real(c_double), intent(out) :: ms(3)
    end function
    ! momentum budget terms (k_uvdiag.hip): DIAGNOSTICS with diag_uv, diagnostics.F
    integer(c_int) function roms_gpu_uvdiag_begin(on, do_avg) bind(c)
      import :: c_int
      integer(c_int), value :: on, do_avg
    end function
    integer(c_int) function roms_gpu_uvdiag_sample(on) bind(c)
      import :: c_int
      integer(c_int), value :: on
    end function
    integer(c_int) function roms_gpu_uvdiag_state(armed, do_avg, navg, sampling) bind(c)
      import :: c_int
      integer(c_int), intent(out) :: armed, do_avg, navg, sampling
    end function
    integer(c_int) function roms_gpu_uvdiag_copy_out(comp, term, dst, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: comp, term
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_wrt_diag(path, rec, total_rec, time, period, t) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: time, period
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_time_uvdiag(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(inout) :: t
      real(c_double), intent(out) :: ms(4)
    end function
    ! baroclinic pressure fluxes (k_pflx.hip): calc_pressure_flux of calc_pflx_mod.F after the corrector's prsgrd
    integer(c_int) function roms_gpu_pflx_begin(timescale, on) bind(c)
      import :: c_int, c_double
      real(c_double), value :: timescale
      integer(c_int), value :: on
    end function
    integer(c_int) function roms_gpu_pflx_state(armed, alpha, nsamples) bind(c)
      import :: c_int, c_double, c_long
      integer(c_int), intent(out) :: armed
      real(c_double), intent(out) :: alpha
      integer(c_long), intent(out) :: nsamples
    end function
    integer(c_int) function roms_gpu_pflx_path(formed, streamed) bind(c)
      import :: c_int, c_long
      integer(c_long), intent(out) :: formed, streamed
    end function
    integer(c_int) function roms_gpu_pflx_copy_out(which, dst, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: which
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_pflx_copy_in(which, src, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: which
      real(c_double), intent(in) :: src(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_time_pflx(n, ms) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: n
      real(c_double), intent(out) :: ms(2)
    end function
    ! z-level slices (k_zslice.hip): calc_zslice / wrt_zslice of zslice_output.F
    integer(c_int) function roms_gpu_zslice_begin(what, ndep, vecdep, nt_z, trc2zsc, do_avg) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: what, ndep, nt_z, do_avg
      real(c_double), intent(in) :: vecdep(*)
      integer(c_int), intent(in) :: trc2zsc(*)
    end function
    integer(c_int) function roms_gpu_calc_zslice(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_wrt_zslice(path, rec, total_rec, time, t) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: time
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_zslice_state(navg, what, ndep, do_avg) bind(c)
      import :: c_int
      integer(c_int), intent(out) :: navg, what, ndep, do_avg
    end function
    integer(c_int) function roms_gpu_zslice_copy_out(what_bit, q, dst, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: what_bit, q
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_time_calc_zslice(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(in) :: t
      real(c_double), intent(out) :: ms
    end function
    ! child-boundary extraction (k_extract.hip): do_extract_data of extract_data.F
    integer(c_int) function roms_gpu_extract_begin(N_chd, theta_s_chd, theta_b_chd, hc_chd) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: N_chd
      real(c_double), value :: theta_s_chd, theta_b_chd, hc_chd
    end function
    integer(c_int) function roms_gpu_extract_angler(angler, count) bind(c)
      import :: c_int, c_long, c_double
      real(c_double), intent(in) :: angler(*)
      integer(c_long), value :: count
    end function
    ! ang: c_null_ptr for a scalar object, else c_loc of the angles
    integer(c_int) function roms_gpu_extract_add_object(name, dname, np_global, ipos, jpos, ang, output_vars) bind(c)
      import :: c_int, c_long, c_double, c_char, c_ptr
      character(kind=c_char), intent(in) :: name(*), dname(*), output_vars(*)
      integer(c_long), value :: np_global
      real(c_double), intent(in) :: ipos(*), jpos(*)
      type(c_ptr), value :: ang
    end function
    integer(c_int) function roms_gpu_extract_objects_file(path) bind(c)
      import :: c_int, c_char
      character(kind=c_char), intent(in) :: path(*)
    end function
    integer(c_int) function roms_gpu_calc_extract(t) bind(c)
      import :: c_int, roms_tlev
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_wrt_extract(path, rec, total_rec, time, t) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: rec, total_rec
      real(c_double), value :: time
      type(roms_tlev), intent(in) :: t
    end function
    integer(c_int) function roms_gpu_extract_state(nobj, mismatch, N_chd, np_total, need_huv) bind(c)
      import :: c_int
      integer(c_int), intent(out) :: nobj, mismatch, N_chd, np_total, need_huv
    end function
    integer(c_int) function roms_gpu_extract_object_info(iobj, np, start_idx, vars, unsupported, scalar) bind(c)
      import :: c_int
      integer(c_int), value :: iobj
      integer(c_int), intent(out) :: np, start_idx, vars, unsupported, scalar
    end function
    integer(c_int) function roms_gpu_extract_object_coef(iobj, grid, ip, jp, coef, cosa, sina) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: iobj, grid
      integer(c_int), intent(out) :: ip(*), jp(*)
      real(c_double), intent(out) :: coef(*), cosa(*), sina(*)
    end function
    integer(c_int) function roms_gpu_extract_child_cs(cs_w) bind(c)
      import :: c_int, c_double
      real(c_double), intent(out) :: cs_w(*)
    end function
    integer(c_int) function roms_gpu_extract_copy_out(iobj, var_bit, dst, count) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: iobj, var_bit
      real(c_double), intent(out) :: dst(*)
      integer(c_long), value :: count
    end function
    integer(c_int) function roms_gpu_time_calc_extract(n, t, ms) bind(c)
      import :: c_int, c_double, roms_tlev
      integer(c_int), value :: n
      type(roms_tlev), intent(in) :: t
      real(c_double), intent(out) :: ms(2)
    end function
    integer(c_int) function roms_gpu_extract_locate(nx, ny, iSW_corn, jSW_corn, npg, ipos, jpos, start_idx, np) bind(c)
      import :: c_int, c_long, c_double
      integer(c_int), value :: nx, ny, iSW_corn, jSW_corn
      integer(c_long), value :: npg
      real(c_double), intent(in) :: ipos(*), jpos(*)
      integer(c_int), intent(out) :: start_idx, np
    end function
    integer(c_int) function roms_gpu_io_wait() bind(c)
      import :: c_int
    end function
    integer(c_int) function roms_gpu_get_init(path, req_rec, tindx, t, start_time) bind(c)
      import :: c_int, c_double, c_char, roms_tlev
      character(kind=c_char), intent(in) :: path(*)
      integer(c_int), value :: req_rec, tindx
      type(roms_tlev), intent(inout) :: t
      real(c_double), intent(out) :: start_time
    end function
    ! set_frc_data / set_tides on the device (k_forcing.hip)
    integer(c_int) function roms_gpu_frc_record(field_id, slot, rec_time, data) bind(c)
      import :: c_int, c_double
      integer(c_int), value :: field_id, slot
      real(c_double), value :: rec_time
      real(c_double), intent(in) :: data(*)
    end function
    integer(c_int) function roms_gpu_frc_interp(modtime, kinds) bind(c)
      import :: c_int, c_double
      real(c_double), value :: modtime
      integer(c_int), value :: kinds
    end function
    ! the tidal arrays are c_loc(...) of (GLOBAL_2D_ARRAY, ntides) arrays, or c_null_ptr
    integer(c_int) function roms_gpu_frc_clock(start_time, on) bind(c)
      import :: c_int, c_double
      real(c_double), value :: start_time
      integer(c_int), value :: on
    end function
    integer(c_int) function roms_gpu_set_tide_data(ntides, ftide, pot_re, pot_im, ztide_re, ztide_im, &
                                                   utide_re, utide_im, vtide_re, vtide_im) bind(c)
      import :: c_int, c_double, c_ptr
      integer(c_int), value :: ntides
      real(c_double), intent(in) :: ftide(*)
      type(c_ptr), value :: pot_re, pot_im, ztide_re, ztide_im, utide_re, utide_im, vtide_re, vtide_im
    end function
    integer(c_int) function roms_gpu_set_tides(time) bind(c)
      import :: c_int, c_double
      real(c_double), value :: time
    end function
    integer(c_int) function roms_gpu_comm_unique_id(id128) bind(c)
      import :: c_int, c_char
      character(kind=c_char), intent(out) :: id128(128)
    end function
    integer(c_int) function roms_gpu_comm_create(id128, nranks, rank, device, comm) bind(c)
      import :: c_int, c_char, c_ptr
      character(kind=c_char), intent(in) :: id128(128)
      integer(c_int), value :: nranks, rank, device
      type(c_ptr), intent(out) :: comm
    end function
    ! host channel: allgather is c_funloc of a bind(c) function
    ! integer(c_int) function f(ctx, send, nbytes, recv) (MPI_Allgather of
    ! MPI_BYTE over the model's communicator; INTEGRATION.md)
    integer(c_int) function roms_gpu_comm_create_host(nranks, rank, device, allgather, ctx, comm) bind(c)
      import :: c_int, c_ptr, c_funptr
      integer(c_int), value :: nranks, rank, device
      type(c_funptr), value :: allgather
      type(c_ptr), value :: ctx
      type(c_ptr), intent(out) :: comm
    end function
    integer(c_int) function roms_gpu_comm_destroy(comm) bind(c)
      import :: c_int, c_ptr
      type(c_ptr), value :: comm
    end function
    ! 1: IPC peer writes, 0: RCCL send/recv (or one rank), -1: a wait timed out
    integer(c_int) function roms_gpu_halo_transport() bind(c)
      import :: c_int
    end function
  end interface

contains

  ! abort with the library's message (error_log%raise + abort_check analogue)
  subroutine roms_gpu_check(rc, what)
    integer(c_int), intent(in) :: rc
    character(*), intent(in) :: what
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if (rc == 0) return
    call c_f_pointer(roms_gpu_last_error(), msg, [1024])
    n = 0
    do while (n < 1024)
      if (msg(n + 1) == c_null_char) exit
      n = n + 1
    end do
    write(*, '(3a,i0,2a)') 'roms_gpu: ', what, ' failed (', rc, '): ', transfer(msg(1:n), repeat(' ', n))
    error stop 1
  end subroutine

end module roms_gpu_mod
