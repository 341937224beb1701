#include "cppdefs.opt"
! harness.F90 -- TEST INFRASTRUCTURE ONLY (see oracle/ref/build_ref.sh).
!
! C entry points around the boundary routines, set_nudgcof and
! set_bulk_frc of the reference, compiled unchanged beside this file.
! The harness allocates the module arrays for one rank that owns the
! whole grid, copies a state in, sets the time indices and scalars,
! calls one routine on the tile (1:Lm,1:Mm) and copies the result out.
! All arrays cross the C boundary flat, in the storage order and with
! the ghost points the modules hold them in, which is also the layout
! of the oracle (oracle/roms_oracle.h).

! the switch sets without boundary forcing (the periodic library) have no ubind and no v_sponge
#if defined T_FRC_BRY || defined M2_FRC_BRY || defined M3_FRC_BRY || defined Z_FRC_BRY
# define HAVE_UBIND
#endif

module ref_harness
  use iso_c_binding, only: c_int, c_double
  implicit none
  private
  logical :: ready = .false.
  real(c_double), allocatable :: scratch(:,:)
  integer :: istr, iend, jstr, jend

contains

  ! compile-time facts of this library: LLm MMm N NT, open sides as the
  ! bits 1 W, 2 E, 4 S, 8 N, and g
  subroutine ref_info(iv, gv) bind(C, name="ref_info")
    use param, only: LLm, MMm, N, nt, obc_west, obc_east, obc_south, obc_north
    use scalars, only: g
    integer(c_int), intent(out) :: iv(5)
    real(c_double), intent(out) :: gv
    iv(1) = LLm; iv(2) = MMm; iv(3) = N; iv(4) = nt
    iv(5) = merge(1, 0, obc_west) + merge(2, 0, obc_east) + merge(4, 0, obc_south) + merge(8, 0, obc_north)
    gv = g
  end subroutine ref_info

  subroutine ref_init() bind(C, name="ref_init")
    use param, only: Lm, Mm, mynode, iSW_corn, jSW_corn, iwest, ieast, jsouth, jnorth, &
                     west_exchng, east_exchng, south_exchng, north_exchng
    use hidden_mpi_vars, only: inode, jnode, west_msg_exch, east_msg_exch, south_msg_exch, north_msg_exch
    use dimensions, only: init_dimensions
    use scalars, only: init, visc2, tnu2, Akv_bak, Akt_bak, rho0, gamma2
#ifdef SPONGE
    use scalars, only: v_sponge
#endif
#ifdef HAVE_UBIND
    use scalars, only: ubind
#endif
    use ocean_vars, only: init_arrays_ocean
    use private_scratch, only: init_arrays_private_scratch
    use grid, only: init_arrays_grid
    use boundary, only: init_arrays_boundary
    use tracers, only: init_arrays_tracers
    use sponge_tune, only: init_arrays_sponge_tune
    use surf_flux, only: init_arrays_surf_flux
    use bulk_frc, only: init_arrays_bulk_frc
    if (ready) return
    ! one rank, one tile, no neighbours
    mynode = 0; inode = 0; jnode = 0; iSW_corn = 0; jSW_corn = 0
    iwest = 1; ieast = Lm; jsouth = 1; jnorth = Mm
    west_exchng = .false.; east_exchng = .false.; south_exchng = .false.; north_exchng = .false.
    west_msg_exch = .false.; east_msg_exch = .false.; south_msg_exch = .false.; north_msg_exch = .false.
    init = 0.0d0; visc2 = 0.0d0; tnu2 = 0.0d0; Akv_bak = 0.0d0; Akt_bak = 0.0d0
    rho0 = 1000.0d0; gamma2 = 1.0d0
#ifdef SPONGE
    v_sponge = 0.0d0
#endif
#ifdef HAVE_UBIND
    ubind = 0.0d0
#endif
    call init_dimensions
    call init_arrays_ocean
    call init_arrays_private_scratch
    call init_arrays_grid
    call init_arrays_boundary
    call init_arrays_tracers
    call init_arrays_sponge_tune
    call init_arrays_surf_flux
    call init_arrays_bulk_frc
    istr = 1; iend = Lm; jstr = 1; jend = Mm
    allocate(scratch(PRIVATE_2D_SCRATCH_ARRAY))
    scratch = 0.0d0
    ready = .true.
  end subroutine ref_init

  subroutine ref_set_grid(a_h, a_pm, a_pn, a_rmask, a_umask, a_vmask, a_pmask) bind(C, name="ref_set_grid")
    use grid, only: h, pm, pn, rmask, umask, vmask, pmask
    real(c_double), intent(in) :: a_h(*), a_pm(*), a_pn(*), a_rmask(*), a_umask(*), a_vmask(*), a_pmask(*)
    h = reshape(a_h(1:size(h)), shape(h))
    pm = reshape(a_pm(1:size(pm)), shape(pm))
    pn = reshape(a_pn(1:size(pn)), shape(pn))
    rmask = reshape(a_rmask(1:size(rmask)), shape(rmask))
    umask = reshape(a_umask(1:size(umask)), shape(umask))
    vmask = reshape(a_vmask(1:size(vmask)), shape(vmask))
    pmask = reshape(a_pmask(1:size(pmask)), shape(pmask))
  end subroutine ref_set_grid

  ! iv: kstp knew nstp nrhs nnew ub_tune;  dv: dt dtfast ubind gamma2 rho0
  subroutine ref_set_scalars(iv, dv) bind(C, name="ref_set_scalars")
    use scalars, only: kstp, knew, nstp, nrhs, nnew, dt, dtfast, gamma2, rho0
#ifdef HAVE_UBIND
    use scalars, only: ubind
#endif
    use sponge_tune, only: ub_tune
    integer(c_int), intent(in) :: iv(6)
    real(c_double), intent(in) :: dv(5)
    kstp = iv(1); knew = iv(2); nstp = iv(3); nrhs = iv(4); nnew = iv(5)
    ub_tune = iv(6) /= 0
    dt = dv(1); dtfast = dv(2); gamma2 = dv(4); rho0 = dv(5)
#ifdef HAVE_UBIND
    ubind = dv(3)
#endif
  end subroutine ref_set_scalars

  subroutine ref_set_ocean(a_zeta, a_ubar, a_vbar, a_u, a_v, a_t) bind(C, name="ref_set_ocean")
    use ocean_vars, only: zeta, ubar, vbar, u, v
    use tracers, only: t
    real(c_double), intent(in) :: a_zeta(*), a_ubar(*), a_vbar(*), a_u(*), a_v(*), a_t(*)
    zeta = reshape(a_zeta(1:size(zeta)), shape(zeta))
    ubar = reshape(a_ubar(1:size(ubar)), shape(ubar))
    vbar = reshape(a_vbar(1:size(vbar)), shape(vbar))
    u = reshape(a_u(1:size(u)), shape(u))
    v = reshape(a_v(1:size(v)), shape(v))
    t = reshape(a_t(1:size(t)), shape(t))
  end subroutine ref_set_ocean

  subroutine ref_get_ocean(a_zeta, a_ubar, a_vbar, a_u, a_v, a_t) bind(C, name="ref_get_ocean")
    use ocean_vars, only: zeta, ubar, vbar, u, v
    use tracers, only: t
    real(c_double), intent(out) :: a_zeta(*), a_ubar(*), a_vbar(*), a_u(*), a_v(*), a_t(*)
    a_zeta(1:size(zeta)) = reshape(zeta, [size(zeta)])
    a_ubar(1:size(ubar)) = reshape(ubar, [size(ubar)])
    a_vbar(1:size(vbar)) = reshape(vbar, [size(vbar)])
    a_u(1:size(u)) = reshape(u, [size(u)])
    a_v(1:size(v)) = reshape(v, [size(v)])
    a_t(1:size(t)) = reshape(t, [size(t)])
  end subroutine ref_get_ocean

  ! side: 0 west, 1 east, 2 south, 3 north
  subroutine ref_set_bry(side, a_zeta, a_ubar, a_vbar, a_u, a_v, a_t) bind(C, name="ref_set_bry")
    use boundary
    integer(c_int), value :: side
    real(c_double), intent(in) :: a_zeta(*), a_ubar(*), a_vbar(*), a_u(*), a_v(*), a_t(*)
    select case (side)
    case (0)
      zeta_west(:) = a_zeta(1:size(zeta_west)); ubar_west(:) = a_ubar(1:size(ubar_west))
      vbar_west(:) = a_vbar(1:size(vbar_west))
      u_west = reshape(a_u(1:size(u_west)), shape(u_west)); v_west = reshape(a_v(1:size(v_west)), shape(v_west))
      t_west = reshape(a_t(1:size(t_west)), shape(t_west))
    case (1)
      zeta_east(:) = a_zeta(1:size(zeta_east)); ubar_east(:) = a_ubar(1:size(ubar_east))
      vbar_east(:) = a_vbar(1:size(vbar_east))
      u_east = reshape(a_u(1:size(u_east)), shape(u_east)); v_east = reshape(a_v(1:size(v_east)), shape(v_east))
      t_east = reshape(a_t(1:size(t_east)), shape(t_east))
    case (2)
      zeta_south(:) = a_zeta(1:size(zeta_south)); ubar_south(:) = a_ubar(1:size(ubar_south))
      vbar_south(:) = a_vbar(1:size(vbar_south))
      u_south = reshape(a_u(1:size(u_south)), shape(u_south)); v_south = reshape(a_v(1:size(v_south)), shape(v_south))
      t_south = reshape(a_t(1:size(t_south)), shape(t_south))
    case (3)
      zeta_north(:) = a_zeta(1:size(zeta_north)); ubar_north(:) = a_ubar(1:size(ubar_north))
      vbar_north(:) = a_vbar(1:size(vbar_north))
      u_north = reshape(a_u(1:size(u_north)), shape(u_north)); v_north = reshape(a_v(1:size(v_north)), shape(v_north))
      t_north = reshape(a_t(1:size(t_north)), shape(t_north))
    end select
  end subroutine ref_set_bry

  ! binding coefficients, handed over on the points 0:Mm+1 / 0:Lm+1 of the
  ! boundary data; the module keeps the interior points 1:ny / 1:nx
  subroutine ref_set_ub(w, e, s, n) bind(C, name="ref_set_ub")
    use sponge_tune, only: ub_west, ub_east, ub_south, ub_north
    real(c_double), intent(in) :: w(0:*), e(0:*), s(0:*), n(0:*)
    ub_west(:) = w(1:size(ub_west)); ub_east(:) = e(1:size(ub_east))
    ub_south(:) = s(1:size(ub_south)); ub_north(:) = n(1:size(ub_north))
  end subroutine ref_set_ub

  subroutine ref_zetabc(zeta_new) bind(C, name="ref_zetabc")
    real(c_double), intent(inout) :: zeta_new(*)
    external :: zetabc_tile
    call zetabc_tile(istr, iend, jstr, jend, zeta_new)
  end subroutine ref_zetabc

  subroutine ref_u2dbc() bind(C, name="ref_u2dbc")
    external :: u2dbc_tile
    call u2dbc_tile(istr, iend, jstr, jend, scratch)
  end subroutine ref_u2dbc

  subroutine ref_v2dbc() bind(C, name="ref_v2dbc")
    external :: v2dbc_tile
    call v2dbc_tile(istr, iend, jstr, jend, scratch)
  end subroutine ref_v2dbc

  subroutine ref_u3dbc() bind(C, name="ref_u3dbc")
    external :: u3dbc_tile
    call u3dbc_tile(istr, iend, jstr, jend, scratch)
  end subroutine ref_u3dbc

  subroutine ref_v3dbc() bind(C, name="ref_v3dbc")
    external :: v3dbc_tile
    call v3dbc_tile(istr, iend, jstr, jend, scratch)
  end subroutine ref_v3dbc

  subroutine ref_t3dbc(itrc) bind(C, name="ref_t3dbc")
    integer(c_int), value :: itrc
    integer :: it
    external :: t3dbc_tile
    it = itrc
    call t3dbc_tile(istr, iend, jstr, jend, it, scratch)
  end subroutine ref_t3dbc

#ifdef SPONGE
  ! init_arrays_mixing sets visc2_r = visc2_p = visc2 and diff2 = tnu2,
  ! set_nudgcof adds the sponge bands
  subroutine ref_set_nudgcof(a_vsponge, a_visc2, a_tnu2, o_visc2_r, o_visc2_p, o_diff2) bind(C, name="ref_set_nudgcof")
    use param, only: mynode
    use scalars, only: v_sponge, visc2, tnu2
    use mixing
    real(c_double), value :: a_vsponge, a_visc2
    real(c_double), intent(in) :: a_tnu2(*)
    real(c_double), intent(out) :: o_visc2_r(*), o_visc2_p(*), o_diff2(*)
    external :: set_nudgcof
    if (allocated(visc2_r)) then
      deallocate(visc2_r, visc2_p, diff2, Akv, Akt)
#ifdef LMD_KPP
      deallocate(bvf, hbls, swr_frac)
#endif
    endif
    v_sponge = a_vsponge; visc2 = a_visc2; tnu2(:) = a_tnu2(1:size(tnu2))
    call init_arrays_mixing
    mynode = 1          ! only rank 0 prints the width of the sponge
    call set_nudgcof(0)
    mynode = 0
    o_visc2_r(1:size(visc2_r)) = reshape(visc2_r, [size(visc2_r)])
    o_visc2_p(1:size(visc2_p)) = reshape(visc2_p, [size(visc2_p)])
    o_diff2(1:size(diff2)) = reshape(diff2, [size(diff2)])
  end subroutine ref_set_nudgcof
#endif

  ! atmosphere in; t, u, v, the masks, nrhs and rho0 as set before.  The
  ! flux arrays go in and out: the routine leaves some ghost points, and
  ! the salinity component of stflx apart from its mask, as they were.
  subroutine ref_bulk(a_uwnd, a_vwnd, a_tair, a_q, a_prate, a_lwrad, a_swrad, &
                      io_sustr, io_svstr, io_sustr_r, io_svstr_r, io_stflx, io_swflx, o_srflx) bind(C, name="ref_bulk")
    use surf_flux, only: uwnd, vwnd, srflx, sustr, svstr, sustr_r, svstr_r, stflx, swflx
    use bulk_frc, only: tair, Q, prate, lwrad, set_bulk_frc
    real(c_double), intent(in) :: a_uwnd(*), a_vwnd(*), a_tair(*), a_q(*), a_prate(*), a_lwrad(*), a_swrad(*)
    real(c_double), intent(inout) :: io_sustr(*), io_svstr(*), io_sustr_r(*), io_svstr_r(*), io_stflx(*), io_swflx(*)
    real(c_double), intent(out) :: o_srflx(*)
    integer :: n2
    n2 = size(uwnd)
    uwnd = reshape(a_uwnd(1:n2), shape(uwnd)); vwnd = reshape(a_vwnd(1:n2), shape(vwnd))
    tair = reshape(a_tair(1:n2), shape(tair)); Q = reshape(a_q(1:n2), shape(Q))
    prate = reshape(a_prate(1:n2), shape(prate)); lwrad = reshape(a_lwrad(1:n2), shape(lwrad))
    srflx = reshape(a_swrad(1:n2), shape(srflx))
    stflx = reshape(io_stflx(1:size(stflx)), shape(stflx))
    sustr = reshape(io_sustr(1:n2), shape(sustr)); svstr = reshape(io_svstr(1:n2), shape(svstr))
    sustr_r = reshape(io_sustr_r(1:n2), shape(sustr_r)); svstr_r = reshape(io_svstr_r(1:n2), shape(svstr_r))
    swflx = reshape(io_swflx(1:n2), shape(swflx))
    call set_bulk_frc(istr, iend, jstr, jend)
    io_sustr(1:n2) = reshape(sustr, [n2]); io_svstr(1:n2) = reshape(svstr, [n2])
    io_sustr_r(1:n2) = reshape(sustr_r, [n2]); io_svstr_r(1:n2) = reshape(svstr_r, [n2])
    io_stflx(1:size(stflx)) = reshape(stflx, [size(stflx)])
    io_swflx(1:n2) = reshape(swflx, [n2]); o_srflx(1:n2) = reshape(srflx, [n2])
  end subroutine ref_bulk

end module ref_harness
