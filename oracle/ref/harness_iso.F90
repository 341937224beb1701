#include "cppdefs.opt"
! harness_iso.F90 -- TEST INFRASTRUCTURE ONLY (see oracle/ref/build_ref.sh).
!
! C entry points around the three routines of the reference that make up
! ADV_ISONEUTRAL -- prsgrd (the slopes dRdx, dRde of the corrector),
! step3d_uv2 (diff3u, diff3v, idRz) and step3d_t (the rotated biharmonic
! operator and Akz) -- compiled unchanged beside this file, for the
! libraries built with that switch.  ref_init, ref_set_grid, ref_set_scalars,
! ref_set_ocean and ref_set_bry of harness.F90 come first; the entry points
! here allocate the further modules, copy the further arrays in and out by
! number, fill the private scratch with a value, and call the routines the
! way the time step does.  Arrays cross flat, in the modules' storage order.

module ref_harness_iso
  use iso_c_binding, only: c_int, c_double
  implicit none
  private
  logical :: ready = .false.

contains

  ! 1 when the library is periodic in (xi, eta), 1 when its EOS is split, 1 with LMD_KPP
  subroutine ref_iso_info(iv) bind(C, name="ref_iso_info")
    integer(c_int), intent(out) :: iv(4)
    iv = 0
#ifdef EW_PERIODIC
    iv(1) = 1
#endif
#ifdef NS_PERIODIC
    iv(2) = 1
#endif
#ifdef SPLIT_EOS
    iv(3) = 1
#endif
#ifdef LMD_KPP
    iv(4) = 1
#endif
  end subroutine ref_iso_info

  subroutine ref_iso_init() bind(C, name="ref_iso_init")
    use eos_vars, only: init_arrays_eos_vars
    use coupling, only: init_arrays_coupling
    use mixing, only: init_arrays_mixing
    if (ready) return
    call init_arrays_eos_vars
    call init_arrays_coupling
    call init_arrays_mixing
    ready = .true.
  end subroutine ref_iso_init

  ! the arrays by number; oracle/ref/__init__.py holds the same table
  subroutine move(id, a, put)
    use ocean_vars, only: Hz, z_r, z_w, FlxU, FlxV, We, Wi
    use eos_vars
    use mixing
    use coupling, only: DU_avg1, DV_avg1, DU_avg2, DV_avg2
    use grid, only: f, dm_r, dn_r, dm_u, dn_u, dm_v, dn_v
    use surf_flux, only: stflx, srflx, swflx
    use private_scratch, only: A3d
    use param, only: Lm, Mm
    use scalars, only: N
    integer, intent(in) :: id
    real(c_double), intent(inout) :: a(*)
    logical, intent(in) :: put
    integer :: nakz
    select case (id)
    case (1); call m3(Hz)
    case (2); call m3(z_r)
    case (3); call m3(z_w)
    case (4); call m3(FlxU)
    case (5); call m3(FlxV)
    case (6); call m3(We)
    case (7); call m3(Wi)
#ifdef SPLIT_EOS
    case (8); call m3(rho1)
    case (9); call m3(qp1)
#else
    case (10); call m3(rho)
#endif
    case (11); call m3(dRdx)
    case (12); call m3(dRde)
    case (13); call m3(idRz)
    case (14); call m3(diff3u)
    case (15); call m3(diff3v)
    case (16)           ! Akz: the second 3-D private scratch array, (istr-2:iend+2, jstr-2:jend+2, 0:N)
      nakz = (Lm + 4) * (Mm + 4) * (N + 1)
      if (put) then
        A3d(1:nakz, 2) = a(1:nakz)
      else
        a(1:nakz) = A3d(1:nakz, 2)
      endif
    case (17); call m4(Akt)
    case (18); call m3(Akv)
#ifdef LMD_KPP
    case (19); call m2(hbls)
    case (21); call m3(swr_frac)
#endif
#ifdef LMD_BKPP
    case (20); call m2(hbbl)
#endif
    case (22); call m2(DU_avg1)
    case (23); call m2(DV_avg1)
    case (24); call m2(DU_avg2)
    case (25); call m2(DV_avg2)
    case (26); call m2(f)
    case (27); call m2(dm_r)
    case (28); call m2(dn_r)
    case (29); call m2(dm_u)
    case (30); call m2(dn_u)
    case (31); call m2(dm_v)
    case (32); call m2(dn_v)
    case (33); call m3(stflx)
    case (34); call m2(srflx)
    case (35); call m2(swflx)
    case default
      error stop "ref_iso: no such array in this library"
    end select
  contains
    subroutine m2(x)
      real(c_double), intent(inout) :: x(:,:)
      if (put) then
        x = reshape(a(1:size(x)), shape(x))
      else
        a(1:size(x)) = reshape(x, [size(x)])
      endif
    end subroutine m2
    subroutine m3(x)
      real(c_double), intent(inout) :: x(:,:,:)
      if (put) then
        x = reshape(a(1:size(x)), shape(x))
      else
        a(1:size(x)) = reshape(x, [size(x)])
      endif
    end subroutine m3
    subroutine m4(x)
      real(c_double), intent(inout) :: x(:,:,:,:)
      if (put) then
        x = reshape(a(1:size(x)), shape(x))
      else
        a(1:size(x)) = reshape(x, [size(x)])
      endif
    end subroutine m4
  end subroutine move

  subroutine ref_iso_set(id, a) bind(C, name="ref_iso_set")
    integer(c_int), value :: id
    real(c_double), intent(inout) :: a(*)
    call move(int(id), a, .true.)
  end subroutine ref_iso_set

  subroutine ref_iso_get(id, a) bind(C, name="ref_iso_get")
    integer(c_int), value :: id
    real(c_double), intent(inout) :: a(*)
    call move(int(id), a, .false.)
  end subroutine ref_iso_get

  ! number of elements of the array id in this library
  function ref_iso_size(id) result(n) bind(C, name="ref_iso_size")
    use mixing, only: Akt
    use surf_flux, only: stflx
    integer(c_int), value :: id
    integer(c_int) :: n
    n = 0
    if (id == 17) n = size(Akt)
    if (id == 33) n = size(stflx)
  end function ref_iso_size

  ! every private scratch array holds v: what a routine reads there without
  ! having written it shows as a result that follows v
  subroutine ref_iso_fill(v) bind(C, name="ref_iso_fill")
    use private_scratch, only: A2d, A3d
    real(c_double), value :: v
    A2d = v
    A3d = v
  end subroutine ref_iso_fill

  ! 1 prsgrd, 2 the exchange of the slopes that step3d_uv1 makes after it,
  ! 3 step3d_uv2(0), 4 step3d_t(0)
  subroutine ref_iso_call(which) bind(C, name="ref_iso_call")
    use eos_vars, only: dRdx, dRde
    use mpi_exchanges, only: exchange_xxx
    integer(c_int), value :: which
    external :: prsgrd, step3d_uv2, step3d_t
    select case (which)
    case (1); call prsgrd
    case (2); call exchange_xxx(dRdx, dRde)
    case (3); call step3d_uv2(0)
    case (4); call step3d_t(0)
    end select
  end subroutine ref_iso_call

end module ref_harness_iso
