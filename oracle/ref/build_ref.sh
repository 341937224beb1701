#!/bin/bash
# build_ref.sh -- TEST INFRASTRUCTURE ONLY.
#
# Compiles the reference's own open-boundary routines (zetabc, u2dbc_im,
# v2dbc_im, u3dbc_im, v3dbc_im, t3dbc_im), set_nudgcof and bulk_frc,
# unchanged, into small shared libraries under oracle/_ref/, so that the
# CPU oracle can be compared with them routine by routine
# (tests/test_ref_pin_obc.py, tests/test_ref_pin_bulk.py).
#
# From the reference tree come, read in place through cpp | mpc.py | flang
# as fortran/refbuild/build_dropins.sh does: param, hidden_mpi_vars,
# dimensions, scalars, ocean_vars, private_scratch, mixing, bulk_frc and the
# seven routine files, with their includes found through -I.  Ours are the
# stand-in modules (standins.F, standins_io.F), the C entry points
# (harness.F90), the MPI shim of fortran/refbuild and the three option files
# written below from the lists SWITCHES and SIZES.  Grid size and open sides
# are compile-time in the reference, hence one library per set of open sides
# (all fifteen, obc1 .. obc15), and one more for the bulk fluxes with LMD_KPP, the switch bulk_frc itself
# asks about (the short-wave flux under ice).
#
# Five more libraries hold prsgrd, step3d_uv2 and step3d_t_ISO.F with ADV_ISONEUTRAL (tests/test_ref_pin_iso.py,
# tests/test_gpu_iso.py): from the tree also eos_vars, coupling, strings and lenstr; ours the stand-ins of
# standins_iso.F (tides, calc_pflx_mod, river_frc, pipe_frc, mpi_exchanges) and the entry points of harness_iso.F90.
# cpp reports an unterminated #ifdef for step3d_uv2.F: its "# ifdef MASKING" at the v correction has no "# endif",
# which costs nothing with MASKING defined, as it is in every library here.
#
# Nothing is written outside oracle/_ref/, which git ignores.  Without a
# reference tree the script does nothing and succeeds.
#   usage: oracle/ref/build_ref.sh            (REF=/path/to/reference)
set -e
REF=${REF:-/root/reference}
[ -d "$REF/src" ] || exit 0
HERE=$(cd "$(dirname "$0")" && pwd)
REPO=$(cd "$HERE/../.." && pwd)
OUT=$REPO/oracle/_ref
FC=${FC:-/opt/rocm/llvm/bin/flang}
MPC=$REF/Tools-Roms/mpc_python/mpc.py
# no fast-math, no contraction: every expression evaluates as written
FFLAGS=${REF_FFLAGS:--O2 -ffp-contract=off -fPIC}

# the Iceland boundary set that the tests' obc_cfg mirrors; no MARBL, RIVERS,
# TIDES, SPHERICAL
SWITCHES="SOLVE3D MASKING CURVGRID OBC_M2FLATHER OBC_M3ORLANSKI OBC_TORLANSKI
 Z_FRC_BRY M2_FRC_BRY M3_FRC_BRY T_FRC_BRY SPONGE SPONGE_TUNE SALINITY UV_VIS2 TS_DIF2"
# non-square on purpose: a swapped extent shows
SIZES="LLm=24 MMm=20 N=6 NP_XI=1 NP_ETA=1 NSUB_X=1 NSUB_E=1 nt=2"
# library : open sides (bits 1 W, 2 E, 4 S, 8 N) : further switches
VARIANTS="$(for b in 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15; do printf 'obc%d:%d: ' $b $b; done)bulk:15:LMD_MIXING,LMD_KPP"
# ADV_ISONEUTRAL: the basin with the split EOS and both boundary layers, closed and with three sets of open sides
# (every side copies and zeroes LapT, every corner lies between one of each), and the doubly periodic Filament set
# with the linear EOS and no LMD, which has its own base list
ISO_MORE="ADV_ISONEUTRAL,UV_ADV,UV_COR,NONLIN_EOS,SPLIT_EOS,LMD_MIXING,LMD_KPP,LMD_BKPP"
VARIANTS="$VARIANTS iso0:0:$ISO_MORE iso6:6:$ISO_MORE iso9:9:$ISO_MORE iso15:15:$ISO_MORE isoper:0:ADV_ISONEUTRAL:per"
PER_SWITCHES="SOLVE3D MASKING UV_ADV UV_COR UV_VIS2 TS_DIF2 EW_PERIODIC NS_PERIODIC"
BULK_FIELDS="uwnd vwnd tair Q prate lwrad swrad"

REFSRC="param hidden_mpi_vars dimensions scalars ocean_vars private_scratch"
ROUTINES="zetabc u2dbc_im v2dbc_im u3dbc_im v3dbc_im t3dbc_im set_nudgcof"
ISO_REFSRC="eos_vars coupling strings lenstr"
ISO_ROUTINES="prsgrd step3d_uv2 step3d_t_ISO"
OURS="build_ref.sh standins.F standins_io.F standins_iso.F harness.F90 harness_iso.F90"

pp() { cpp -P -traditional -D__IFC -I"$REF/src" < "$1" | python3 "$MPC" > "$2"; }
fc() { $FC -c $FFLAGS "$1" -o "${1%.*}.o"; }

mkdir -p "$OUT"
for v in $VARIANTS; do
  IFS=: read -r name obc more base <<< "$v"
  switches=$SWITCHES; [ "$base" = per ] && switches=$PER_SWITCHES
  iso=; case $name in iso*) iso=1;; esac
  lib=$OUT/libref_$name.so
  # up to date: newer than everything of ours that goes into it
  if [ -f "$lib" ] && [ -z "$(cd "$HERE" && find $OURS "$REPO/fortran/refbuild/mpi_f08_shim.f90" -newer "$lib")" ]; then
    continue
  fi
  W=$OUT/build_$name
  rm -rf "$W" && mkdir -p "$W" && cd "$W"
  # option files: quoted includes are looked up in the working directory first
  {
    for s in $switches ${more//,/ }; do echo "#define $s"; done
    [ $((obc & 1)) -ne 0 ] && echo "#define OBC_WEST"
    [ $((obc & 2)) -ne 0 ] && echo "#define OBC_EAST"
    [ $((obc & 4)) -ne 0 ] && echo "#define OBC_SOUTH"
    [ $((obc & 8)) -ne 0 ] && echo "#define OBC_NORTH"
    echo '#include "set_global_definitions.h"'
  } > cppdefs.opt
  for s in $SIZES; do echo "      integer, parameter :: $s"; done > param.opt
  {
    echo "      integer :: interp_frc = 0"
    echo "      logical :: do_check_units = .false."
    for f in $BULK_FIELDS; do echo "      type (ncforce) :: nc_$f = ncforce(vname='$f', tname='time')"; done
  } > bulk_frc.opt

  cp "$REPO/fortran/refbuild/mpi_f08_shim.f90" . && fc mpi_f08_shim.f90
  for m in $REFSRC; do pp "$REF/src/$m.F" $m.f && fc $m.f; done
  pp "$HERE/standins.F" standins.f && fc standins.f
  pp "$REF/src/mixing.F" mixing.f && fc mixing.f
  pp "$HERE/standins_io.F" standins_io.f && fc standins_io.f
  if [ -n "$iso" ]; then
    for m in $ISO_REFSRC; do pp "$REF/src/$m.F" $m.f && fc $m.f; done
    pp "$HERE/standins_iso.F" standins_iso.f && fc standins_iso.f
  fi
  for m in $ROUTINES; do pp "$REF/src/$m.F" $m.f && fc $m.f; done
  pp "$REF/src/bulk_frc.F" bulk_frc.f && fc bulk_frc.f
  cpp -P -traditional -I"$REF/src" < "$HERE/harness.F90" > harness.f90 && fc harness.f90
  if [ -n "$iso" ]; then
    for m in $ISO_ROUTINES; do pp "$REF/src/$m.F" $m.f && fc $m.f; done
    cpp -P -traditional -I"$REF/src" < "$HERE/harness_iso.F90" > harness_iso.f90 && fc harness_iso.f90
  fi
  # the Fortran runtime is linked in from its archive, so the library loads
  # wherever oracle/_ref/ is copied; the rpath covers a shared runtime
  $FC -shared -Wl,-Bsymbolic -o "$lib.tmp" *.o -Wl,-rpath,/opt/rocm/llvm/lib -Wl,-rpath,/opt/rocm/lib/llvm/lib
  mv "$lib.tmp" "$lib"
  cd "$OUT" && rm -rf "$W"
done
