"""Records tests/golden/tdiag_golden.npz: the tracer budget terms Tdiag of the reference's own corrector --
the whole of step3d_t_iso_tile (src/step3d_t_ISO.F) and the routines of src/diagnostics.F it calls, compiled
unchanged with -DDIAGNOSTICS and diag_trc = .true., diag_avg = .false. through cpp | mpc.py | flang -O2
-ffp-contract=off, the way oracle/ref/build_ref.sh compiles its routines -- on fixed pseudo-random inputs: an
8 x 8 x 4 grid, closed on every side, MASKING with one land cell, SALINITY, NT = 2, both tracers armed.
tests/test_tdiag_ref.py requires the numpy restatement (tests/tdiag_ref.py) to reproduce it bit for bit.

The routine is reached through a small harness library that is not part of this repository (stand-in modules for
what the corrector does not exercise: netCDF, exchanges, pipes, rivers, bulk fluxes); it exports
  tdg_info(int iv[4])                        LLm, MMm, N, nt
  tdg_shapes(int iv[10])                     shape(Tdiag) (5), shape(Akt) (4)
  tdg_run(int iv[3], dt, t, FlxU, FlxV, We, Wi, Hz, Akt, pm, pn, rmask, umask, vmask, sentinel, Tdiag, t_out)
with iv = nstp, nrhs, nnew and every array flat in the module's storage order (GLOBAL_2D_ARRAY = -1:Lm+2, -1:Mm+2;
t with its three time slots and NT tracers; Tdiag (0:nx+1, 0:ny+1, nz, 7, ntdia)).  It sets one rank that owns the
whole grid, copies the inputs into the modules, calls init_diagnostics, fills Tdiag with the sentinel below -- so
the ranges the corrector writes show in the recording -- and calls step3d_t(0).  stflx, srflx and swflx are 0.

usage: python tests/golden/tdiag_golden.py libtdg.so
"""
import ctypes
import os
import sys

import numpy as np

SEED = 20261021
SENTINEL = -777.0
NSTP, NRHS, NNEW = 2, 3, 1
DT = 30.0
LAND = (4, 5)   # (i, j) of the land cell


def inputs(Lm, Mm, N, NT, akt_shape):
    """Fixed pseudo-random inputs, every ghost cell included; Hz, pm, pn, Akt positive; masks of one land cell."""
    r = np.random.default_rng(SEED)
    sh = (Mm + 4, Lm + 4)
    t = r.normal(10.0, 1.0, (NT, 3, N) + sh)
    t[:, NNEW - 1] = r.normal(100.0, 10.0, (NT, N) + sh)        # Hz*t of pre_step3d
    d = dict(t=t, FlxU=r.normal(0.0, 50.0, (N,) + sh), FlxV=r.normal(0.0, 50.0, (N,) + sh),
             We=r.normal(0.0, 20.0, (N + 1,) + sh), Wi=r.normal(0.0, 5.0, (N + 1,) + sh),
             Hz=r.uniform(5.0, 20.0, (N,) + sh), Akt=r.uniform(1e-4, 1e-2, akt_shape),
             pm=r.uniform(0.8e-3, 1.3e-3, sh), pn=r.uniform(0.7e-3, 1.4e-3, sh))
    rmask, umask, vmask = np.ones(sh), np.ones(sh), np.ones(sh)
    i, j = LAND
    rmask[j + 1, i + 1] = 0.0
    umask[j + 1, i + 1] = umask[j + 1, i + 2] = 0.0
    vmask[j + 1, i + 1] = vmask[j + 2, i + 1] = 0.0
    d.update(rmask=rmask, umask=umask, vmask=vmask)
    return {k: np.ascontiguousarray(a) for k, a in d.items()}


def main(path):
    L = ctypes.CDLL(os.path.abspath(path))
    iv = (ctypes.c_int * 4)()
    L.tdg_info(iv)
    Lm, Mm, N, NT = list(iv)
    x = inputs(Lm, Mm, N, NT, (2, N + 1, Mm + 4, Lm + 4))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    D = lambda v: ctypes.byref(ctypes.c_double(v))
    Td = np.zeros((NT, 7, N, Mm + 2, Lm + 2))
    tout = np.zeros_like(x["t"])
    L.tdg_run((ctypes.c_int * 3)(NSTP, NRHS, NNEW), D(DT), P(x["t"]), P(x["FlxU"]), P(x["FlxV"]), P(x["We"]), P(x["Wi"]),
              P(x["Hz"]), P(x["Akt"]), P(x["pm"]), P(x["pn"]), P(x["rmask"]), P(x["umask"]), P(x["vmask"]), D(SENTINEL),
              P(Td), P(tout))
    sv = (ctypes.c_int * 10)()
    L.tdg_shapes(sv)
    assert list(sv)[:5] == [Lm + 2, Mm + 2, N, 7, NT] and list(sv)[5:9] == [Lm + 4, Mm + 4, N + 1, 2], list(sv)
    out = dict(x)
    out.update(dims=np.array([Lm, Mm, N, NT, NSTP, NRHS, NNEW]), dt=np.array(DT), sentinel=np.array(SENTINEL),
               Tdiag=Td, t_out=tout)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tdiag_golden.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
