"""Records tests/golden/uvdiag_golden.npz: the momentum budget terms Udiag, Vdiag of the reference's own corrector --
src/prsgrd.F, src/step3d_uv1.F (with compute_horiz_rhs_uv_terms.h and compute_vert_rhs_uv_terms.h), src/visc3d_S.F,
src/step3d_uv2.F and src/diagnostics.F, compiled unchanged with -DDIAGNOSTICS, diag_uv = .true., diag_avg = .false.
through cpp | mpc.py | flang -O2 -ffp-contract=off, the way oracle/ref/build_ref.sh compiles its routines -- on fixed
pseudo-random inputs: an 8 x 6 x 4 grid, closed on every side, MASKING with one land cell, UV_COR UV_ADV UV_VIS2.
tests/test_uvdiag_ref.py requires the numpy restatement (tests/uvdiag_ref.py) to reproduce it bit for bit.

The routines are reached through a small harness library that is not part of this repository.  Beside the five files
above it compiles the reference's param, hidden_mpi_vars, dimensions, scalars, ocean_vars, private_scratch, strings,
mixing, eos_vars, coupling and lenstr unchanged, and declaration-only stand-in modules for what the four routines
do not exercise here (grid, tracers, surf_flux, tides, calc_pflx_mod, river_frc, mpi_exchanges, error_handling_mod,
netcdf, nc_read_write, roms_read_write).  It exports
  uvg_info(int iv[3])                 LLm, MMm, N
  uvg_init()                          one rank that owns the whole grid, no neighbours; allocates the modules' arrays
  uvg_scalars(int iv[4], double dv[3])  nstp, nrhs, nnew, knew; dt, (unused), rho0
  uvg_set(int id, const double*)      copies a flat array into the module array SET[id] below, in its storage order
                                      (GLOBAL_2D_ARRAY = -1:Lm+2, -1:Mm+2; u, v with their three time slots)
  uvg_init_diag(double sentinel, int shape[4])  init_diagnostics, then Udiag = Vdiag = sentinel; shape(Udiag)
  uvg_call(int which)                 1 prsgrd, 2 step3d_uv1(0), 3 visc3d, 4 step3d_uv2(0)
  uvg_get(int id, int n, double*)     1 u, 2 v; 50, 51: the first n elements of private_scratch's A3d(:,1), A3d(:,2),
                                      where prsgrd and step3d_uv1 keep ru and rv (istr-2:iend+2, jstr-2:jend+2, N);
                                      60 Udiag, 61 Vdiag (nx, ny, nz, 7)

usage: python tests/golden/uvdiag_golden.py libuvg.so
"""
import ctypes
import os
import sys

import numpy as np

SEED = 20261021
SENTINEL = -777.0
NSTP, NRHS, NNEW, KNEW = 2, 3, 1, 2
DT = 30.0
RHO0 = 1027.5
LAND = (4, 3)   # (i, j) of the land cell
SET = {1: "u", 2: "v", 3: "Hz", 4: "z_r", 5: "z_w", 6: "FlxU", 7: "FlxV", 8: "We", 9: "Wi", 10: "rho", 11: "Akv", 12: "pm",
       13: "pn", 14: "f", 15: "fomn", 16: "umask", 17: "vmask", 18: "pmask", 19: "rmask", 20: "dm_r", 21: "dn_r",
       22: "dm_u", 23: "dn_u", 24: "dm_v", 25: "dn_v", 26: "dm_p", 27: "dn_p", 28: "visc2_r", 29: "visc2_p", 30: "sustr",
       31: "svstr", 32: "r_D", 33: "DU_avg1", 34: "DV_avg1", 35: "DU_avg2", 36: "DV_avg2", 37: "pn_u", 38: "pm_v"}


def inputs(Lm, Mm, N):
    """Fixed pseudo-random inputs, every ghost point included; Hz, the metrics and the mixing coefficients positive;
    masks of one land cell."""
    r = np.random.default_rng(SEED)
    sh = (Mm + 4, Lm + 4)
    X = lambda a, di=0, dj=0: np.roll(a, (-dj, -di), axis=(-2, -1))
    d = {}
    for c in "uv":
        q = r.normal(0.0, 0.1, (3, N) + sh)
        q[NNEW - 1] = r.normal(0.0, 1.0, (N,) + sh)            # Hz*u of pre_step3d
        d[c] = q
    d["Hz"] = r.uniform(5.0, 20.0, (N,) + sh)
    zw = np.zeros((N + 1,) + sh)
    zw[0] = -d["Hz"].sum(axis=0)
    for k in range(1, N + 1):
        zw[k] = zw[k - 1] + d["Hz"][k - 1]
    d["z_w"], d["z_r"] = zw, 0.5 * (zw[1:] + zw[:-1])
    d.update(FlxU=r.normal(0.0, 50.0, (N,) + sh), FlxV=r.normal(0.0, 50.0, (N,) + sh),
             We=r.normal(0.0, 20.0, (N + 1,) + sh), Wi=r.normal(0.0, 5.0, (N + 1,) + sh),
             rho=r.uniform(20.0, 28.0, (N,) + sh), Akv=r.uniform(1e-4, 1e-2, (N + 1,) + sh),
             pm=r.uniform(0.8e-3, 1.3e-3, sh), pn=r.uniform(0.7e-3, 1.4e-3, sh), f=r.uniform(0.8e-4, 1.2e-4, sh),
             visc2_r=r.uniform(20.0, 60.0, sh), visc2_p=r.uniform(20.0, 60.0, sh), sustr=r.normal(0.0, 1e-4, sh),
             svstr=r.normal(0.0, 1e-4, sh), r_D=r.uniform(1e-4, 1e-3, sh), DU_avg1=r.normal(0.0, 3e3, sh),
             DV_avg1=r.normal(0.0, 3e3, sh), DU_avg2=r.normal(0.0, 3e3, sh), DV_avg2=r.normal(0.0, 3e3, sh))
    pm, pn = d["pm"], d["pn"]
    d["fomn"] = d["f"] / (pm * pn)
    d["dm_r"], d["dn_r"] = 1.0 / pm, 1.0 / pn
    d["dm_u"], d["dn_u"] = 2.0 / (pm + X(pm, -1)), 2.0 / (pn + X(pn, -1))
    d["dm_v"], d["dn_v"] = 2.0 / (pm + X(pm, 0, -1)), 2.0 / (pn + X(pn, 0, -1))
    d["dm_p"] = 4.0 / (pm + X(pm, -1) + X(pm, 0, -1) + X(pm, -1, -1))
    d["dn_p"] = 4.0 / (pn + X(pn, -1) + X(pn, 0, -1) + X(pn, -1, -1))
    d["pn_u"], d["pm_v"] = 0.5 * (pn + X(pn, -1)), 0.5 * (pm + X(pm, 0, -1))
    rmask = np.ones(sh)
    i, j = LAND
    rmask[j + 1, i + 1] = 0.0
    d["rmask"] = rmask
    d["umask"], d["vmask"] = rmask * X(rmask, -1), rmask * X(rmask, 0, -1)
    d["pmask"] = rmask * X(rmask, -1) * X(rmask, 0, -1) * X(rmask, -1, -1)
    return {k: np.ascontiguousarray(a) for k, a in d.items()}


def main(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.uvg_set.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.uvg_get.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.uvg_init_diag.argtypes = [ctypes.c_double, ctypes.c_void_p]
    L.uvg_call.argtypes = [ctypes.c_int]
    iv = (ctypes.c_int * 3)()
    L.uvg_info(iv)
    Lm, Mm, N = list(iv)
    L.uvg_init()
    L.uvg_scalars((ctypes.c_int * 4)(NSTP, NRHS, NNEW, KNEW), (ctypes.c_double * 3)(DT, 0.0, RHO0))
    x = inputs(Lm, Mm, N)
    for i, name in SET.items():
        L.uvg_set(i, x[name].ctypes.data)
    shp = (ctypes.c_int * 4)()
    L.uvg_init_diag(SENTINEL, shp)
    assert list(shp) == [Lm, Mm, N, 7], list(shp)
    n3 = N * (Mm + 4) * (Lm + 4)

    def get(i, shape):
        a = np.zeros(shape)
        L.uvg_get(i, a.size, a.ctypes.data)
        return a

    out = dict(x)
    r3, q4 = (N, Mm + 4, Lm + 4), (3, N, Mm + 4, Lm + 4)
    L.uvg_call(1)
    out["ru_pgr"], out["rv_pgr"] = get(50, r3), get(51, r3)
    L.uvg_call(2)
    out["ru_fin"], out["rv_fin"] = get(50, r3), get(51, r3)
    out["u_uv1"], out["v_uv1"] = get(1, q4), get(2, q4)
    L.uvg_call(3)
    out["u_visc"], out["v_visc"] = get(1, q4), get(2, q4)
    L.uvg_call(4)
    out["u_uv2"], out["v_uv2"] = get(1, q4), get(2, q4)
    out["Udiag"], out["Vdiag"] = get(60, (7, N, Mm, Lm)), get(61, (7, N, Mm, Lm))
    out.update(dims=np.array([Lm, Mm, N, NSTP, NRHS, NNEW, KNEW]), dt=np.array(DT), sentinel=np.array(SENTINEL))
    assert n3 == out["ru_pgr"].size
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "uvdiag_golden.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
