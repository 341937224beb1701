"""romsgpu -- host-side mirror of the UCLA-ROMS hot-path routines on MI355X.

The reference drives its split-explicit step from Fortran (main.F:333-520)
by calling argument-less / (tile) / (tidx) subroutines that operate on module
arrays.  ``Model`` exposes the same routines with the same names and the same
time-index bookkeeping (scalars.F: iic, kstp, knew, nstp, nrhs, nnew), backed
by ``libromsgpu.so`` (HIP kernels for gfx950 behind the C ABI declared in
include/roms_gpu.h).  There is no CPU fallback: constructing a Model without
the built library or without a GPU raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("ROMS_GPU_LIB") or os.path.join(_PKG, "libromsgpu.so")   # ROMS_GPU_LIB: A/B builds only
MAX_FAST = 288

FIELDS = ["h", "hinv", "f", "fomn", "pm", "pn", "dm_r", "dn_r", "dm_u", "dn_u", "dm_v", "dn_v", "dm_p", "dn_p",
          "pmon_u", "pnom_v", "rmask", "pmask", "umask", "vmask", "Cs_w", "Cs_r",
          "zeta", "ubar", "vbar", "u", "v", "t", "FlxU", "FlxV", "We", "Wi", "Hz", "Hz_u", "Hz_v", "z_r", "z_w",
          "rufrc", "rvfrc", "rhoA", "rhoS", "r_D", "Zt_avg1", "DU_avg1", "DV_avg1", "DU_avg2", "DV_avg2",
          "DU_avg_bak", "DV_avg_bak", "rho", "rho1", "qp1", "bvf", "Akv", "Akt", "visc2_r", "visc2_p", "diff2",
          "hbls", "hbbl", "ghat", "swr_frac", "sustr", "svstr", "stflx", "srflx", "swflx", "ru", "rv"] + \
         ["%s_%s" % (v, e) for v in ("zeta", "ubar", "vbar", "u", "v", "t") for e in ("west", "east", "south", "north")] + \
         ["dndx", "dmde", "ptide", "uwnd", "vwnd", "tair", "qair", "prate", "swrad", "lwrad", "sustr_r", "svstr_r"]
# ADV_ISONEUTRAL's arrays (ROMS_dRdx .. ROMS_Akz), apart from FIELDS: what copies a whole state walks FIELDS, and
# these exist with the switch only (size 0 and every get/put refused without it)
ISO_FIELDS = ["dRdx", "dRde", "idRz", "diff3u", "diff3v", "Akz"]
FIELD_ID = {n: i for i, n in enumerate(FIELDS + ISO_FIELDS)}
CASE_FILAMENT, CASE_BASIN, CASE_PIPES, CASE_RIVERS = 0, 1, 2, 3
# LMD switch bits (ROMS_LMD_* of include/roms_gpu.h)
LMD_MIXING, LMD_KPP, LMD_BKPP, LMD_RIMIX, LMD_CONVEC, LMD_NONLOCAL = 1, 2, 4, 8, 16, 32
LMD_DDMIX = 64    # double diffusion (lmd_vmix.F:279-360), needs salinity
LMD_ALL = 63       # tests/Pipes_ana/cppdefs.opt
LMD_ICELAND = 47   # Examples/Iceland/Iceland_parent/cppdefs.opt: no LMD_CONVEC


def lmd_bits(lmd):
    """True -> every LMD switch (the Pipes_ana set), False -> 0, else the bits."""
    if lmd is True:
        return LMD_ALL
    return int(lmd)


class Dims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in
                ("Lm", "Mm", "N", "NT", "LLm", "MMm", "np_xi", "np_eta", "inode", "jnode", "iSW_corn", "jSW_corn",
                 "ew_periodic", "ns_periodic", "west_exchng", "east_exchng", "south_exchng", "north_exchng")]


class Cfg(ctypes.Structure):
    _fields_ = [("nonlin_eos", ctypes.c_int), ("salinity", ctypes.c_int), ("lmd_mixing", ctypes.c_int),
                ("uv_vis2", ctypes.c_int), ("ts_dif2", ctypes.c_int), ("dt", ctypes.c_double),
                ("ndtfast", ctypes.c_int), ("nfast", ctypes.c_int), ("weight", (ctypes.c_double * MAX_FAST) * 2),
                ("g", ctypes.c_double), ("rho0", ctypes.c_double), ("rdrg", ctypes.c_double),
                ("rdrg2", ctypes.c_double), ("Zob", ctypes.c_double), ("gamma2", ctypes.c_double),
                ("Akv_bak", ctypes.c_double), ("Akt_bak", ctypes.c_double * 2), ("Tcoef", ctypes.c_double),
                ("T0", ctypes.c_double), ("Scoef", ctypes.c_double), ("S0", ctypes.c_double),
                ("theta_s", ctypes.c_double), ("theta_b", ctypes.c_double), ("hc", ctypes.c_double),
                ("obc", ctypes.c_int), ("ubind", ctypes.c_double), ("curvgrid", ctypes.c_int),
                ("uv_adv", ctypes.c_int), ("uv_cor", ctypes.c_int), ("pot_tides", ctypes.c_int),
                ("bulk_frc", ctypes.c_int), ("adv_isoneutral", ctypes.c_int)]


class Tlev(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in
                ("iic", "ntstart", "forw_start", "iif", "nfast", "kstp", "knew", "nstp", "nrhs", "nnew")]

    def as_list(self):
        return [self.iic, self.kstp, self.knew, self.nstp, self.nrhs, self.nnew]


class Case(ctypes.Structure):
    _fields_ = [("case_id", ctypes.c_int), ("LLm", ctypes.c_int), ("MMm", ctypes.c_int), ("N", ctypes.c_int),
                ("NT", ctypes.c_int), ("salinity", ctypes.c_int), ("nonlin_eos", ctypes.c_int),
                ("lmd_mixing", ctypes.c_int), ("dt", ctypes.c_double), ("ndtfast", ctypes.c_int),
                ("sizex", ctypes.c_double), ("sizey", ctypes.c_double), ("surf_flux", ctypes.c_int),
                ("obc", ctypes.c_int), ("v_sponge", ctypes.c_double), ("island", ctypes.c_int),
                ("curvgrid", ctypes.c_int), ("uv_adv", ctypes.c_int), ("uv_cor", ctypes.c_int),
                ("bulk_frc", ctypes.c_int), ("adv_isoneutral", ctypes.c_int)]


ROUTINES_T = ["set_huv", "omega", "prsgrd", "pre_step3d", "set_huv1", "step3d_uv1", "visc3d", "step2d",
              "step3d_uv2", "step3d_t", "t3dmix", "set_depth", "swr_frac", "step", "init_sequence"]

_lib = None


def load_library(path=LIB_PATH):
    """Load libromsgpu.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError("romsgpu: %s not built -- run __graft_entry__.build()" % path)
    L = ctypes.CDLL(path)
    P = ctypes.POINTER
    L.roms_gpu_last_error.restype = ctypes.c_char_p
    L.roms_gpu_init.argtypes = [P(Dims), P(Cfg), ctypes.c_int, ctypes.c_void_p]
    L.roms_gpu_init_case.argtypes = [P(Case), ctypes.c_int, P(Tlev)]
    L.roms_gpu_field_size.argtypes = [ctypes.c_int]
    L.roms_gpu_field_size.restype = ctypes.c_long
    for fn in ("roms_gpu_copy_in", "roms_gpu_copy_out", "roms_gpu_register"):
        getattr(L, fn).argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_upload.argtypes = [ctypes.c_int]
    L.roms_gpu_download.argtypes = [ctypes.c_int]
    for fn in ROUTINES_T:
        getattr(L, "roms_gpu_" + fn).argtypes = [P(Tlev)]
    L.roms_gpu_rho_eos.argtypes = [ctypes.c_int, P(Tlev)]
    L.roms_gpu_lmd_vmix.argtypes = [ctypes.c_int, P(Tlev)]
    L.roms_gpu_set_pipe_frc.argtypes = [ctypes.c_int, P(ctypes.c_int), P(ctypes.c_double), P(ctypes.c_double),
                                        P(ctypes.c_double)]
    L.roms_gpu_set_river_frc.argtypes = [ctypes.c_int, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double),
                                         P(ctypes.c_double)]
    L.roms_gpu_bulk_flux.argtypes = [P(Tlev)]
    L.roms_gpu_set_ub_tune.argtypes = [P(ctypes.c_double)] * 4
    L.roms_gpu_frc_record.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, P(ctypes.c_double)]
    L.roms_gpu_frc_interp.argtypes = [ctypes.c_double, ctypes.c_int]
    L.roms_gpu_frc_clock.argtypes = [ctypes.c_double, ctypes.c_int]
    L.roms_gpu_set_tide_data.argtypes = [ctypes.c_int] + [P(ctypes.c_double)] * 9
    L.roms_gpu_set_tides.argtypes = [ctypes.c_double]
    L.roms_gpu_diag.argtypes = [P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_time_steps.argtypes = [P(Tlev), ctypes.c_int, P(ctypes.c_double)]
    L.roms_gpu_stream.restype = ctypes.c_void_p
    L.roms_gpu_time_routine.argtypes = [ctypes.c_int, ctypes.c_int, P(Tlev), P(ctypes.c_double), P(ctypes.c_long)]
    L.roms_gpu_init_case_comm.argtypes = [P(Case), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, P(Tlev)]
    L.roms_gpu_comm_unique_id.argtypes = [ctypes.c_void_p]
    L.roms_gpu_comm_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       P(ctypes.c_void_p)]
    L.roms_gpu_comm_create_local.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(ctypes.c_void_p)]
    L.roms_gpu_comm_create_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, HOST_ALLGATHER_FN,
                                            ctypes.c_void_p, P(ctypes.c_void_p)]
    L.roms_gpu_comm_destroy.argtypes = [ctypes.c_void_p]
    L.roms_gpu_horizontal_path.argtypes = [P(ctypes.c_int)]
    L.roms_gpu_halo_plan.argtypes = [ctypes.c_int] * 8 + [P(ctypes.c_int), P(ctypes.c_long), P(ctypes.c_int)]
    L.roms_gpu_halo_map.argtypes = [ctypes.c_int] * 10 + [P(ctypes.c_int), P(ctypes.c_int), ctypes.c_long]
    L.roms_gpu_halo_map.restype = ctypes.c_long
    L.roms_gpu_halo_map_wide.argtypes = [ctypes.c_int] * 11 + [P(ctypes.c_int), P(ctypes.c_int), ctypes.c_long]
    L.roms_gpu_halo_map_wide.restype = ctypes.c_long
    L.roms_gpu_wrt_rst.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, P(Tlev)]
    L.roms_gpu_wrt_his.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, P(Tlev), ctypes.c_int]
    L.roms_gpu_get_init.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_io_tracer_name.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    L.roms_gpu_avg_begin.argtypes = [ctypes.c_int]
    L.roms_gpu_calc_avg.argtypes = [P(Tlev), ctypes.c_double]
    L.roms_gpu_wrt_avg.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, P(Tlev)]
    L.roms_gpu_avg_state.argtypes = [P(ctypes.c_int), P(ctypes.c_double), P(ctypes.c_int)]
    L.roms_gpu_avg_copy_out.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_time_calc_avg.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_wvlcty.argtypes = [P(Tlev)]
    L.roms_gpu_wvlcty_copy_out.argtypes = [ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_time_wvlcty.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_part_begin.argtypes = [ctypes.c_long, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    L.roms_gpu_part_add.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.roms_gpu_do_particles.argtypes = [P(Tlev)]
    L.roms_gpu_part_state.argtypes = [P(ctypes.c_long)]
    L.roms_gpu_part_copy_out.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int]
    L.roms_gpu_wrt_part.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    L.roms_gpu_time_do_particles.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_tdiag_begin.argtypes = [ctypes.c_int, P(ctypes.c_int), ctypes.c_int]
    L.roms_gpu_tdiag_sample.argtypes = [ctypes.c_int]
    L.roms_gpu_tdiag_state.argtypes = [P(ctypes.c_int)] * 4
    L.roms_gpu_tdiag_copy_out.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_wrt_tdiag.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                     P(Tlev)]
    L.roms_gpu_time_tdiag.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_uvdiag_begin.argtypes = [ctypes.c_int, ctypes.c_int]
    L.roms_gpu_uvdiag_sample.argtypes = [ctypes.c_int]
    L.roms_gpu_uvdiag_state.argtypes = [P(ctypes.c_int)] * 4
    L.roms_gpu_uvdiag_copy_out.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_wrt_diag.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                    P(Tlev)]
    L.roms_gpu_time_uvdiag.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_pflx_begin.argtypes = [ctypes.c_double, ctypes.c_int]
    L.roms_gpu_pflx_state.argtypes = [P(ctypes.c_int), P(ctypes.c_double), P(ctypes.c_long)]
    L.roms_gpu_pflx_path.argtypes = [P(ctypes.c_long), P(ctypes.c_long)]
    L.roms_gpu_pflx_copy_out.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_pflx_copy_in.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_time_pflx.argtypes = [ctypes.c_int, P(ctypes.c_double)]
    L.roms_gpu_zslice_begin.argtypes = [ctypes.c_int, ctypes.c_int, P(ctypes.c_double), ctypes.c_int, P(ctypes.c_int),
                                        ctypes.c_int]
    L.roms_gpu_calc_zslice.argtypes = [P(Tlev)]
    L.roms_gpu_wrt_zslice.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, P(Tlev)]
    L.roms_gpu_zslice_state.argtypes = [P(ctypes.c_int)] * 4
    L.roms_gpu_zslice_copy_out.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_time_calc_zslice.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_extract_begin.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    L.roms_gpu_extract_angler.argtypes = [ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_extract_add_object.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_long, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p]
    L.roms_gpu_extract_objects_file.argtypes = [ctypes.c_char_p]
    L.roms_gpu_calc_extract.argtypes = [P(Tlev)]
    L.roms_gpu_wrt_extract.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, P(Tlev)]
    L.roms_gpu_extract_state.argtypes = [P(ctypes.c_int)] * 5
    L.roms_gpu_extract_object_info.argtypes = [ctypes.c_int] + [P(ctypes.c_int)] * 5
    L.roms_gpu_extract_object_coef.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.roms_gpu_extract_child_cs.argtypes = [ctypes.c_void_p]
    L.roms_gpu_extract_copy_out.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    L.roms_gpu_time_calc_extract.argtypes = [ctypes.c_int, P(Tlev), P(ctypes.c_double)]
    L.roms_gpu_extract_locate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_int), P(ctypes.c_int)]
    _lib = L
    return L


class RomsGpuError(RuntimeError):
    pass


def _check(L, rc, what):
    if rc != 0:
        raise RomsGpuError("%s failed (%d): %s" % (what, rc, L.roms_gpu_last_error().decode()))


def rank_extent(LL, np_, node):
    """(length, SW-corner offset) of a subdomain along one direction (mpi_setup.F:110-154)."""
    base = (LL + np_ - 1) // np_
    off = np_ * base - LL
    sw = 0 if node == 0 else node * base - off // 2
    n = base
    if node == 0:
        n -= off // 2
    if node == np_ - 1:
        n -= (off + 1) // 2
    return n, sw


def halo_plan(Lm, Mm, np_xi, np_eta, inode, jnode, ew_periodic, ns_periodic):
    """Neighbour ranks, per-level message sizes (W,E,S,N,SW,SE,NW,NE) and strip
    extents (i0,i1,j0,j1) of the library's halo exchange (host-only call)."""
    L = load_library()
    peer = (ctypes.c_int * 8)()
    cnt = (ctypes.c_long * 8)()
    strip = (ctypes.c_int * 4)()
    rc = L.roms_gpu_halo_plan(Lm, Mm, np_xi, np_eta, inode, jnode, int(ew_periodic), int(ns_periodic), peer, cnt, strip)
    if rc != 0:
        raise ValueError("bad halo plan arguments")
    return list(peer), list(cnt), tuple(strip)


def halo_map(Lm, Mm, np_xi, np_eta, inode, jnode, ew_periodic, ns_periodic, direction, unpack, width=2):
    """(i, j) arrays of the cells direction `direction` packs (unpack=False) or
    fills (unpack=True), in message order (host-only call); width > 2: the
    fast loop's width-deep exchange (roms_gpu_halo_map_wide)."""
    L = load_library()
    cap = max(width, 2) * (max(Lm, Mm) + 4)
    iv = (ctypes.c_int * cap)()
    jv = (ctypes.c_int * cap)()
    if width == 2:
        n = L.roms_gpu_halo_map(Lm, Mm, np_xi, np_eta, inode, jnode, int(ew_periodic), int(ns_periodic), direction,
                                int(unpack), iv, jv, cap)
    else:
        n = L.roms_gpu_halo_map_wide(Lm, Mm, np_xi, np_eta, inode, jnode, int(ew_periodic), int(ns_periodic), width,
                                     direction, int(unpack), iv, jv, cap)
    if n < 0:
        raise ValueError("bad halo map arguments")
    return np.array(iv[:n]), np.array(jv[:n])


HALO_DIRS = ("W", "E", "S", "N", "SW", "SE", "NW", "NE")
# ROMS_WRT_* of include/roms_gpu.h (ocean_vars.opt wrt_* switches)
WRT = dict(Z=1, Ub=2, Vb=4, U=8, V=16, T=32, R=64, O=128, Akv=256, Akt=512, Aks=1024, Hbls=2048, Hbbl=4096, W=8192)
WRT_DEFAULT = 63
WRT_ALL = 16383
# Model.avg names -> (ROMS_WRT_* bit, levels: 0 one plane, 1 N, 2 N+1)
AVG_FIELDS = dict(zeta=(1, 0), ubar=(2, 0), vbar=(4, 0), u=(8, 1), v=(16, 1), t=(32, 1), temp=(32, 1), salt=(32, 1),
                  rho=(64, 1), omega=(128, 2), Akv=(256, 2), Akt=(512, 2), Aks=(1024, 2), hbls=(2048, 0),
                  hbbl=(4096, 0), w=(8192, 1))
# Lagrangian particles (particles.F): words of a particle, ROMS_PART_SORT, the tag offset per rank
PART_NPV = 13
PART_WORDS = ("tag", "px", "py", "pz", "pu", "pv", "pw", "prx", "pry", "prz", "prxm", "prym", "przm")
PART_SORT = 1
PART_BIG_NUMBER = 10000000
PART_STATE = ("np", "ntag", "n_sur", "n_bot", "n_lost", "n_moved", "n_range", "n_overflow")
# ROMS_ZSL_* of include/roms_gpu.h (zslice_output.opt wrt_*_zsl switches)
ZSL_T, ZSL_U, ZSL_V = 1, 2, 4
ZSL_MAXDEP = 32
# ROMS_TDIA_* of include/roms_gpu.h (diagnostics.F:83-88; snap: the pre-vertical Hz*t, for budget closure)
TDIA = dict(advx=1, advy=2, advz=3, mixx=4, mixy=5, mixz=6, snap=7)
# ROMS_UVD_* of include/roms_gpu.h (diagnostics.F:56-63; prev: u, v(nnew) as step3d_uv1 got them, for budget closure)
UVD = dict(pgr=1, cor=2, adv=3, dis=4, hmx=5, vmx=6, cpl=7, prev=8)
UVD_COMP = dict(u=0, v=1)
PFLX = dict(up=1, vp=2, u_slow=3, v_slow=4, p_slow=5)   # ROMS_PFLX_*
# ROMS_EXT_* of include/roms_gpu.h (the output_vars of an extraction object); w, bgc are reported, not produced, and so
# are up, vp of an object added while the pressure fluxes are not armed (pflx_begin)
EXT = dict(zeta=1, ubar=2, vbar=4, u=8, v=16, temp=32, salt=64, up=128, vp=256, w=512, bgc=1024)
EXT_3D = ("u", "v", "temp", "salt")


def extract_locate(nx, ny, iSW_corn, jSW_corn, ipos, jpos):
    """find_local_points of extract_data.F (host-only call): (start_idx, np) of the first contiguous run of
    points inside the subdomain, start_idx 1-based; (0, 0) when there is none."""
    L = load_library()
    i = np.ascontiguousarray(ipos, dtype=np.float64).ravel()
    j = np.ascontiguousarray(jpos, dtype=np.float64).ravel()
    if i.size != j.size:
        raise ValueError("extract_locate: ipos and jpos differ in length")
    s, n = ctypes.c_int(), ctypes.c_int()
    if L.roms_gpu_extract_locate(nx, ny, iSW_corn, jSW_corn, i.size, i.ctypes.data, j.ctypes.data, ctypes.byref(s),
                                 ctypes.byref(n)) != 0:
        raise ValueError("bad extract_locate arguments")
    return s.value, n.value
# enum roms_routine of include/roms_gpu.h
ROUTINES = ("rho_eos", "set_HUV", "omega", "prsgrd", "pre_step3d", "set_HUV1", "step3d_uv1", "visc3d", "step2d",
            "step3d_uv2", "step3d_t", "t3dmix", "lmd_vmix",
            "k_s2d_fb",  # kernel level: the fused barotropic kernel alone
            "k_pre_uv_seg", "k_uv1_seg", "k_step3d_t_seg", "k_prsgrd_uv",  # kernel level: the N > 63 column solvers
            "k_halo_pack", "k_halo_wait", "k_halo_unpack")  # halo path: pack / transport / unpack of every exchange
HALO_OPP = (1, 0, 3, 2, 7, 6, 5, 4)


def comm_unique_id():
    """128-byte RCCL id (rank 0); broadcast it with the host's own collective."""
    L = load_library()
    buf = ctypes.create_string_buffer(128)
    _check(L, L.roms_gpu_comm_unique_id(buf), "roms_gpu_comm_unique_id")
    return buf.raw


def comm_create(uid, nranks, rank, device=0):
    """RCCL communicator handle for roms_gpu_init / init_case_comm."""
    L = load_library()
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(bytes(uid), 128)
    _check(L, L.roms_gpu_comm_create(buf, nranks, rank, device, ctypes.byref(h)), "roms_gpu_comm_create")
    return h


def comm_create_local(group, nranks, rank):
    """Handle for subdomains driven by threads of this process (one per thread)."""
    L = load_library()
    h = ctypes.c_void_p()
    _check(L, L.roms_gpu_comm_create_local(group, nranks, rank, ctypes.byref(h)), "roms_gpu_comm_create_local")
    return h


# roms_host_allgather_fn of include/roms_gpu.h
HOST_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p)
_host_channels = {}   # comm handle value -> the ctypes callback (kept alive while the handle is)


def comm_create_host(nranks, rank, allgather, device=0):
    """Host-channel communicator: `allgather(data: bytes) -> list of nranks
    bytes objects` is the host's own collective (the MPI_Allgather a Fortran
    host passes); halos then move by IPC peer writes with RCCL out of the loop."""
    L = load_library()

    def fn(_ctx, send, nbytes, recv):
        try:
            parts = allgather(ctypes.string_at(send, nbytes))
            if len(parts) != nranks or any(len(x) != nbytes for x in parts):
                return -1
            ctypes.memmove(recv, b"".join(parts), nbytes * nranks)
            return 0
        except Exception:   # a failed collective is reported as a status, never raised through C
            return -1

    cb = HOST_ALLGATHER_FN(fn)
    h = ctypes.c_void_p()
    _check(L, L.roms_gpu_comm_create_host(nranks, rank, device, cb, None, ctypes.byref(h)), "roms_gpu_comm_create_host")
    _host_channels[h.value] = cb
    return h


class FileAllgather:
    """A host allgather through files in a shared directory (tests and
    single-node runs without MPI): call k of every rank writes its bytes to
    ag<k>.<rank> and reads everyone's.  A rank's file of call k-2 is removed at
    call k: by then every rank has finished reading it."""

    def __init__(self, path, nranks, rank, timeout=120.0):
        self.path, self.n, self.r, self.timeout, self.k = path, nranks, rank, timeout, 0

    def _f(self, k, r):
        return os.path.join(self.path, "ag%d.%d" % (k, r))

    def __call__(self, data):
        import time
        k = self.k
        self.k += 1
        tmp = self._f(k, self.r) + ".tmp"
        with open(tmp, "wb") as fh:
            fh.write(data)
        os.rename(tmp, self._f(k, self.r))
        if k >= 2:
            try:
                os.remove(self._f(k - 2, self.r))
            except OSError:
                pass
        out, t0 = [], time.time()
        for r in range(self.n):
            f = self._f(k, r)
            while not os.path.exists(f):
                if time.time() - t0 > self.timeout:
                    raise TimeoutError("allgather %d: rank %d missing" % (k, r))
                time.sleep(0.001)
            with open(f, "rb") as fh:
                out.append(fh.read())
        return out


def comm_destroy(h):
    load_library().roms_gpu_comm_destroy(h)
    _host_channels.pop(getattr(h, "value", h), None)


def part_full_seed(model, ppm3, rng):
    """The full_seed branch of init_particles with seed_particles (particles.F:146-163, 358-387) on the host:
    floor(h/(pm*pn)*ppm3) particles in every column of the rank, columns in the order j then i, uniform in the
    cell and uniform in depth between z_w(0) and z_w(N) (depths ascending within a column, as zlev2kidx leaves
    them), drawn from the numpy Generator `rng` and handed to part_add with zmode 1.  Returns their number."""
    nx, ny = model.Lm, model.Mm
    inner = (slice(2, ny + 2), slice(2, nx + 2))
    h, pm, pn = (model.get(k)[0][inner] for k in ("h", "pm", "pn"))
    zw = model.get("z_w")
    lnp = np.floor(h / (pm * pn) * ppm3).astype(np.int64).ravel()
    lnp[lnp < 0] = 0
    col = np.repeat(np.arange(nx * ny), lnp)
    n = col.size
    z0, z1 = zw[0][inner].ravel()[col], zw[-1][inner].ravel()[col]
    z = rng.random(n) * (z1 - z0) + z0
    order = np.lexsort((z, col))
    px = rng.random(n) + (col % nx)
    py = rng.random(n) + (col // nx)
    model.part_add(px, py, z[order], zmode=1)
    return n


class Model:
    """One rank's device-resident model state and the reference's routines."""

    def __init__(self):
        self.L = load_library()
        self.t = Tlev()
        self.shape2 = None

    def _chk(self, rc, what):
        if rc != 0:
            raise RomsGpuError("%s failed (%d): %s" % (what, rc, self.L.roms_gpu_last_error().decode()))

    # ---- construction ----
    @classmethod
    def from_case(cls, case_id, LLm, MMm, N, NT=1, salinity=False, nonlin_eos=False, dt=5.0, ndtfast=60,
                  sizex=12.8e3, sizey=3.2e3, device=0, np_xi=1, np_eta=1, comm=None, rank=0, lmd=False,
                  surf_flux=False, obc=0, v_sponge=0.0, island=False, curvgrid=False, uv_adv=True, uv_cor=True,
                  bulk_frc=False, adv_isoneutral=False):
        """Analytic case on the whole grid, or on subdomain `rank` of an
        np_xi x np_eta processor grid when a communicator is given.
        lmd: False, True (all LMD switches) or ROMS_LMD_* bits."""
        m = cls()
        c = Case(case_id, LLm, MMm, N, NT, int(salinity), int(nonlin_eos), lmd_bits(lmd), dt, ndtfast, sizex, sizey,
                 int(surf_flux), int(obc), float(v_sponge), int(island), int(curvgrid), int(uv_adv), int(uv_cor),
                 int(bulk_frc), int(adv_isoneutral))
        if comm is None and np_xi * np_eta == 1:
            m._chk(m.L.roms_gpu_init_case(ctypes.byref(c), device, ctypes.byref(m.t)), "roms_gpu_init_case")
        else:
            m._chk(m.L.roms_gpu_init_case_comm(ctypes.byref(c), np_xi, np_eta, comm, device, ctypes.byref(m.t)),
                   "roms_gpu_init_case_comm")
        m.LLm, m.MMm, m.N, m.NT = LLm, MMm, N, NT
        m.salinity = bool(salinity)
        m.jnode, m.inode = divmod(rank, np_xi)
        m.Lm, m.iSW = rank_extent(LLm, np_xi, m.inode)
        m.Mm, m.jSW = rank_extent(MMm, np_eta, m.jnode)
        m.shape2 = (m.Mm + 4, m.Lm + 4)
        return m

    @classmethod
    def from_dims(cls, dims, cfg, device=0):
        m = cls()
        m._chk(m.L.roms_gpu_init(ctypes.byref(dims), ctypes.byref(cfg), device, None), "roms_gpu_init")
        m.LLm, m.MMm, m.N, m.NT = dims.Lm, dims.Mm, dims.N, dims.NT
        m.salinity = bool(cfg.salinity)
        m.shape2 = (dims.Mm + 4, dims.Lm + 4)
        return m

    def close(self):
        self.L.roms_gpu_finalize()
        self._host = {}

    # ---- host mirrors (roms_gpu_register / upload / download): the way a
    # Fortran host hands its module arrays to the library ----
    def register(self, name, arr):
        """Borrow the host array `arr` (float64, C-contiguous, the field's
        Fortran layout) as the mirror of field `name` until close()."""
        fid = FIELD_ID[name]
        if arr.dtype != np.float64 or not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("register: %s must be a contiguous float64 array" % name)
        self._chk(self.L.roms_gpu_register(fid, arr.ctypes.data, arr.size), "register " + name)
        if not hasattr(self, "_host"):
            self._host = {}
        self._host[name] = arr   # keep the borrowed buffer alive

    def upload(self, name=None):
        self._chk(self.L.roms_gpu_upload(-1 if name is None else FIELD_ID[name]), "upload")

    def download(self, name=None):
        self._chk(self.L.roms_gpu_download(-1 if name is None else FIELD_ID[name]), "download")

    # ---- state access (Fortran layout, returned as (levels, j, i) C arrays) ----
    def get(self, name):
        fid = FIELD_ID[name]
        n = self.L.roms_gpu_field_size(fid)
        a = np.empty(n, dtype=np.float64)
        self._chk(self.L.roms_gpu_copy_out(fid, a.ctypes.data, n), "copy_out " + name)
        n2 = self.shape2[0] * self.shape2[1]
        return a.reshape((n // n2,) + self.shape2) if n % n2 == 0 else a

    def put(self, name, arr):
        fid = FIELD_ID[name]
        a = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        n = self.L.roms_gpu_field_size(fid)
        if a.size != n:
            raise ValueError("%s: expected %d elements, got %d" % (name, n, a.size))
        self._chk(self.L.roms_gpu_copy_in(fid, a.ctypes.data, n), "copy_in " + name)

    def set_tindex(self, iic, kstp, knew, nstp, nrhs, nnew, iif=1, forw_start=1, ntstart=1, nfast=None):
        self.t.iic, self.t.kstp, self.t.knew, self.t.nstp, self.t.nrhs, self.t.nnew = iic, kstp, knew, nstp, nrhs, nnew
        self.t.iif, self.t.forw_start, self.t.ntstart = iif, forw_start, ntstart
        if nfast is not None:
            self.t.nfast = nfast

    def sync(self):
        self._chk(self.L.roms_gpu_sync(), "sync")

    # ---- reference routines ----
    def rho_eos(self, tidx):
        self._chk(self.L.roms_gpu_rho_eos(tidx, ctypes.byref(self.t)), "rho_eos")

    def lmd_vmix(self, tind):
        self._chk(self.L.roms_gpu_lmd_vmix(tind, ctypes.byref(self.t)), "lmd_vmix")

    def set_pipe_frc(self, pipe_idx, pipe_flx, pipe_prf, pipe_trc):
        """pipe_frc.F:set_pipe_frc: pipe_idx/pipe_flx on the (Mm+4, Lm+4) grid,
        pipe_prf (npip, N) and pipe_trc (npip, NT)."""
        prf = np.asarray(pipe_prf, dtype=np.float64)
        npip = prf.shape[0]
        idx = np.ascontiguousarray(pipe_idx, dtype=np.int32).ravel()
        flx = np.ascontiguousarray(pipe_flx, dtype=np.float64).ravel()
        prf = np.asfortranarray(prf).ravel(order="F")
        trc = np.asarray(pipe_trc, dtype=np.float64).ravel(order="F")
        P = ctypes.POINTER
        self._chk(self.L.roms_gpu_set_pipe_frc(npip, idx.ctypes.data_as(P(ctypes.c_int)), flx.ctypes.data_as(P(ctypes.c_double)),
                                               prf.ctypes.data_as(P(ctypes.c_double)), trc.ctypes.data_as(P(ctypes.c_double))),
                  "set_pipe_frc")

    def set_river_frc(self, riv_vol, riv_trc, riv_uflx=None, riv_vflx=None):
        """river_frc.F:set_river_frc: riv_vol (nriv,), riv_trc (nriv, NT) for the
        current time; riv_uflx/riv_vflx on the (Mm+4, Lm+4) grid as
        calc_river_flux leaves them (None: keep the faces already set).  No
        river (riv_vol empty) switches river_source off."""
        vol = np.ascontiguousarray(riv_vol, dtype=np.float64).ravel()
        nriv = vol.shape[0]
        trc = np.asarray(riv_trc, dtype=np.float64)
        trc = np.asfortranarray(trc.reshape(nriv, -1)).ravel(order="F") if nriv else trc.ravel()
        P = ctypes.POINTER
        D = P(ctypes.c_double)
        uf, vf = (None if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (riv_uflx, riv_vflx))
        self._chk(self.L.roms_gpu_set_river_frc(nriv, uf.ctypes.data_as(D) if uf is not None else None,
                                                vf.ctypes.data_as(D) if vf is not None else None,
                                                vol.ctypes.data_as(D), trc.ctypes.data_as(D)), "set_river_frc")

    def set_ub_tune(self, ub):
        """SPONGE_TUNE: ub_west, ub_east (Mm+2), ub_south, ub_north (Lm+2); None = edge off."""
        D = ctypes.POINTER(ctypes.c_double)
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in ub]
        self._chk(self.L.roms_gpu_set_ub_tune(*[None if a is None else a.ctypes.data_as(D) for a in keep]),
                  "set_ub_tune")

    # ---- forcing / boundary producers on the device (set_frc_data, set_tides) ----
    FRC_SURFACE, FRC_BRY = 1, 2

    def frc_record(self, name, slot, rec_time, arr):
        """One forcing record (time in days) of field `name` into slot 0/1."""
        a = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        if a.size != self.L.roms_gpu_field_size(FIELD_ID[name]):
            raise ValueError("frc_record: %s has %d elements" % (name, a.size))
        self._chk(self.L.roms_gpu_frc_record(FIELD_ID[name], slot, rec_time,
                                             a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "frc_record")

    def frc_interp(self, modtime, kinds=3):
        self._chk(self.L.roms_gpu_frc_interp(modtime, kinds), "frc_interp")

    def frc_clock(self, start_time, on=True):
        """In-step forcing: every step interpolates the recorded fields at
        roms_step's set_forces / set_bry_all points (and runs set_tides)."""
        self._chk(self.L.roms_gpu_frc_clock(start_time, int(on)), "frc_clock")

    def set_tide_data(self, ftide, pot=None, bry=None):
        """ftide (ntides,) [1/s]; pot = (re, im), bry = ((zre, zim), (ure, uim), (vre, vim)),
        each (ntides, Mm+4, Lm+4) or None."""
        D = ctypes.POINTER(ctypes.c_double)
        keep = [np.ascontiguousarray(ftide, dtype=np.float64)]
        def ptr(a):
            if a is None:
                return None
            keep.append(np.ascontiguousarray(a, dtype=np.float64))
            return keep[-1].ctypes.data_as(D)
        pr, pi = pot if pot is not None else (None, None)
        (zr, zi), (ur, ui), (vr, vi) = bry if bry is not None else ((None, None),) * 3
        self._chk(self.L.roms_gpu_set_tide_data(len(keep[0]), keep[0].ctypes.data_as(D), ptr(pr), ptr(pi), ptr(zr),
                                                ptr(zi), ptr(ur), ptr(ui), ptr(vr), ptr(vi)), "set_tide_data")

    def set_tides(self, time):
        self._chk(self.L.roms_gpu_set_tides(time), "set_tides")

    def bulk_flux(self):
        """set_bulk_frc -> calc_all_bulk_forces on the device at the current nrhs."""
        self._chk(self.L.roms_gpu_bulk_flux(ctypes.byref(self.t)), "bulk_flux")

    def _r(self, fn):
        self._chk(getattr(self.L, "roms_gpu_" + fn)(ctypes.byref(self.t)), fn)

    def set_HUV(self): self._r("set_huv")
    def omega(self): self._r("omega")
    def prsgrd(self): self._r("prsgrd")
    def pre_step3d(self): self._r("pre_step3d")
    def set_HUV1(self): self._r("set_huv1")
    def step3d_uv1(self): self._r("step3d_uv1")
    def visc3d(self): self._r("visc3d")
    def step2d(self): self._r("step2d")
    def step3d_uv2(self): self._r("step3d_uv2")
    def step3d_t(self): self._r("step3d_t")
    def t3dmix(self): self._r("t3dmix")
    def set_depth(self): self._r("set_depth")
    def swr_frac(self): self._r("swr_frac")
    def init_sequence(self): self._r("init_sequence")

    def step(self, n=1):
        """roms_step (main.F:333-520) n times; updates the time indices."""
        for _ in range(n):
            self._r("step")

    def time_routine(self, routine, nsteps):
        """Mean duration [ms] of one call of `routine` (name in ROUTINES) and
        the number of calls, from HIP events around its launches over
        `nsteps` eager steps (the model advances by nsteps)."""
        ms = ctypes.c_double()
        n = ctypes.c_long()
        self._chk(self.L.roms_gpu_time_routine(ROUTINES.index(routine), nsteps, ctypes.byref(self.t), ctypes.byref(ms),
                                               ctypes.byref(n)), "time_routine")
        return ms.value, n.value

    def selftest_zero_fill(self, n, chunks=1):
        """roms_gpu_selftest_zero_fill: nonzero elements that fresh zero-filled
        allocations (chunks x n doubles, recycled memory) show to the
        library's stream (0 expected)."""
        nz = ctypes.c_long()
        self._chk(self.L.roms_gpu_selftest_zero_fill(ctypes.c_long(n), ctypes.c_int(chunks), ctypes.byref(nz)),
                  "selftest_zero_fill")
        return nz.value

    def halo_transport(self):
        """'ipc', 'rccl' (or single rank / in-process), or 'ipc-timeout'."""
        r = self.L.roms_gpu_halo_transport()
        return {1: "ipc", 0: "rccl", -1: "ipc-timeout"}.get(r, "error")

    def halo_overlap(self):
        """True when whole steps defer 3-D exchanges onto the halo stream
        (roms_gpu_halo_overlap: the default with > 1 rank, one GPU each)."""
        return bool(self.L.roms_gpu_halo_overlap())

    def s2d_window(self):
        """True when the fused fast step reads its 2-D fields through one
        buffer window (roms_gpu_s2d_window; ROMS_GPU_S2D_WIN=0: pointers)."""
        return bool(self.L.roms_gpu_s2d_window())

    def kpp_lean(self):
        """(mask, keep): the parts of lmd_vmix that leave out work past the
        boundary layers (ROMS_GPU_KPP_LEAN) and the FC levels k_kpp_ext keeps
        in LDS (ROMS_GPU_KPP_FCKEEP), as read at init (roms_gpu_kpp_lean)."""
        r = self.L.roms_gpu_kpp_lean()
        self._chk(min(r, 0), "kpp_lean")
        return r % 256, r // 256

    def kpp_pf(self):
        """Levels of k_kpp_ext's descending sweep whose loads are in flight
        ahead of the level formed (ROMS_GPU_KPP_PF, as read at init; 1: the
        single level ahead; roms_gpu_kpp_pf)."""
        r = self.L.roms_gpu_kpp_pf()
        self._chk(min(r, 0), "kpp_pf")
        return r

    def vgrid(self):
        """(mask, valid): the kernels that form Hz, z_r, z_w themselves
        (ROMS_GPU_VGRID, as read at init) and whether the stored arrays are
        set_depth's own, so that they do (roms_gpu_vgrid)."""
        r = self.L.roms_gpu_vgrid()
        self._chk(min(r, 0), "vgrid")
        return r % 256, bool(r // 256)

    def vgrid2(self):
        """(mask, valid): the same for the column kernels of omega, set_HUV1
        and step3d_uv2 (ROMS_GPU_VGRID2, as read at init; roms_gpu_vgrid2)."""
        r = self.L.roms_gpu_vgrid2()
        self._chk(min(r, 0), "vgrid2")
        return r % 256, bool(r // 256)

    def tracer_pair(self):
        """(mask, same, (pre, cor)): the tracer segment solvers that carry T
        and S in one block (ROMS_GPU_T_PAIR, as read at init: 1 pre_step3d,
        2 step3d_t), whether Akt(isalt) is known to equal Akt(itemp) so that
        they do, and the pair-form launches of the two routines enqueued since
        init (roms_gpu_tracer_pair)."""
        n = (ctypes.c_long * 2)(0, 0)
        r = self.L.roms_gpu_tracer_pair(n)
        self._chk(min(r, 0), "tracer_pair")
        return r % 256, bool(r // 256), (n[0], n[1])

    def lean_stores(self):
        """(mask, (uv, akt)): the stores whole steps leave out
        (ROMS_GPU_LEAN_ST, as read at init: 1 the predictor's u, v(indx),
        2 lmd_vmix's Akt(isalt)) and the pre_step3d and lmd_vmix launches
        enqueued since init that left theirs out (roms_gpu_lean_stores)."""
        n = (ctypes.c_long * 2)(0, 0)
        r = self.L.roms_gpu_lean_stores(n)
        self._chk(min(r, 0), "lean_stores")
        return r, (n[0], n[1])

    def tracer_hstg(self):
        """(mask, valid, (pre, cor, pre_hz)): the horizontal tracer kernels
        that walk the levels over staged windows (ROMS_GPU_T_HSTG, as read at
        init: 1 pre_step3d, 2 step3d_t, 4 Hz formed in pre_step3d), whether
        the grid is valid so that bit 4 is in force, and the launches of
        k_pre_tracer_stg, of k_step3d_t_stg and of the k_pre_tracer_stg that
        formed Hz enqueued since init (roms_gpu_tracer_hstg)."""
        n = (ctypes.c_long * 3)(0, 0, 0)
        r = self.L.roms_gpu_tracer_hstg(n)
        self._chk(min(r, 0), "tracer_hstg")
        return r % 256, bool(r // 256), (n[0], n[1], n[2])

    def vgrid_mismatch(self):
        """(z_w, z_r, Hz): stored values that differ bitwise from the ones
        formed from the kept free surface, h and hinv, over set_depth's range
        and the halos (roms_gpu_vgrid_check)."""
        out = (ctypes.c_long * 3)()
        self._chk(self.L.roms_gpu_vgrid_check(out), "vgrid_check")
        return out[0], out[1], out[2]

    def column_path(self):
        """(segment solvers on, column scratch in global memory) as chosen at
        init from N, ROMS_GPU_COLSEG and ROMS_GPU_COL_GLOBAL (roms_gpu_column_path)."""
        r = self.L.roms_gpu_column_path()
        self._chk(min(r, 0), "column_path")
        return bool(r & 1), bool(r & 2)

    def horizontal_path(self):
        """The horizontal paths of this rank (roms_gpu_horizontal_path), from
        the host functions the launchers call: {"edges": the fast step's
        closed-edge mode, 0 none / 1 separate edge launches / 2 folded into
        k_s2d_fb; "strips": (strips per row, jA, jB) of whole-step prsgrd or
        None when tiles run everywhere; "omega_seg": omega takes k_omega_seg}."""
        out = (ctypes.c_int * 8)()
        self._chk(self.L.roms_gpu_horizontal_path(out), "horizontal_path")
        return {"edges": out[0], "strips": (out[2], out[3], out[4]) if out[1] else None, "omega_seg": bool(out[5])}

    def fast_step_edge_modes(self):
        """The set of closed-edge modes (0 / 1 / 2 as "edges" of
        horizontal_path()) the fast steps of the last enqueued whole step
        took (roms_gpu_horizontal_path out[6]); empty before the first step.
        A multi-rank fast step decides the fold on the bounds it widens, so
        the set can hold 1 and 2 where "edges" names one of them."""
        out = (ctypes.c_int * 8)()
        self._chk(self.L.roms_gpu_horizontal_path(out), "horizontal_path")
        return {m for m in range(3) if out[6] >> m & 1}

    def halo_exchanges(self):
        """(exchanges in the last enqueued step, fast-loop exchange interval)
        -- roms_gpu_halo_exchanges."""
        n, k = ctypes.c_long(), ctypes.c_int()
        self._chk(self.L.roms_gpu_halo_exchanges(ctypes.byref(n), ctypes.byref(k)), "halo_exchanges")
        return n.value, k.value

    def diag(self):
        out = (ctypes.c_double * 4)()
        self._chk(self.L.roms_gpu_diag(ctypes.byref(self.t), out), "diag")
        return list(out)

    # ---- on-disk formats (basic_output.F, get_init.F) ----
    def time(self, dt):
        """Model time at the end of the last step (main.F:487, start_time 0)."""
        return dt * (self.t.iic - self.t.ntstart + 1) + getattr(self, "start_time", 0.0)

    def wrt_rst(self, path, rec, total_rec, time):
        """wrt_restart_file: record rec (1-based) of this rank's restart file."""
        self._chk(self.L.roms_gpu_wrt_rst(path.encode(), rec, total_rec, time, ctypes.byref(self.t)), "wrt_rst")

    def wrt_his(self, path, rec, total_rec, time, mask=WRT_DEFAULT):
        """wrt_his_ocean_vars: record rec of this rank's history file."""
        self._chk(self.L.roms_gpu_wrt_his(path.encode(), rec, total_rec, time, ctypes.byref(self.t), mask), "wrt_his")

    def io_wait(self):
        self._chk(self.L.roms_gpu_io_wait(), "io_wait")

    # ---- time-averaged output (calc_avg_ocean_vars / wrt_avg_ocean_vars, basic_output.F) ----
    def avg_begin(self, mask=WRT_DEFAULT):
        """Arm averaging of the WRT bits in `mask` (0: disarm and free)."""
        self._chk(self.L.roms_gpu_avg_begin(mask), "avg_begin")

    def calc_avg(self, time):
        """One sample after a step (main.F:486): zeta/ubar/vbar(knew), u/v/t(nstp), `time` at n+1."""
        self._chk(self.L.roms_gpu_calc_avg(ctypes.byref(self.t), time), "calc_avg")

    def wrt_avg(self, path, rec, total_rec, period):
        """wrt_avg_ocean_vars: record rec of this rank's averages file; starts a fresh window."""
        self._chk(self.L.roms_gpu_wrt_avg(path.encode(), rec, total_rec, period, ctypes.byref(self.t)), "wrt_avg")

    def avg_state(self):
        """(navg, t_avg, mask) of the open window."""
        n, m, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        self._chk(self.L.roms_gpu_avg_state(ctypes.byref(n), ctypes.byref(t), ctypes.byref(m)), "avg_state")
        return n.value, t.value, m.value

    def avg(self, name, itrc=0):
        """The running mean of `name` (AVG_FIELDS; "t" with itrc 0.., or "temp" /
        "salt") as a (levels, j, i) array like get(); only the reference's
        write ranges (dimensions.F:40-45) are specified."""
        if name not in AVG_FIELDS:
            raise ValueError("avg: unknown field %s" % name)
        bit, lev = AVG_FIELDS[name]
        if name == "salt":
            itrc = 1
            if self.NT < 2 or not self.salinity:
                raise RomsGpuError("avg: this run has no salinity")
        levels = (1, self.N, self.N + 1)[lev]
        a = np.empty(levels * self.shape2[0] * self.shape2[1], dtype=np.float64)
        self._chk(self.L.roms_gpu_avg_copy_out(bit, itrc + 1, a.ctypes.data, a.size), "avg_copy_out " + name)
        return a.reshape((levels,) + self.shape2)

    def step_avg(self, n, dt):
        """n times: one step, then one sample at self.time(dt)."""
        for _ in range(n):
            self._r("step")
            self.calc_avg(self.time(dt))

    # ---- true vertical velocity (wvlcty.F) ----
    def wvlcty(self):
        """w at rho points [m/s] of the current state (FlxU, FlxV, u, v(nstp), z_r) as an (N, Mm+4, Lm+4)
        array like get(); cells outside wvlcty_tile's range and its edge copies hold 0."""
        self._chk(self.L.roms_gpu_wvlcty(ctypes.byref(self.t)), "wvlcty")
        a = np.empty(self.N * self.shape2[0] * self.shape2[1], dtype=np.float64)
        self._chk(self.L.roms_gpu_wvlcty_copy_out(a.ctypes.data, a.size), "wvlcty_copy_out")
        return a.reshape((self.N,) + self.shape2)

    def time_wvlcty(self, n):
        """(ms of n store launches, ms of n running-mean launches; the latter 0 unless W is armed)."""
        ms = (ctypes.c_double * 2)()
        self._chk(self.L.roms_gpu_time_wvlcty(n, ctypes.byref(self.t), ms), "time_wvlcty")
        return ms[0], ms[1]

    # ---- Lagrangian particles (do_particles, particles.F) ----
    def part_begin(self, npmx, fac_x=0.0, fac_y=0.0, fac_c=0.0, sort=False):
        """Arm an empty list of at most npmx particles; the factors size the messages to the N/S, E/W and corner
        neighbours as fractions of npmx (0: the reference's 0.1, 0.1, 0.01).  sort: every do_particles ends with
        sort_particles' cell ordering (off by default: profiles/part_cost.txt)."""
        self._chk(self.L.roms_gpu_part_begin(npmx, fac_x, fac_y, fac_c, PART_SORT if sort else 0), "part_begin")

    def part_add(self, px, py, pz, zmode=0):
        """Append particles at index-space positions (px, py) and pz: an index-space level (zmode 0) or a depth in
        metres, negative down (zmode 1)."""
        a = [np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (px, py, pz)]
        if not a[0].size == a[1].size == a[2].size:
            raise ValueError("part_add: px, py and pz differ in length")
        self._chk(self.L.roms_gpu_part_add(a[0].size, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, zmode),
                  "part_add")

    def do_particles(self):
        """One call of do_particles after a step (main.F:501): rhs, advance, exchange, removal of the dead."""
        self._chk(self.L.roms_gpu_do_particles(ctypes.byref(self.t)), "do_particles")

    def part_state(self):
        """dict of np, ntag, n_sur, n_bot, n_lost, n_moved, n_range, n_overflow."""
        out = (ctypes.c_long * 8)()
        self._chk(self.L.roms_gpu_part_state(out), "part_state")
        return dict(zip(PART_STATE, out))

    def particles(self, global_=False):
        """The live list as an (np, 13) array (PART_WORDS); global_: px, py as the file holds them."""
        n = self.part_state()["np"]
        a = np.empty((PART_NPV, n), dtype=np.float64)
        self._chk(self.L.roms_gpu_part_copy_out(a.ctypes.data, a.size, int(global_)), "part_copy_out")
        return np.ascontiguousarray(a.T)

    def wrt_part(self, path, rec, total_rec, time):
        """wrt_particles: record rec of this rank's particles file."""
        self._chk(self.L.roms_gpu_wrt_part(path.encode(), rec, total_rec, time), "wrt_part")

    def time_do_particles(self, n):
        """(ms of n whole calls, ms of n launches of the rhs and advance kernel), on a copy of the list."""
        ms = (ctypes.c_double * 2)()
        self._chk(self.L.roms_gpu_time_do_particles(n, ctypes.byref(self.t), ms), "time_do_particles")
        return ms[0], ms[1]

    # ---- tracer budget terms (DIAGNOSTICS with diag_trc, diagnostics.F) ----
    def tdiag_begin(self, tracers, avg=False):
        """Arm the six budget terms of the corrector for the 1-based tracer indices `tracers` (empty: disarm and
        free); avg: running means, one sample per corrector.  Sampling is on afterwards."""
        tr = np.ascontiguousarray(tracers, dtype=np.int32).ravel()
        self._chk(self.L.roms_gpu_tdiag_begin(tr.size, tr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(avg)),
                  "tdiag_begin")

    def tdiag_sample(self, on=True):
        """The reference's calc_diag: whether the next correctors form (and average) the terms."""
        self._chk(self.L.roms_gpu_tdiag_sample(int(on)), "tdiag_sample")

    def tdiag_state(self):
        """(ntd, avg, navg, sampling)."""
        v = [ctypes.c_int() for _ in range(4)]
        self._chk(self.L.roms_gpu_tdiag_state(*[ctypes.byref(x) for x in v]), "tdiag_state")
        return v[0].value, bool(v[1].value), v[2].value, bool(v[3].value)

    def tdiag(self, itrc, term):
        """Term `term` (TDIA: "advx" .. "mixz", "snap") of armed tracer itrc (1-based) as an (N, Mm+4, Lm+4) array
        like get(): the mean with avg, else the last sample; 0 outside the term's range."""
        if term not in TDIA:
            raise ValueError("tdiag: unknown term %s" % term)
        a = np.empty(self.N * self.shape2[0] * self.shape2[1], dtype=np.float64)
        self._chk(self.L.roms_gpu_tdiag_copy_out(itrc, TDIA[term], a.ctypes.data, a.size), "tdiag_copy_out " + term)
        return a.reshape((self.N,) + self.shape2)

    def wrt_tdiag(self, path, rec, total_rec, time, period=0.0):
        """wrt_diag_trc: record rec of this rank's diagnostics file; with avg it starts a fresh window."""
        self._chk(self.L.roms_gpu_wrt_tdiag(path.encode(), rec, total_rec, time, period, ctypes.byref(self.t)),
                  "wrt_tdiag")

    def time_tdiag(self, n):
        """(ms of n snapshot launches, of n horizontal-term launches, of n vertical-term launches)."""
        ms = (ctypes.c_double * 3)()
        self._chk(self.L.roms_gpu_time_tdiag(n, ctypes.byref(self.t), ms), "time_tdiag")
        return ms[0], ms[1], ms[2]

    # ---- momentum budget terms (DIAGNOSTICS with diag_uv, diagnostics.F) ----
    def uvdiag_begin(self, avg=False, on=True):
        """Arm the seven budget terms of u and of v (on=False: disarm and free); avg: running means, one sample per
        corrector.  Sampling is on afterwards."""
        self._chk(self.L.roms_gpu_uvdiag_begin(int(on), int(avg)), "uvdiag_begin")

    def uvdiag_sample(self, on=True):
        """The reference's calc_diag: whether the next correctors form (and average) the terms."""
        self._chk(self.L.roms_gpu_uvdiag_sample(int(on)), "uvdiag_sample")

    def uvdiag_state(self):
        """(armed, avg, navg, sampling)."""
        v = [ctypes.c_int() for _ in range(4)]
        self._chk(self.L.roms_gpu_uvdiag_state(*[ctypes.byref(x) for x in v]), "uvdiag_state")
        return bool(v[0].value), bool(v[1].value), v[2].value, bool(v[3].value)

    def uvdiag(self, comp, term):
        """Term `term` (UVD: "pgr" .. "cpl", "prev") of component "u" or "v" as an (N, Mm+4, Lm+4) array like get():
        the mean with avg, else the last sample; 0 outside the component's range."""
        if term not in UVD or comp not in UVD_COMP:
            raise ValueError("uvdiag: unknown component or term %s %s" % (comp, term))
        a = np.empty(self.N * self.shape2[0] * self.shape2[1], dtype=np.float64)
        self._chk(self.L.roms_gpu_uvdiag_copy_out(UVD_COMP[comp], UVD[term], a.ctypes.data, a.size),
                  "uvdiag_copy_out " + term)
        return a.reshape((self.N,) + self.shape2)

    def wrt_diag(self, path, rec, total_rec, time, period=0.0):
        """do_diagnostics' record of this rank's diagnostics file: the momentum terms and, if tracers are armed too,
        theirs; with avg it starts fresh windows."""
        self._chk(self.L.roms_gpu_wrt_diag(path.encode(), rec, total_rec, time, period, ctypes.byref(self.t)),
                  "wrt_diag")

    def time_uvdiag(self, n):
        """(ms of n launches of the snapshots, of k_uvdiag_rhs, of k_uvdiag_hmx, of k_uvdiag_cpl)."""
        ms = (ctypes.c_double * 4)()
        self._chk(self.L.roms_gpu_time_uvdiag(n, ctypes.byref(self.t), ms), "time_uvdiag")
        return tuple(ms)

    # ---- baroclinic pressure fluxes (calc_pflx_mod.F) ----
    def pflx_begin(self, timescale=0.0, on=True):
        """Arm calc_pressure_flux after every corrector prsgrd with alpha = dt/timescale (timescale <= 0: the
        reference's 86400 s), the filter states zero; on=False: disarm and free."""
        self._chk(self.L.roms_gpu_pflx_begin(float(timescale), int(on)), "pflx_begin")

    def pflx_state(self):
        """(armed, alpha, nsamples): nsamples counts the correctors filtered since arming."""
        a, al, n = ctypes.c_int(), ctypes.c_double(), ctypes.c_long()
        self._chk(self.L.roms_gpu_pflx_state(ctypes.byref(a), ctypes.byref(al), ctypes.byref(n)), "pflx_state")
        return bool(a.value), al.value, n.value

    def pflx_path(self):
        """(formed, streamed): k_pflx_p launches since arming that formed the vertical grid from the free surface, and
        that streamed z_r, z_w."""
        a, b = ctypes.c_long(), ctypes.c_long()
        self._chk(self.L.roms_gpu_pflx_path(ctypes.byref(a), ctypes.byref(b)), "pflx_path")
        return a.value, b.value

    def pflx(self, name):
        """PFLX array `name`: "up", "vp" as (Mm+4, Lm+4), "u_slow", "v_slow", "p_slow" as (N, Mm+4, Lm+4), like get();
        0 outside the array's range."""
        if name not in PFLX:
            raise ValueError("pflx: unknown array %s" % name)
        shape = self.shape2 if name in ("up", "vp") else (self.N,) + self.shape2
        a = np.empty(int(np.prod(shape)), dtype=np.float64)
        self._chk(self.L.roms_gpu_pflx_copy_out(PFLX[name], a.ctypes.data, a.size), "pflx_copy_out " + name)
        return a.reshape(shape)

    def pflx_set(self, name, a):
        """Set a filter state ("u_slow", "v_slow", "p_slow") from an (N, Mm+4, Lm+4) array."""
        if name not in PFLX:
            raise ValueError("pflx_set: unknown array %s" % name)
        a = np.ascontiguousarray(a, dtype=np.float64)
        self._chk(self.L.roms_gpu_pflx_copy_in(PFLX[name], a.ctypes.data, a.size), "pflx_copy_in " + name)

    def time_pflx(self, n):
        """(ms of n launches of k_pflx_p, of k_pflx_uv)."""
        ms = (ctypes.c_double * 2)()
        self._chk(self.L.roms_gpu_time_pflx(n, ms), "time_pflx")
        return tuple(ms)

    # ---- z-level slices (calc_zslice / wrt_zslice, zslice_output.F) ----
    def zslice_begin(self, depths, what=ZSL_U | ZSL_V, tracers=(1, 2), avg=False):
        """Arm slicing of the ZSL bits in `what` at `depths` (relative to the free surface, negative below it);
        `tracers`: 1-based indices sliced with ZSL_T; avg: running means sampled by every calc_zslice.
        what=0 disarms and frees."""
        d = np.ascontiguousarray(depths, dtype=np.float64).ravel()
        tr = np.ascontiguousarray(tracers if what & ZSL_T else (), dtype=np.int32).ravel()
        self._chk(self.L.roms_gpu_zslice_begin(what, d.size, d.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tr.size,
                                               tr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(avg)), "zslice_begin")
        self._zsl_tracers = [int(x) for x in tr] if what else []

    def calc_zslice(self):
        """One sample of u, v, t(nnew) after a step; with avg it also advances the means."""
        self._chk(self.L.roms_gpu_calc_zslice(ctypes.byref(self.t)), "calc_zslice")

    def wrt_zslice(self, path, rec, total_rec, time):
        """wrt_zslice: record rec of this rank's slices file (samples first without avg); starts a fresh window."""
        self._chk(self.L.roms_gpu_wrt_zslice(path.encode(), rec, total_rec, time, ctypes.byref(self.t)), "wrt_zslice")

    def zslice_state(self):
        """(navg, what, ndep, avg) of the armed slicing."""
        v = [ctypes.c_int() for _ in range(4)]
        self._chk(self.L.roms_gpu_zslice_state(*[ctypes.byref(x) for x in v]), "zslice_state")
        return v[0].value, v[1].value, v[2].value, bool(v[3].value)

    def zslice(self, name, q=None):
        """The current slices (the means with avg) of "u", "v", "t" (q = 1..nt_z in the order of `tracers`) or of
        "temp" / "salt" when they are among the sliced tracers, as (ndep, j, i) like get(); cells outside
        1..Lm x 1..Mm hold 0."""
        if name in ("temp", "salt"):
            it = 1 if name == "temp" else 2
            if it not in getattr(self, "_zsl_tracers", []) or (it == 2 and not self.salinity):
                raise RomsGpuError("zslice: %s is not being sliced" % name)
            name, q = "t", self._zsl_tracers.index(it) + 1
        if name not in ("t", "u", "v"):
            raise ValueError("zslice: unknown field %s" % name)
        bit = dict(t=ZSL_T, u=ZSL_U, v=ZSL_V)[name]
        ndep = self.zslice_state()[2]
        a = np.empty(max(ndep, 1) * self.shape2[0] * self.shape2[1], dtype=np.float64)
        self._chk(self.L.roms_gpu_zslice_copy_out(bit, 1 if q is None else q, a.ctypes.data, a.size),
                  "zslice_copy_out " + name)
        return a.reshape((ndep,) + self.shape2)

    # ---- child-boundary extraction (do_extract_data, extract_data.F) ----
    def extract_begin(self, N_chd, theta_s_chd, theta_b_chd, hc_chd, angler=None):
        """Clear every extraction object and set the child's vertical grid (the remap is used unless all four
        equal the parent's); angler: the grid angle as (Mm+4, Lm+4), default 0."""
        self._chk(self.L.roms_gpu_extract_begin(N_chd, theta_s_chd, theta_b_chd, hc_chd), "extract_begin")
        if angler is not None:
            a = np.ascontiguousarray(angler, dtype=np.float64).ravel()
            self._chk(self.L.roms_gpu_extract_angler(a.ctypes.data, a.size), "extract_angler")

    def extract_add(self, name, ipos, jpos, output_vars, ang=None, dname=None):
        """Add one object: fractional positions in absolute index space, `ang` per point for a vector object.
        Returns its 1-based index; names of requested but unsupported variables are in extract_info()."""
        i = np.ascontiguousarray(ipos, dtype=np.float64).ravel()
        j = np.ascontiguousarray(jpos, dtype=np.float64).ravel()
        a = None if ang is None else np.ascontiguousarray(ang, dtype=np.float64).ravel()
        if i.size != j.size or (a is not None and a.size != i.size):
            raise ValueError("extract_add: ipos, jpos and ang differ in length")
        self._chk(self.L.roms_gpu_extract_add_object(name.encode(), (dname or "n_" + name).encode(), i.size, i.ctypes.data,
                                                     j.ctypes.data, None if a is None else a.ctypes.data,
                                                     output_vars.encode()), "extract_add " + name)
        return self.extract_state()[0]

    def extract_objects_file(self, path):
        """Add every object of the reference's objects netCDF file; returns their number so far."""
        self._chk(self.L.roms_gpu_extract_objects_file(path.encode()), "extract_objects_file")
        return self.extract_state()[0]

    def calc_extract(self):
        """One sample: zeta, ubar, vbar(knew), u, v, temp, salt(nstp) at every object's points."""
        self._chk(self.L.roms_gpu_calc_extract(ctypes.byref(self.t)), "calc_extract")

    def wrt_extract(self, path, rec, total_rec, time):
        """Sample, then write record rec of this rank's extraction file."""
        self._chk(self.L.roms_gpu_wrt_extract(path.encode(), rec, total_rec, time, ctypes.byref(self.t)), "wrt_extract")

    def extract_state(self):
        """(nobj, mismatch, N_chd, np_total, need_huv)."""
        v = [ctypes.c_int() for _ in range(5)]
        self._chk(self.L.roms_gpu_extract_state(*[ctypes.byref(x) for x in v]), "extract_state")
        return v[0].value, bool(v[1].value), v[2].value, v[3].value, bool(v[4].value)

    def extract_info(self, iobj):
        """dict(np, start_idx, vars, unsupported, scalar) of object iobj; vars/unsupported as name tuples."""
        v = [ctypes.c_int() for _ in range(5)]
        self._chk(self.L.roms_gpu_extract_object_info(iobj, *[ctypes.byref(x) for x in v]), "extract_object_info")
        names = lambda m: tuple(k for k, b in EXT.items() if m & b)
        return dict(np=v[0].value, start_idx=v[1].value, vars=names(v[2].value), unsupported=names(v[3].value),
                    scalar=bool(v[4].value))

    def extract_coef(self, iobj, grid):
        """(ip, jp, coef(4, np), cosa, sina) of object iobj on grid "r", "u" or "v"."""
        n = self.extract_info(iobj)["np"]
        ip, jp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        cf, ca, sa = np.zeros((4, n)), np.zeros(n), np.zeros(n)
        self._chk(self.L.roms_gpu_extract_object_coef(iobj, "ruv".index(grid), ip.ctypes.data, jp.ctypes.data,
                                                      cf.ctypes.data, ca.ctypes.data, sa.ctypes.data), "extract_object_coef")
        return ip, jp, cf, ca, sa

    def extract_child_cs(self):
        """Cs_w_chd(0:N_chd) of set_chd_scoord."""
        a = np.zeros(self.extract_state()[2] + 1)
        self._chk(self.L.roms_gpu_extract_child_cs(a.ctypes.data), "extract_child_cs")
        return a

    def extract(self, iobj, name):
        """Variable `name` of object iobj from the last sample: (levels, np) for u, v, temp, salt (levels = N_chd
        with the remap, else N), (np,) for zeta, ubar, vbar."""
        if name not in EXT:
            raise ValueError("extract: unknown variable %s" % name)
        _, mismatch, nchd, _, _ = self.extract_state()
        n = self.extract_info(iobj)["np"]
        rows = (nchd if mismatch else self.N) if name in EXT_3D else 1
        a = np.empty(rows * n, dtype=np.float64)
        self._chk(self.L.roms_gpu_extract_copy_out(iobj, EXT[name], a.ctypes.data, a.size), "extract_copy_out " + name)
        return a.reshape(rows, n) if name in EXT_3D else a

    def time_calc_extract(self, n):
        """(ms of n interpolation launches, ms of n remap launches)."""
        ms = (ctypes.c_double * 2)()
        self._chk(self.L.roms_gpu_time_calc_extract(n, ctypes.byref(self.t), ms), "time_calc_extract")
        return ms[0], ms[1]

    def get_init(self, path, req_rec, tindx):
        """get_init(req_rec, tindx); returns 0 (read) or 1 (exact restart not possible)."""
        st = ctypes.c_double()
        rc = self.L.roms_gpu_get_init(path.encode(), req_rec, tindx, ctypes.byref(self.t), ctypes.byref(st))
        if rc < 0:
            self._chk(rc, "get_init")
        if tindx == 1:
            self.start_time = st.value
        return rc

    def restart(self, path, rec=0, exact=True):
        """main.F:244-288: get_init(rec-1, 2) [EXACT_RESTART], get_init(rec, 1),
        then set_depth, set_HUV, omega, rho_eos(nrhs) (roms_gpu_init_sequence).
        rec 0 = the last record."""
        self.t.forw_start = 0
        if exact:
            nrec = rec if rec > 0 else self._nrecs(path)
            if nrec >= 2:
                self.get_init(path, nrec - 1, 2)
            rec = nrec
        self.get_init(path, rec, 1)
        self.init_sequence()

    @staticmethod
    def _nrecs(path):
        with open(path, "rb") as f:
            h = f.read(8)
        return int.from_bytes(h[4:8], "big")

    def time_steps(self, n):
        ms = ctypes.c_double()
        self._chk(self.L.roms_gpu_time_steps(ctypes.byref(self.t), n, ctypes.byref(ms)), "time_steps")
        return ms.value
