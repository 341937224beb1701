"""TEST INFRASTRUCTURE ONLY -- the reference's own boundary, sponge and bulk-flux routines.

ctypes binding of oracle/_ref/libref_<name>.so, which build_ref.sh
compiles from the reference tree, unchanged, around stand-in modules and the
C entry points of harness.F90.  Grid size and open sides are compile-time in
the reference, so there is one library per set of open sides (obc1 .. obc15,
every non-empty set of the bits 1 W, 2 E, 4 S, 8 N), one for the bulk fluxes under LMD_KPP (bulk) and five with
ADV_ISONEUTRAL that also hold prsgrd, step3d_uv2 and step3d_t (iso0, iso6, iso9, iso15, isoper; harness_iso.F90,
tests/test_ref_pin_iso.py, tests/test_gpu_iso.py), all at one small non-square grid.  tests/test_ref_pin_obc.py and
tests/test_ref_pin_bulk.py hold the CPU oracle against these libraries on
identical states; tests/test_gpu_bulk.py holds the HIP kernel against them.

The libraries are built where the reference tree is present and travel with
oracle/_ref/; nothing here reads the tree at run time.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_OUT = os.path.join(os.path.dirname(_HERE), "_ref")
REF_TREE = os.environ.get("REF", "/root/reference")
VARIANTS = tuple(range(1, 16))  # open sides of the libraries obc1 .. obc15: every non-empty set (bits 1 W, 2 E, 4 S, 8 N)
BULK = "bulk"                   # the library with LMD_KPP, for set_bulk_frc
# ADV_ISONEUTRAL: prsgrd, step3d_uv2 and step3d_t with the switch.  The basin with the split EOS and both boundary
# layers, closed and with three sets of open sides, and the doubly periodic Filament set (linear EOS, no LMD)
ISO = {"iso0": 0, "iso6": 6, "iso9": 9, "iso15": 15, "isoper": 0}
ISO_VARIANTS = tuple(ISO)
# harness_iso.F90's table: number, levels per plane set (0: N levels, 1: N+1, None: a plane; "akt", "nt": see iso_shape)
ISO_ARRAYS = {"Hz": (1, 0), "z_r": (2, 0), "z_w": (3, 1), "FlxU": (4, 0), "FlxV": (5, 0), "We": (6, 1), "Wi": (7, 1),
              "rho1": (8, 0), "qp1": (9, 0), "rho": (10, 0), "dRdx": (11, 0), "dRde": (12, 0), "idRz": (13, 1),
              "diff3u": (14, 0), "diff3v": (15, 0), "Akz": (16, 1), "Akt": (17, "akt"), "Akv": (18, 1),
              "hbls": (19, None), "hbbl": (20, None), "swr_frac": (21, 1), "DU_avg1": (22, None),
              "DV_avg1": (23, None), "DU_avg2": (24, None), "DV_avg2": (25, None), "f": (26, None),
              "dm_r": (27, None), "dn_r": (28, None), "dm_u": (29, None), "dn_u": (30, None), "dm_v": (31, None),
              "dn_v": (32, None), "stflx": (33, "nt"), "srflx": (34, None), "swflx": (35, None)}
ISO_PRSGRD, ISO_EXCH_SLOPES, ISO_UV2, ISO_T = 1, 2, 3, 4
SIDES = ("west", "east", "south", "north")
_P = ctypes.POINTER(ctypes.c_double)


def lib_path(which):
    return os.path.join(_OUT, "libref_%s.so" % (which if isinstance(which, str) else "obc%d" % which))


def have_tree():
    return os.path.isdir(os.path.join(REF_TREE, "src"))


def build():
    """Run the recipe: a no-op without the reference tree, an error if it fails."""
    subprocess.run(["bash", os.path.join(_HERE, "build_ref.sh")], check=True, env=dict(os.environ, REF=REF_TREE))


def available(which=15):
    """True when the library is there, building it first where the tree allows."""
    if not os.path.exists(lib_path(which)) and have_tree():
        build()
    return os.path.exists(lib_path(which))


def _ptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_P)


_libs = {}


class RefLib:
    """One library: the reference routines at its grid size and open sides."""

    def __init__(self, which):
        obc = 15 if which == BULK else ISO[which] if which in ISO else which
        if which not in _libs:
            L = ctypes.CDLL(lib_path(which))
            if which in ISO:
                L.ref_iso_set.argtypes = L.ref_iso_get.argtypes = [ctypes.c_int, _P]
                L.ref_iso_size.argtypes = L.ref_iso_call.argtypes = [ctypes.c_int]
                L.ref_iso_fill.argtypes = [ctypes.c_double]
            if which != "isoper":     # no SPONGE, no set_nudgcof in the periodic library
                L.ref_set_nudgcof.argtypes = [ctypes.c_double, ctypes.c_double, _P, _P, _P, _P]
            L.ref_set_bry.argtypes = [ctypes.c_int] + [_P] * 6
            L.ref_t3dbc.argtypes = [ctypes.c_int]
            L.ref_init()
            if which in ISO:
                L.ref_iso_init()
            _libs[which] = L
        self.L = _libs[which]
        iv, g = (ctypes.c_int * 5)(), ctypes.c_double()
        self.L.ref_info(iv, ctypes.byref(g))
        self.LLm, self.MMm, self.N, self.NT, self.obc = list(iv)
        self.g = g.value
        assert self.obc == obc
        self.ny2, self.nx2 = self.MMm + 4, self.LLm + 4
        self.iso = which in ISO
        if self.iso:
            iv = (ctypes.c_int * 4)()
            self.L.ref_iso_info(iv)
            self.per, self.split_eos, self.kpp = (bool(iv[0]), bool(iv[1])), bool(iv[2]), bool(iv[3])

    def matches(self, cfg):
        if self.iso and (self.per, self.split_eos, self.kpp) != ((bool(cfg.ew_periodic), bool(cfg.ns_periodic)),
                                                                  bool(cfg.nonlin_eos), bool(cfg.lmd)):
            return False
        return (cfg.LLm, cfg.MMm, cfg.N, cfg.NT, cfg.obc) == (self.LLm, self.MMm, self.N, self.NT, self.obc)

    def matches_size(self, cfg):
        return (cfg.LLm, cfg.MMm, cfg.N, cfg.NT) == (self.LLm, self.MMm, self.N, self.NT)

    # ---- state in ------------------------------------------------------
    def load(self, o, ub=None, any_sides=False):
        """Copy grid, scalars, time indices, prognostic state, boundary data
        and binding coefficients (ub: 4 arrays, or None for ub_tune off) of
        the Oracle o into the reference's module arrays.  any_sides: for the
        routines in which the open sides play no part (set_bulk_frc)."""
        assert self.matches(o.cfg) or (any_sides and self.matches_size(o.cfg))
        f = o.field
        self.L.ref_set_grid(*[_ptr(f(n)) for n in ("h", "pm", "pn", "rmask", "umask", "vmask", "pmask")])
        sc = o.scalars()
        assert sc["g"] == self.g          # a parameter in the reference
        iic, kstp, knew, nstp, nrhs, nnew = o.tindex()
        iv = (ctypes.c_int * 6)(kstp, knew, nstp, nrhs, nnew, int(ub is not None))
        dv = (ctypes.c_double * 5)(sc["dt"], sc["dtfast"], o.cfg.ubind, sc["gamma2"], sc["rho0"])
        self.L.ref_set_scalars(iv, dv)
        self.L.ref_set_ocean(*[_ptr(f(n)) for n in ("zeta", "ubar", "vbar", "u", "v", "t")])
        if self.iso:
            self.iso_put(o, [n for n in self.iso_names() if n != "Akz"])
        for q, side in enumerate(SIDES):
            self.L.ref_set_bry(q, *[_ptr(f("%s_%s" % (n, side))) for n in ("zeta", "ubar", "vbar", "u", "v", "t")])
        if ub is not None:
            keep = [np.ascontiguousarray(a, dtype=np.float64) for a in ub]
            assert [a.size for a in keep] == [self.MMm + 2] * 2 + [self.LLm + 2] * 2
            self.L.ref_set_ub(*[_ptr(a) for a in keep])

    # ---- ADV_ISONEUTRAL ------------------------------------------------------
    def iso_names(self):
        """The arrays of ISO_ARRAYS this library has (the EOS and the boundary layers are compile-time)."""
        no = ("rho",) if self.split_eos else ("rho1", "qp1")
        no += () if self.kpp else ("hbls", "hbbl", "swr_frac")
        return [n for n in ISO_ARRAYS if n not in no]

    def iso_shape(self, name):
        id_, lev = ISO_ARRAYS[name]
        if lev in ("akt", "nt"):
            return (self.L.ref_iso_size(id_) // (self.ny2 * self.nx2), self.ny2, self.nx2)
        return (1 if lev is None else self.N + lev, self.ny2, self.nx2)

    def iso_put(self, o, names):
        """Copy the oracle's arrays `names` into the modules (Akz: into the scratch array step3d_t keeps it in).
        Akt is the one array whose extent may differ: the oracle holds one coefficient set where the reference
        holds one per active tracer, each a copy of the first here."""
        for n in names:
            a = np.ascontiguousarray(o.field(n), dtype=np.float64)
            shape = self.iso_shape(n)
            if n == "Akt" and a.shape != shape:
                assert shape[0] % a.shape[0] == 0, (a.shape, shape)
                a = np.ascontiguousarray(np.concatenate([a] * (shape[0] // a.shape[0])))
            assert a.shape == shape, (n, a.shape, shape)
            self.L.ref_iso_set(ISO_ARRAYS[n][0], _ptr(a))

    def iso_get(self, name):
        a = np.empty(self.iso_shape(name))
        self.L.ref_iso_get(ISO_ARRAYS[name][0], _ptr(a))
        return a

    def iso_fill(self, value):
        """Every private scratch array of the reference holds `value`."""
        self.L.ref_iso_fill(float(value))

    def iso_call(self, which):
        """ISO_PRSGRD, ISO_EXCH_SLOPES (what step3d_uv1 does to the slopes after prsgrd), ISO_UV2, ISO_T."""
        self.L.ref_iso_call(which)

    # ---- routines --------------------------------------------------------
    def zetabc(self, zeta_new):
        """zetabc_tile on zeta_new, a (Mm+4, Lm+4) array, in place."""
        assert zeta_new.shape == (self.ny2, self.nx2)
        self.L.ref_zetabc(_ptr(zeta_new))

    def call(self, routine, *args):
        getattr(self.L, "ref_" + routine)(*args)

    def ocean(self):
        """zeta, ubar, vbar, u, v, t as the reference now holds them, shaped as Oracle.field shapes them."""
        n2, N, NT = self.ny2 * self.nx2, self.N, self.NT
        out = {"zeta": np.empty(4 * n2), "ubar": np.empty(4 * n2), "vbar": np.empty(4 * n2),
               "u": np.empty(3 * N * n2), "v": np.empty(3 * N * n2), "t": np.empty(3 * N * NT * n2)}
        self.L.ref_get_ocean(*[_ptr(out[n]) for n in ("zeta", "ubar", "vbar", "u", "v", "t")])
        return {n: a.reshape(-1, self.ny2, self.nx2) for n, a in out.items()}

    def set_nudgcof(self, v_sponge, visc2, tnu2):
        """init_arrays_mixing then set_nudgcof: visc2_r, visc2_p, diff2."""
        n2 = self.ny2 * self.nx2
        tn = np.ascontiguousarray(tnu2, dtype=np.float64)
        assert tn.size == self.NT
        out = [np.empty(n2), np.empty(n2), np.empty(self.NT * n2)]
        self.L.ref_set_nudgcof(v_sponge, visc2, _ptr(tn), *[_ptr(a) for a in out])
        return {n: a.reshape(-1, self.ny2, self.nx2) for n, a in zip(("visc2_r", "visc2_p", "diff2"), out)}

    def bulk(self, atm, flux):
        """set_bulk_frc.  atm: uwnd vwnd tair qair prate lwrad swrad; flux:
        the arrays sustr svstr sustr_r svstr_r stflx swflx as they stand
        before the call (the routine leaves some of their points alone).
        t, u, v, the masks, nrhs and rho0 come from load().  Returns the six
        and srflx."""
        shp = (self.ny2, self.nx2)
        a = [np.ascontiguousarray(atm[n], dtype=np.float64).reshape(shp)
             for n in ("uwnd", "vwnd", "tair", "qair", "prate", "lwrad", "swrad")]
        names = ("sustr", "svstr", "sustr_r", "svstr_r", "stflx", "swflx")
        out = {n: np.array(flux[n], dtype=np.float64, order="C") for n in names}
        assert out["stflx"].size == self.NT * shp[0] * shp[1] and out["sustr"].size == shp[0] * shp[1]
        out["srflx"] = np.empty(shp)
        self.L.ref_bulk(*[_ptr(x) for x in a], *[_ptr(out[n]) for n in names], _ptr(out["srflx"]))
        return {n: x.reshape(-1, *shp) for n, x in out.items()}
