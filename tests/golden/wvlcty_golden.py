"""Records tests/golden/wvlcty_golden.npz: the output of the reference's own
wvlcty (src/wvlcty.F, compiled unchanged through cpp | mpc.py | flang -O2
-ffp-contract=off, the way oracle/ref/build_ref.sh compiles its routines) on
fixed pseudo-random inputs, for two builds on a 9 x 6 x 4 grid: closed, and
EW_PERIODIC + NS_PERIODIC.  tests/test_wvlcty_ref.py requires the numpy
restatement (tests/wvlcty_ref.py) to reproduce it bit for bit.

The routine is reached through a small harness library per build that is not
part of this repository; it exports
  wvl_info(int iv[5])                       LLm, MMm, N, ew_periodic, ns_periodic
  wvl_run(FlxU, FlxV, u, v, z_r, pm, pn, int nstp, Wvlc)
with every array flat in the module's storage order (GLOBAL_2D_ARRAY = -1:Lm+2,
-1:Mm+2; u, v with their three time slots; Wvlc (.., 0:N), in and out): it sets
one rank that owns the whole grid, copies the inputs into the modules ocean_vars
and grid, sets nstp and calls  wvlcty(0, Wvlc).  Wvlc goes in filled with the
sentinel below, so the cells the routine leaves alone show in the recording.

usage: python tests/golden/wvlcty_golden.py libwvl_closed.so libwvl_periodic.so
"""
import ctypes
import os
import sys

import numpy as np

SEED = 20251021
SENTINEL = -777.0
NSTP = 2


def inputs(Lm, Mm, N):
    """Fixed pseudo-random inputs, every ghost cell included; z_r ascending in k, pm and pn positive."""
    r = np.random.default_rng(SEED)
    sh = (Mm + 4, Lm + 4)
    d = dict(FlxU=r.normal(0.0, 50.0, (N,) + sh), FlxV=r.normal(0.0, 50.0, (N,) + sh),
             u=r.normal(0.0, 0.3, (3, N) + sh), v=r.normal(0.0, 0.3, (3, N) + sh),
             z_r=np.sort(r.uniform(-400.0, 1.0, (N,) + sh), axis=0),
             pm=r.uniform(0.8e-3, 1.3e-3, sh), pn=r.uniform(0.7e-3, 1.4e-3, sh))
    return {k: np.ascontiguousarray(a) for k, a in d.items()}


def main(paths):
    out = {}
    for path in paths:
        L = ctypes.CDLL(os.path.abspath(path))
        iv = (ctypes.c_int * 5)()
        L.wvl_info(iv)
        Lm, Mm, N, ewp, nsp = list(iv)
        name = "periodic" if ewp and nsp else "closed"
        assert (ewp, nsp) in ((0, 0), (1, 1))
        x = inputs(Lm, Mm, N)
        w = np.full((N + 1, Mm + 4, Lm + 4), SENTINEL)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        L.wvl_run(P(x["FlxU"]), P(x["FlxV"]), P(x["u"]), P(x["v"]), P(x["z_r"]), P(x["pm"]), P(x["pn"]),
                  ctypes.c_int(NSTP), P(w))
        out["dims_" + name] = np.array([Lm, Mm, N, ewp, nsp, NSTP])
        out["Wvlc_" + name] = w
        for k, a in x.items():   # the inputs themselves: the test does not depend on numpy's generator
            out.setdefault(k, a)
            assert np.array_equal(out[k], a)
    out["sentinel"] = np.array(SENTINEL)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "wvlcty_golden.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1:])
