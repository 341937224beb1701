"""The oracle's open-boundary and sponge code against the reference's own routines.

oracle/ref/build_ref.sh compiles zetabc_tile, u2dbc_tile, v2dbc_tile,
u3dbc_tile, v3dbc_tile, t3dbc_tile and set_nudgcof from the reference tree,
unchanged, for the Iceland boundary switch set (OBC_M2FLATHER, OBC_M3ORLANSKI,
OBC_TORLANSKI, *_FRC_BRY, SPONGE, SPONGE_TUNE, MASKING) at 24 x 20 x 6 with
open sides 15, 5 and 10.  Each test hands one state to the reference routine
and to its restatement in oracle/oracle_obc.c (or_set_nudgcof in
oracle_main.c) and compares every element of every array the routine can
write, ghost rows and corners included.

Agreement is bitwise: the routines use + - * / sqrt min max in IEEE double,
both sides are built without contraction, so any difference is a difference
in the order of evaluation or in the arm taken.  No tolerance.

The state is a perturbed twin of a mid-run state (branch_states.flather_state
at the library's size): seeded noise of the fields' own size on every time
level, a sign-changing wave on the boundary velocities, land on one cell of
every edge, binding coefficients below 0, inside (0, 1) and above 1.  From the
arrays handed to the reference each test restates the data-dependent branch
conditions of its routine and asserts that every arm is taken on every open
side: inflow and outflow, both choices of the tangential gradient, the cy
clamp at both ends and inside, boundary data against ubind, the three ranges
of ub, Flather's cx on both sides of 1 - 1/sqrt(2), wet and dry edge points.

Not marked gpu.  Skips only where neither the libraries nor the reference
tree exist.
"""
import ctypes
import functools

import numpy as np
import pytest

import branch_states as bs
import oracle
import oracle.ref as ref

SIZE = dict(LLm=24, MMm=20, N=6)
EPS = 1.0e-33
OPEN = {"west": 1, "east": 2, "south": 4, "north": 8}
STATE = ("zeta", "ubar", "vbar", "u", "v", "t")
MASKS = ("rmask", "umask", "vmask", "pmask")
BRY = ["%s_%s" % (v, e) for v in STATE for e in ref.SIDES]
# one land cell on every edge, with its ghost neighbour: (i, j) in Fortran indices
LAND = {"west": [(0, 7), (1, 7)], "east": [(24, 11), (25, 11)], "south": [(9, 0), (9, 1)], "north": [(15, 20), (15, 21)]}

pytestmark = pytest.mark.skipif(not (ref.have_tree() or all(ref.available(v) for v in ref.VARIANTS)),
                                reason="neither oracle/_ref libraries nor a reference tree")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ub_arrays(cfg):
    """Binding coefficients below 0, inside (0, 1) and above 1 on every edge, on the points 0:Mm+1 / 0:Lm+1."""
    x = lambda n, ph: 0.5 + 1.5 * np.sin(np.arange(n) * 0.37 + ph)
    return [x(cfg.MMm + 2, 0.0), x(cfg.MMm + 2, 1.0), x(cfg.LLm + 2, 2.0), x(cfg.LLm + 2, 3.0)]


@functools.lru_cache(maxsize=None)
def twin(obc):
    """(cfg, oracle, time indices, snapshot of every array the tests touch).  The snapshot is never written."""
    assert ref.available(obc)
    cfg, o, tix = bs.flather_state(obc, **SIZE)
    rng = np.random.default_rng(100 + obc)
    for name in STATE:
        a = o.field(name)
        amp = max(float(np.abs(a).max()), 0.05) * (0.1 if name == "t" else 1.0)
        a += amp * rng.standard_normal(a.shape)
        if name in ("u", "v"):
            # a smooth offset that differs between the time levels: along every edge the change in time
            # outweighs the gradients in places and not in others, so the cy clamp binds at both ends
            J, I = np.meshgrid(np.arange(a.shape[-2]), np.arange(a.shape[-1]), indexing="ij")
            for l in range(3):
                lev(a, l + 1, cfg.N)[...] += 2.0 * amp * np.cos(2.1 * l + 0.15 * J + 0.1 * I)
    rm = o.field("rmask")[0]
    for side in LAND.values():
        for i, j in side:
            rm[j + 1, i + 1] = 0.0
    um, vm, pm_ = o.field("umask")[0], o.field("vmask")[0], o.field("pmask")[0]
    um[:, 1:] = rm[:, 1:] * rm[:, :-1]
    vm[1:, :] = rm[1:, :] * rm[:-1, :]
    pm_[1:, 1:] = rm[1:, 1:] * rm[1:, :-1] * rm[:-1, 1:] * rm[:-1, :-1]
    for name, m in (("zeta", rm), ("ubar", um), ("vbar", vm), ("u", um), ("v", vm), ("t", rm)):
        o.field(name)[...] *= m
    for q, side in enumerate(ref.SIDES):           # boundary velocities of both signs, as bs.cext_state
        for comp in ("u", "v"):
            a = o.field("%s_%s" % (comp, side)).reshape(cfg.N, -1)
            m, k = np.arange(a.shape[1])[None, :], np.arange(cfg.N)[:, None]
            a += 2.0 * max(float(np.abs(a).max()), 0.01) * np.sin(2.0 * np.pi * 3.0 * m / a.shape[1] + 0.4 * k + q)
    snap = {n: o.field(n).copy() for n in STATE + MASKS + tuple(BRY) + ("h", "pm", "pn")}
    for a in snap.values():
        a.setflags(write=False)
    return cfg, o, tix, snap


def restore(o, snap):
    for n, a in snap.items():
        o.field(n)[...] = a


def setup(obc, mode, tuned):
    """The twin state in the oracle and in the reference, indices of the given stage set in both."""
    cfg, o, tix, snap = twin(obc)
    restore(o, snap)
    iic, kstp, knew, nstp = bs.fast_indices(tix, 2)[:4]
    tix = [iic, kstp, knew, nstp, 3, 3 - nstp] if mode == "corr" else [iic, kstp, knew, nstp, nstp, 3]
    o.set_tindex(tix)
    ub = ub_arrays(cfg) if tuned else None
    o.set_ub(ub if tuned else [None] * 4)
    r = ref.RefLib(obc)
    r.load(o, ub)
    S = dict(snap, cfg=cfg, tix=tix, ub=ub, dt=o.scalars()["dt"], dtfast=o.scalars()["dtfast"])
    return cfg, o, r, S


def compare(o, r, snap, wrote):
    """Every prognostic array bitwise; those in `wrote` moved off the input."""
    out = r.ocean()
    bad = [(n, int(np.sum(bits(out[n]) != bits(o.field(n))))) for n in STATE if not same(out[n], o.field(n))]
    assert not bad, bad
    for n in wrote:
        assert not same(out[n], snap[n]), n
        corners_written(o.cfg, n, out[n], snap[n])


def corners_written(cfg, name, out, snap):
    """The routine wrote the corner points it owns: those between two open sides for the velocities
    (u2dbc_im.F:455-478 and its twins), all four for zeta and the tracers."""
    L, M = cfg.LLm, cfg.MMm
    lo = {"u": (1, 0), "ubar": (1, 0), "v": (0, 1), "vbar": (0, 1)}.get(name, (0, 0))
    for ew, ns, i, j in (("west", "south", lo[0], lo[1]), ("east", "south", L + 1, lo[1]),
                         ("west", "north", lo[0], M + 1), ("east", "north", L + 1, M + 1)):
        both_open = bool(cfg.obc & OPEN[ew]) and bool(cfg.obc & OPEN[ns])
        if both_open or name in ("zeta", "t"):
            assert not same(out[..., j + 1, i + 1], snap[..., j + 1, i + 1]), (name, ew, ns)


def open_sides(cfg):
    return [s for s, bit in OPEN.items() if cfg.obc & bit]


def line(a, normal, c, m):
    """a (.., Mm+4, Lm+4) on the line of normal index c ('x': i = c, 'y': j = c) at the along-edge indices m."""
    return a[..., m + 1, c + 1] if normal == "x" else a[..., c + 1, m + 1]


def lev(a, l, N):
    return a[(l - 1) * N:l * N]


def all_taken(arms, where):
    missing = [(where, k) for k, v in arms.items() if not bool(np.any(v))]
    assert not missing, missing


def mask_arms(S, name, normal, c, m):
    w = line(S[name][0], normal, c, m)
    return {"wet edge point": w == 1.0, "dry edge point": w == 0.0}


def ub_arms(S, side, m):
    if S["ub"] is None:
        return {}
    b = S["ub"][ref.SIDES.index(side)][m]
    return {"ub < 0": b < 0.0, "0 < ub < 1": (b > 0.0) & (b < 1.0), "ub > 1": b > 1.0}


def normal_arms(S, comp, side):
    """Orlanski radiation of the normal component (u on west / east, v on south / north)."""
    cfg, N = S["cfg"], S["cfg"].N
    nstp, nnew = S["tix"][3], S["tix"][5]
    normal, nal, nmax = ("x", cfg.MMm, cfg.LLm) if comp == "u" else ("y", cfg.LLm, cfg.MMm)
    low = side in ("west", "south")
    b, i1, i2 = (1, 2, 3) if low else (nmax + 1, nmax, nmax - 1)
    m, m1 = np.arange(1, nal + 1), np.arange(1, nal + 2)
    old, new = lev(S[comp], nstp, N), lev(S[comp], nnew, N)
    gi = (line(old, normal, i1, m1) - line(old, normal, i1, m1 - 1)) * line(S["pmask"][0], normal, i1, m1)
    dft = line(old, normal, i1, m) - line(new, normal, i1, m)
    dfx = line(new, normal, i1, m) - line(new, normal, i2, m)
    first = dft * (gi[:, :-1] + gi[:, 1:]) > 0.0
    dfy = np.where(first, gi[:, :-1], gi[:, 1:])
    cff = np.maximum(dfx * dfx + dfy * dfy, EPS)
    raw = dft * dfy
    inflow = dft * dfx < 0.0
    data = S["%s_%s" % (comp, side)].reshape(N, -1)[:, 1:-1]
    data_in = data > 0.0 if low else data < 0.0
    arms = {"outflow": ~inflow, "inflow, boundary data bind": inflow & data_in, "inflow, ubind binds": inflow & ~data_in,
            "first tangential gradient": first, "second tangential gradient": ~first,
            "cy clamped at +cff": ~inflow & (raw > cff), "cy clamped at -cff": ~inflow & (raw < -cff),
            "cy inside": ~inflow & (np.abs(raw) <= cff)}
    arms.update(mask_arms(S, comp + "mask", normal, b, m))
    arms.update(ub_arms(S, side, m))
    return arms


def tangential_arms(S, comp, side, fast=False):
    """The tangential component (u on south / north, v on west / east): radiates for cx > 0, binds otherwise."""
    cfg, N = S["cfg"], S["cfg"].N
    normal, nal, nmax = ("y", cfg.LLm, cfg.MMm) if comp == "u" else ("x", cfg.MMm, cfg.LLm)
    other = "v" if comp == "u" else "u"
    low = side in ("west", "south")
    m = np.arange(2, nal + 1)
    if fast:
        vel = S[other + "bar"][S["tix"][1] - 1]
    else:
        vel = lev(S[other], S["tix"][4], N)
    c = 1 if low else nmax + 1
    s = line(vel, normal, c, m) + line(vel, normal, c, m - 1)
    cx_pos = (-s if low else s) > 0.0
    arms = {"radiates (cx > 0)": cx_pos, "binds (cx <= 0)": ~cx_pos}
    arms.update(mask_arms(S, comp + "mask", normal, 0 if low else nmax + 1, m))
    if not fast:
        arms.update(ub_arms(S, side, m))
    return arms


def tracer_arms(S, side):
    cfg, N = S["cfg"], S["cfg"].N
    normal, nal, nmax = ("x", cfg.MMm, cfg.LLm) if side in ("west", "east") else ("y", cfg.LLm, cfg.MMm)
    low = side in ("west", "south")
    m = np.arange(1, nal + 1)
    vel = line(lev(S["u" if normal == "x" else "v"], S["tix"][4], N), normal, 1 if low else nmax + 1, m)
    cx_pos = (-vel if low else vel) > 0.0
    arms = {"radiates (cx > 0)": cx_pos, "binds (cx <= 0)": ~cx_pos}
    arms.update(mask_arms(S, "rmask", normal, 0 if low else nmax + 1, m))
    arms.update(ub_arms(S, side, m))
    return arms


def check_metrics(S):
    assert float(S["pm"].min()) > 0.0 and float(S["pn"].min()) > 0.0 and S["dt"] > 0.0 and S["dtfast"] > 0.0


CASES3D = [(obc, mode, tuned) for obc in ref.VARIANTS for mode in ("pred", "corr") for tuned in (False, True)]


def test_libraries_cover_both_corner_kinds():
    """Open-open corners with sides 15, open-closed and closed-closed with 5 and 10; the sizes are what the tests assume."""
    kinds = set()
    for obc in ref.VARIANTS:
        r = ref.RefLib(obc)
        assert (r.LLm, r.MMm, r.N, r.NT) == (SIZE["LLm"], SIZE["MMm"], SIZE["N"], 2) and r.LLm != r.MMm
        for ew, ns in ((1, 4), (2, 4), (1, 8), (2, 8)):
            kinds.add((bool(obc & ew), bool(obc & ns)))
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("obc", ref.VARIANTS)
def test_zetabc(obc):
    cfg, o, r, S = setup(obc, "corr", False)
    check_metrics(S)
    for side in open_sides(cfg):
        normal, nal, nmax = ("x", cfg.MMm, cfg.LLm) if side in ("west", "east") else ("y", cfg.LLm, cfg.MMm)
        all_taken(mask_arms(S, "rmask", normal, 0 if side in ("west", "south") else nmax + 1, np.arange(1, nal + 1)),
                  ("zetabc", side))
    zin = S["zeta"][S["tix"][2] - 1] * 1.25
    zo, zr = zin.copy(), zin.copy()
    o.L.or_zetabc(o.h, zo.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    r.zetabc(zr)
    assert same(zo, zr), int(np.sum(bits(zo) != bits(zr)))
    assert not same(zr, zin)
    corners_written(cfg, "zeta", zr, zin)
    compare(o, r, S, ())


@pytest.mark.parametrize("routine,comp", [("u2dbc", "u"), ("v2dbc", "v")])
@pytest.mark.parametrize("obc", ref.VARIANTS)
def test_2d_momentum(obc, routine, comp):
    cfg, o, r, S = setup(obc, "corr", False)
    check_metrics(S)
    cxs = bs.flather_cx(o, cfg)
    for side in open_sides(cfg):
        if (side in ("west", "east")) == (comp == "u"):          # normal: Flather
            nmax = cfg.LLm if comp == "u" else cfg.MMm
            arms = {"cx > 1 - 1/sqrt(2)": cxs[side] > bs.K_FL, "cx < 1 - 1/sqrt(2)": cxs[side] < bs.K_FL}
            arms.update(mask_arms(S, comp + "mask", "x" if comp == "u" else "y",
                                  1 if side in ("west", "south") else nmax + 1, np.arange(1, cxs[side].size + 1)))
        else:
            arms = tangential_arms(S, comp, side, fast=True)
        all_taken(arms, (routine, side))
    o.call(routine)
    r.call(routine)
    compare(o, r, S, (comp + "bar",))


@pytest.mark.parametrize("routine,comp", [("u3dbc", "u"), ("v3dbc", "v")])
@pytest.mark.parametrize("obc,mode,tuned", CASES3D)
def test_3d_momentum(obc, mode, tuned, routine, comp):
    cfg, o, r, S = setup(obc, mode, tuned)
    check_metrics(S)
    for side in open_sides(cfg):
        if (side in ("west", "east")) == (comp == "u"):
            arms = normal_arms(S, comp, side)
        else:
            arms = tangential_arms(S, comp, side)
        all_taken(arms, (routine, side, mode, tuned))
    o.call(routine)
    r.call(routine)
    compare(o, r, S, (comp,))


@pytest.mark.parametrize("obc,mode,tuned", CASES3D)
def test_t3dbc(obc, mode, tuned):
    cfg, o, r, S = setup(obc, mode, tuned)
    check_metrics(S)
    for side in open_sides(cfg):
        all_taken(tracer_arms(S, side), ("t3dbc", side, mode, tuned))
    for itrc in range(1, cfg.NT + 1):
        o.call("t3dbc", itrc)
        r.call("t3dbc", itrc)
    compare(o, r, S, ("t",))


@pytest.mark.parametrize("obc", ref.VARIANTS)
def test_set_nudgcof(obc):
    """visc2_r, visc2_p and diff2 after init_arrays_mixing and set_nudgcof, over non-zero background values."""
    cfg = bs.flather_cfg(obc, **SIZE)
    cfg.visc2, cfg.tnu2, cfg.v_sponge = 5.0, 2.0, 37.5
    o = oracle.Oracle(cfg)
    o.init()
    out = ref.RefLib(obc).set_nudgcof(cfg.v_sponge, cfg.visc2, [cfg.tnu2] * cfg.NT)
    for n, a in out.items():
        assert same(a, o.field(n)), (n, int(np.sum(bits(a) != bits(o.field(n)))))
        assert float(a.max()) > float(a.min()) >= min(cfg.visc2, cfg.tnu2)
