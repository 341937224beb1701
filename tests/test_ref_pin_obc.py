"""The oracle's open-boundary and sponge code against the reference's own routines.

oracle/ref/build_ref.sh compiles zetabc_tile, u2dbc_tile, v2dbc_tile,
u3dbc_tile, v3dbc_tile, t3dbc_tile and set_nudgcof from the reference tree,
unchanged, for the Iceland boundary switch set (OBC_M2FLATHER, OBC_M3ORLANSKI,
OBC_TORLANSKI, *_FRC_BRY, SPONGE, SPONGE_TUNE, MASKING) at 24 x 20 x 6 with
every non-empty set of open sides, 1 .. 15 (bits 1 W, 2 E, 4 S, 8 N), so that
each of the four corners is seen open-open, open on one side only (either
one) and closed-closed.  Each test hands one state to the reference routine
and to its restatement in oracle/oracle_obc.c (or_set_nudgcof in
oracle_main.c) and compares every element of every array the routine can
write, ghost rows and corners included.

Agreement is bitwise: the routines use + - * / sqrt min max in IEEE double,
both sides are built without contraction, so any difference is a difference
in the order of evaluation or in the arm taken.  No tolerance.

The state is a perturbed twin of a mid-run state (branch_states.twin_state:
flather_state at the library's size): seeded noise of the fields' own size on every time
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

import numpy as np
import pytest

import branch_states as bs
import oracle
import oracle.ref as ref

SIZE = bs.TWIN_SIZE
OPEN = bs.OPEN
STATE = bs.TWIN_STATE
# the twin state and the arm restatements live in branch_states, shared with tests/test_gpu_open_sides.py
ub_arrays, restore, open_sides, all_taken = bs.ub_arrays, bs.twin_restore, bs.open_sides, bs.all_taken
mask_arms, ub_arms, normal_arms, tangential_arms, tracer_arms = (bs.mask_arms, bs.ub_arms, bs.normal_arms,
                                                                 bs.tangential_arms, bs.tracer_arms)
CORNERS = (("west", "south"), ("east", "south"), ("west", "north"), ("east", "north"))

pytestmark = pytest.mark.skipif(not (ref.have_tree() or all(ref.available(v) for v in ref.VARIANTS)),
                                reason="neither oracle/_ref libraries nor a reference tree")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def twin(obc):
    """(cfg, oracle, time indices, snapshot of every array the tests touch).  The snapshot is never written."""
    assert ref.available(obc)
    return bs.twin_state(obc, **SIZE)


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


def corner_points(cfg, name):
    """(E/W side, N/S side, i, j) of the four corner points of the field, Fortran indices."""
    L, M = cfg.LLm, cfg.MMm
    lo = {"u": (1, 0), "ubar": (1, 0), "v": (0, 1), "vbar": (0, 1)}.get(name, (0, 0))
    return (("west", "south", lo[0], lo[1]), ("east", "south", L + 1, lo[1]),
            ("west", "north", lo[0], M + 1), ("east", "north", L + 1, M + 1))


def corners_written(cfg, name, out, snap):
    """The routine wrote the corner points it owns: those between two open sides for the velocities
    (u2dbc_im.F:455-478 and its twins), all four for zeta and the tracers -- the mixed corners, between
    an open and a closed side, among them."""
    for ew, ns, i, j in corner_points(cfg, name):
        o_ew, o_ns = bool(cfg.obc & OPEN[ew]), bool(cfg.obc & OPEN[ns])
        kind = "open-open" if o_ew and o_ns else "mixed" if o_ew or o_ns else "closed-closed"
        if kind == "open-open" or name in ("zeta", "t"):
            assert not same(out[..., j + 1, i + 1], snap[..., j + 1, i + 1]), (name, ew, ns, kind)


def check_metrics(S):
    assert float(S["pm"].min()) > 0.0 and float(S["pn"].min()) > 0.0 and S["dt"] > 0.0 and S["dtfast"] > 0.0


CASES3D = [(obc, mode, tuned) for obc in ref.VARIANTS for mode in ("pred", "corr") for tuned in (False, True)]


def test_libraries_cover_every_kind_at_every_corner():
    """Each of the four corners, which have hand-written lines of their own in every boundary routine, sees
    all four kinds across the libraries: open-open, E/W open only, N/S open only, closed-closed.  The sizes
    are what the tests assume."""
    kinds = {c: set() for c in CORNERS}
    for obc in ref.VARIANTS:
        r = ref.RefLib(obc)
        assert (r.LLm, r.MMm, r.N, r.NT) == (SIZE["LLm"], SIZE["MMm"], SIZE["N"], 2) and r.LLm != r.MMm
        assert r.obc == obc
        for ew, ns in CORNERS:
            kinds[(ew, ns)].add((bool(obc & OPEN[ew]), bool(obc & OPEN[ns])))
    every = {(True, True), (True, False), (False, True), (False, False)}
    short = {c: sorted(every - k) for c, k in kinds.items() if k != every}
    assert not short, short


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
