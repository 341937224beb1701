"""Open-side sweep: parity for every set of open boundaries at every corner.

Every other open-boundary test runs the sides 15 (all four), 5 (west +
south) and 10 (east + north) -- bits 1 W, 2 E, 4 S, 8 N.  Those three leave
four of the twelve corner / kind pairs to nothing: the south-west and
north-east corners are never open on one side only.  Each corner has lines of
its own in every boundary kernel (k_obc.hip, k_bc_exchange.hip, k_s2d_zetabc
and k_s2d_edges of k_step2d.hip), so here all fifteen non-empty sets run, at
24 x 20 x 6 (the size at which tests/test_ref_pin_obc.py pins the oracle's
boundary code to the reference, for all fifteen sets) and at its transpose
20 x 24 x 6: every other open grid of the suite has Lm > Mm, and the edge
launches are sized by max(Lm, Mm) + 4 over per-side strides Mm + 2 (W, E) and
Lm + 2 (S, N).  Cells are 2.3 km, curvilinear, with the island
(branch_states.flather_cfg).

  init        the 24 boundary arrays, visc2_r, visc2_p, diff2 and the four
              masks bitwise against the oracle; the sponge band restated in
              numpy: full strength on every open side's ghost line, nothing
              of its own on a closed side
  routines    step2d at iif = 1, 2, pre_step3d, step3d_uv2, step3d_t (the
              last three with ub_tune off and on) on branch_states' twin
              state, whole arrays with ghost rows and corners, within
              RTOL_ROUTINE; before comparing, every data-dependent arm is
              asserted taken on every open side; a failure names the corner
              points and edge lines that are off
  runs        12 steps of the Iceland switch set, PROGNOSTIC on the interior
              and zeta ubar vbar u v t over whole arrays within RMS_RUN;
              every open side moved, every closed wall's normal velocity is 0
  decomposed  sides 6 and 9 on 2 x 2 (each rank a different local mix: one
              open-open, two mixed and one closed-closed corner) and 3 x 2
              (the middle column owns no W / E edge), bitwise
  tides       sides 6 and 9: the open sides' zeta / ubar / vbar sums bitwise
              (tides.F:131-226 in numpy), the closed sides' arrays untouched

The ISO edge copies at sides 6 and 9 are in tests/test_iso.py.

The sponge test runs over a zero background: the analytic-case entry of the
library has no background visc2 / tnu2 (the oracle's non-zero background is
pinned to the reference in test_ref_pin_obc.test_set_nudgcof).  On these
grids a closed side's mid-point lies within the 15-point band of a
neighbouring open side, so "absent" is asserted as: the value there is what
the open sides alone give, below full strength, and exactly the background
where no open side is within 15 points.

The arms of the 3-D routines are restated, as in the pin, from the state
handed in: the routines proper form u, v, t (nnew) inside the domain before
their boundary code reads them, so for the Orlanski terms that depend on the
new level the assertion says that the state carries every arm, not that the
call took it; the arms that depend on inputs alone (boundary data, ub,
masks, the tangential and tracer cx, all of step2d's) are exact.

Measured on the MI355X as the library stood (nothing had to be fixed):
init, the decompositions and the tides bitwise; all five routine calls equal
to the oracle bitwise (error 0) for all fifteen sets at both sizes, ub_tune
off and on; the 12-step runs 0 (sides 6) to 2.3e-15 (sides 12) over whole
arrays and at most 3.2e-12 on the interior (Wi, relative to its RMS).

What the sweep catches: three value-only changes, one at a time, in a
scratch copy of the kernels (a predicate or an index range, no access moved).
  * k_u3dbc_obc phase 1, the closed arm's first column `is` -> `b.istrU`
    (k_obc.hip:130): test_3d_routine_parity fails pre_step3d and step3d_uv2,
    ub_tune off and on, for every set with the south or north side closed
    (1 .. 11; 88 cases) -- u 1.7e-4 to 0.54 of its maximum, reported at
    "corner SW" and "corner NW" alone -- and test_whole_run_rms fails the
    sets 1, 3, 5, 7, 9, 11 (v 6.5e-10 to 1.5e-8, We to 2.3e-8).  Of the 15 / 5 /
    10 tests, test_open_boundary_routine_parity[5-pre_step3d] fails (u
    6.7e-6: a stale value of the step before, where the twin state holds
    noise); the rest of test_gpu_obc.py and test_gpu_branches.py passes.
  * k_s2d_edges phase 2, the south-west ubar corner's `S && W` -> `S`
    (k_step2d.hip:870): test_step2d_parity and test_whole_run_rms fail for
    the sets with the south open and the west closed, 4, 6, 12, 14, at both
    sizes (16 cases; ubar 1.2e-2 to 0.14 at "corner SW", DU_avg1 to 7e-3).
    Every single-domain test on 15 / 5 / 10 passes (test_gpu_obc.py,
    test_gpu_branches.py, the open families of the width sweep, coasts,
    configs, forcing, ISO, register).  Only decomposed runs of sides 15
    notice, by the accident that a rank off the west edge has `W` false: 8
    bitwise decomposition tests (test_gpu_obc, subdomains, coasts, configs).
  * k_s2d_zetabc's south arm `obc & 4` -> `obc & 8` (k_step2d.hip:101):
    test_step2d_parity and test_whole_run_rms fail for every set with one of
    south and north open and the other closed, 4 .. 11 (32 cases; zeta to
    0.17 on "south line" and the two southern corners, run zeta to 7.8e-3).
    The 15 / 5 / 10 tests see it too: sides 5 and 10 are such sets
    (test_open_boundary_routine_parity[5-step2d] zeta 8.0e-2, [10-step2d]
    1.1e-2, test_flather_high_courant[5], [10]).
"""
import functools
import math

import numpy as np
import pytest

import branch_states as bs
import oracle
import romsgpu
from test_gpu_branches import obc_model
from test_gpu_obc import BRY, full, obc_cfg
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, check_fields, copy_state

pytestmark = pytest.mark.gpu

SETS = tuple(range(1, 16))
SIZES = ((24, 20, 6), (20, 24, 6))
SWEEP = [(obc, size) for size in SIZES for obc in SETS]
SWEEP_IDS = ["obc%d-%dx%dx%d" % ((obc,) + size) for obc, size in SWEEP]
MASKS = ("rmask", "umask", "vmask", "pmask")
STATE = ("zeta", "ubar", "vbar", "u", "v", "t")
V_SPONGE = 37.5                   # not a power of two: the product with the band's weight rounds
SPONGE_WIDTH = 15                 # set_nudgcof.F: isp = 15 + 1 points of linear decay
RUN_STEPS = 12
# staggering of every compared field: its first column / row inside the ghost ring (Fortran i, j)
FIRST = dict(ubar=(1, 0), u=(1, 0), DU_avg1=(1, 0), FlxU=(1, 0), vbar=(0, 1), v=(0, 1), DV_avg1=(0, 1), FlxV=(0, 1))


def size_kw(size):
    return dict(LLm=size[0], MMm=size[1], N=size[2])


# -------------------------------------------------------------- reporting ----
def places(cfg, name):
    """The four corner points and the four edge lines of a field, as index tuples into (.., Mm+4, Lm+4)."""
    L, M = cfg.LLm, cfg.MMm
    i0, j0 = FIRST.get(name, (0, 0))
    w, e, s, n = i0 + 1, L + 2, j0 + 1, M + 2
    inner_i, inner_j = slice(w + 1, e), slice(s + 1, n)
    return {"corner SW": (Ellipsis, s, w), "corner SE": (Ellipsis, s, e), "corner NW": (Ellipsis, n, w),
            "corner NE": (Ellipsis, n, e), "west line": (Ellipsis, inner_j, w), "east line": (Ellipsis, inner_j, e),
            "south line": (Ellipsis, s, inner_i), "north line": (Ellipsis, n, inner_i)}


def by_place(cfg, name, a, b):
    """Error of a against b at each corner point and on each edge line, relative to max|b| as `full`."""
    scale = max(float(np.max(np.abs(b))), 1e-300)
    return {k: float(np.max(np.abs(a[ix] - b[ix]))) / scale for k, ix in places(cfg, name).items()}


def judge(tag, cfg, pairs, tol, err=full):
    """pairs: {label: (field name, got, want)}.  Prints every whole-array figure, then asserts; a failure
    carries the figures of the four corners and four edge lines of each field that is off."""
    errs = {k: err(a, b) for k, (n, a, b) in pairs.items()}
    for k, e in errs.items():
        print("%s %s %.3e" % (tag, k, e))
    bad = {k: e for k, e in errs.items() if not e <= tol}
    where = {k: {p: "%.2e" % v for p, v in by_place(cfg, pairs[k][0], pairs[k][1], pairs[k][2]).items() if v > 0.0}
             for k in bad}
    assert not bad, (tag, bad, where)
    return errs


def rms_whole(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2))) / max(1.0, float(np.sqrt(np.mean(b ** 2))))


# ------------------------------------------------------------------- init ----
def sponge_weight(cfg):
    """set_nudgcof.F:42-64 on the rho points 0..Lm+1 x 0..Mm+1: (isp - ibnd) / isp with ibnd the distance
    to the nearest open side, capped at isp."""
    L, M, isp = cfg.LLm, cfg.MMm, SPONGE_WIDTH + 1
    J, I = np.meshgrid(np.arange(M + 2), np.arange(L + 2), indexing="ij")
    ibnd = np.full(I.shape, isp)
    for bit, dist in ((1, I), (2, L + 1 - I), (4, J), (8, M + 1 - J)):
        if cfg.obc & bit:
            ibnd = np.minimum(ibnd, dist)
    return (isp - ibnd).astype(np.float64) / float(isp)


def check_sponge(cfg, o):
    """The band is there along each open side and not along a closed one."""
    L, M = cfg.LLm, cfg.MMm
    wk = sponge_weight(cfg)
    mid = {"west": (M // 2, 0), "east": (M // 2, L + 1), "south": (0, L // 2), "north": (M + 1, L // 2)}   # (j, i)
    away = {"west": lambda j, i: i, "east": lambda j, i: L + 1 - i, "south": lambda j, i: j,
            "north": lambda j, i: M + 1 - j}
    for name in ("visc2_r", "diff2"):
        a = o.field(name)[..., 1:-1, 1:-1]
        assert np.array_equal(a, np.broadcast_to(0.0 + V_SPONGE * wk, a.shape)), name
        for side, (j, i) in mid.items():
            v = a[..., j, i]
            if cfg.obc & bs.OPEN[side]:
                assert np.all(v == V_SPONGE), (name, side, "band missing on an open side")
            else:
                assert np.all(v < V_SPONGE) and np.all(v == V_SPONGE * wk[j, i]), (name, side)
                near = min(away[s](j, i) for s in bs.open_sides(cfg))
                assert (near > SPONGE_WIDTH) == bool(np.all(v == 0.0)), (name, side, near)
    vp = o.field("visc2_p")[0]
    for side, (j, i) in mid.items():
        jj, ii = max(j, 1), max(i, 1)           # psi points start at 1
        assert (vp[jj + 1, ii + 1] > 0.75 * V_SPONGE) == bool(cfg.obc & bs.OPEN[side]), ("visc2_p", side)


@pytest.mark.parametrize("obc,size", SWEEP, ids=SWEEP_IDS)
def test_init_boundary_data_sponge_and_masks_match_oracle(obc, size):
    cfg = bs.flather_cfg(obc, ndtfast=30, **size_kw(size))
    cfg.v_sponge = V_SPONGE
    o = oracle.Oracle(cfg)
    o.init()
    check_sponge(cfg, o)
    assert float(np.min(o.field("rmask"))) == 0.0
    m = obc_model(cfg)
    try:
        bad = [(n, full(m.get(n), o.field(n))) for n in BRY + ["visc2_r", "visc2_p", "diff2"] + list(MASKS)]
    finally:
        m.close()
    bad = [x for x in bad if not x[1] == 0.0]
    assert not bad, bad


# --------------------------------------------------------------- routines ----
@functools.lru_cache(maxsize=None)
def twin(obc, size):
    """An oracle of this file's own in branch_states' twin state, and a copy of every field: each test
    starts from the copy, whatever ran before."""
    cfg, o, tix, _ = bs.build_twin(obc, **size_kw(size))
    snap = {n: o.field(n).copy() for n in romsgpu.FIELDS}
    for a in snap.values():
        a.setflags(write=False)
    return cfg, o, tix, snap


def stage(obc, size, mode, tuned):
    """The twin state back in the oracle, indices of the stage set, ub_tune off or on."""
    cfg, o, tix, snap = twin(obc, size)
    for n, a in snap.items():
        o.field(n)[...] = a
    iic, kstp, knew, nstp = bs.fast_indices(tix, 2)[:4]
    tix = [iic, kstp, knew, nstp, 3, 3 - nstp] if mode == "corr" else [iic, kstp, knew, nstp, nstp, 3]
    o.set_tindex(tix)
    ub = bs.ub_arrays(cfg) if tuned else None
    o.set_ub(ub if tuned else [None] * 4)
    return cfg, o, tix, ub


def arm_view(o, cfg, tix, ub):
    """What the arm restatements read, from the oracle's arrays as they stand."""
    S = {n: o.field(n) for n in STATE + MASKS + tuple(bs.TWIN_BRY)}
    S.update(cfg=cfg, tix=tix, ub=ub)
    return S


def momentum_arms(S, cfg, tag):
    for side in bs.open_sides(cfg):
        for comp in ("u", "v"):
            normal = (side in ("west", "east")) == (comp == "u")
            arms = bs.normal_arms(S, comp, side) if normal else bs.tangential_arms(S, comp, side)
            bs.all_taken(arms, (tag, comp, side))


def tracer_arms(S, cfg, tag):
    for side in bs.open_sides(cfg):
        bs.all_taken(bs.tracer_arms(S, side), (tag, "t", side))


def fast_arms(S, o, cfg, tag):
    """u2dbc / v2dbc and zetabc: Flather's cx on both sides of 1 - 1/sqrt(2), the tangential cx of both
    signs (from ubar, vbar at kstp: inputs of this fast step), wet and dry points."""
    cxs = bs.flather_cx(o, cfg)
    for side in bs.open_sides(cfg):
        ew = side in ("west", "east")
        comp, normal, nmax, nal = ("u", "x", cfg.LLm, cfg.MMm) if ew else ("v", "y", cfg.MMm, cfg.LLm)
        low = side in ("west", "south")
        arms = {"cx > 1 - 1/sqrt(2)": cxs[side] > bs.K_FL, "cx < 1 - 1/sqrt(2)": cxs[side] < bs.K_FL}
        arms.update(bs.mask_arms(S, comp + "mask", normal, 1 if low else nmax + 1, np.arange(1, nal + 1)))
        bs.all_taken(arms, (tag, comp, side))
        bs.all_taken(bs.tangential_arms(S, "v" if ew else "u", side, fast=True), (tag, "tangential", side))
        bs.all_taken(bs.mask_arms(S, "rmask", normal, 0 if low else nmax + 1, np.arange(1, nal + 1)),
                     (tag, "zeta", side))


def all_finite(o, names):
    bad = [n for n in names if not np.isfinite(o.field(n)).all()]
    assert not bad, bad


STEP2D_OUT = ["zeta", "ubar", "vbar", "DU_avg1", "DV_avg1", "Zt_avg1"]
ROUTINES3D = {"pre_step3d": ("pred", ["u", "v", "t"]),
              "step3d_uv2": ("corr", ["u", "v", "ubar", "vbar", "FlxU", "FlxV"]),
              "step3d_t": ("corr", ["t"])}


def oracle_step2d(obc, size, iif, before=None):
    """Fast step iif on the oracle, arms asserted from its inputs; `before` runs between the two."""
    cfg, o, tix, _ = twin(obc, size)
    fast = bs.fast_indices(tix, iif)
    o.set_tindex(fast)
    o.L.or_set_iif(o.h, iif)
    fast_arms(arm_view(o, cfg, fast, None), o, cfg, "step2d iif=%d obc=%d" % (iif, obc))
    if before is not None:
        before(fast)
    o.call("step2d")
    all_finite(o, STEP2D_OUT)
    return fast


def oracle_3d_arms(obc, size, routine, tuned):
    mode = ROUTINES3D[routine][0]
    cfg, o, tix, ub = stage(obc, size, mode, tuned)
    S = arm_view(o, cfg, tix, ub)
    tag = "%s obc=%d ub_tune=%d" % (routine, obc, tuned)
    if routine != "step3d_t":
        momentum_arms(S, cfg, tag)
    if routine != "step3d_uv2":
        tracer_arms(S, cfg, tag)
    return cfg, o, tix, ub


@pytest.mark.parametrize("obc,size", SWEEP, ids=SWEEP_IDS)
def test_step2d_parity(obc, size):
    cfg, o, tix, ub = stage(obc, size, "corr", False)
    m = obc_model(cfg)
    pairs = {}
    try:
        copy_state(o, m)
        for iif in (1, 2):
            oracle_step2d(obc, size, iif, lambda fast: m.set_tindex(*fast, iif=iif, nfast=o.nfast()))
            m.step2d()
            m.sync()
            for n in STEP2D_OUT:
                pairs["iif=%d %s" % (iif, n)] = (n, m.get(n), o.field(n).copy())
    finally:
        m.close()
    judge("step2d obc=%d %dx%dx%d" % ((obc,) + size), cfg, pairs, RTOL_ROUTINE)


@pytest.mark.parametrize("tuned", [False, True], ids=["ub_off", "ub_on"])
@pytest.mark.parametrize("routine", list(ROUTINES3D))
@pytest.mark.parametrize("obc,size", SWEEP, ids=SWEEP_IDS)
def test_3d_routine_parity(obc, size, routine, tuned):
    cfg, o, tix, ub = oracle_3d_arms(obc, size, routine, tuned)
    outs = ROUTINES3D[routine][1]
    m = obc_model(cfg)
    try:
        if tuned:
            m.set_ub_tune(ub)
        copy_state(o, m)
        m.set_tindex(*tix, iif=2, nfast=o.nfast())
        o.call(routine)
        all_finite(o, outs)
        getattr(m, routine)()
        m.sync()
        pairs = {n: (n, m.get(n), o.field(n)) for n in outs}
    finally:
        m.close()
    judge("%s obc=%d %dx%dx%d ub_tune=%d" % ((routine, obc) + size + (tuned,)), cfg, pairs, RTOL_ROUTINE)


# ------------------------------------------------------------------- runs ----
def run_cfg(obc, size):
    """The Iceland switch set on the sweep's grid: open sides, sponge, island, CURVGRID, KPP without CONVEC."""
    L, M, N = size
    return obc_cfg(obc=obc, lmd=oracle.LMD_ICELAND, curv=1, LLm=L, MMm=M, N=N, sizex=bs.FLATHER_CELL * L,
                   sizey=bs.FLATHER_CELL * M)


def side_lines(cfg):
    """Per side: (normal barotropic and 3-D velocity, index of its boundary line, index of zeta's ghost line)."""
    L, M = cfg.LLm, cfg.MMm
    return {"west": ("ubar", "u", (Ellipsis, slice(2, M + 2), 2), (Ellipsis, slice(2, M + 2), 1)),
            "east": ("ubar", "u", (Ellipsis, slice(2, M + 2), L + 2), (Ellipsis, slice(2, M + 2), L + 2)),
            "south": ("vbar", "v", (Ellipsis, 2, slice(2, L + 2)), (Ellipsis, 1, slice(2, L + 2))),
            "north": ("vbar", "v", (Ellipsis, M + 2, slice(2, L + 2)), (Ellipsis, M + 2, slice(2, L + 2)))}


def check_sides_moved(cfg, first, get):
    """Every open side carried flow: its normal velocity and its zeta ghost line left the initial state.
    Every closed side is a wall: its normal velocity is exactly 0 at every level and time index."""
    for side, (bar, vel, at, ghost) in side_lines(cfg).items():
        if cfg.obc & bs.OPEN[side]:
            for n, ix in ((bar, at), (vel, at), ("zeta", ghost)):
                assert not np.array_equal(get(n)[ix], first[n][ix]), (side, n, "did not move")
        else:
            for n in (bar, vel):
                assert np.all(get(n)[at] == 0.0), (side, n, "flow through a wall")


@pytest.mark.parametrize("obc,size", SWEEP, ids=SWEEP_IDS)
def test_whole_run_rms(obc, size):
    cfg = run_cfg(obc, size)
    o = oracle.Oracle(cfg)
    o.init()
    first = {n: o.field(n).copy() for n in STATE}
    o.step(RUN_STEPS)
    all_finite(o, PROGNOSTIC)
    check_sides_moved(cfg, first, o.field)
    m = obc_model(cfg)
    try:
        m.step(RUN_STEPS)
        m.sync()
        assert o.tindex() == m.t.as_list()
        tag = "run obc=%d %dx%dx%d" % ((obc,) + size)
        for n, e in check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms").items():
            print("%s interior %s %.3e" % (tag, n, e))
        got = {n: m.get(n) for n in STATE}
    finally:
        m.close()
    judge(tag + " whole", cfg, {n: (n, got[n], o.field(n)) for n in STATE}, RMS_RUN, err=rms_whole)
    check_sides_moved(cfg, first, got.__getitem__)


# ---------------------------------------------------------- decomposition ----
@pytest.mark.parametrize("npx,npe", [(2, 2), (3, 2)])
@pytest.mark.parametrize("obc", [6, 9])
def test_decomposition_bitwise(obc, npx, npe):
    """East + south (6) and west + north (9) open: on 2 x 2 the four ranks hold an open-open, two mixed and
    a closed-closed corner; on 3 x 2 the middle column has neither a west nor an east edge.  No sponge."""
    from test_gpu_multirank import _case, check_decomposition
    check_decomposition(dict(_case("basin_obc"), obc=obc), npx, npe, nsteps=4)


# ------------------------------------------------------------------ tides ----
def tide_lines(L, M):
    """tides.F:131-226 on a single domain: per side and variable, (first index written, index of the line
    in a (Mm+4, Lm+4) plane).  West / east arrays run over j = 0..Mm+1, south / north over i = 0..Lm+1."""
    col = lambda i, a: (a, (slice(a + 1, M + 3), i + 1))
    row = lambda j, a: (a, (j + 1, slice(a + 1, L + 3)))
    return {"west": {"zeta": col(0, 0), "ubar": col(1, 0), "vbar": col(0, 1)},
            "east": {"zeta": col(L + 1, 0), "ubar": col(L + 1, 0), "vbar": col(L + 1, 1)},
            "south": {"zeta": row(0, 0), "ubar": row(0, 1), "vbar": row(1, 0)},
            "north": {"zeta": row(M + 1, 0), "ubar": row(M + 1, 1), "vbar": row(M + 1, 0)}}


@pytest.mark.parametrize("obc", [6, 9])
def test_set_tides_bitwise(obc):
    from test_gpu_forcing import open_basin
    c, m = open_basin(obc=obc)
    try:
        rng = np.random.default_rng(5 + obc)
        ftide = np.array([1.405e-4, 1.454e-4, 7.29e-5])
        nt = ftide.size
        shp = (nt,) + m.get("zeta").shape[1:]
        bry = [(rng.standard_normal(shp), rng.standard_normal(shp)) for _ in range(3)]
        m.set_tide_data(ftide, pot=(0.1 * rng.standard_normal(shp), 0.1 * rng.standard_normal(shp)), bry=bry)
        names = ["%s_%s" % (v, s) for v in ("zeta", "ubar", "vbar") for s in bs.SIDES]
        base = {n: m.get(n).copy() for n in names}
        time = 3600.0 * 7
        m.set_tides(time)
        got = {n: m.get(n) for n in names}
    finally:
        m.close()
    cs = [math.cos(f * (time + 0.5 * c.dt)) for f in ftide]
    sn = [math.sin(f * (time + 0.5 * c.dt)) for f in ftide]
    lines = tide_lines(c.LLm, c.MMm)
    for side in bs.SIDES:
        for q, var in enumerate(("zeta", "ubar", "vbar")):
            name = "%s_%s" % (var, side)
            want = base[name].copy()
            if c.obc & bs.OPEN[side]:
                a, ix = lines[side][var]
                flat = want.reshape(-1)
                for t in range(nt):
                    flat[a:] = flat[a:] + bry[q][0][t][ix] * cs[t] - bry[q][1][t][ix] * sn[t]
                assert not np.array_equal(want, base[name]), name
            assert np.array_equal(got[name], want), (name, "open" if c.obc & bs.OPEN[side] else "closed")
