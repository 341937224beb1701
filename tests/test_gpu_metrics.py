"""Metric sweep: GPU parity on grids whose pm, pn and f vary along both axes.

Every analytic case has constant pm and pn, except the basin with
curvgrid = 1, and that grid is separable (pm = pm(j), pn = pn(i), f
constant): on it dm_u == dm_r and dn_v == dn_r bit for bit, dm_p is dm_v and
dn_p is dn_u to an ulp, and nothing derived from pm varies along i, nothing
derived from pn along j.  One metric array read for another, or one read a
column or a row off, passes every other test; and the paths that run only
with curvgrid off -- the prsgrd strips (k_prsgrd.hip:383), the fused
prsgrd + uv (:427), the hoisted pre_step3d (k_pre_step3d.hip:514),
uv_horiz_rhs without CURVGRID (k_common.h:623) with their staged windows of
dn_u, dm_v, fomn, pm and pn (k_prsgrd_strip.hip:93, k_tracer_strip.hip:79) --
have only ever seen constant metrics, though the reference reads pm(i, j)
whatever CURVGRID says and a host that registers a real grid uploads metrics
that vary both ways.

Here the grids of tests/metrics.py (its docstring describes them;
tests/test_metrics.py checks on the CPU that they restate setup_grid1, that
on `rough` every entry differs from its 24 neighbours, that every array
shifted one cell any way moves some oracle routine by more than 1e3 *
RTOL_ROUTINE, and that the reference-pinned restatements of the budget terms
agree with the oracle's corrector on it) go into the oracle and the model
after init.  CURVGRID in the configuration only adds the curvature terms:
both settings run on the same planes.  Tolerances are the project's:
RTOL_ROUTINE per routine in the max norm, RMS_RUN per run, decompositions
bitwise.  Every model of the KPP basin asserts the paths it took as
test_gpu_coasts.coast_model does: strips with curvgrid = 0, none with 1.

All cases passed as the library stood: no metric read had to be fixed.
Measured on the MI355X: routines <= 1.3e-16 at N = 12 and <= 8.1e-16 at
N = 100 (the segment solvers' reciprocals); whole runs bitwise equal to the
oracle at N = 12 on every closed, curvilinear, open, coast, ADV_ISONEUTRAL
and river case, 4.7e-15 under LMD_DDMIX, 3.6e-13 and 4.1e-13 at 61 x 6 x 100,
7.1e-12 (Wi) on the C4 set, 1.4e-11 (We) on the filament; both
decompositions and the three diagnostics cases bitwise.

What the sweep catches, one changed read each in a scratch copy of the
kernels (every one an in-bounds read of another array at the same cell, or
of the same array at the lane's own cell), run against this file and against
test_gpu_coasts, test_gpu_widths, test_gpu_obc, test_gpu_open_sides,
test_gpu_parity and test_gpu_depths (547 cases):
  - the hoisted momentum r.h.s. taking fomn(i, j) for fomn(i-1, j)
    (k_pre_step3d.hip:495; runs only with curvgrid off): fails the four
    curvgrid = 0 routine cases here (pre_step3d's u 2e-6 to 3e-6, step3d_uv1's
    u 1e-4 to 8e-4 of the scale) and none of the 547: f does not vary along
    xi in any analytic case.  The whole runs pass: a whole step forms these
    terms in the prsgrd strips.
  - k_visc3d_stg reading dn_u for dn_p (k_step3d_uv.hip:715): fails 23 of
    the 26 cases here (visc3d's u, v 3e-4 to 7e-4; whole runs u from 1e-6;
    the filament has no viscosity and the decompositions compare the library
    with itself) and none of the 547: the two arrays agree to an ulp on
    every analytic grid.
  - the prsgrd strips reading dm_u for dn_u (k_prsgrd_strip.hip:93): fails
    every whole run here that takes the strips (13: t to 3.6e-4 at
    121 x 12 x 12; the curvgrid = 1 runs and the C4 set take none) and no
    routine case (a routine call never takes the strips).  The older sweeps
    see it too wherever dx differs from dy (28 of the 547: the filament
    widths, the depth sweep's runs); on their square cells they do not.
  - k_s2d_fb taking its dn_u from dm_v (k_step2d.hip:403): fails 21 cases
    here (step2d's DU_avg1 to 7e-2) and 32 of the 547 (dx differs from dy,
    or curvgrid = 1).
"""
import numpy as np
import pytest

import coasts
import metrics
import oracle
import romsgpu
from branch_states import kpp_cfg
from test_gpu_coasts import ENV_OFF, band_errors, coast_model, rank_case, sid
from test_gpu_depths import routine_case, routine_errors
from test_gpu_multirank import check_decomposition, run_decomposed
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, check_fields, copy_state, interior, relerr
from test_gpu_widths import environ

pytestmark = pytest.mark.gpu

STEP2D_OUT = ["zeta", "ubar", "vbar", "DU_avg1", "DV_avg1", "Zt_avg1"]


def model_of(cfg, spec=None):
    """A model of cfg.  The KPP basin at a size of test_gpu_coasts.SIZES
    asserts its paths (coast_model); ADV_ISONEUTRAL, which coast_model does
    not pass on, and the other cases take every switch from cfg."""
    if spec is not None and spec["kind"] == "kpp" and not cfg.adv_isoneutral:
        return coast_model(cfg, spec["size"])
    with environ(ENV_OFF):
        return romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                       nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex,
                                       sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux), obc=cfg.obc,
                                       v_sponge=cfg.v_sponge, island=bool(cfg.island), curvgrid=bool(cfg.curvgrid),
                                       bulk_frc=bool(cfg.bulk_frc), adv_isoneutral=bool(cfg.adv_isoneutral))


# ------------------------------------------------------- routine parity ----
def step2d_errors(cfg, m, setup, tag):
    """step2d at iif = 1, 2, 3 on routine_case's state, set up as
    test_gpu_obc.test_open_boundary_routine_parity: {(id, field): error}."""
    cfg, o, snap, tix, _ = routine_case(cfg, setup, tag)
    iic, kstp, knew, nstp = tix[:4]
    errs = {}
    for iif in (1, 2, 3):
        for n, a in snap.items():
            o.field(n)[...] = a
        ix = [iic, knew, knew % 4 + 1, nstp, 3, 3 - nstp]
        o.set_tindex(ix)
        o.L.or_set_iif(o.h, iif)
        copy_state(o, m)
        m.set_tindex(*ix, iif=iif, nfast=o.nfast())
        o.call("step2d")
        m.step2d()
        m.sync()
        for f in STEP2D_OUT:
            errs["step2d_iif%d" % iif, f] = float(relerr(interior(m.get(f), cfg.LLm, cfg.MMm),
                                                         interior(o.field(f), cfg.LLm, cfg.MMm)))
    return errs


@pytest.mark.parametrize("curv", [0, 1], ids=["curv0", "curv1"])
@pytest.mark.parametrize("grid", ["rough", "signs"])
@pytest.mark.parametrize("size", [(121, 12, 12), (61, 6, 100)], ids=sid)
def test_metric_routine_parity(size, grid, curv):
    """Every routine of the depth sweep's routine_list (visc3d and t3dmix
    live under coasts.VISC), then step2d at iif = 1, 2, 3, on one mid-run
    state of the grid -- 3 oracle steps on it, then perturbed Akv, Akt, Wi --
    within RTOL_ROUTINE in the max norm: the tile kernels with their windows
    at 121 x 12 (tile edges 48 / 49, 64 / 65, 112 / 113; strips 60 / 61,
    120 / 121), the segment solvers on 16-column blocks at 61 x 6 x 100.
    Every failing (routine, field, error) is reported at once."""
    cfg = kpp_cfg(*size)
    cfg.curvgrid = curv
    g = metrics.GRIDS[grid](cfg.LLm, cfg.MMm)

    def setup(o):
        metrics.apply_grid(o, None, g)
        coasts.apply_coast(o, None, coasts.empty(cfg.LLm, cfg.MMm), coasts.VISC)

    tag = ("metrics " + grid).encode()
    m = coast_model(cfg, size)
    try:
        errs = routine_errors(cfg, m, setup=setup, tag=tag)
        errs.update(step2d_errors(cfg, m, setup, tag))
    finally:
        m.close()
    name = "%s %s curvgrid %d" % (grid, sid(size), curv)
    for (rid, f), e in errs.items():
        print("%s %s %s %.3e" % (name, rid, f, e))
    print("%s worst routine error %.3e" % (name, max(errs.values())))
    bad = [(rid, f, e) for (rid, f), e in errs.items() if not e <= RTOL_ROUTINE]
    assert not bad, (name, bad)


# ------------------------------------------------------------ whole runs ----
@pytest.mark.parametrize("name", list(metrics.RUNS))
def test_metric_run_rms(name):
    """12 whole steps of every case of metrics.RUNS (graph replay; between
    closed walls with curvgrid off the prsgrd strips, the fused prsgrd + uv,
    the hoisted pre_step3d and the staged tracer windows): field RMS against
    the oracle below RMS_RUN.  The six sizes of test_gpu_coasts.SIZES with
    curvgrid = 0; curvgrid = 1 at 121 x 12 x 12 and 61 x 6 x 100; four open
    edges with sponge bands at 121 x 12 x 12 and 65 x 8 x 12; the random
    coast on top (also over the coast band alone); the periodic filament;
    the C4 switch set with BULK_FRC; ADV_ISONEUTRAL and LMD_DDMIX on `signs`;
    rivers on u and v faces.  tests/test_metrics.py runs each on the oracle
    alone first (finite, max |u| >= 1e-2 m/s, asserted here again)."""
    cfg, o, m, rmask = metrics.start_run(name, model_of)
    try:
        o.step(metrics.RUN_STEPS)
        m.step(metrics.RUN_STEPS)
        m.sync()
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, float("inf"), kind="rms")
        near = {}
        if metrics.RUNS[name].get("coast"):
            band = coasts.coast_band(rmask)
            assert band.sum() >= 30
            near = band_errors(o, m, cfg, band)
    finally:
        m.close()
    print(name, {k: "%.2e" % v for k, v in errs.items()})
    print("%s worst run rms %.3e%s" % (name, max(errs.values()),
                                      ", in the coast band %.3e" % max(near.values()) if near else ""))
    assert float(np.abs(interior(o.field("u"), cfg.LLm, cfg.MMm)).max()) >= 1.0e-2
    bad = [("interior", n, e) for n, e in errs.items() if not e <= RMS_RUN]
    bad += [("band", n, e) for n, e in near.items() if not e <= RMS_RUN]
    assert not bad, (name, bad)


# -------------------------------------------------------- decomposed runs ----
RANK_GRID = (60, 24)   # 2 x 2: ranks of 30 x 12; 3 x 2: 20 x 12 -- all at least 2K + 2 = 10 wide


@pytest.mark.parametrize("npx,npe", [(2, 2), (3, 2)])
def test_metric_decomposition_bitwise(npx, npe):
    """The closed KPP basin on 60 x 24 with `rough`: every rank puts its
    window of the global planes (metrics.put_grid) and the viscosity.  At the
    default exchange interval (K = 4, asserted) the fast steps run on
    subdomains widened into the halo, and the wide exchange before a step's
    first fast step carries h, pm, pn, dn_u and dm_v (k_step2d.hip:978-980):
    every subdomain equals the single domain bitwise, so the widened fast
    step reads no other metric beyond the two-cell halo."""
    Lm, Mm = RANK_GRID
    assert min(romsgpu.rank_extent(Lm, npx, r)[0] for r in range(npx)) >= 10
    assert min(romsgpu.rank_extent(Mm, npe, r)[0] for r in range(npe)) >= 10
    case = rank_case()
    o = oracle.Oracle(kpp_cfg(Lm, Mm, case["N"]))
    o.init()
    planes = metrics.grid_planes(o, metrics.rough(Lm, Mm))
    masks = coasts.coast_masks(o, coasts.empty(Lm, Mm))

    def setup(m):
        metrics.put_grid(m, planes)
        coasts.put_coast(m, masks, coasts.VISC)

    check_decomposition(case, npx, npe, setup=setup)
    parts, _ = run_decomposed(case, npx, npe, 1, fields=("zeta",), probe=lambda m: m.halo_exchanges(), setup=setup)
    assert {p[5][1] for p in parts} == {4}, [p[5] for p in parts]
