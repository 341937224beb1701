"""The grids of tests/metrics.py, checked on the CPU oracle alone.

tests/test_gpu_metrics.py compares the HIP kernels with the oracle on grids
whose pm, pn and f vary along both axes; here stand the premises of that
comparison: derive_metrics restates the oracle's own setup_grid1 bit for
bit, on `rough` every entry of every metric array differs from its 24
neighbours within two cells, every metric array shifted by one cell in any
of the four directions moves the output of some oracle routine by far more
than RTOL_ROUTINE (so a kernel that reads a metric one cell off, or one
array for another, cannot pass unnoticed), the reference-pinned numpy
restatements of the budget terms agree with the oracle's corrector on such a
grid (so the oracle's momentum and tracer correctors are sound on it), and
the oracle runs every whole-run case finite and with a live flow.
"""
import numpy as np
import pytest

import coasts
import metrics
import oracle
import test_tdiag_ref as ttr
import test_uvdiag_ref as tur
from branch_states import kpp_cfg
from test_gpu_depths import routine_list
from test_gpu_parity import PROGNOSTIC, RTOL_ROUTINE, interior, relerr

POWER = 1.0e3 * RTOL_ROUTINE
STEP2D_OUT = ["zeta", "ubar", "vbar", "DU_avg1", "DV_avg1", "Zt_avg1"]
SHIFTS = {"west": (1, 1), "east": (1, -1), "south": (0, 1), "north": (0, -1)}   # the entry read: (axis, np.roll's shift)


# --------------------------------------------------------- derive_metrics ----
@pytest.mark.parametrize("case", ["basin", "curvgrid", "filament"])
def test_derive_metrics_restates_the_oracle(case):
    """fomn .. pnom_v (and dndx, dmde under curvgrid) from the oracle's pm, pn
    and f equal the oracle's own (oracle_main.c setup_grid1) bit for bit on
    the uniform basin, the curvgrid = 1 basin and the periodic filament.
    Between walls every entry outside metrics.ranges() keeps the value it
    had; on the periodic grid the wrap reaches every ghost cell."""
    if case == "filament":
        cfg = oracle.filament_cfg(LLm=40, MMm=30, N=4, np_xi=1, np_eta=1)
    else:
        cfg = kpp_cfg(37, 22, 4)
        cfg.curvgrid = int(case == "curvgrid")
    per = (bool(cfg.ew_periodic), bool(cfg.ns_periodic))
    o = oracle.Oracle(cfg)
    o.init()
    pm, pn, f = (o.field(n)[0].copy() for n in metrics.BASE)
    names = metrics.DERIVED + (metrics.CURV if cfg.curvgrid else ())
    mine = metrics.derive_metrics(pm, pn, f, bool(cfg.curvgrid), {n: np.full(pm.shape, -7.0) for n in metrics.NAMES}, per)
    R = metrics.ranges(cfg.LLm, cfg.MMm, per)
    for n in names:
        ref, a, r = o.field(n)[0], mine[n], metrics.box(R[n])
        assert np.array_equal(a[r], ref[r]), n
        assert np.abs(ref[r]).max() > 0 or n in metrics.CURV
        if per[0] and per[1]:
            assert np.array_equal(a, ref), n
        else:
            kept = np.ones(a.shape, dtype=bool)
            kept[r] = False
            assert (a[kept] == -7.0).all() and (a[r] != -7.0).all(), n
    if not cfg.curvgrid:
        assert (mine["dndx"] == -7.0).all() and (mine["dmde"] == -7.0).all()
    # on top of the oracle's own arrays the restatement is the oracle's arrays
    again = metrics.derive_metrics(pm, pn, f, bool(cfg.curvgrid), {n: o.field(n)[0] for n in metrics.NAMES}, per)
    for n in metrics.DERIVED + metrics.CURV:
        assert np.array_equal(again[n], o.field(n)[0]), n


def test_the_analytic_curvgrid_grid_is_separable():
    """What the sweep is there for: on the curvgrid = 1 basin dm_u == dm_r and
    dn_v == dn_r bit for bit over their common cells, dm_p is dm_v and dn_p is
    dn_u to an ulp, pm and what derives from it do not vary along i, pn and
    its family not along j, f not at all."""
    cfg = kpp_cfg(37, 22, 4)
    cfg.curvgrid = 1
    o = oracle.Oracle(cfg)
    o.init()
    g = lambda n: o.field(n)[0][2:-2, 2:-2]
    assert np.array_equal(g("dm_u"), g("dm_r")) and np.array_equal(g("dn_v"), g("dn_r"))
    for a, b in (("dm_p", "dm_v"), ("dn_p", "dn_u")):     # four-point means of two values each: equal to an ulp or two
        assert np.abs(g(a) - g(b)).max() <= 2.0 * np.spacing(g(b)).max(), (a, b)
    for n in ("pm", "dm_r", "dm_u", "dm_v", "dm_p", "dmde"):
        assert np.ptp(g(n), axis=1).max() == 0.0 and np.ptp(g(n), axis=0).max() > 0.0, n
    for n in ("pn", "dn_r", "dn_u", "dn_v", "dn_p", "dndx"):
        assert np.ptp(g(n), axis=0).max() == 0.0 and np.ptp(g(n), axis=1).max() > 0.0, n
    assert np.ptp(g("f")) == 0.0


# ------------------------------------------------------------ distinctness ----
def _planes(name, Lm, Mm, curv=1):
    cfg = oracle.filament_cfg(LLm=Lm, MMm=Mm, N=4, np_xi=1, np_eta=1) if name == "periodic_rough" else kpp_cfg(Lm, Mm, 4)
    cfg.curvgrid = curv
    o = oracle.Oracle(cfg)
    o.init()
    return cfg, metrics.grid_planes(o, metrics.GRIDS[name](Lm, Mm))


@pytest.mark.parametrize("name,Lm,Mm", [("rough", 121, 12), ("rough", 61, 6), ("rough", 60, 24), ("signs", 121, 12),
                                        ("periodic_rough", 40, 30)])
def test_every_entry_differs_from_its_neighbours(name, Lm, Mm):
    """On `rough` (and the grids made from it) every entry of each of the
    sixteen arrays differs from each of its 24 neighbours within two cells,
    over the cells setup_grid1 computes: the condition that turns an offset
    error into a changed number.  The amplitudes are the docstring's: pm and
    pn within 9 % of uniform, f within 35 %."""
    cfg, planes = _planes(name, Lm, Mm)
    per = (bool(cfg.ew_periodic), bool(cfg.ns_periodic))
    R = metrics.ranges(Lm, Mm, per)
    whole = (-1, Mm + 2, -1, Lm + 2)
    for n in metrics.NAMES:
        if per[0] and n in metrics.CURV:
            continue                      # the filament has no CURVGRID
        r = (1, Mm, 1, Lm) if per[0] else R.get(n, whole)
        assert metrics.neighbours_differ(planes[n], r) == 0, n
    dx, dy = cfg.sizex / Lm, cfg.sizey / Mm
    assert np.abs(planes["pm"] * dx - 1.0).max() <= metrics.WAVE + metrics.NOISE
    assert np.abs(planes["pn"] * dy - 1.0).max() <= metrics.WAVE + metrics.NOISE
    if name == "signs":
        f = planes["f"][2:-2, 2:-2]
        assert (f > 0).any() and (f < 0).any() and (f[0, 0] < 0) and (f[-1, -1] > 0) and not (f == 0).any()
    else:
        assert np.abs(planes["f"] / metrics.F0 - 1.0).max() <= metrics.F_WAVE + metrics.F_NOISE
    if per[0]:
        for n in metrics.BASE:
            a = planes[n].copy()
            metrics.wrap(a, per)
            assert np.array_equal(a, planes[n]), n


def test_neighbours_differ_counts_pairs():
    a = np.arange(63.0).reshape(7, 9)
    assert metrics.neighbours_differ(a, (-1, 5, -1, 7)) == 0
    a[3, 4] = a[5, 6]
    assert metrics.neighbours_differ(a, (-1, 5, -1, 7)) == 1
    a[3, 4] = a[3, 7]                     # three cells apart: not a neighbour
    assert metrics.neighbours_differ(a, (-1, 5, -1, 7)) == 0


# ------------------------------------------------------------- power table ----
POWER_SIZE = (36, 20, 8)


def _power_state(grid):
    """The oracle of the KPP basin with curvgrid = 1 (every one of the
    sixteen arrays is read), LMD_ICELAND and coasts.VISC, on `grid` (None:
    the analytic curvgrid grid), 3 steps in, with perturbed mixing as
    test_gpu_depths.routine_case; a copy of its state and the routines."""
    import romsgpu
    cfg = kpp_cfg(*POWER_SIZE)
    cfg.curvgrid, cfg.lmd = 1, oracle.LMD_ICELAND
    o = oracle.Oracle(cfg)
    o.init()
    if grid is not None:
        metrics.apply_grid(o, None, metrics.GRIDS[grid](cfg.LLm, cfg.MMm))
    coasts.apply_coast(o, None, coasts.empty(cfg.LLm, cfg.MMm), coasts.VISC)
    o.step(3)
    rng = np.random.default_rng(11)
    for name in ("Akv", "Akt"):
        a = o.field(name)
        a[...] = a * (1.0 + 0.5 * rng.random(a.shape))
    snap = {n: o.field(n).copy() for n in romsgpu.FIELDS}
    return cfg, o, snap, o.tindex(), routine_list(cfg) + [("step2d", "step2d", "fast", STEP2D_OUT)]


def _call(cfg, o, snap, tix, routine, mode, outs):
    iic, kstp, knew, nstp = tix[:4]
    nrhs, nnew = (nstp, 3) if mode is None else (3, 3 - nstp)
    if mode == "fast":                    # as test_gpu_obc.test_open_boundary_routine_parity
        kstp, knew = knew, knew % 4 + 1
        o.L.or_set_iif(o.h, 2)
    o.set_tindex([iic, kstp, knew, nstp, nrhs, nnew])
    if routine in ("rho_eos", "lmd_vmix"):
        o.call(routine, nrhs)
    else:
        o.call(routine)
    return {f: interior(o.field(f), cfg.LLm, cfg.MMm).copy() for f in outs}


def _restore(o, snap):
    for n, a in snap.items():
        o.field(n)[...] = a


def _power_table(grid):
    """{(array, direction): (routine, field, relative change) of the first
    routine that sees the array shifted by one cell that way, or None}."""
    cfg, o, snap, tix, routines = _power_state(grid)
    refs = {}
    for rid, routine, mode, outs in routines:
        _restore(o, snap)
        refs[rid] = _call(cfg, o, snap, tix, routine, mode, outs)
    table = {}
    for n in metrics.NAMES:
        for d, (axis, by) in SHIFTS.items():
            seen = None
            for rid, routine, mode, outs in routines:
                _restore(o, snap)
                o.field(n)[0][...] = np.roll(snap[n][0], by, axis=axis)
                got = _call(cfg, o, snap, tix, routine, mode, outs)
                for f in outs:
                    e = float(relerr(got[f], refs[rid][f]))
                    if e > POWER and (seen is None or e > seen[2]):
                        seen = (rid, f, e)
                if seen:
                    break
            table[n, d] = seen
    return table


def test_every_shifted_metric_moves_a_routine():
    """The power table.  On the mid-run state of `rough` (36 x 20 x 8,
    curvgrid = 1 so that dndx and dmde are read, LMD_ICELAND, coasts.VISC so
    that visc3d and t3dmix are live), each of the sixteen arrays in turn is
    replaced by itself shifted one cell west, east, south or north, and every
    routine of test_gpu_depths.routine_list, then step2d at iif = 2, is
    called: for every (array, direction) some output moves by more than
    1e3 * RTOL_ROUTINE of its maximum.  No array is left out: every one of
    the sixteen is read by some oracle routine (f by lmd_vmix, as f * f).

    The same probe on the analytic curvgrid = 1 grid is printed: it cannot
    see the 28 pairs it lists (pm and its family shifted along xi, pn and its
    family along eta, f at all)."""
    table = _power_table("rough")
    for (n, d), seen in table.items():
        print("rough %-7s %-5s %s" % (n, d, "%s %s %.2e" % seen if seen else "BLIND"))
    blind = [k for k, seen in table.items() if seen is None]
    assert not blind, blind
    analytic = _power_table(None)
    blind = sorted(k for k, seen in analytic.items() if seen is None)
    print("the analytic curvgrid = 1 grid cannot see %d of %d (array, direction) pairs: %s" % (len(blind), len(analytic), blind))
    # pm, dm_r, dm_u, dm_v, dm_p, dmde along xi; pn, dn_r, dn_u, dn_v, dn_p, dndx along eta; the constant f both ways
    want = {(n, d) for n in ("pm", "dm_r", "dm_u", "dm_v", "dm_p", "dmde") for d in ("west", "east")}
    want |= {(n, d) for n in ("pn", "dn_r", "dn_u", "dn_v", "dn_p", "dndx") for d in ("south", "north")}
    want |= {("f", d) for d in SHIFTS}
    assert set(blind) == want, set(blind) ^ want


# ------------------------------------------------- chain to the reference ----
FLAGS = {"plain": {}, "island": dict(island=1), "curvgrid": dict(curvgrid=1)}


def _on_rough(cfg, visc2=0.0):
    o = oracle.Oracle(cfg)
    o.init()
    if visc2:
        o.field("visc2_r")[...] = visc2
        o.field("visc2_p")[...] = visc2
    metrics.apply_grid(o, None, metrics.rough(cfg.LLm, cfg.MMm))
    o.step(3)
    return o


@pytest.mark.parametrize("flags", list(FLAGS))
def test_uvdiag_ref_closes_on_rough(flags):
    """tests/uvdiag_ref.py is pinned bit for bit to the reference's own
    corrector on random metrics (tests/golden/uvdiag_golden.npz); here it
    agrees with the oracle's corrector on `rough`, on the state and within
    the bound of test_uvdiag_ref.test_budget_closes (CLOSURE_ULPS): the
    oracle's prsgrd, step3d_uv1, visc3d and step3d_uv2 are sound on such a
    grid."""
    cfg = tur.small_basin(**FLAGS[flags])
    worst = tur.budget_closes("rough " + flags, cfg, _on_rough(cfg, tur.VISC2))
    print("rough %s: uvdiag_ref vs the oracle's corrector, worst %.2f ulp (bound %d)" % (flags, worst, tur.CLOSURE_ULPS))


@pytest.mark.parametrize("flags", list(FLAGS))
def test_tdiag_ref_closes_on_rough(flags):
    """tests/tdiag_ref.py (pinned to the reference's step3d_t_iso_tile,
    tests/golden/tdiag_golden.npz) against the oracle's corrector on `rough`:
    the budget closes within test_tdiag_ref's CLOSURE_ULPS and, without
    diffusion, Hz * t_new is the restatement's S - dt pm pn dFC within its
    1e-13."""
    cfg = ttr.small_basin(**FLAGS[flags])
    worst = ttr.budget_closes("rough " + flags, cfg, _on_rough(cfg), False)
    e, _, _ = ttr.horizontal_and_spline_vs_oracle(cfg, _on_rough(cfg))
    print("rough %s: tdiag_ref closure %.2f ulp (bound %d), fluxes %.3e (bound 1e-13)" % (flags, worst, ttr.CLOSURE_ULPS, e))
    assert e <= 1e-13


def test_wvlcty_ref_is_pinned_on_metrics_that_vary_both_ways():
    """tests/wvlcty_ref.py has no counterpart in the oracle: it is pinned to
    the reference's wvlcty.F alone (test_wvlcty_ref.py), and the recording's
    pm and pn are pseudo-random planes already, every entry different from
    its neighbours; the GPU case on `rough` leans on that pin directly."""
    from test_wvlcty_ref import G
    Lm, Mm = (int(x) for x in G["dims_closed"][:2])
    for n in ("pm", "pn"):
        assert metrics.neighbours_differ(G[n], (-1, Mm + 2, -1, Lm + 2)) == 0, n


# ------------------------------------------------------------ oracle runs ----
@pytest.mark.parametrize("name", list(metrics.RUNS))
def test_oracle_runs_the_case(name):
    """Each whole-run case of tests/test_gpu_metrics.py, 12 steps of the
    oracle alone: every field finite and max |u| >= 1e-2 m/s (the liveness
    bound of test_gpu_coasts.coast_run).  The amplitudes chosen for which
    this holds are those of metrics.py: waves of 6 % and noise of 3 % in pm
    and pn, 30 % and 5 % in f, on every case alike."""
    cfg, o, _, _ = metrics.start_run(name)
    o.step(metrics.RUN_STEPS)
    for n in PROGNOSTIC:
        assert np.isfinite(o.field(n)).all(), n
    u = np.abs(interior(o.field("u"), cfg.LLm, cfg.MMm)).max()
    print("%s: max|u| %.3f m/s" % (name, u))
    assert u >= 1.0e-2
