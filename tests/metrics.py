"""Grids whose metrics pm, pn and the Coriolis parameter f vary along both axes.

Every analytic case has constant pm and pn, except the basin with
curvgrid = 1, and that grid is separable: pm = pm(j), pn = pn(i), f = 1e-4
(oracle_main.c or_ana_grid, host_init.cpp).  On it dm_u == dm_r and dn_v ==
dn_r bit for bit, dm_p equals dm_v and dn_p equals dn_u to an ulp, nothing derived
from pm varies along i and nothing derived from pn along j: one metric array
read in place of another, or one read a column or a row off, changes no
number.  The builders below make planes on which every entry of every metric
array differs from all its neighbours within two cells; apply_grid puts them
into an oracle and a model after init, and tests/test_metrics.py (CPU) and
tests/test_gpu_metrics.py (GPU) run them.  In the style of tests/coasts.py:
made from the CPU oracle alone, with a numpy restatement of setup_grid1
beside.

All arrays are on the (Mm+4, Lm+4) layout, cell (i, j) at [j+1, i+1].  A
grid is {"pm", "pn", "f": multipliers of 1/dx, 1/dy and F0 = 1e-4 1/s,
"per": (ew_periodic, ns_periodic)}.

  waves   smooth oblique waves, two per plane, of wavelengths that are
          irrational numbers of cells (multiples of sqrt 2, sqrt 3, sqrt 5,
          sqrt 7 between 9 and 24): incommensurate with the 4-row tiles, the
          8-row strip chunks, the 16-column blocks, the 60-column strips and
          the 64-column tiles.  pm and pn within +-6 % (the analytic curvgrid
          grid has +-10 %), f within +-30 %
  rough   waves plus per-cell noise from a fixed seed, +-3 % in pm and pn,
          +-5 % in f: neighbouring entries differ (test_metrics.py checks
          all 24 neighbours within two cells for every array)
  signs   rough with f times 2 (x + y - 1) + 0.013, x = (i - 0.5) / Lm,
          y = (j - 0.5) / Mm: f changes sign along the diagonal from the
          north-west to the south-east corner (k_iso forms f(i) + f(i-1),
          k_lmd reads f only squared)
  periodic_rough  rough for a doubly periodic grid: integer wave numbers
          over LLm and MMm, the noise of the interior wrapped into the ghost
          cells
"""
import numpy as np

from test_gpu_parity import PROGNOSTIC, RTOL_ROUTINE, interior, relerr

BASE = ("pm", "pn", "f")
DERIVED = ("fomn", "dm_r", "dn_r", "dm_u", "dn_u", "dm_v", "dn_v", "dm_p", "dn_p", "pmon_u", "pnom_v")
CURV = ("dndx", "dmde")
NAMES = BASE + DERIVED + CURV            # the sixteen
EXCHANGED = tuple(n for n in DERIVED if n != "fomn") + CURV   # setup_grid1's exchanges (oracle_main.c:218-227)
F0 = 1.0e-4
WAVE, NOISE = 0.06, 0.03                  # pm, pn
F_WAVE, F_NOISE = 0.30, 0.05
SEED = 31


# --------------------------------------------------------------- ranges ----
def ranges(Lm, Mm, per=(False, False)):
    """{name: (j0, j1, i0, i1)}: the cells, ends included, that setup_grid1
    computes (oracle_main.c:177-228, host_init.cpp:301-345) before its
    exchanges: R bounds 0 .. Lm+1 between closed or open walls and 1 .. Lm on
    a periodic axis, E bounds 0 .. Lm+1 and -1 .. Lm+2."""
    ewp, nsp = per
    iR0, iR1 = (1, Lm) if ewp else (0, Lm + 1)
    jR0, jR1 = (1, Mm) if nsp else (0, Mm + 1)
    iE0, iE1 = (-1, Lm + 2) if ewp else (0, Lm + 1)
    jE0, jE1 = (-1, Mm + 2) if nsp else (0, Mm + 1)
    rho, u, v, p = (jR0, jR1, iR0, iR1), (jR0, jR1, 1, iR1), (1, jR1, iR0, iR1), (1, jR1, 1, iR1)
    return dict(fomn=(jE0, jE1, iE0, iE1), dm_r=rho, dn_r=rho, dm_u=u, dn_u=u, pmon_u=u, dm_v=v, dn_v=v, pnom_v=v,
                dm_p=p, dn_p=p, dndx=(jR0, jR1, 1, Lm), dmde=(1, Mm, iR0, iR1))


def box(r, dj=0, di=0):
    """Index of the cells r = (j0, j1, i0, i1), shifted by (dj, di)."""
    j0, j1, i0, i1 = r
    return slice(j0 + 1 + dj, j1 + 2 + dj), slice(i0 + 1 + di, i1 + 2 + di)


def wrap(a, per):
    """The periodic exchange of a plane, in place (oracle_step.c exch_lev)."""
    Mm, Lm = a.shape[0] - 4, a.shape[1] - 4
    ewp, nsp = per
    if ewp:
        J = slice(1, Mm + 3)
        a[J, 0:2] = a[J, Lm:Lm + 2]
        a[J, Lm + 2:] = a[J, 2:4]
    if nsp:
        I = slice(1, Lm + 3)
        a[0:2, I] = a[Mm:Mm + 2, I]
        a[Mm + 2:, I] = a[2:4, I]
    if ewp and nsp:
        a[0:2, 0:2], a[0:2, Lm + 2:] = a[Mm:Mm + 2, Lm:Lm + 2], a[Mm:Mm + 2, 2:4]
        a[Mm + 2:, 0:2], a[Mm + 2:, Lm + 2:] = a[2:4, Lm:Lm + 2], a[2:4, 2:4]


def derive_metrics(pm, pn, f, curv, into=None, per=(False, False)):
    """setup_grid1.F's fomn, dm_r, dn_r, dm_u, dn_u, dm_v, dn_v, dm_p, dn_p,
    pmon_u, pnom_v, and dndx, dmde when curv is set, from pm, pn and f, in the
    reference's operation order, over ranges(): {name: plane}.  Every entry
    outside the ranges keeps the value it has in into[name] (0 without
    `into`); on a periodic axis the ghost cells are wrapped as setup_grid1's
    exchanges wrap them."""
    Mm, Lm = pm.shape[0] - 4, pm.shape[1] - 4
    R = ranges(Lm, Mm, per)
    out = {n: np.zeros_like(pm) if into is None else np.array(into[n], dtype=np.float64) for n in DERIVED + CURV}
    b = R["fomn"]
    out["fomn"][box(b)] = f[box(b)] / (pm[box(b)] * pn[box(b)])
    b = R["dm_r"]
    out["dm_r"][box(b)], out["dn_r"][box(b)] = 1.0 / pm[box(b)], 1.0 / pn[box(b)]
    b, w = box(R["dm_u"]), box(R["dm_u"], 0, -1)
    out["pmon_u"][b] = (pm[b] + pm[w]) / (pn[b] + pn[w])
    out["dm_u"][b], out["dn_u"][b] = 2.0 / (pm[b] + pm[w]), 2.0 / (pn[b] + pn[w])
    b, s = box(R["dm_v"]), box(R["dm_v"], -1, 0)
    out["pnom_v"][b] = (pn[b] + pn[s]) / (pm[b] + pm[s])
    out["dm_v"][b], out["dn_v"][b] = 2.0 / (pm[b] + pm[s]), 2.0 / (pn[b] + pn[s])
    b, s, w, sw = (box(R["dm_p"], dj, di) for dj, di in ((0, 0), (-1, 0), (0, -1), (-1, -1)))
    out["dm_p"][b] = 4.0 / (pm[b] + pm[s] + pm[w] + pm[sw])
    out["dn_p"][b] = 4.0 / (pn[b] + pn[s] + pn[w] + pn[sw])
    if curv:
        r = R["dndx"]
        out["dndx"][box(r)] = 0.5 / pn[box(r, 0, 1)] - 0.5 / pn[box(r, 0, -1)]
        r = R["dmde"]
        out["dmde"][box(r)] = 0.5 / pm[box(r, 1, 0)] - 0.5 / pm[box(r, -1, 0)]
    for n in EXCHANGED:
        if curv or n not in CURV:
            wrap(out[n], per)
    return out


# ------------------------------------------------------------- builders ----
def _ij(Lm, Mm):
    return np.arange(-1.0, Lm + 3)[None, :], np.arange(-1.0, Mm + 3)[:, None]


def _wave(i, j, li, lj, phase):
    """A plane wave of li cells along xi and lj along eta (a negative one runs the other way)."""
    return np.sin(2.0 * np.pi * (i / li + j / lj) + phase)


def waves(Lm, Mm):
    i, j = _ij(Lm, Mm)
    r2, r3, r5, r7 = np.sqrt(2.0), np.sqrt(3.0), np.sqrt(5.0), np.sqrt(7.0)
    return {"pm": 1.0 + WAVE * (0.6 * _wave(i, j, 9 * r2, 7 * r3, 0.3) + 0.4 * _wave(i, j, -10 * r5, 4 * r7, 1.1)),
            "pn": 1.0 + WAVE * (0.6 * _wave(i, j, 8 * r3, -6 * r5, 2.0) + 0.4 * _wave(i, j, 7 * r7, 9 * r2, 0.7)),
            "f": 1.0 + F_WAVE * (0.6 * _wave(i, j, 11 * r2, 5 * r5, 1.7) + 0.4 * _wave(i, j, -6 * r7, 8 * r3, 0.2)),
            "per": (False, False)}


def _noise(Lm, Mm):
    return 2.0 * np.random.default_rng(SEED).random((3, Mm + 4, Lm + 4)) - 1.0


def rough(Lm, Mm):
    g, z = waves(Lm, Mm), _noise(Lm, Mm)
    for q, (n, amp) in enumerate((("pm", NOISE), ("pn", NOISE), ("f", F_NOISE))):
        g[n] = g[n] + amp * z[q]
    return g


def signs(Lm, Mm):
    g = rough(Lm, Mm)
    i, j = _ij(Lm, Mm)
    g["f"] = g["f"] * (2.0 * ((i - 0.5) / Lm + (j - 0.5) / Mm - 1.0) + 0.013)
    return g


def periodic_rough(Lm, Mm):
    i, j = _ij(Lm, Mm)
    z = _noise(Lm, Mm)
    w = lambda a, b, phase: np.sin(2.0 * np.pi * (a * i / Lm + b * j / Mm) + phase)
    g = {"pm": 1.0 + WAVE * (0.6 * w(3, 2, 0.3) + 0.4 * w(-2, 5, 1.1)) + NOISE * z[0],
         "pn": 1.0 + WAVE * (0.6 * w(2, -3, 2.0) + 0.4 * w(5, 1, 0.7)) + NOISE * z[1],
         "f": 1.0 + F_WAVE * (0.6 * w(1, 2, 1.7) + 0.4 * w(-4, 3, 0.2)) + F_NOISE * z[2], "per": (True, True)}
    for n in BASE:
        wrap(g[n], (True, True))     # every ghost cell: the strips, then the 2 x 2 corners
    return g


GRIDS = {"waves": waves, "rough": rough, "signs": signs, "periodic_rough": periodic_rough}


# ------------------------------------------------------------- applying ----
def grid_planes(o, grid):
    """The sixteen planes of `grid` on the oracle's grid: pm, pn and f whole
    (ana_grid sets every cell), the rest restated from them over setup_grid1's
    ranges on top of the oracle's own arrays (copies)."""
    cfg = o.cfg
    assert grid["per"] == (bool(cfg.ew_periodic), bool(cfg.ns_periodic))
    pm = grid["pm"] * (1.0 / (cfg.sizex / cfg.LLm))
    pn = grid["pn"] * (1.0 / (cfg.sizey / cfg.MMm))
    f = grid["f"] * F0
    assert pm.shape == o.field("pm")[0].shape
    planes = derive_metrics(pm, pn, f, bool(cfg.curvgrid), {n: o.field(n)[0] for n in DERIVED + CURV}, grid["per"])
    planes.update(pm=pm, pn=pn, f=f)
    return planes


def put_grid(m, planes):
    """Model side of apply_grid: this rank's window of the global planes (the
    whole of them on a single domain), then the rest-state sequence."""
    win = (slice(m.jSW, m.jSW + m.Mm + 4), slice(m.iSW, m.iSW + m.Lm + 4))
    for n in NAMES:
        m.put(n, planes[n][win])
    m.init_sequence()


def apply_grid(o, m, grid):
    """Put the grid into the oracle o and the model m (None: the oracle
    alone) after init and before any step, then the rest-state sequence of
    main.F:244-288 on both sides.  Asserts that both sides agree at step 0
    over PROGNOSTIC, rho and the sixteen arrays; returns the planes."""
    cfg = o.cfg
    planes = grid_planes(o, grid)
    for n in NAMES:
        o.field(n)[0][...] = planes[n]
    for routine in ("set_depth", "set_HUV", "omega"):
        o.call(routine)
    o.call("rho_eos", o.tindex()[4])
    if m is not None:
        put_grid(m, planes)
        m.sync()
        bad = []
        we = float(np.abs(interior(o.field("We"), cfg.LLm, cfg.MMm)).max())
        for n in PROGNOSTIC + ["rho"] + list(NAMES):
            a, b = interior(m.get(n), cfg.LLm, cfg.MMm), interior(o.field(n), cfg.LLm, cfg.MMm)
            # Wi to We's maximum, as the sweeps' routine_errors: at rest it is cancellation noise of We
            e = float(np.abs(a - b).max()) / max(we, 1e-300) if n == "Wi" else relerr(a, b)
            if not e <= RTOL_ROUTINE:
                bad.append((n, e))
        assert not bad, ("step 0", bad)
    return planes


def neighbours_differ(a, r):
    """The number of pairs of equal entries of plane a within two cells of
    each other (the 24 neighbours), both inside the cells r = (j0, j1, i0, i1)."""
    w = a[box(r)]
    nj, ni = w.shape
    same = 0
    for dj in range(-2, 3):
        for di in range(-2, 3):
            if (dj, di) > (0, 0):      # each unordered pair once
                x = w[max(dj, 0):nj + min(dj, 0), max(di, 0):ni + min(di, 0)]
                y = w[max(-dj, 0):nj + min(-dj, 0), max(-di, 0):ni + min(-di, 0)]
                same += int((x == y).sum())
    return same


# ------------------------------------------------------------ whole runs ----
KPP_SIZES = ((121, 12, 12), (65, 8, 12), (49, 12, 12), (48, 11, 12), (112, 12, 12), (61, 6, 100))   # test_gpu_coasts.SIZES
RUNS = {"closed-%dx%dx%d" % s: dict(kind="kpp", size=s) for s in KPP_SIZES}
RUNS.update({
    "curv-121x12x12": dict(kind="kpp", size=(121, 12, 12), curv=1),
    "curv-61x6x100": dict(kind="kpp", size=(61, 6, 100), curv=1),
    "open-121x12x12": dict(kind="kpp", size=(121, 12, 12), obc=15),
    "open-65x8x12": dict(kind="kpp", size=(65, 8, 12), obc=15),
    "random-121x12x12": dict(kind="kpp", size=(121, 12, 12), coast="random"),
    "filament-40x30x12": dict(kind="filament", size=(40, 30, 12), grid="periodic_rough"),
    "c4-bulk-48x40x20": dict(kind="c4", size=(48, 40, 20)),
    "iso-signs-121x12x12": dict(kind="kpp", size=(121, 12, 12), grid="signs", iso=1),
    "ddmix-signs-121x12x12": dict(kind="kpp", size=(121, 12, 12), grid="signs", ddmix=1),
    "river-65x9x6": dict(kind="river", size=(65, 9, 6)),
})
RUN_STEPS = 12
FILAMENT_U = 0.05     # [m/s]


def run_cfg(spec):
    """The configuration of a whole-run case: "kpp" the closed basin with KPP
    and surface fluxes on 2 km cells (test_gpu_coasts.coast_cfg: obc = 15 with
    sponge bands of 1e3 m2/s; iso: ADV_ISONEUTRAL; ddmix: LMD_ICELAND +
    LMD_DDMIX), "filament" test_gpu_multirank's periodic case, "c4" the
    Iceland switch set with BULK_FRC (test_gpu_configs.c4_cfg) on 15 km
    cells, "river" the river sweep's basin (test_rivers.sweep_cfg)."""
    import oracle
    from branch_states import kpp_cfg
    Lm, Mm, N = spec["size"]
    if spec["kind"] == "filament":
        return oracle.filament_cfg(LLm=Lm, MMm=Mm, N=N, sizex=8.0e3, sizey=1.5e3, np_xi=1, np_eta=1)
    if spec["kind"] == "c4":
        from test_gpu_configs import c4_cfg
        cfg = c4_cfg(L=Lm)
        cfg.MMm, cfg.sizey = Mm, 15.0e3 * Mm
        return cfg
    if spec["kind"] == "river":
        from test_rivers import sweep_cfg
        return sweep_cfg(Lm, Mm, N)
    cfg = kpp_cfg(Lm, Mm, N)
    cfg.curvgrid, cfg.adv_isoneutral = spec.get("curv", 0), spec.get("iso", 0)
    if spec.get("obc"):
        cfg.obc, cfg.ubind, cfg.v_sponge = spec["obc"], 0.1, 1.0e3
    if spec.get("ddmix"):
        cfg.lmd = oracle.LMD_ICELAND | oracle.LMD_DDMIX
    return cfg


def start_run(name, model=None):
    """The oracle of whole-run case `name` after init with the case's grid
    in (rough unless the case names another), and the model model(cfg, spec)
    with the same (None: the oracle alone): (cfg, o, m, rmask).  A "kpp" case
    gets coasts.VISC on top of its mixing coefficients, so that visc3d and
    t3dmix, the only readers of dm_p, dn_p, dm_r, dn_r, pmon_u and pnom_v in a
    step, are live, and the coast it names; ddmix re-stratifies T and S first
    (test_ddmix.restratify: both LMD_DDMIX branches); the filament, whose own
    flow is along eta (u = 0 at the start and 5e-4 m/s after 12 steps, on any
    grid), gets a depth-uniform periodic wave of FILAMENT_U in u and ubar, so
    that it meets the liveness bound the runs hold on u; the river case gets
    rivers.speck_mouths, faces on u and on v points.  Every helper asserts
    agreement of both sides at step 0."""
    import coasts
    import oracle
    spec = RUNS[name]
    cfg = run_cfg(spec)
    Lm, Mm = cfg.LLm, cfg.MMm
    o = oracle.Oracle(cfg)
    o.init()
    m = model(cfg, spec) if model is not None else None
    try:
        if spec.get("ddmix"):
            from test_ddmix import restratify
            restratify(o, cfg)
            if m is not None:
                m.put("t", o.field("t"))
        if spec["kind"] == "filament":
            i, j = _ij(Lm, Mm)
            stir = FILAMENT_U * np.sin(2.0 * np.pi * (2.0 * i / Lm + j / Mm))
            for n in ("u", "ubar"):
                o.field(n)[...] += stir
                if m is not None:
                    m.put(n, o.field(n))
        apply_grid(o, m, GRIDS[spec.get("grid", "rough")](Lm, Mm))
        if spec["kind"] == "kpp":
            land = coasts.COASTS[spec["coast"]](Lm, Mm) if spec.get("coast") else coasts.empty(Lm, Mm)
            coasts.apply_coast(o, m, land, coasts.VISC)
        if spec["kind"] == "river":
            import rivers
            nriv = 3
            land, rfrc, ridx = rivers.speck_mouths(Lm, Mm, nriv)
            _, uf, vf, _ = rivers.apply_rivers(o, m, land, (rfrc, ridx), None, rivers.river_tracers(nriv), coasts.VISC)
            assert (np.abs(uf) > 1e-3).any() and (np.abs(vf) > 1e-3).any()
    except BaseException:
        if m is not None:
            m.close()
        raise
    return cfg, o, m, o.field("rmask")[0].copy()
