"""CPU checks of tests/uvdiag_ref.py, the numpy restatement of the momentum budget terms that
tests/test_gpu_uvdiag.py holds the kernels to.

The restatement is held here to the CPU oracle's corrector (oracle_step.c, itself pinned to the reference by its
golden logs), stepped routine by routine -- prsgrd, step3d_uv1, visc3d, step3d_uv2 -- with ru, rv and u, v(nnew)
copied between the calls:
  pgr + cor + adv + dis + vmx == (u1 - u_prev)/dt   the five terms of step3d_uv1 are its whole tendency
  u_after_visc == u1 + dt*hmx                       bit for bit: 0.5*dxdyi_u and visc3d's 0.125*(pm+pm)*(pn+pn) differ
                                                    by powers of two only
  Hz_u*u_final == u_prev + dt*(sum of the seven)    the full budget, at water points that are neither river faces
                                                    nor boundary points
Negative controls: u, v(nstp) in place of u, v(nrhs) (adv and cor differ), fourth-order fluxes at the walls (the
first and last points differ), the Hz pair of the wrong neighbour in cpl.

The closure bound: over the four oracle states below the restatement's residual is at most CLOSURE_MEASURED ulp of
the largest of |u_prev| and dt*|term| at the point (printed by the test); CLOSURE_ULPS is the next power of two at
or above four times that, the margin for the u/cff*cff and /dt*dt roundings of another evaluation order.

The restatement is also pinned bit for bit to the reference's own prsgrd, step3d_uv1, visc3d and step3d_uv2 and the
routines of diagnostics.F they call, compiled unchanged with -DDIAGNOSTICS and diag_uv = .true.
(tests/golden/uvdiag_golden.npz, recorded by tests/golden/uvdiag_golden.py): all fourteen terms, the written ranges
against a sentinel, and the three negative controls on the recording as well.
"""
import numpy as np
import pytest

import branch_states as bs
import oracle
import uvdiag_ref as ur
from test_gpu_parity import basin_cfg

CLOSURE_MEASURED = 28.88   # ulp, the largest over the cases of test_budget_closes (v on the stirred filament; 16 on the basin)
CLOSURE_ULPS = 128         # the next power of two at or above 4 * 28.88 = 115.5
VISC2 = 40.0              # m2/s on 2 km cells (tests/coasts.py VISC)

STATIC = ("pm", "pn", "fomn", "dndx", "dmde", "umask", "vmask", "pmask", "dm_r", "dn_r", "dm_p", "dn_p", "dn_u", "dm_v",
          "visc2_r", "visc2_p")


def small_basin(LLm=36, MMm=11, N=5, **kw):
    c = basin_cfg(nonlin=True, LLm=LLm, MMm=MMm, N=N, NT=2, sizex=2.0e3 * LLm, sizey=2.0e3 * MMm)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def started(cfg, visc2=VISC2):
    o = oracle.Oracle(cfg)
    o.init()
    if visc2:
        o.field("visc2_r")[...] = visc2
        o.field("visc2_p")[...] = visc2
    o.step(3)
    return o


def stirred_filament(LLm=40, MMm=30, N=12):
    """The periodic filament after 3 steps is uniform in eta: u, v, FlxU and FlxV get a fixed pseudo-random part,
    halos wrapped as an exchange would, so that every flux of the periodic seams carries a value of its own."""
    cfg = oracle.filament_cfg(LLm=LLm, MMm=MMm, N=N, np_xi=1, np_eta=1)
    o = started(cfg, visc2=5.0)
    rng = np.random.default_rng(12)
    for name, amp in (("u", 0.02), ("v", 0.02), ("rho", 0.01), ("FlxU", 20.0), ("FlxV", 20.0)):
        a = o.field(name)
        a += amp * rng.standard_normal(a.shape)
        a[..., :, 0:2] = a[..., :, LLm:LLm + 2]
        a[..., :, LLm + 2:] = a[..., :, 2:4]
        a[..., 0:2, :] = a[..., MMm:MMm + 2, :]
        a[..., MMm + 2:, :] = a[..., 2:4, :]
    return cfg, o


def slot(a, N, l):
    return a[(l - 1) * N:l * N]


def entry_state(o, cfg, tix):
    """What the restatement reads of the corrector's entry state."""
    N, nstp, nrhs, nnew = cfg.N, tix[3], tix[4], tix[5]
    s = {n: o.field(n)[0].copy() for n in STATIC}
    s.update({n: o.field(n).copy() for n in ("FlxU", "FlxV", "We", "Wi", "Hz", "DU_avg1", "DV_avg1")})
    s["DU_avg1"], s["DV_avg1"] = s["DU_avg1"][0], s["DV_avg1"][0]
    for c in "uv":
        a = o.field(c)
        s[c + "_rhs"], s[c + "_stp"] = slot(a, N, nrhs).copy(), slot(a, N, nstp).copy()
        s[c + "_prev"] = slot(a, N, nnew).copy()
    return s


def stages(call, get, cfg, tix, s):
    """Run prsgrd, step3d_uv1, visc3d, step3d_uv2 through call(name), copying ru, rv and u, v(nnew) between them with
    get(name) into s; returns the u, v(nnew) the last routine leaves."""
    N, nnew = cfg.N, tix[5]
    new = lambda c: slot(get(c), N, nnew).copy()
    call("prsgrd")
    s["ru_pgr"], s["rv_pgr"] = get("ru").copy(), get("rv").copy()
    call("step3d_uv1")
    s["ru_fin"], s["rv_fin"] = get("ru").copy(), get("rv").copy()
    s["u_uv1"], s["v_uv1"] = new("u"), new("v")
    call("visc3d")
    s["u_in2"], s["v_in2"], s["Hz2"] = new("u"), new("v"), get("Hz").copy()
    call("step3d_uv2")
    return new("u"), new("v")


def oracle_sample(cfg, o):
    tix = bs.set_mode(o, "corr")
    s = entry_state(o, cfg, tix)
    fin = stages(o.call, o.field, cfg, tix, s)
    return tix, s, fin


def edges_of(cfg):
    return (not cfg.ew_periodic,) * 2 + (not cfg.ns_periodic,) * 2


def restated(cfg, s, **kw):
    return ur.terms(s, cfg.LLm, cfg.MMm, edges_of(cfg), cfg.dt, uv_cor=bool(cfg.uv_cor),
                    curv=bool(cfg.curvgrid and cfg.uv_adv), **kw)


def cases():
    yield "basin", small_basin()
    yield "island", small_basin(island=1)
    yield "curvgrid", small_basin(curvgrid=1)
    yield "stirred filament", None


def inner(cfg, comp):
    """Water-independent part of the closure's points: the component's range without the rows and columns next to a
    physical edge (u3dbc / v3dbc and the wall values live there)."""
    L, M = cfg.LLm, cfg.MMm
    w, e, s_, n = edges_of(cfg)
    i0, i1 = (3 if w else 1) if comp == "u" else (2 if w else 1), L - 1 if e else L
    j0, j1 = (2 if s_ else 1) if comp == "u" else (3 if s_ else 1), M - 1 if n else M
    return slice(j0 + 1, j1 + 2), slice(i0 + 1, i1 + 2)


@pytest.mark.parametrize("name,cfg", list(cases()), ids=[c[0] for c in cases()])
def test_budget_closes(name, cfg):
    cfg, o = stirred_filament() if cfg is None else (cfg, started(cfg))
    budget_closes(name, cfg, o)


def budget_closes(name, cfg, o):
    """The checks of test_budget_closes on the oracle o of cfg, three steps in (tests/test_metrics.py runs them on
    grids whose metrics vary along both axes); returns the worst of the two ulp figures."""
    worst = 0.0
    tix, s, fin = oracle_sample(cfg, o)
    t = restated(cfg, s)
    for comp, q_fin in zip("uv", fin):
        d, mask = t[comp], s[comp + "mask"]
        r, c = inner(cfg, comp)
        water = mask[r, c] > 0
        # every term is there
        for k in ur.TERMS:
            assert np.abs(d[k]).max() > 0, (comp, k)
        # step3d_uv1's five terms are its tendency
        five = d["pgr"] + d["cor"] + d["adv"] + d["dis"] + d["vmx"]
        tend = (s[comp + "_uv1"] - s[comp + "_prev"]) / cfg.dt
        scale = np.abs(tend)
        for k in ("pgr", "cor", "adv", "dis", "vmx"):
            scale = np.maximum(scale, np.abs(d[k]))
        e5 = (np.abs(five - tend) / np.spacing(scale))[:, r, c][:, water].max()
        # visc3d's update is dt*hmx, bit for bit
        assert np.array_equal((s[comp + "_uv1"] + cfg.dt * d["hmx"])[:, r, c], s[comp + "_in2"][:, r, c]), comp
        res, sc = ur.closure_residual(d, s[comp + "_prev"], q_fin, s["Hz2"], cfg.dt, comp)
        ulps = (np.abs(res) / np.spacing(sc))[:, r, c][:, water].max()
        print("%s %s: five terms vs tendency %.2f ulp of the largest term, closure %.2f ulp" % (name, comp, e5, ulps))
        assert e5 <= CLOSURE_ULPS
        assert ulps <= CLOSURE_ULPS
        worst = max(worst, float(e5), float(ulps))
        # the ranges
        L, M = cfg.LLm, cfg.MMm
        i0 = 3 if edges_of(cfg)[0] else 2
        j0 = 3 if edges_of(cfg)[2] else 2
        for k in ur.TERMS:
            z = d[k].copy()
            if comp == "u":
                z[:, 2:M + 2, i0:L + 2] = 0
            else:
                z[:, j0:M + 2, 2:L + 2] = 0
            assert not z.any(), (comp, k)
    return worst


def test_negative_control_slot():
    """u, v(nstp) in place of u, v(nrhs): adv and cor are other fields from the first corrector on."""
    cfg = small_basin()
    tix, s, _ = oracle_sample(cfg, started(cfg))
    assert tix[3] != tix[4]
    a = restated(cfg, s)
    b = restated(cfg, dict(s, u_rhs=s["u_stp"], v_rhs=s["v_stp"]))
    for comp in "uv":
        for k in ("adv", "cor", "dis"):
            assert not np.array_equal(a[comp][k], b[comp][k]), (comp, k)
        for k in ("pgr", "vmx", "hmx", "cpl"):
            assert np.array_equal(a[comp][k], b[comp][k]), (comp, k)


def test_negative_control_fourth_order_at_the_walls():
    """With the fourth-order form at the walls too, adv differs at the first and last points of each direction and
    nowhere else; on the periodic filament the switch changes nothing."""
    cfg = small_basin()
    _, s, _ = oracle_sample(cfg, started(cfg))
    L, M = cfg.LLm, cfg.MMm
    a, b = restated(cfg, s), restated(cfg, s, order4_at_walls=True)
    for comp in "uv":
        bad = np.argwhere(a[comp]["adv"] != b[comp]["adv"])
        assert len(bad) > 0, comp
        cols, rows = set(bad[:, 2]), set(bad[:, 1])
        edge_cols = {3, L + 1} if comp == "u" else {2, L + 1}     # u: i = 2, Lm; v: i = 1, Lm
        edge_rows = {2, M + 1} if comp == "u" else {3, M + 1}     # u: j = 1, Mm; v: j = 2, Mm
        for kk, jj, ii in bad:
            assert ii in edge_cols or jj in edge_rows, (comp, kk, jj, ii)
        assert cols & edge_cols and rows & edge_rows, (comp, cols, rows)
        assert not np.array_equal(a[comp]["dis"], b[comp]["dis"])
        assert np.array_equal(a[comp]["cor"], b[comp]["cor"])
    cfg, o = stirred_filament()
    _, s, _ = oracle_sample(cfg, o)
    a, b = restated(cfg, s), restated(cfg, s, order4_at_walls=True)
    for comp in "uv":
        assert np.array_equal(a[comp]["adv"], b[comp]["adv"])


def test_negative_control_cpl_neighbour():
    cfg = small_basin()
    _, s, _ = oracle_sample(cfg, started(cfg))
    for comp, dn, avg in (("u", "dn_u", "DU_avg1"), ("v", "dm_v", "DV_avg1")):
        args = (s[comp + "_in2"], s["Hz2"], s[dn], s[avg], s[comp + "mask"], cfg.dt, comp)
        good = ur.clip(ur.cpl(*args), comp, cfg.LLm, cfg.MMm, edges_of(cfg))
        wrong = ur.clip(ur.cpl(*args, neighbour=1), comp, cfg.LLm, cfg.MMm, edges_of(cfg))
        assert not np.array_equal(good, wrong), comp


def test_vertical_orders():
    """N = 3 has no fourth-order vertical face, N = 4 one: FZ4 of k = 2 is the only one that reads four levels."""
    for N, n4 in ((3, 0), (4, 1), (5, 2)):
        q = np.arange(1.0, N + 1)[:, None, None] ** 2 * np.ones((N, 6, 6))
        W = np.ones((N + 1, 6, 6))
        out = ur._vertical(np.zeros_like(q), W, q, np.ones((6, 6)))
        # rebuild FZ from the differences: FZ(k) = -sum_{m<=k} out(m)
        FZ = -np.cumsum(out[:, 0, 0])
        second = [0.25 * (k * k + (k + 1) ** 2) for k in range(1, N)]
        fourth = [ur.INV24 * (-(k - 1) ** 2 + 7 * k * k - (k + 2) ** 2 + 7 * (k + 1) ** 2) for k in range(1, N)]
        want = [second[k - 1] if k in (1, N - 1) else fourth[k - 1] for k in range(1, N)]
        assert np.allclose(FZ[:N - 1], want, rtol=1e-14) and abs(FZ[N - 1]) < 1e-12
        assert sum(1 for k in range(1, N) if k not in (1, N - 1)) == n4


# ---- the pin to the reference's own corrector (tests/golden/uvdiag_golden.py) ----
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvdiag_golden.npz"))


def golden_state(g):
    """The restatement's inputs from the recording: the inputs, ru, rv after prsgrd and after step3d_uv1 (the
    reference's private scratch), u, v(nnew) after step3d_uv1 and after visc3d."""
    Lm, Mm, N, nstp, nrhs, nnew, knew = [int(x) for x in g["dims"]]
    s = {k: g[k] for k in ("FlxU", "FlxV", "We", "Wi", "Hz", "DU_avg1", "DV_avg1", "pm", "pn", "fomn", "umask", "vmask",
                           "pmask", "dm_r", "dn_r", "dm_p", "dn_p", "dn_u", "dm_v", "visc2_r", "visc2_p", "ru_pgr",
                           "rv_pgr", "ru_fin", "rv_fin")}
    s["dndx"] = s["dmde"] = np.zeros_like(g["pm"])   # no CURVGRID in the recording
    for c in "uv":
        s[c + "_rhs"], s[c + "_stp"], s[c + "_prev"] = g[c][nrhs - 1], g[c][nstp - 1], g[c][nnew - 1]
        s[c + "_uv1"], s[c + "_in2"] = g[c + "_uv1"][nnew - 1], g[c + "_visc"][nnew - 1]
    s["Hz2"] = g["Hz"]   # no fast loop between the calls
    return s, (Lm, Mm, N), float(g["dt"])


def golden_terms(g, **kw):
    s, (Lm, Mm, N), dt = golden_state(g)
    over = {k: kw.pop(k) for k in list(kw) if k in s}
    t = ur.terms(dict(s, **over), Lm, Mm, (True,) * 4, dt, **kw)
    return {c: {k: t[c][k][:, 2:Mm + 2, 2:Lm + 2] for k in ur.TERMS} for c in "uv"}   # Udiag's (1:nx, 1:ny)


def kept(ref, sen, comp):
    """Where the reference wrote and wrt_diag_uv does not zero: not the first u column, not the first v row."""
    w = ref != sen
    if comp == "u":
        w[:, :, 0] = False
    else:
        w[:, 0, :] = False
    return w


def test_restatement_is_the_references_udiag_vdiag_bit_for_bit():
    """Udiag, Vdiag of the reference's prsgrd; step3d_uv1(0); visc3d; step3d_uv2(0) with DIAGNOSTICS, diag_uv: 8 x 6 x 4,
    closed, one land cell, UV_COR UV_ADV UV_VIS2.  Both went in filled with a sentinel: where the reference wrote
    (and its writer does not zero), the restatement holds the same bits; elsewhere it holds 0."""
    g = golden()
    Lm, Mm, N = [int(v) for v in g["dims"][:3]]
    sen = float(g["sentinel"])
    assert (Lm, Mm, N) == (8, 6, 4) and (g["rmask"] == 0).sum() == 1 and (g["umask"] == 0).sum() == 2
    t = golden_terms(g)
    for comp, D in (("u", g["Udiag"]), ("v", g["Vdiag"])):
        for q, k in enumerate(ur.TERMS):
            ref, mine = D[q], t[comp][k]
            w = kept(ref, sen, comp)
            # the range: i = 2..Lm (u), j = 2..Mm (v), every level
            want = np.zeros_like(w)
            if comp == "u":
                want[:, :, 1:] = True
            else:
                want[:, 1:, :] = True
            assert np.array_equal(w, want), (comp, k)
            assert np.array_equal(ref[w], mine[w]), (comp, k, float(np.abs(ref[w] - mine[w]).max()))
            assert not mine[~w].any(), (comp, k)
            assert np.abs(ref[w]).max() > 0
    # the reference leaves the first v row of dis, vmx, cpl unwritten (its v block starts at jstrV)
    for q in (3, 5, 6):
        assert (g["Vdiag"][q][:, 0] == sen).all()


def test_golden_negative_controls():
    g = golden()
    sen = float(g["sentinel"])
    s, (Lm, Mm, N), dt = golden_state(g)
    good = golden_terms(g)
    slot = golden_terms(g, u_rhs=s["u_stp"], v_rhs=s["v_stp"])
    walls = golden_terms(g, order4_at_walls=True)
    for comp, D in (("u", g["Udiag"]), ("v", g["Vdiag"])):
        for q, k in enumerate(ur.TERMS):
            w = kept(D[q], sen, comp)
            assert np.array_equal(D[q][w], good[comp][k][w])
            if k in ("adv", "cor", "dis"):
                assert not np.array_equal(D[q][w], slot[comp][k][w]), (comp, k)
        # fourth order at the walls: the first and last points of each direction and no others
        bad = np.argwhere((D[2] != walls[comp]["adv"]) & kept(D[2], sen, comp))
        assert len(bad) > 0
        cols = {1, Lm - 1} if comp == "u" else {0, Lm - 1}
        rows = {0, Mm - 1} if comp == "u" else {1, Mm - 1}
        assert all(ii in cols or jj in rows for _, jj, ii in bad), (comp, bad)
        # cpl with the Hz pair of the wrong neighbour
        dn, avg = ("dn_u", "DU_avg1") if comp == "u" else ("dm_v", "DV_avg1")
        wrong = ur.cpl(s[comp + "_in2"], s["Hz2"], s[dn], s[avg], s[comp + "mask"], dt, comp, neighbour=1)
        wrong = wrong[:, 2:Mm + 2, 2:Lm + 2]
        w = kept(D[6], sen, comp)
        assert not np.array_equal(D[6][w], wrong[w]), comp
