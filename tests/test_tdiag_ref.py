"""CPU checks of tests/tdiag_ref.py, the numpy restatement of the tracer budget terms that tests/test_gpu_tdiag.py
holds the kernels to.

The restatement is held here to the CPU oracle's corrector (oracle_step.c, itself pinned to the reference by its
golden logs): with Akt = 0 and Wi = 0 the implicit solve is the identity, so Hz*t_new must be the restatement's
S - dt*pm*pn*(FC(k)-FC(k-1)) with S = t_entry - dt*pm*pn*div(FX, FE) -- which pins FX, FE (edge rule, masks, river
faces) and the spline flux; and the budget identity must close within the bound tests/test_gpu_tdiag.py uses, on the
inputs it uses.  Negative controls: slot nstp in place of nrhs, and the edge rule of diag_t_adv_hc4 as written.

The restatement is also pinned bit for bit to the reference's own step3d_t_iso_tile and the routines of diagnostics.F
it calls, compiled unchanged with -DDIAGNOSTICS and diag_trc = .true. (tests/golden/tdiag_golden.npz, recorded by
tests/golden/tdiag_golden.py): all six terms, the written ranges against a sentinel, and a negative control each for
the slot and for the edge rule.
"""
import numpy as np
import pytest

import branch_states as bs
import oracle
import tdiag_ref
from test_gpu_parity import basin_cfg

CLOSURE_ULPS = 32


def small_basin(LLm=36, MMm=11, N=5, **kw):
    c = basin_cfg(nonlin=True, LLm=LLm, MMm=MMm, N=N, NT=2, sizex=2.0e3 * LLm, sizey=2.0e3 * MMm)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def slot(a, N, itrc, l):
    q = (itrc - 1) * 3 + (l - 1)
    return a[q * N:(q + 1) * N]


def started(cfg):
    o = oracle.Oracle(cfg)
    o.init()
    o.step(3)
    return o


def stirred_filament(LLm=40, MMm=30, N=12):
    """The periodic filament after 3 steps is uniform in eta and symmetric in xi (FlxU is exactly 0 at face 1, every
    eta difference 0), which hides the faces and the terms the periodic case is there for: t, FlxU and FlxV get a
    fixed pseudo-random part, halos wrapped as an exchange would."""
    cfg = oracle.filament_cfg(LLm=LLm, MMm=MMm, N=N, np_xi=1, np_eta=1)
    o = started(cfg)
    rng = np.random.default_rng(11)
    for name, amp in (("t", 0.02), ("FlxU", 20.0), ("FlxV", 20.0)):
        a = o.field(name)
        a += amp * rng.standard_normal(a.shape)
        a[..., :, 0:2] = a[..., :, LLm:LLm + 2]
        a[..., :, LLm + 2:] = a[..., :, 2:4]
        a[..., 0:2, :] = a[..., MMm:MMm + 2, :]
        a[..., MMm + 2:, :] = a[..., 2:4, :]
    return cfg, o


def corrector(cfg, o, no_diffusion=False):
    tix = bs.set_mode(o, "corr")
    if no_diffusion:
        o.field("Akt")[...] = 0.0
        o.field("Wi")[...] = 0.0
    E = {n: o.field(n).copy() for n in ("t", "FlxU", "FlxV", "We", "Hz", "pm", "pn", "umask", "vmask", "rmask", "z_w")}
    o.call("step3d_t")
    return tix, E, o.field("t").copy()


def snapshot(cfg, E, h, te):
    L, M = cfg.LLm, cfg.MMm
    r, c = slice(2, M + 2), slice(2, L + 2)
    FX, FE = h["FX"], h["FE"]
    S = np.zeros_like(te)
    S[:, r, c] = te[:, r, c] - cfg.dt * E["pm"][0][r, c] * E["pn"][0][r, c] * (
        FX[:, r, 3:L + 3] - FX[:, r, c] + FE[:, 3:M + 3, c] - FE[:, r, c])
    return S


def cases():
    yield "basin", small_basin(), False
    yield "island", small_basin(island=1), False
    yield "curvgrid", small_basin(curvgrid=1), False
    yield "kpp", small_basin(lmd=oracle.LMD_ALL, surf_flux=1), False
    yield "narrow", small_basin(LLm=65, MMm=3, N=4), False
    yield "filament", oracle.filament_cfg(LLm=40, MMm=30, N=12, np_xi=1, np_eta=1), True
    yield "stirred filament", None, True


@pytest.mark.parametrize("name,cfg,per", list(cases()), ids=[c[0] for c in cases()])
def test_budget_closes_within_the_gpu_tests_bound(name, cfg, per):
    cfg, o = stirred_filament() if cfg is None else (cfg, started(cfg))
    budget_closes(name, cfg, o, per)


def budget_closes(name, cfg, o, per):
    """The checks of test_budget_closes_within_the_gpu_tests_bound on the oracle o of cfg, three steps in
    (tests/test_metrics.py runs them on grids whose metrics vary along both axes); returns the worst closure in ulp."""
    worst = 0.0
    tix, E, t2 = corrector(cfg, o)
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    pm, pn = E["pm"][0], E["pn"][0]
    water = E["rmask"][0][2:M + 2, 2:L + 2] > 0
    for itrc in range(1, cfg.NT + 1):
        tr, te, tn = slot(E["t"], N, itrc, tix[4]), slot(E["t"], N, itrc, tix[5]), slot(t2, N, itrc, tix[5])
        h = tdiag_ref.horizontal(tr, E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M, (not per,) * 4)
        d = tdiag_ref.terms(tr, E["FlxU"], E["FlxV"], E["We"], E["Hz"], pm, pn, E["umask"][0], E["vmask"][0],
                            snapshot(cfg, E, h, te), tn, cfg.dt, per, per)
        res, scale = tdiag_ref.closure_residual(d, te, tn, E["Hz"], pm, pn, cfg.dt, L, M)
        ulps = (np.abs(res) / np.spacing(scale))[:, water].max()
        print(name, itrc, "closure %.2f ulp" % ulps)
        assert ulps <= CLOSURE_ULPS
        worst = max(worst, float(ulps))
        for k in ("advx", "advy", "advz", "mixz"):
            assert np.abs(d[k]).max() > 0, k
        # the written ranges
        assert not d["advx"][:, :, :2].any() and not d["advx"][:, :, L + 3:].any() and not d["advx"][:, M + 2:].any()
        assert not d["advy"][:, :2].any() and not d["advy"][:, M + 3:].any() and not d["advy"][:, :, L + 2:].any()
        assert not d["advz"][-1].any() and not d["mixz"][:, :, L + 2:].any()
    return worst


def horizontal_and_spline_vs_oracle(cfg, o, per=False, rivers=None):
    tix, E, t2 = corrector(cfg, o, no_diffusion=True)
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    r, c = slice(2, M + 2), slice(2, L + 2)
    worst = 0.0
    for itrc in range(1, cfg.NT + 1):
        tr, te, tn = slot(E["t"], N, itrc, tix[4]), slot(E["t"], N, itrc, tix[5]), slot(t2, N, itrc, tix[5])
        h = tdiag_ref.horizontal(tr, E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M, (not per,) * 4,
                                 rivers, itrc, E["Hz"], E["z_w"])
        S = snapshot(cfg, E, h, te)
        fc = tdiag_ref.spline_flux(tr, E["Hz"], E["We"], L, M)
        dfc = fc.copy()
        dfc[1:] -= fc[:-1]
        want = (S - cfg.dt * E["pm"][0] * E["pn"][0] * dfc)[:, r, c] * E["rmask"][0][r, c]
        got = (E["Hz"] * tn)[:, r, c]
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    return worst, tix, E


# (under KPP the surface and non-local terms enter the solve's right-hand side: the closure covers that case)
@pytest.mark.parametrize("name,cfg,per", [c for c in cases() if c[1] is None or not c[1].lmd],
                         ids=[c[0] for c in cases() if c[1] is None or not c[1].lmd])
def test_fluxes_reproduce_the_oracles_corrector(name, cfg, per):
    cfg, o = stirred_filament() if cfg is None else (cfg, started(cfg))
    e, _, _ = horizontal_and_spline_vs_oracle(cfg, o, per)
    print(name, "Hz*t_new vs S - dt*pm*pn*dFC: %.3e" % e)
    assert e <= 1e-13


def river_oracle():
    import coasts
    import rivers
    from test_rivers import sweep_cfg
    size, nriv = (65, 9, 6), 3
    cfg = sweep_cfg(*size)
    o = oracle.Oracle(cfg)
    o.init()
    land, rfrc, ridx = rivers.speck_mouths(size[0], size[1], nriv)
    trc = rivers.river_tracers(nriv)
    _, uf, vf, vol = rivers.apply_rivers(o, None, land, (rfrc, ridx), None, trc, coasts.VISC)
    o.step(3)
    return cfg, o, (uf, vf, vol, trc)


def test_river_faces_reproduce_the_oracles_corrector():
    cfg, o, riv = river_oracle()
    assert (np.abs(riv[0]) > 1e-3).any() and (np.abs(riv[1]) > 1e-3).any()
    e, _, _ = horizontal_and_spline_vs_oracle(cfg, o, rivers=riv)
    assert e <= 1e-13
    cfg, o, riv = river_oracle()
    dry, _, _ = horizontal_and_spline_vs_oracle(cfg, o, rivers=None)   # negative control: the override matters
    assert dry > 1e-6


def test_negative_control_slot():
    """t(nstp) in place of t(nrhs): another field from the first corrector on."""
    cfg = small_basin()
    o = started(cfg)
    tix, E, _ = corrector(cfg, o)
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    a = tdiag_ref.horizontal(slot(E["t"], N, 1, tix[4]), E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M, (True,) * 4)
    b = tdiag_ref.horizontal(slot(E["t"], N, 1, tix[3]), E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M, (True,) * 4)
    assert tix[3] != tix[4]
    for k in ("advx", "advy", "mixx", "mixy"):
        assert not np.array_equal(a[k], b[k]), k
    # and with it the oracle's corrector is no longer reproduced
    o = started(cfg)
    tix, E, t2 = corrector(cfg, o, no_diffusion=True)
    r, c = slice(2, M + 2), slice(2, L + 2)
    h = tdiag_ref.horizontal(slot(E["t"], N, 1, tix[3]), E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M, (True,) * 4)
    S = snapshot(cfg, E, h, slot(E["t"], N, 1, tix[5]))
    fc = tdiag_ref.spline_flux(slot(E["t"], N, 1, tix[3]), E["Hz"], E["We"], L, M)
    dfc = fc.copy()
    dfc[1:] -= fc[:-1]
    want = (S - cfg.dt * E["pm"][0] * E["pn"][0] * dfc)[:, r, c]
    got = (E["Hz"] * slot(t2, N, 1, tix[5]))[:, r, c]
    assert np.abs(got - want).max() / np.abs(want).max() > 1e-9


def test_negative_control_edge_rule():
    """On a rank whose southern side is physical and whose northern side is a rank boundary, diag_t_adv_hc4 as
    written (:645-646) copies at the north and not at the south; the intended rule is the corrector's own.  With
    all four sides physical (a closed single-rank grid) the two coincide."""
    cfg = small_basin()
    o = started(cfg)
    tix, E, _ = corrector(cfg, o)
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    tr = slot(E["t"], N, 1, tix[4])
    args = (tr, E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M)
    closed_i = tdiag_ref.horizontal(*args, (True,) * 4)
    closed_w = tdiag_ref.horizontal(*args, (True,) * 4, edge_rule="as_written")
    for k in ("advx", "advy", "mixx", "mixy"):
        assert np.array_equal(closed_i[k], closed_w[k]), k
    # the basin's wall rows carry no flux and no difference, which hides the copy: the control takes the stirred
    # filament's fields (flux and gradients everywhere) as a rank with a physical southern and an exchanged northern side
    cfg, o = stirred_filament()
    tix, E, _ = corrector(cfg, o)
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    args = (slot(E["t"], N, 1, tix[4]), E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], L, M)
    south_i = tdiag_ref.horizontal(*args, (True, True, True, False))
    south_w = tdiag_ref.horizontal(*args, (True, True, True, False), edge_rule="as_written")
    assert np.array_equal(south_i["advx"], south_w["advx"])
    assert not np.array_equal(south_i["advy"], south_w["advy"])
    # the copy reaches the first and the last face row only, and the corrector's own flux not at all
    diff = np.argwhere(south_i["advy"] != south_w["advy"])
    assert set(diff[:, 1]) == {2, M + 2}
    assert np.array_equal(south_i["FX"], south_w["FX"])


# ---- the pin to the reference's own corrector (tests/golden/tdiag_golden.py) ----
GOLDEN_TERMS = ("advx", "advy", "advz", "mixx", "mixy", "mixz")   # Tdiag slots 1..6, diagnostics.F:83-88


def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tdiag_golden.npz"))


def restated(g, itrc, slot_rhs=None, edges=(True,) * 4, edge_rule="intended"):
    """The restatement over the recorded inputs, S from its own FX, FE in the corrector's order
    (step3d_t_ISO.F:208-211), t_new the reference's; cropped to Tdiag's (0:nx+1, 0:ny+1)."""
    Lm, Mm, N, NT, nstp, nrhs, nnew = [int(v) for v in g["dims"]]
    dt = float(g["dt"])
    tr = g["t"][itrc - 1, (slot_rhs or nrhs) - 1]
    te, tn = g["t"][itrc - 1, nnew - 1], g["t_out"][itrc - 1, nnew - 1]
    r, c = slice(2, Mm + 2), slice(2, Lm + 2)
    h = tdiag_ref.horizontal(tr, g["FlxU"], g["FlxV"], g["umask"], g["vmask"], Lm, Mm, edges, edge_rule=edge_rule)
    FX, FE = h["FX"], h["FE"]
    S = np.zeros_like(te)
    S[:, r, c] = te[:, r, c] - dt * g["pm"][r, c] * g["pn"][r, c] * (FX[:, r, 3:Lm + 3] - FX[:, r, c]
                                                                    + FE[:, 3:Mm + 3, c] - FE[:, r, c])
    d = tdiag_ref.terms(tr, g["FlxU"], g["FlxV"], g["We"], g["Hz"], g["pm"], g["pn"], g["umask"], g["vmask"], S, tn, dt,
                        False, False, edges=edges, edge_rule=edge_rule)
    return {k: d[k][:, 1:Mm + 3, 1:Lm + 3] for k in GOLDEN_TERMS}


def test_restatement_is_the_references_tdiag_bit_for_bit():
    """Tdiag of the reference's step3d_t_iso_tile with DIAGNOSTICS, diag_trc: 8 x 8 x 4, closed, one land cell,
    NT = 2.  Tdiag went in filled with a sentinel: where the reference wrote, the restatement holds the same bits;
    where it did not, the restatement holds 0; the written ranges are the ones the restatement documents."""
    g = golden()
    Lm, Mm, N, NT = [int(v) for v in g["dims"][:4]]
    sen = float(g["sentinel"])
    assert (Lm, Mm, N, NT) == (8, 8, 4, 2) and (g["rmask"] == 0).sum() == 1
    for itrc in (1, 2):
        d = restated(g, itrc)
        for q, k in enumerate(GOLDEN_TERMS):
            ref = g["Tdiag"][itrc - 1, q]
            written = ref != sen
            want = np.zeros(ref.shape, dtype=bool)
            ni, nj = Lm + (k in ("advx", "mixx")), Mm + (k in ("advy", "mixy"))
            want[:, 1:nj + 1, 1:ni + 1] = True
            assert np.array_equal(written, want), (itrc, k)
            assert np.array_equal(ref[written], d[k][written]), (itrc, k, float(np.abs(ref[written] - d[k][written]).max()))
            assert not d[k][~written].any(), (itrc, k)
            assert np.abs(ref[written]).max() > 0
        assert (g["Tdiag"][itrc - 1, 6] == sen).all()   # the seventh slot is never written


def test_golden_negative_control_slot():
    g = golden()
    nstp = int(g["dims"][4])
    sen = float(g["sentinel"])
    d = restated(g, 1, slot_rhs=nstp)
    for q, k in enumerate(GOLDEN_TERMS):
        ref = g["Tdiag"][0, q]
        w = ref != sen
        assert not np.array_equal(ref[w], d[k][w]), k


def test_golden_negative_control_edge_rule():
    """Without the copies at the physical edges the first and last faces' advx, advy differ from the reference's;
    diag_t_adv_hc4's rule as written coincides with the intended one on this square, closed, single-rank grid."""
    g = golden()
    sen = float(g["sentinel"])
    none = restated(g, 1, edges=(False,) * 4)
    written = restated(g, 1, edge_rule="as_written")
    for q, k in enumerate(GOLDEN_TERMS):
        ref = g["Tdiag"][0, q]
        w = ref != sen
        assert np.array_equal(ref[w], written[k][w]), k
        if k in ("advx", "advy", "mixx", "mixy"):
            assert not np.array_equal(ref[w], none[k][w]), k
            bad = np.argwhere((ref != none[k]) & w)
            ax = 2 if k in ("advx", "mixx") else 1
            assert set(bad[:, ax]) <= {1, 2, 8, 9}, (k, sorted(set(bad[:, ax])))
