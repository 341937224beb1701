"""River sweep: GPU parity with river faces of both directions and signs,
several rivers, and mouths on every tile, strip, block, wall and rank edge.

Every other test that compares rivers with the oracle runs Rivers_ana: one
river, 20 mouths in a straight coast with water to the north only (v faces
of positive sign, one wet neighbour per mouth), dx = dy.  Here the mouths of
tests/rivers.py (its docstring says where they are; tests/test_rivers.py
checks that on the CPU, and that the oracle's u and negative arms conserve
volume and set the face velocity as the v arm that Rivers_ana's golden log
pins) go into the closed split-EOS basin on cells of 2 km by 1.5 km
(dn_u != dm_v) with NT = 2, nriv = 3 (16 once, the oracle's limit) and
riv_vol, riv_trc distinct per river and tracer.  What the cases pin:
  * the dir == 0 arms of k_river_s2d and k_river_uv (k_river.hip:31-38,
    62-65), river_velocity(.., 0, ..) and river_tracer_flux(.., 0, ..)
    (k_common.h:216-238), with dn_u where a swap with dm_v moves a number;
  * lround(flx / 10) and flx - 10 * iriver on negative fractions and on
    river indices up to 16; riv_vol[iriver - 1] and the column-major
    riv_trc[(iriver - 1) + (itrc - 1) * nriv] with nriv > 1;
  * the rx0 / rx1 / re0 / re1 lanes of the staged tracer kernels
    (k_step3d_t.hip:143-170, k_pre_step3d.hip:222-276) and their twins in
    the per-level kernels (k_step3d_t.hip:36, 102; k_pre_step3d.hip:52, 155)
    under every kernel-path setting of test_gpu_tracer_stg, with a face at e
    and e+1 of every edge of coasts.all_edges: riv_uflx[ij + 1] at a tile's
    last column is the next block's face;
  * the ranges: faces at i = 1 and j = 1 (walls), which the fast step and
    the predictor skip (istrU, jstrV) and the corrector and the tracer
    fluxes take; decomposed, the owner-only guards of k_river.hip with a
    mouth on one rank and its face on the next, bitwise against the single
    domain, at the every-fast-step exchange interval rivers switch on
    (k_step2d.hip:961).
Each routine is run a second time with the rivers switched off (nriv = 0):
the result must differ at the faces of every (direction, sign) class, so a
kernel that ignored an arm on both sides could not pass for one that
honours it.  Tolerances are the project's: RTOL_ROUTINE per routine in the
max norm over whole arrays, ghost lines included, RMS_RUN per run, 1e-11 on
the diag norms (test_gpu_rivers), decompositions bitwise.

Found and fixed by it:
  - test_river_decomposition_rank_mouths_bitwise[2-1] (and 1 x 2, 2 x 2,
    3 x 2): rank 0's zeta 6.6e-8, ubar 1.8e-9, u 4.4e-9, t 8.7e-9 off the
    single domain after 4 steps.  k_river_s2d (k_river.hip:36, 44) divides a
    face's flux by zeta(knew) + h of the two cells beside it; for a face in
    a rank's first owned column or row one of them is a halo cell, and
    launch_step2d (k_step2d.hip) ran the hook before zeta(knew) had been
    exchanged, so that cell still held the level's value of four fast steps
    before (the reference forms Dnew one cell beyond its own points,
    step2d_FB.F:538, 549).  With rivers on a decomposed grid zeta(knew) now
    crosses before the hook, ubar and vbar after it.
  - the same test's probe: roms_gpu_halo_exchanges reported the configured
    fast-loop interval (4) while rivers had switched the loop to an exchange
    after every fast step; it reports the interval in force (k_step2d.hip,
    s2d_exchange_interval).
Everything else passed as the library stood: every routine case and both
20-step runs bitwise equal to the oracle but hbls (2.7e-17) under KPP.

What the sweep catches, one change each in a scratch copy of the kernels,
run against this file on the MI355X:
  - dn_u and dm_v swapped in river_velocity (k_common.h:224): fails the six
    momentum routine cases, both runs and the mid-run update (9 of 25);
  - k_river_uv's dir == 0 arm left out (k_river.hip:62-65): the same 9;
  - riv_trc indexed row-major (k_common.h:237): those 9 and all ten tracer
    routine cases (19 of 25);
  - rx1 taken from riv_uflx[ij] (k_step3d_t.hip:143, k_pre_step3d.hip:222):
    all ten tracer routine cases, both runs and the mid-run update (13).

Departures from the plan this was written to, and why:
  * the decompositions run on test_gpu_coasts.RANK_GRID (60 x 24), not on
    36 x 28: coasts.rank_edges keeps its two families of land apart only
    with every cut column at 20 or beyond, and 36 columns cut at 18, or at
    12 and 24;
  * "whose water came in" is read off twin runs with one river 1 PSU
    saltier (rivers.own_water), not off the salinity of one run: the
    basin's 35 is farther from each river's salinity than the rivers are
    from one another, so after 20 steps every receiving cell is nearest the
    saltiest river whichever feeds it;
  * roms_gpu_set_river_frc accepts nriv = 0 (it is how a host switches
    river_source off, and what the sensitivity runs use); the test holds it
    to a run that never had rivers, bitwise, instead of expecting an error.
"""
import numpy as np
import pytest

import coasts
import oracle
import rivers
import romsgpu
import test_gpu_tracer_stg as stg
from test_gpu_coasts import RANK_GRID
from test_gpu_multirank import check_decomposition, run_decomposed
from test_gpu_obc import full
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, check_fields
from test_gpu_tracer_stg import oracle_state  # noqa: F401  (the fixture _routine_under_every_mask takes)
from test_rivers import sweep_cfg

pytestmark = pytest.mark.gpu

NRIV = 3
LMD_OUT = ["Akv", "Akt", "hbls", "hbbl", "ghat"]
SIZES = {
    (121, 12, 6): "all tile edges 48 / 64 / 112, strip edges 60 / 120, every 16-column block edge",
    (24, 37, 5): "tall: the 8-row staged tracer blocks and the 4-row tiles in every residue",
    (65, 9, 6): "one column past a tile",
}
BUILDERS = {"specks": rivers.speck_mouths, "blocks": rivers.block_mouths, "walls": rivers.wall_mouths}
CASES = [("specks", (121, 12, 6)), ("blocks", (121, 12, 6)), ("walls", (121, 12, 6)), ("specks", (24, 37, 5)),
         ("specks", (65, 9, 6))]
ROUTINES = [
    # (id, routine, indices, fast step, outputs, {field: face direction} for the sensitivity)
    ("step2d_iif1", "step2d", "fast", 1, ["zeta", "ubar", "vbar", "DU_avg1", "DV_avg1", "Zt_avg1"], {"ubar": 0, "vbar": 1}),
    ("step2d_iif2", "step2d", "fast", 2, ["zeta", "ubar", "vbar", "DU_avg1", "DV_avg1", "Zt_avg1"], {"ubar": 0, "vbar": 1}),
    ("pre_step3d", "pre_step3d", "pred", 0, ["u", "v", "t"], {"u": 0, "v": 1}),
    ("step3d_uv2", "step3d_uv2", "corr", 0, ["u", "v", "ubar", "vbar", "FlxU", "FlxV"], {"u": 0, "v": 1}),
]


def cid(case):
    return "%s-%dx%dx%d" % ((case[0],) + case[1])


def sweep_model(cfg):
    return romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=True, nonlin_eos=True,
                                   dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd,
                                   surf_flux=bool(cfg.surf_flux), curvgrid=bool(cfg.curvgrid))


def mouths_of(name, size, nriv=NRIV):
    land, rfrc, ridx = BUILDERS[name](size[0], size[1], nriv)
    return land, (rfrc, ridx)


def assert_census(uf, vf, nriv):
    """The arms the case is there for are in it."""
    c = rivers.census(uf, vf, nriv)
    assert all(n > 0 for n in c["class"].values()) and all(c["river"][r] > 0 for r in range(1, nriv + 1)), c
    assert len(c["fraction"]) >= 2, c["fraction"]
    return c


# ------------------------------------------------------- routine parity ----
_STATES = {}


def routine_state(name, size, curv=0):
    """The oracle with the mouths of builder `name` after 3 steps, a copy of
    its state, and the per-routine reference outputs (formed once, shared by
    the parity and the sensitivity of every routine)."""
    key = (name, size, curv)
    if key not in _STATES:
        cfg = sweep_cfg(*size, curv=curv)
        assert cfg.sizex / cfg.LLm != cfg.sizey / cfg.MMm
        o = oracle.Oracle(cfg)
        o.init()
        land, mouths = mouths_of(name, size)
        _, uf, vf, vol = rivers.apply_rivers(o, None, land, mouths, None, rivers.river_tracers(NRIV), coasts.VISC)
        assert_census(uf, vf, NRIV)
        o.step(3)
        for n in ("zeta", "u", "v", "t"):
            assert np.isfinite(o.field(n)).all(), n
        _STATES[key] = dict(cfg=cfg, o=o, uf=uf, vf=vf, vol=vol, trc=rivers.river_tracers(NRIV), tix=o.tindex(),
                            snap={n: o.field(n).copy() for n in romsgpu.FIELDS}, refs={})
    return _STATES[key]


def run_routine(c, m, rid, routine, mode, iif, outs):
    """The routine on the state's copy, oracle (once) and model: {field: whole array} of the model."""
    o = c["o"]
    iic, kstp, knew, nstp = c["tix"][:4]
    for n, a in c["snap"].items():
        o.field(n)[...] = a
        m.put(n, a)
    if mode == "fast":
        kstp, knew = knew, knew % 4 + 1
    nrhs, nnew = (nstp, 3) if mode == "pred" else (3, 3 - nstp)
    o.set_tindex([iic, kstp, knew, nstp, nrhs, nnew])
    m.set_tindex(iic, kstp, knew, nstp, nrhs, nnew, iif=iif or 1, nfast=o.nfast())
    if rid not in c["refs"]:
        if iif:
            o.L.or_set_iif(o.h, iif)
        o.call(routine)
        o.L.or_set_iif(o.h, o.nfast())
        c["refs"][rid] = {f: o.field(f).copy() for f in outs}
    getattr(m, routine)()
    m.sync()
    return {f: m.get(f) for f in outs}


def momentum_case(name, size, curv=0, only=None):
    c = routine_state(name, size, curv)
    cls = rivers.class_masks(c["uf"], c["vf"])
    m = sweep_model(c["cfg"])
    bad, got = [], {}
    try:
        rivers.put_rivers(m, c["vol"], c["trc"], c["uf"], c["vf"])
        todo = [r for r in ROUTINES if only is None or r[0] in only]
        for rid, routine, mode, iif, outs, _ in todo:
            got[rid] = run_routine(c, m, rid, routine, mode, iif, outs)
            for f in outs:
                e = full(got[rid][f], c["refs"][rid][f])
                print("%s %s %s %s %.3e" % (name, size, rid, f, e))
                if not e <= RTOL_ROUTINE:
                    bad.append((rid, f, e))
        m.set_river_frc([], [])       # river_source off: every class of faces must have mattered
        for rid, routine, mode, iif, outs, faces in todo:
            off = run_routine(c, m, rid, routine, mode, iif, outs)
            for f, d in faces.items():
                for s in (-1, 1):
                    at = cls[d, s]
                    assert at.any()
                    if np.array_equal(off[f][..., at], got[rid][f][..., at]):
                        bad.append((rid, f, "rivers off changes nothing at the faces of class", (d, s)))
    finally:
        m.close()
    assert not bad, (name, size, bad)


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_river_momentum_routines(case):
    """step2d at iif = 1 and 2, pre_step3d and step3d_uv2 on one mid-run
    state (3 oracle steps with the rivers on) within RTOL_ROUTINE over whole
    arrays, ghost lines included; then the same calls with nriv = 0 differ
    at the u faces and at the v faces of either sign."""
    momentum_case(*case)


def test_river_momentum_routines_curvgrid():
    """pre_step3d and step3d_uv2 with speck_mouths at 121 x 12 on non-uniform
    metrics (curvgrid = 1): dn_u and dm_v differ from face to face."""
    momentum_case("specks", (121, 12, 6), curv=1, only=("pre_step3d", "step3d_uv2"))


_SETUPS = {}


def tracer_setup(name, size):
    """(tag, on_oracle, on_model) for stg._routine_under_every_mask, and the faces."""
    key = (name, size)
    if key not in _SETUPS:
        land, mouths = mouths_of(name, size)
        box = {}

        def on_oracle(o):
            box["faces"] = rivers.apply_rivers(o, None, land, mouths, None, rivers.river_tracers(NRIV), coasts.VISC)[1:]

        def on_model(m):
            uf, vf, vol = box["faces"]
            rivers.put_rivers(m, vol, rivers.river_tracers(NRIV), uf, vf)

        _SETUPS[key] = (("rivers " + cid((name, size))), on_oracle, on_model), box
    return _SETUPS[key]


@pytest.mark.parametrize("routine", ["pre_step3d", "step3d_t"])
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_river_tracer_routines_every_path(case, routine, oracle_state, monkeypatch):  # noqa: F811
    """pre_step3d's and step3d_t's t under every kernel-path setting of
    test_gpu_tracer_stg (the per-level kernels, the staged walks, Hz formed
    in the walk): bitwise equal among them and within RTOL_ROUTINE of the
    oracle, so each river-carrying kernel of both files sees u and v faces
    of both signs; with nriv = 0 the cells that every class of faces flows
    into hold another t."""
    name, size = case
    setup, box = tracer_setup(name, size)
    cfg = sweep_cfg(*size)
    on = stg._routine_under_every_mask(cfg, size[0], size[1], size[2], routine, oracle_state, monkeypatch, setup=setup)
    uf, vf, _ = box["faces"]
    assert_census(uf, vf, NRIV)
    cfg, tix, nfast, before, _ = oracle_state(cfg, size[0], size[1], size[2], routine, setup)
    m = stg._model(cfg, monkeypatch, None)
    try:
        stg._prepare(m, tix, nfast, before)      # no rivers on this one
        getattr(m, routine)()
        m.sync()
        off = m.get("t")
    finally:
        m.close()
    for (d, s), at in rivers.class_masks(uf, vf).items():
        into = rivers.receiving(at, d, s)
        into[:2] = into[size[1] + 2:] = False
        into[:, :2] = into[:, size[0] + 2:] = False
        assert into.any() and not np.array_equal(off[..., into], on["t"][..., into]), (d, s)


# ------------------------------------------------------------ whole runs ----
def river_run(name, lmd=0, surf_flux=0, steps=20):
    size = (121, 12, 6)
    cfg = sweep_cfg(*size, lmd=lmd, surf_flux=surf_flux)
    o = oracle.Oracle(cfg)
    o.init()
    m = sweep_model(cfg)
    try:
        land, mouths = mouths_of(name, size)
        trc = rivers.river_tracers(NRIV)
        masks, uf, vf, vol = rivers.apply_rivers(o, m, land, mouths, None, trc, coasts.VISC)
        assert_census(uf, vf, NRIV)
        N = cfg.N
        worst = 0.0
        for step in range(steps):
            o.step()
            m.step()
            d, w = m.diag(), o.norms()
            for a, b in zip(d, w):
                worst = max(worst, abs(a - b) / max(abs(b), 1e-300))
                assert abs(a - b) <= 1e-11 * max(abs(b), 1e-300), (step, d, w)
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC + (LMD_OUT if lmd else []), cfg.LLm, cfg.MMm, float("inf"), kind="rms")
        print("%s lmd %d: diag norms within %.3e, worst run rms %.3e" % (name, lmd, worst, max(errs.values())),
              {k: "%.2e" % v for k, v in errs.items()})
        bad = [(n, e) for n, e in errs.items() if not e <= RMS_RUN]
        assert not bad, bad
        nnew = m.t.as_list()[5]
        S = m.get("t")[3 * N + (nnew - 1) * N:3 * N + nnew * N]
    finally:
        m.close()
    fed = rivers.fed_cells(uf, vf, NRIV)
    for r in range(1, NRIV + 1):      # twins: river r alone 1 PSU saltier
        trc_r = trc.copy()
        trc_r[r - 1, 1] += 1.0
        m = sweep_model(cfg)
        try:
            coasts.put_coast(m, masks, coasts.VISC)
            rivers.put_rivers(m, vol, trc_r, uf, vf)
            m.step(steps)
            m.sync()
            own, other = rivers.own_water(m.get("t")[3 * N + (nnew - 1) * N:3 * N + nnew * N] - S, fed, r)
        finally:
            m.close()
        print("river %d 1 PSU saltier: %.3e where it alone flows in, %.3e where another does" % (r, own, other))
        assert own > 1e-3 and other <= 0.25 * own, (r, own, other)


def test_river_run_specks():
    """20 steps with speck_mouths at 121 x 12 x 6: the diag norms of every
    step within 1e-11 relative of the oracle's, the fields within RMS_RUN,
    and a twin run with one river 1 PSU saltier changes the salinity where
    that river alone flows in, and at most a quarter as much where another
    does (rivers.own_water)."""
    river_run("specks")


def test_river_run_blocks_kpp():
    """The same with block_mouths under KPP (LMD_ICELAND) and surface fluxes,
    Akv, Akt, hbls, hbbl, ghat among the fields."""
    river_run("blocks", lmd=oracle.LMD_ICELAND, surf_flux=1)


def test_river_update_in_mid_run_16_rivers():
    """nriv = 16: after 2 steps new riv_vol / riv_trc with the faces kept, 3
    steps; then new faces (block_mouths for speck_mouths, on one land that
    holds both), 3 steps: the fields within RMS_RUN of the oracle given the
    same changes."""
    size, nriv = (121, 12, 6), 16
    cfg = sweep_cfg(*size)
    o = oracle.Oracle(cfg)
    o.init()
    m = sweep_model(cfg)
    try:
        land, specks, blocks = rivers.both_mouths(size[0], size[1], nriv)
        trc = rivers.river_tracers(nriv)
        masks, uf, vf, vol = rivers.apply_rivers(o, m, land, specks, None, trc, coasts.VISC)
        assert_census(uf, vf, nriv)
        o.step(2)
        m.step(2)
        vol2, trc2 = vol[::-1] * 0.75, trc[::-1] + 0.5
        o.set_river(vol2, trc2)
        m.set_river_frc(vol2, trc2)
        o.step(3)
        m.step(3)
        e1 = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms")
        uf3, vf3 = rivers.calc_river_flux(masks["rmask"], *blocks)
        assert_census(uf3, vf3, nriv)
        assert not np.array_equal(uf3, uf)
        vol3 = rivers.river_volumes(o, uf3, vf3, nriv)
        o.set_river_faces(vol3, trc2, uf3, vf3)
        m.set_river_frc(vol3, trc2, uf3, vf3)
        o.step(3)
        m.step(3)
        e2 = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms")
        print("new vol / trc %.3e, new faces %.3e" % (max(e1.values()), max(e2.values())))
    finally:
        m.close()


# -------------------------------------------------------- decomposed runs ----
def rank_case(lmd=False):
    Lm, Mm = RANK_GRID
    return dict(case_id=1, LLm=Lm, MMm=Mm, N=6, NT=2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30,
                sizex=2.0e3 * Lm, sizey=1.5e3 * Mm, lmd=lmd, surf_flux=bool(lmd))


def rank_setup(case, land, mouths):
    """setup(model) for check_decomposition: every rank puts its window of
    the global mask planes (coasts.put_coast) and of the global face planes,
    halo included."""
    cfg = sweep_cfg(case["LLm"], case["MMm"], case["N"], lmd=oracle.LMD_ALL if case["lmd"] else 0,
                    surf_flux=int(case["surf_flux"]))
    o = oracle.Oracle(cfg)
    o.init()
    masks = coasts.coast_masks(o, land)
    uf, vf = rivers.calc_river_flux(masks["rmask"], *mouths)
    assert_census(uf, vf, NRIV)
    vol, trc = rivers.river_volumes(o, uf, vf, NRIV), rivers.river_tracers(NRIV)

    def setup(m):
        coasts.put_coast(m, masks, coasts.VISC)
        rivers.put_rivers(m, vol, trc, uf, vf)
    return setup


def rank_cuts(npx, npe):
    Lm, Mm = RANK_GRID
    return ([romsgpu.rank_extent(Lm, npx, r)[1] for r in range(1, npx)],
            [romsgpu.rank_extent(Mm, npe, r)[1] for r in range(1, npe)])


@pytest.mark.parametrize("npx,npe", [(2, 1), (1, 2), (2, 2), (3, 2)])
def test_river_decomposition_rank_mouths_bitwise(npx, npe):
    """rank_mouths about every cut of the processor grid (a mouth on one
    rank, its face the first u or v point of the next, and the mirror image;
    faces at a rank's istr that is not its istrU), 4 steps: every subdomain
    equals the single domain bitwise; KPP and surface fluxes on at 3 x 2.
    With rivers on the fast loop exchanges after every fast step (K = 1)."""
    Lm, Mm = RANK_GRID
    case = rank_case(lmd=(npx, npe) == (3, 2))
    land, rfrc, ridx = rivers.rank_mouths(Lm, Mm, *rank_cuts(npx, npe), NRIV)
    setup = rank_setup(case, land, (rfrc, ridx))
    check_decomposition(case, npx, npe, nsteps=4, setup=setup)
    if (npx, npe) == (2, 2):
        parts, _ = run_decomposed(case, npx, npe, 1, fields=("zeta",), probe=lambda m: m.halo_exchanges(), setup=setup)
        assert {p[5][1] for p in parts} == {1}, [p[5] for p in parts]


def test_river_decomposition_speck_mouths_bitwise():
    Lm, Mm = RANK_GRID
    case = rank_case()
    land, rfrc, ridx = rivers.speck_mouths(Lm, Mm, NRIV)
    check_decomposition(case, 2, 2, nsteps=4, setup=rank_setup(case, land, (rfrc, ridx)))


# -------------------------------------------------------------- ABI edges ----
def test_river_abi_edges():
    """A face whose river index is above nriv and riv_uflx without riv_vflx
    are refused; nriv = 0 after rivers were on switches them off: the next 3
    steps equal a run that never had rivers, bitwise."""
    size = (65, 9, 6)
    cfg = sweep_cfg(*size)
    o = oracle.Oracle(cfg)
    o.init()
    land, mouths = mouths_of("specks", size)
    masks = coasts.coast_masks(o, land)
    uf, vf = rivers.calc_river_flux(masks["rmask"], *mouths)
    vol, trc = rivers.river_volumes(o, uf, vf, NRIV), rivers.river_tracers(NRIV)
    with pytest.raises(ValueError):
        o.set_river_faces(vol[:2], trc[:2], uf, vf)
    out = []
    for had in (True, False):
        m = sweep_model(cfg)
        try:
            coasts.put_coast(m, masks, coasts.VISC)
            if had:
                with pytest.raises(romsgpu.RomsGpuError, match="out of 1..nriv"):
                    m.set_river_frc(vol[:2], trc[:2], uf, vf)
                with pytest.raises(romsgpu.RomsGpuError, match="bad argument"):
                    m.set_river_frc(vol, trc, uf, None)
                m.set_river_frc(vol, trc, uf, vf)
                m.step(1)
                with_rivers = m.get("zeta")
                m.close()
                m = sweep_model(cfg)
                coasts.put_coast(m, masks, coasts.VISC)
                m.set_river_frc(vol, trc, uf, vf)
                m.set_river_frc([], [])
            m.step(3)
            m.sync()
            out.append({n: m.get(n) for n in ("zeta", "ubar", "vbar", "u", "v", "t", "DU_avg1", "DV_avg1")})
        finally:
            m.close()
    assert float(np.abs(with_rivers).max()) > 0.0
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n
