"""Hz, z_r, z_w formed inside the kernels (ROMS_GPU_VGRID, the default)
against the streamed arrays (ROMS_GPU_VGRID=0): bitwise equal fields.

k_set_depth keeps the free surface it used (z_sd); k_rho_eos_split,
k_kpp_ext, k_set_huv and (opt-in, ROMS_GPU_VGRID=15) k_kpp_int form a column's
levels from z_sd, h, hinv and the Cs tables with set_depth's own expressions
(VGrid, roms_dev.h) while the stored arrays are set_depth's own.  Every
comparison runs the default mask, every kernel (15) and the streaming forms
(0).  Covered here, always on states with a non-zero free surface:
  * stored == recomputed (Model.vgrid_mismatch) after init and after whole
    steps, on closed and on doubly periodic grids (the wrap must carry z_sd);
  * routine level, on vs off bitwise and both within RTOL_ROUTINE of the
    oracle: rho_eos then lmd_vmix at both time indices, set_HUV; at the depths
    that switch a path (N = 2; 3 and 5 around the 4-level rho_eos ring; 17 /
    18 around the 16-level scan batches; 100) and at widths 40 and 70.
    prsgrd's P, which rho_eos also forms, has no field id: the whole-step
    cases cover it through ru, rv and everything after them;
  * whole steps, every field of romsgpu.FIELDS;
  * 2 x 2 subdomains;
  * validity: a host-written Hz turns the in-kernel grid off until the next
    set_depth.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_lmd import LMD_OUT, lmd_basin_cfg
from test_gpu_lmd_lean import _restore, _snapshot, _tindex
from test_gpu_multirank import _case, run_decomposed
from test_gpu_parity import RTOL_ROUTINE, interior, relerr

pytestmark = pytest.mark.gpu

ALL, DEFAULT = 15, 11   # kVgAll, kVgDefault (roms_dev.h): k_kpp_int's form (bit 4) is opt-in
VARIANTS = (None, ALL, 0)   # the default mask, every kernel, the streaming forms
RHO_OUT = ["rho1", "qp1", "bvf", "rhoA", "rhoS"]
HUV_OUT = ["FlxU", "FlxV", "Hz_u", "Hz_v"]


def _cfg(case, N=None, LLm=40):
    if case == "pipes":
        return oracle.pipes_cfg(np_xi=1, np_eta=1)
    if case == "filament":   # doubly periodic
        return oracle.filament_cfg(LLm=32, MMm=16, N=10, np_xi=1, np_eta=1)
    return lmd_basin_cfg(surf_flux=1, LLm=LLm, MMm=32, N=N)


def _model(cfg, monkeypatch, vgrid=None):
    """A model of cfg under ROMS_GPU_VGRID=vgrid (None: unset, the default)."""
    if vgrid is None:
        monkeypatch.delenv("ROMS_GPU_VGRID", raising=False)
    else:
        monkeypatch.setenv("ROMS_GPU_VGRID", str(vgrid))
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")   # whole steps keep Hz_u, Hz_v readable
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    assert m.vgrid() == (DEFAULT if vgrid is None else vgrid, True)   # init ran set_depth
    return m


# ---- 1. stored equals recomputed ----
@pytest.mark.parametrize("case,N", [("basin", 2), ("basin", 5), ("basin", 100), ("filament", 10)])
def test_stored_grid_equals_recomputed(case, N, monkeypatch):
    cfg = _cfg(case, N)
    m = _model(cfg, monkeypatch)
    assert m.vgrid_mismatch() == (0, 0, 0)
    m.step(3)
    m.sync()
    assert np.max(np.abs(m.get("zeta"))) > 0.0
    assert m.vgrid_mismatch() == (0, 0, 0)
    assert m.vgrid() == (DEFAULT, True)
    m.close()


# ---- 2. routine level ----
def _routines(o, state, tix, tind, cfg, monkeypatch, huv):
    outs = []
    for vgrid in VARIANTS:
        m = _model(cfg, monkeypatch, vgrid)
        for n, a in state.items():
            m.put(n, a)
        m.set_tindex(*tix, nfast=o.nfast())
        assert m.vgrid()[1] is False   # the host wrote Hz
        m.set_depth()
        assert m.vgrid()[1] is True
        assert m.vgrid_mismatch() == (0, 0, 0)
        m.rho_eos(tind)
        m.lmd_vmix(tind)
        if huv:
            m.set_HUV()
        m.sync()
        outs.append({n: m.get(n) for n in RHO_OUT + LMD_OUT + (HUV_OUT if huv else [])})
        m.close()
    return outs


@pytest.mark.parametrize("N,LLm", [(2, 40), (3, 40), (5, 40), (17, 40), (18, 40), (100, 40), (5, 70), (18, 70)])
def test_routines_on_equals_off_bitwise(N, LLm, monkeypatch):
    cfg = _cfg("basin", N, LLm)
    o = oracle.Oracle(cfg)
    o.init()
    o.step(4)
    state = _snapshot(o)
    assert np.max(np.abs(state["zeta"])) > 0.0
    for which in ("nstp", "nrhs"):
        _restore(o, state)
        tix, tind = _tindex(o, which)
        o.set_tindex(tix)
        huv = which == "nstp"
        outs = _routines(o, state, tix, tind, cfg, monkeypatch, huv)
        o.call("set_depth")
        o.L.or_rho_eos(o.h, tind)
        o.L.or_lmd_vmix(o.h, tind)
        names = RHO_OUT + LMD_OUT
        if huv:
            o.call("set_HUV")
            names = names + ["FlxU", "FlxV"]
        bad = []
        for q, out in enumerate(outs):
            for n in names:
                e = relerr(interior(out[n], cfg.LLm, cfg.MMm), interior(o.field(n), cfg.LLm, cfg.MMm))
                print("N=%d LLm=%d %s variant %d %s: relerr %.3e" % (N, LLm, which, q, n, e))
                if not (e <= RTOL_ROUTINE):
                    bad.append((which, q, n, e))
        assert not bad, bad
        for out in outs[1:]:
            for n in outs[0]:
                assert np.array_equal(outs[0][n], out[n]), (which, n)


# ---- 3. whole steps ----
@pytest.mark.parametrize("case,N", [("basin", 20), ("basin", 100), ("pipes", None), ("filament", None)])
def test_whole_steps_bitwise(case, N, monkeypatch):
    cfg = _cfg(case, N)
    outs = []
    for vgrid in VARIANTS:
        m = _model(cfg, monkeypatch, vgrid)
        m.step(3)
        m.sync()
        outs.append({n: m.get(n) for n in romsgpu.FIELDS})
        m.close()
    assert np.max(np.abs(outs[0]["zeta"])) > 0.0
    for out in outs[1:]:
        for n in romsgpu.FIELDS:
            assert np.array_equal(outs[0][n], out[n], equal_nan=True), n


# ---- 4. decomposed ----
def test_decomposed_2x2_bitwise(monkeypatch):
    case = _case("basin_flux")
    fields = ("zeta", "u", "v", "t", "Hz", "z_r", "z_w", "FlxU", "FlxV", "rho1", "qp1", "bvf", "rhoA", "rhoS",
              "Akv", "Akt", "hbls", "hbbl", "ghat")
    runs = []
    for vgrid in VARIANTS:
        if vgrid is None:
            monkeypatch.delenv("ROMS_GPU_VGRID", raising=False)
        else:
            monkeypatch.setenv("ROMS_GPU_VGRID", str(vgrid))
        parts, _ = run_decomposed(case, 2, 2, 3, fields=fields, probe=lambda m: (m.vgrid(), m.vgrid_mismatch()))
        runs.append(parts)
    for rank in range(4):
        on = runs[0][rank]
        assert np.max(np.abs(on[4]["zeta"])) > 0.0
        for vgrid, parts in zip(VARIANTS, runs):
            mask = DEFAULT if vgrid is None else vgrid
            assert parts[rank][5] == ((mask, True), (0, 0, 0)), (rank, vgrid, parts[rank][5])
            for n in fields:
                assert np.array_equal(on[4][n], parts[rank][4][n]), (rank, vgrid, n)


# ---- 5. validity ----
def test_host_written_hz_turns_the_grid_off(monkeypatch):
    cfg = _cfg("basin", 18)
    o = oracle.Oracle(cfg)
    o.init()
    o.step(4)
    state = _snapshot(o)
    tix, tind = _tindex(o, "nstp")
    res = {}
    for vgrid in (None, 0):
        m = _model(cfg, monkeypatch, vgrid)
        for n, a in state.items():
            m.put(n, a)
        m.set_tindex(*tix, nfast=o.nfast())
        m.set_depth()
        m.rho_eos(tind)
        m.sync()
        base = {n: m.get(n) for n in RHO_OUT}
        m.put("Hz", 1.5 * m.get("Hz"))
        assert m.vgrid() == (DEFAULT if vgrid is None else 0, False)
        m.rho_eos(tind)
        m.sync()
        pert = {n: m.get(n) for n in RHO_OUT}
        m.set_depth()
        assert m.vgrid() == (DEFAULT if vgrid is None else 0, True)
        m.rho_eos(tind)
        m.sync()
        again = {n: m.get(n) for n in RHO_OUT}
        m.close()
        res[vgrid] = (base, pert, again)
    for n in RHO_OUT:
        for q in range(3):
            assert np.array_equal(res[None][q][n], res[0][q][n]), (q, n)
        assert np.array_equal(res[None][0][n], res[None][2][n]), n
    # Hz enters rho_eos through the column integrals
    assert not np.array_equal(res[None][0]["rhoS"], res[None][1]["rhoS"])
