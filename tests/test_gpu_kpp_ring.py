"""k_kpp_ext with a ring of levels in flight (ROMS_GPU_KPP_PF = 2, 3, 4)
against the single level ahead (ROMS_GPU_KPP_PF=1): bitwise equal fields,
all within RTOL_ROUTINE of the oracle.

The descending sweep of k_kpp_ext (k_lmd.hip) loads the inputs of PF levels
ahead of the level it forms: the ring is filled with levels N-1 .. N-PF before
the sweep and refilled with level k-PF at the top of level k, and the swr_frac
load of a level is left out once the wavefront's flag `vdone` is set when the
level's loads go out.  Covered here:
  * columns shorter than, as long as and just longer than the deepest ring
    (N = 2, 3, 4, 5), the depths around the kept FC levels (N = 17, 18, 33),
    N = 100 once, and Pipes_ana for the land mask;
  * each of them with the repeated FC sweep forced (ROMS_GPU_KPP_FCKEEP=1),
    with the full forms (ROMS_GPU_KPP_LEAN=0: the flag never sets, every level
    loads swr_frac; the whole FC column) and with the streamed Hz, z_r, z_w
    (ROMS_GPU_VGRID=0);
  * surface layers of very different depth inside one wavefront, so that the
    flag sets deep in the column for some wavefronts and at the top for others;
  * whole steps, every field of romsgpu.FIELDS;
  * a value outside 1..4 counts as 1.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_lmd import LMD_OUT, lmd_basin_cfg
from test_gpu_parity import RTOL_ROUTINE, interior, relerr

pytestmark = pytest.mark.gpu

PFS = (1, 2, 3, 4)   # 1 .. kKppPfMax (roms_dev.h): every compiled ring
MODES = {"default": {}, "fckeep1": {"ROMS_GPU_KPP_FCKEEP": "1"}, "full": {"ROMS_GPU_KPP_LEAN": "0"},
         "stream": {"ROMS_GPU_VGRID": "0"}}
KNOBS = ("ROMS_GPU_KPP_PF", "ROMS_GPU_KPP_FCKEEP", "ROMS_GPU_KPP_LEAN", "ROMS_GPU_VGRID")


def _cfg(case, N=None):
    if case == "pipes":
        return oracle.pipes_cfg(np_xi=1, np_eta=1)
    return lmd_basin_cfg(surf_flux=1, LLm=40, MMm=32, N=N)


def _model(cfg, monkeypatch, pf, env=None):
    """A model of cfg under ROMS_GPU_KPP_PF=pf (None: unset, the default) and
    the knobs of env; every other knob of KNOBS unset."""
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)
    if pf is not None:
        monkeypatch.setenv("ROMS_GPU_KPP_PF", str(pf))
    for var, val in (env or {}).items():
        monkeypatch.setenv(var, val)
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")   # whole steps keep Hz_u, Hz_v readable
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    if pf is None:
        assert m.kpp_pf() in PFS
    else:
        assert m.kpp_pf() == pf
    return m


def _tindex(o, which):
    iic, kstp, knew, nstp, nrhs, nnew = o.tindex()
    if which == "nstp":
        return [iic, kstp, knew, nstp, nstp, 3], nstp
    return [iic, kstp, knew, nstp, 3, 3 - nstp], 3


_REF = {}


def _reference(case, N, uneven=False):
    """Once per (case, N, uneven): the oracle's state after 4 steps (uneven:
    every second group of 8 columns along i vertically uniform in T and S, as
    test_gpu_lmd_lean builds it) and, for lmd_vmix(nstp) and lmd_vmix(nrhs)
    from that state after set_depth (and rho_eos if uneven), the time indices
    and the interior of every LMD_OUT field.  Shared and never written."""
    key = (case, N, uneven)
    if key not in _REF:
        cfg = _cfg(case, N)
        o = oracle.Oracle(cfg)
        o.init()
        o.step(4)
        info = None
        if uneven:
            t = o.field("t")
            nx2 = t.shape[-1]
            cols = (np.arange(nx2) // 8) % 2 == 1
            tv = t.reshape(cfg.NT, 3, cfg.N, t.shape[-2], nx2)
            tv[:, :, :, :, cols] = tv[:, :, cfg.N - 1:cfg.N, :, cols]
        state = {n: o.field(n).copy() for n in romsgpu.FIELDS}
        runs = []
        for which in ("nstp", "nrhs"):
            for n, a in state.items():
                o.field(n)[...] = a
            tix, tind = _tindex(o, which)
            o.set_tindex(tix)
            o.call("set_depth")
            if uneven:
                o.L.or_rho_eos(o.h, tind)
            o.L.or_lmd_vmix(o.h, tind)
            if uneven:   # w levels k = 1..N-1 above the surface layer's base, per column
                zw, hbls = o.field("z_w"), o.field("hbls")[0]
                nin = interior(np.sum(zw[1:cfg.N] > zw[cfg.N] - hbls, axis=0), cfg.LLm, cfg.MMm)
                info = (int(nin.min()), int(nin.max()))
            runs.append((which, tix, tind, {n: interior(o.field(n), cfg.LLm, cfg.MMm).copy() for n in LMD_OUT}, info))
        _REF[key] = (cfg, state, o.nfast(), runs)
    return _REF[key]


def _ring_check(case, N, mode, monkeypatch, uneven=False):
    """lmd_vmix(nstp) and lmd_vmix(nrhs) from one oracle state on one model per
    ROMS_GPU_KPP_PF: every LMD_OUT field bitwise that of PF = 1 and within
    RTOL_ROUTINE of the oracle."""
    cfg, state, nfast, runs = _reference(case, N, uneven)
    models = [_model(cfg, monkeypatch, pf, MODES[mode]) for pf in PFS]
    try:
        want_vg = mode != "stream"
        for which, tix, tind, ref, info in runs:
            outs = []
            for m in models:
                for n, a in state.items():
                    m.put(n, a)
                m.set_tindex(*tix, nfast=nfast)
                m.set_depth()   # the grid is valid again, so the VGrid instance runs where ROMS_GPU_VGRID has it
                mask, valid = m.vgrid()
                assert valid and bool(mask & 2) is want_vg
                if uneven:
                    m.rho_eos(tind)
                m.lmd_vmix(tind)
                m.sync()
                outs.append({n: m.get(n) for n in LMD_OUT})
            bad = []
            for pf, out in zip(PFS, outs):
                for n in LMD_OUT:
                    e = relerr(interior(out[n], cfg.LLm, cfg.MMm), ref[n])
                    if not (e <= RTOL_ROUTINE):
                        bad.append((which, pf, n, e))
            assert not bad, bad
            for pf, out in zip(PFS[1:], outs[1:]):
                for n in LMD_OUT:
                    assert np.array_equal(outs[0][n], out[n]), (which, pf, n)
    finally:
        for m in models:
            m.close()


# N = 2, 3, 4, 5: the sweep's levels N-1 .. 1 are fewer than, as many as and one more than the deepest ring's 4
# (N = 2, 3, 4: one to three levels, so the rings of 2, 3 and 4 in turn are never refilled); 17 / 18 / 33: the
# kept FC levels (keep = 16 = N-1, < N-1) and whole scan batches; pipes: N = 10 with the land mask
SHAPES = [("basin_flux", 2), ("basin_flux", 3), ("basin_flux", 4), ("basin_flux", 5), ("basin_flux", 17),
          ("basin_flux", 18), ("basin_flux", 33), ("pipes", 10)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case,N", SHAPES)
def test_ring_equals_single_level_bitwise(case, N, mode, monkeypatch):
    assert _cfg(case, N).N == N
    _ring_check(case, N, mode, monkeypatch)


def test_ring_n100(monkeypatch):
    _ring_check("basin_flux", 100, "default", monkeypatch)


@pytest.mark.parametrize("mode", ["default", "stream"])
def test_flag_sets_at_different_levels_inside_a_wavefront(mode, monkeypatch):
    """Vertically uniform T and S in every second group of 8 columns: their
    surface layers reach many levels down while their neighbours' in the same
    wavefront stay thin, so a wavefront's flag sets deep in the column -- with
    levels issued before it set still in the ring -- and elsewhere at the top."""
    N = 33
    cfg, state, nfast, runs = _reference("basin_flux", N, uneven=True)
    for which, tix, tind, ref, (lo, hi) in runs:
        print("N = %d %s: levels inside hbls %d..%d" % (N, which, lo, hi))
        assert lo <= 3 and hi >= N / 4.0, (which, lo, hi)
    _ring_check("basin_flux", N, mode, monkeypatch, uneven=True)


@pytest.mark.parametrize("case", ["basin_flux", "pipes"])
def test_whole_steps_bitwise(case, monkeypatch):
    """Four whole steps: PF = 1 against the default and against the deepest
    ring, every field of romsgpu.FIELDS."""
    cfg = _cfg(case, 20)
    outs = []
    for pf in (1, None, PFS[-1]):
        m = _model(cfg, monkeypatch, pf)
        m.step(4)
        m.sync()
        outs.append({n: m.get(n) for n in romsgpu.FIELDS})
        m.close()
    for out in outs[1:]:
        for n in outs[0]:
            assert np.array_equal(outs[0][n], out[n], equal_nan=True), n


@pytest.mark.parametrize("value", ["0", "5", "-2", "99"])
def test_unsupported_value_counts_as_one(value, monkeypatch):
    cfg = _cfg("basin_flux", 5)
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("ROMS_GPU_KPP_PF", value)
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    try:
        assert m.kpp_pf() == 1
    finally:
        m.close()
