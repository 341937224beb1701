"""lmd_vmix without the work past the boundary layers (ROMS_GPU_KPP_LEAN, the
default) against the full forms (ROMS_GPU_KPP_LEAN=0): bitwise equal fields,
both within RTOL_ROUTINE of the oracle.

The lean forms (k_lmd.hip) stop forming Vtsq and loading swr_frac once every
column of a wavefront has its surface layer, keep only FC(0:keep) of the bulk
Richardson integral (in LDS, with a repeated FC sweep for a bottom layer that
reaches higher), and end k_kpp_int's kbls scan at the first level outside the
layer.  Covered here:
  * the depths that switch a path: N = 2 (the smallest column), 17 / 18 and
    33 (N-1 = 16, 32: whole scan batches, and keep = 16 = N-1 and < N-1),
    100 (global column scratch in the full form); Pipes_ana and Rivers_ana;
  * surface layers of very different depth inside one wavefront;
  * the repeated FC sweep, forced with ROMS_GPU_KPP_FCKEEP=1;
  * whole steps.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_lmd import LMD_OUT, lmd_basin_cfg
from test_gpu_parity import RTOL_ROUTINE, interior, relerr

pytestmark = pytest.mark.gpu

KEEP_MAX = 16   # kKppFcKeepMax (roms_dev.h)


def _cfg(case, N=None):
    if case == "pipes":
        return oracle.pipes_cfg(np_xi=1, np_eta=1)
    if case == "rivers":
        return oracle.rivers_cfg(np_xi=1, np_eta=1)
    return lmd_basin_cfg(surf_flux=1, LLm=40, MMm=32, N=N)   # basin_flux of test_gpu_lmd


def _model(cfg, monkeypatch, lean=None, keep=None):
    """A model of cfg (as test_gpu_lmd.make_pair builds it) under the given
    knobs; None leaves a knob unset, i.e. the default."""
    for var, val in (("ROMS_GPU_KPP_LEAN", lean), ("ROMS_GPU_KPP_FCKEEP", keep)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    assert m.kpp_lean() == (7 if lean is None else lean, KEEP_MAX if keep is None else keep)
    return m


def _tindex(o, which):
    iic, kstp, knew, nstp, nrhs, nnew = o.tindex()
    if which == "nstp":
        return [iic, kstp, knew, nstp, nstp, 3], nstp
    return [iic, kstp, knew, nstp, 3, 3 - nstp], 3


def _snapshot(o):
    return {n: o.field(n).copy() for n in romsgpu.FIELDS}


def _restore(o, state):
    for n, a in state.items():
        o.field(n)[...] = a


def _routine_on_models(o, state, tix, tind, cfg, monkeypatch, variants, rho_eos=False):
    """lmd_vmix(tind) (after rho_eos(tind) if asked) from `state` on one model
    per variant (lean, keep); returns the LMD_OUT fields of each."""
    outs = []
    for lean, keep in variants:
        m = _model(cfg, monkeypatch, lean, keep)
        for n, a in state.items():
            m.put(n, a)
        m.set_tindex(*tix, nfast=o.nfast())
        if rho_eos:
            m.rho_eos(tind)
        m.lmd_vmix(tind)
        m.sync()
        outs.append({n: m.get(n) for n in LMD_OUT})
        m.close()
    return outs


def _check(o, outs, cfg, tag):
    """Every variant within RTOL_ROUTINE of the oracle, and bitwise the first."""
    bad = []
    for q, out in enumerate(outs):
        for n in LMD_OUT:
            e = relerr(interior(out[n], cfg.LLm, cfg.MMm), interior(o.field(n), cfg.LLm, cfg.MMm))
            if not (e <= RTOL_ROUTINE):
                bad.append((tag, q, n, e))
    assert not bad, bad
    for out in outs[1:]:
        for n in LMD_OUT:
            assert np.array_equal(outs[0][n], out[n]), (tag, n)


def _levels_in_layer(o, N):
    """Per column, the w levels k = 1..N-1 above the surface layer's base."""
    zw, hbls = o.field("z_w"), o.field("hbls")[0]
    return np.sum(zw[1:N] > zw[N] - hbls, axis=0)


@pytest.mark.parametrize("case,N", [("basin_flux", 2), ("basin_flux", 17), ("basin_flux", 18), ("basin_flux", 33),
                                    ("basin_flux", 100), ("pipes", 10), ("rivers", 10)])
def test_lean_equals_full_bitwise(case, N, monkeypatch):
    cfg = _cfg(case, N)
    assert cfg.N == N
    o = oracle.Oracle(cfg)
    o.init()
    o.step(4)
    state = _snapshot(o)
    for which in ("nstp", "nrhs"):
        _restore(o, state)
        tix, tind = _tindex(o, which)
        o.set_tindex(tix)
        outs = _routine_on_models(o, state, tix, tind, cfg, monkeypatch, [(None, None), (0, None)])
        o.L.or_lmd_vmix(o.h, tind)
        _check(o, outs, cfg, which)


@pytest.mark.parametrize("N", [18, 100])
def test_layer_depths_differ_inside_a_wavefront(N, monkeypatch):
    """Every second group of 8 columns along i gets vertically uniform T and S
    (the surface values, all three time levels): their surface layers reach
    many levels down while their neighbours' in the same wavefront stay thin,
    so lanes find kbls at very different levels of one sweep."""
    cfg = _cfg("basin_flux", N)
    o = oracle.Oracle(cfg)
    o.init()
    o.step(4)
    t = o.field("t")
    nx2 = t.shape[-1]
    cols = (np.arange(nx2) // 8) % 2 == 1
    tv = t.reshape(cfg.NT, 3, N, t.shape[-2], nx2)
    tv[:, :, :, :, cols] = tv[:, :, N - 1:N, :, cols]
    state = _snapshot(o)
    for which in ("nstp", "nrhs"):
        _restore(o, state)
        tix, tind = _tindex(o, which)
        o.set_tindex(tix)
        outs = _routine_on_models(o, state, tix, tind, cfg, monkeypatch, [(None, None), (0, None)], rho_eos=True)
        o.L.or_rho_eos(o.h, tind)
        o.L.or_lmd_vmix(o.h, tind)
        nin = interior(_levels_in_layer(o, N), cfg.LLm, cfg.MMm)
        print("N = %d %s: levels inside hbls %d..%d in the uniform columns, %d..%d in the others"
              % (N, which, nin[:, cols[2:cfg.LLm + 2]].min(), nin[:, cols[2:cfg.LLm + 2]].max(),
                 nin[:, ~cols[2:cfg.LLm + 2]].min(), nin[:, ~cols[2:cfg.LLm + 2]].max()))
        assert np.any(nin <= 3) and np.any(nin >= N / 4.0), (which, int(nin.min()), int(nin.max()))
        _check(o, outs, cfg, which)


def test_fc_fallback_sweep(monkeypatch):
    """Rivers_ana after 16 steps has bottom layers several levels thick: with
    one FC level kept (ROMS_GPU_KPP_FCKEEP=1) their wavefronts repeat the FC
    sweep, and the fields equal the default model's bitwise."""
    cfg = _cfg("rivers")
    N = cfg.N
    o = oracle.Oracle(cfg)
    o.init()
    o.step(16)
    state = _snapshot(o)
    for which in ("nstp", "nrhs"):
        _restore(o, state)
        tix, tind = _tindex(o, which)
        o.set_tindex(tix)
        outs = _routine_on_models(o, state, tix, tind, cfg, monkeypatch, [(None, None), (None, 1), (0, None)])
        o.L.or_lmd_vmix(o.h, tind)
        zw, hbbl, wet = o.field("z_w"), o.field("hbbl")[0], o.field("rmask")[0] > 0.5
        above2 = interior(wet & (zw[0] + hbbl > zw[2]), cfg.LLm, cfg.MMm)
        above3 = interior(wet & (zw[0] + hbbl > zw[3]), cfg.LLm, cfg.MMm)
        print("%s: bottom layer above z_w(2) in %d, above z_w(3) in %d of %d wet columns"
              % (which, above2.sum(), above3.sum(), interior(wet, cfg.LLm, cfg.MMm).sum()))
        assert above2.sum() >= 50, (which, int(above2.sum()))
        _check(o, outs, cfg, which)


@pytest.mark.parametrize("case", ["basin_flux", "pipes"])
def test_whole_steps_bitwise(case, monkeypatch):
    """Three whole steps: the lean model equals the full one in every field,
    ghat included."""
    cfg = _cfg(case, 20)
    outs = []
    for lean in (None, 0):
        m = _model(cfg, monkeypatch, lean)
        m.step(3)
        m.sync()
        outs.append({n: m.get(n) for n in ["u", "v", "t", "zeta"] + LMD_OUT})
        m.close()
    for n in outs[0]:
        assert np.array_equal(outs[0][n], outs[1][n]), n
    if case == "basin_flux":
        assert np.min(outs[0]["ghat"]) < 0.0   # the nonlocal flux is on
