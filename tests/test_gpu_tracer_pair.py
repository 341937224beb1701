"""T and S in one block of the tracer segment solvers (k_pre_tracer_segb_pair,
k_step3d_t_segb_pair; ROMS_GPU_T_PAIR bits 1 and 2, both the default) against
one block per tracer (ROMS_GPU_T_PAIR=0): bitwise equal fields, both within
RTOL_ROUTINE of the oracle.

Without LMD_DDMIX and with equal background values lmd_vmix leaves Akt(isalt)
bit for bit Akt(itemp), so the two tracers' spline and implicit-diffusion
systems are one matrix each with two right-hand sides; the pair forms load and
factorise them once.  They run only while the library knows that equality
(set by lmd_vmix, ended by a host write of Akt).  Covered here:
  * the segment path's depths N = 88, 100, 104 (segments of 11, of 12/13 and
    of 13 rows, the surface row in the last segment) on 40x32 and on 21x9 (a
    last block with inactive lanes, widths that are no multiple of 16);
  * pre_step3d and step3d_t as single routines from an oracle state under
    ROMS_GPU_T_PAIR = 0, 1, 2, 3 and unset, and whole steps (eager first
    step, graph capture and replay, both nstp phases);
  * the path query: the pair forms really ran, and did not where they must not;
  * a host write of Akt ends the pairing until the next lmd_vmix, and the
    host's Akt(isalt) is then what S sees;
  * LMD_DDMIX and unequal backgrounds never pair.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_ddmix import ddmix_cfg
from test_gpu_lmd import lmd_basin_cfg
from test_gpu_parity import RTOL_ROUTINE, interior, relerr
from test_gpu_register import host_model

pytestmark = pytest.mark.gpu

GRIDS = [(40, 32), (21, 9)]
DEPTHS = [88, 100, 104]
SEG_ROWS = {88: (11, 11), 100: (12, 13), 104: (13, 13)}   # fewest, most rows of the 8 segments


def _cfg(LLm, MMm, N):
    return lmd_basin_cfg(surf_flux=1, LLm=LLm, MMm=MMm, N=N)


def _model(cfg, monkeypatch, pair):
    if pair is None:
        monkeypatch.delenv("ROMS_GPU_T_PAIR", raising=False)
    else:
        monkeypatch.setenv("ROMS_GPU_T_PAIR", str(pair))
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    assert m.column_path()[0]   # the segment solvers
    assert m.tracer_pair() == (3 if pair is None else pair, False, (0, 0))
    return m


def _all_fields(m):
    return {n: m.get(n) for n in romsgpu.FIELDS}


def _assert_same(a, b, tag):
    diff = [n for n in a if not np.array_equal(a[n], b[n])]
    assert not diff, (tag, diff)


@pytest.fixture(scope="module")
def oracle_state():
    """Per (LLm, MMm, N, routine): the oracle after 4 steps with the routine's
    indices set (the predictor's for pre_step3d, the corrector's for
    step3d_t), its fields before and after lmd_vmix + the routine (formed
    once, left unchanged)."""
    cache = {}

    def get(LLm, MMm, N, routine):
        key = (LLm, MMm, N, routine)
        if key not in cache:
            cfg = _cfg(LLm, MMm, N)
            o = oracle.Oracle(cfg)
            o.init()
            o.step(4)
            iic, kstp, knew, nstp, nrhs, nnew = o.tindex()
            tix = [iic, kstp, knew, nstp, nstp, 3] if routine == "pre_step3d" else [iic, kstp, knew, nstp, 3, 3 - nstp]
            o.set_tindex(tix)
            before = {n: o.field(n).copy() for n in romsgpu.FIELDS}
            o.L.or_lmd_vmix(o.h, tix[4])
            o.call(routine)
            after = {n: o.field(n).copy() for n in ("t", "Akt")}
            cache[key] = (cfg, tix, o.nfast(), before, after)
        return cache[key]
    return get


def _prepare(m, tix, nfast, before):
    """The oracle's state, then lmd_vmix(nrhs) as the step runs it ahead of the routine."""
    for n, a in before.items():
        m.put(n, a)
    m.set_tindex(*tix, nfast=nfast)
    m.lmd_vmix(tix[4])


@pytest.mark.parametrize("routine,bit", [("pre_step3d", 1), ("step3d_t", 2)])
@pytest.mark.parametrize("N", DEPTHS)
@pytest.mark.parametrize("LLm,MMm", GRIDS)
def test_routine_pair_equals_per_tracer(LLm, MMm, N, routine, bit, oracle_state, monkeypatch):
    cfg, tix, nfast, before, after = oracle_state(LLm, MMm, N, routine)
    assert (N // 8, -(-N // 8)) == SEG_ROWS[N]
    outs = []
    for pair in (0, 1, 2, 3, None):
        m = _model(cfg, monkeypatch, pair)
        _prepare(m, tix, nfast, before)
        mask, same, n0 = m.tracer_pair()
        assert same and n0 == (0, 0)
        getattr(m, routine)()
        m.sync()
        ran = 1 if mask & bit else 0   # the pair form ran, or did not
        assert m.tracer_pair() == (mask, True, (ran, 0) if bit == 1 else (0, ran))
        outs.append(_all_fields(m))
        m.close()
    for out in outs:
        akt = interior(out["Akt"], LLm, MMm)
        assert np.array_equal(akt[N + 1:], akt[:N + 1])
        for n in ("t", "Akt"):
            e = relerr(interior(out[n], LLm, MMm), interior(after[n], LLm, MMm))
            print("%dx%dx%d %s %s: relative error against the oracle %.3e" % (LLm, MMm, N, routine, n, e))
            assert e <= RTOL_ROUTINE, (n, e)
    for q, out in enumerate(outs[1:]):
        _assert_same(outs[0], out, (1, 2, 3, "default")[q])
    assert not np.array_equal(outs[0]["t"], before["t"])


@pytest.mark.parametrize("LLm,MMm,N", [(40, 32, 100), (21, 9, 88), (21, 9, 104)])
def test_whole_steps_pair_bitwise(LLm, MMm, N, monkeypatch):
    """6 steps: the eager first step, the captured graphs of both nstp phases
    and their replays."""
    cfg = _cfg(LLm, MMm, N)
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")   # whole steps keep Hz_u, Hz_v: every field can be read
    outs = []
    for pair in (0, 1, 2, 3):
        m = _model(cfg, monkeypatch, pair)
        m.step(6)
        m.sync()
        mask, same, n = m.tracer_pair()
        assert same
        # the first step and one capture per phase at least
        assert (n[0] >= 3 if pair & 1 else n[0] == 0) and (n[1] >= 3 if pair & 2 else n[1] == 0), n
        outs.append(_all_fields(m))
        m.close()
    for out in outs[1:]:
        _assert_same(outs[0], out, "6 steps")


@pytest.mark.parametrize("routine", ["pre_step3d", "step3d_t"])
def test_host_write_of_akt_ends_the_pairing(routine, oracle_state, monkeypatch):
    """After lmd_vmix the host puts an Akt whose S slot is twice its T slot:
    the routine on its own then runs one block per tracer on the host's
    Akt(isalt), as the library without pairing does, until lmd_vmix runs again."""
    LLm, MMm, N = 21, 9, 100
    cfg, tix, nfast, before, after = oracle_state(LLm, MMm, N, routine)
    outs = []
    for pair in (0, 3):
        m = _model(cfg, monkeypatch, pair)
        _prepare(m, tix, nfast, before)
        akt = m.get("Akt")
        assert m.tracer_pair()[1]    # a read leaves it
        akt[N + 1:] = 2.0 * akt[:N + 1]
        m.put("Akt", akt)
        assert m.tracer_pair() == (pair, False, (0, 0))
        getattr(m, routine)()
        m.sync()
        assert m.tracer_pair() == (pair, False, (0, 0))
        outs.append(_all_fields(m))
        m.lmd_vmix(tix[4])
        assert m.tracer_pair()[1]
        m.close()
    _assert_same(outs[0], outs[1], "host Akt")
    S = slice(3 * N + (tix[5] - 1) * N, 3 * N + tix[5] * N)   # S(nnew)
    assert not np.array_equal(interior(outs[0]["t"][S], LLm, MMm), interior(after["t"][S], LLm, MMm))


def test_ddmix_never_pairs(monkeypatch):
    cfg = ddmix_cfg(LLm=21, MMm=9, N=100)
    m = _model(cfg, monkeypatch, 3)
    m.step(3)
    m.sync()
    assert m.tracer_pair() == (3, False, (0, 0))
    m.close()


def test_unequal_backgrounds_never_pair(monkeypatch):
    monkeypatch.setenv("ROMS_GPU_T_PAIR", "3")
    cfg = _cfg(21, 9, 100)
    cfg.Akt_bak[1] = 2.0e-5
    o = oracle.Oracle(cfg)
    o.init()
    m, host = host_model(o, cfg)
    m.step(3)
    m.sync()
    assert m.tracer_pair() == (3, False, (0, 0))
    akt = interior(m.get("Akt"), cfg.LLm, cfg.MMm)
    assert not np.array_equal(akt[cfg.N + 1:], akt[:cfg.N + 1])
    m.close()
