"""The horizontal tracer kernels as level walks over staged windows
(k_pre_tracer_stg, k_step3d_t_stg; ROMS_GPU_T_HSTG bits 1 and 2, bit 4: Hz
formed inside the predictor's walk) against one block per tile and level
(ROMS_GPU_T_HSTG=0, the k_*_h1 kernels): bitwise equal fields, within
RTOL_ROUTINE of the oracle.

One block of 64x8 cells walks k = 1..N: the lane's umask / vmask values, pm,
pn and the river tests once per block, each level's FlxU, FlxV, T, S windows
staged in LDS with the next level's in flight; a lane reads its stencil of
the windows once and forms its four faces from it.  Covered here:
  * pre_step3d and step3d_t as single routines from an oracle state (the
    model's own set_depth first, so that bit 4 is in force) under every mask
    0..7 and unset: all of romsgpu.FIELDS bitwise equal across the masks, the
    routine's t within RTOL_ROUTINE of the oracle, and the path query shows
    the staged kernel ran exactly where its bit is set;
  * grids whose tile and window edges differ: 70x10 (a second x-tile with 6
    live lanes, Mm no multiple of 4 or 8, a second block row of 2 rows), 21x9
    (one partial tile; the predictor's ring row opens a second block row),
    130x6 (three x-tiles), 70x18 (three block rows, the last of 2 rows);
  * depths N = 5 (column solvers) and N = 88 (segment solvers; in whole steps
    the predictor then takes Hz_bak from omega, as a single routine it forms
    it in either case);
  * boundaries: the closed basin (wall clamps of tracer_fx / tracer_fe), the
    doubly periodic Filament with salinity, the rivers case (river faces per
    level);
  * whole steps on 70x10x88, 130x6x88, 70x18x88 (Hz_bak from omega over
    several x-tiles and block rows) and 70x10x5: eager first step, graph
    capture and replay, both nstp phases;
  * validity: a host write of Hz makes the predictor read the stored Hz (mask
    7 then equals mask 3 bitwise), the next set_depth turns forming back on;
  * NT = 1 takes the per-level kernels.
Unset, the mask is 7 on the segment path and 2 (the corrector's walk only)
with the column solvers of N <= 63.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_lmd import lmd_basin_cfg
from test_gpu_parity import RTOL_ROUTINE, interior, relerr

pytestmark = pytest.mark.gpu

PRE, COR, HZ = 1, 2, 4   # kTHstgPre, kTHstgCor, kTHstgHz (roms_dev.h)


def _default(N):
    """kTHstgDefault on the segment path (N > 63), kTHstgDefaultCol with the column solvers."""
    return 7 if N > 63 else 2


MASKS = (0, 1, 2, 3, 4, 5, 6, 7, None)
GRIDS = [(70, 10), (21, 9), (130, 6), (70, 18)]
DEPTHS = [5, 88]


def _cfg(case, LLm, MMm, N):
    if not isinstance(case, str):   # a configuration of the caller's (tests/test_gpu_rivers_sweep.py)
        assert (case.LLm, case.MMm, case.N) == (LLm, MMm, N)
        return case
    if case == "filament":   # doubly periodic, T and S
        return oracle.filament_cfg(LLm=LLm, MMm=MMm, N=N, NT=2, salinity=True, sizex=200.0 * LLm, sizey=50.0 * MMm,
                                   np_xi=1, np_eta=1)
    if case == "rivers":
        return oracle.rivers_cfg(LLm=LLm, MMm=MMm, N=N, np_xi=1, np_eta=1)
    return lmd_basin_cfg(surf_flux=1, LLm=LLm, MMm=MMm, N=N)   # closed on all four sides


def _model(cfg, monkeypatch, mask):
    """A model of cfg under ROMS_GPU_T_HSTG=mask (None: unset, the default)."""
    if mask is None:
        monkeypatch.delenv("ROMS_GPU_T_HSTG", raising=False)
    else:
        monkeypatch.setenv("ROMS_GPU_T_HSTG", str(mask))
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")   # whole steps keep Hz_u, Hz_v: every field can be read
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    assert m.tracer_hstg() == (_default(cfg.N) if mask is None else mask, True, (0, 0, 0))   # init ran set_depth
    return m


def _all_fields(m):
    return {n: m.get(n) for n in romsgpu.FIELDS}


def _assert_same(a, b, tag):
    diff = [n for n in a if not np.array_equal(a[n], b[n], equal_nan=True)]
    assert not diff, (tag, diff)


def _expected(routine, mask, N):
    """Launches (pre, cor, pre with Hz formed) one call of the routine adds, as ran / did not."""
    mask = _default(N) if mask is None else mask
    if routine == "pre_step3d":
        return (bool(mask & PRE), False, bool(mask & PRE) and bool(mask & HZ))
    return (False, bool(mask & COR), False)


@pytest.fixture(scope="module")
def oracle_state():
    """Per (case, LLm, MMm, N, routine): the oracle after 4 steps with the
    routine's indices set (the predictor's for pre_step3d, the corrector's
    for step3d_t), its fields before the routine and t after set_depth + the
    routine (formed once, left unchanged).  setup = (tag, on_oracle,
    on_model): on_oracle(o) runs between init and the steps, tag tells its
    states from the plain ones."""
    cache = {}

    def get(case, LLm, MMm, N, routine, setup=None):
        key = (case if isinstance(case, str) else bytes(case), LLm, MMm, N, routine, setup[0] if setup else None)
        if key not in cache:
            cfg = _cfg(case, LLm, MMm, N)
            o = oracle.Oracle(cfg)
            o.init()
            if setup is not None:
                setup[1](o)
            o.step(4)
            iic, kstp, knew, nstp, nrhs, nnew = o.tindex()
            tix = [iic, kstp, knew, nstp, nstp, 3] if routine == "pre_step3d" else [iic, kstp, knew, nstp, 3, 3 - nstp]
            o.set_tindex(tix)
            before = {n: o.field(n).copy() for n in romsgpu.FIELDS}
            assert np.max(np.abs(before["zeta"])) > 0.0
            o.call("set_depth")
            o.call(routine)
            cache[key] = (cfg, tix, o.nfast(), before, o.field("t").copy())
        return cache[key]
    return get


def _prepare(m, tix, nfast, before):
    """The oracle's state, then the model's own set_depth: the host wrote Hz, which ends the grid's validity."""
    for n, a in before.items():
        m.put(n, a)
    m.set_tindex(*tix, nfast=nfast)
    assert m.tracer_hstg()[1] is False
    m.set_depth()
    assert m.tracer_hstg()[1] is True


def _routine_under_every_mask(case, LLm, MMm, N, routine, oracle_state, monkeypatch, setup=None):
    """setup = (tag, on_oracle, on_model) as oracle_state takes it; on_model(m)
    runs on every model before the oracle's state goes in.  Returns the
    fields of the per-level kernels' model (mask 0) after the routine."""
    cfg, tix, nfast, before, t_after = oracle_state(case, LLm, MMm, N, routine, setup)
    assert cfg.NT == 2
    outs = []
    for mask in MASKS:
        m = _model(cfg, monkeypatch, mask)
        if setup is not None:
            setup[2](m)
        _prepare(m, tix, nfast, before)
        assert m.tracer_hstg()[2] == (0, 0, 0)
        getattr(m, routine)()
        m.sync()
        n = m.tracer_hstg()[2]
        assert tuple(q > 0 for q in n) == _expected(routine, mask, N), (mask, n)
        outs.append(_all_fields(m))
        m.close()
    for mask, out in zip(MASKS, outs):
        e = relerr(interior(out["t"], LLm, MMm), interior(t_after, LLm, MMm))
        print("%s %dx%dx%d %s mask %s: t relative error against the oracle %.3e" % (case, LLm, MMm, N, routine, mask, e))
        assert e <= RTOL_ROUTINE, (mask, e)
    for mask, out in zip(MASKS[1:], outs[1:]):
        _assert_same(outs[0], out, mask)
    assert not np.array_equal(outs[0]["t"], before["t"])
    return outs[0]


# ---- 1.-3. routine parity on the grids and depths, closed basin ----
@pytest.mark.parametrize("routine", ["pre_step3d", "step3d_t"])
@pytest.mark.parametrize("N", DEPTHS)
@pytest.mark.parametrize("LLm,MMm", GRIDS)
def test_routine_every_mask_bitwise(LLm, MMm, N, routine, oracle_state, monkeypatch):
    _routine_under_every_mask("basin", LLm, MMm, N, routine, oracle_state, monkeypatch)


# ---- 4. boundaries: doubly periodic with salinity; the rivers case ----
@pytest.mark.parametrize("routine", ["pre_step3d", "step3d_t"])
def test_routine_doubly_periodic(routine, oracle_state, monkeypatch):
    _routine_under_every_mask("filament", 70, 10, 10, routine, oracle_state, monkeypatch)


@pytest.mark.parametrize("routine", ["pre_step3d", "step3d_t"])
def test_routine_rivers(routine, oracle_state, monkeypatch):
    o = oracle.Oracle(_cfg("rivers", 40, 40, 10))
    o.init()
    assert np.count_nonzero(np.abs(o.field("riv_vflx")) > 1e-3) > 0   # river faces at this size
    _routine_under_every_mask("rivers", 40, 40, 10, routine, oracle_state, monkeypatch)


# ---- 5. whole steps ----
@pytest.mark.parametrize("LLm,MMm,N", [(70, 10, 88), (70, 10, 5), (130, 6, 88), (70, 18, 88)])
def test_whole_steps_bitwise(LLm, MMm, N, monkeypatch):
    """4 steps: the eager first step, the captured graphs of both nstp phases
    and a replay.  At N = 88 the predictor's walk takes Hz_bak from omega
    (k_pre_tracer_stg<true, .>), which the routine alone never does: 130x6 has
    three x-tiles, 70x18 three block rows."""
    cfg = _cfg("basin", LLm, MMm, N)
    outs = []
    for mask in (0, 3, 7, None):
        m = _model(cfg, monkeypatch, mask)
        m.step(4)
        m.sync()
        on = _default(N) if mask is None else mask
        mk, valid, n = m.tracer_hstg()
        assert mk == on and valid
        # the first step and one capture per phase
        assert (n[0] >= 3 if on & PRE else n[0] == 0) and (n[1] >= 3 if on & COR else n[1] == 0), n
        assert (n[2] >= 3 if on & PRE and on & HZ else n[2] == 0), n
        outs.append(_all_fields(m))
        m.close()
    assert np.max(np.abs(outs[0]["zeta"])) > 0.0
    for out in outs[1:]:
        _assert_same(outs[0], out, "4 steps")


# ---- 6. validity ----
def test_host_written_hz_is_what_the_predictor_reads(oracle_state, monkeypatch):
    """pre_step3d alone after the host scaled Hz: every mask reads the stored
    Hz (no launch forms it), bitwise the per-level kernels, and the result
    differs from the one on set_depth's Hz; after set_depth forming is back."""
    LLm, MMm, N = 70, 10, 88
    cfg, tix, nfast, before, t_after = oracle_state("basin", LLm, MMm, N, "pre_step3d")
    res = {}
    for mask in (0, 3, 7):
        m = _model(cfg, monkeypatch, mask)
        _prepare(m, tix, nfast, before)
        hz = m.get("Hz")
        assert m.tracer_hstg()[1] is True    # a read leaves it
        m.put("Hz", 1.5 * hz)
        assert m.tracer_hstg() == (mask, False, (0, 0, 0))
        m.pre_step3d()
        m.sync()
        assert m.tracer_hstg() == (mask, False, (1 if mask & PRE else 0, 0, 0))
        pert = _all_fields(m)
        _prepare(m, tix, nfast, before)
        m.pre_step3d()
        m.sync()
        assert m.tracer_hstg() == (mask, True, (2 if mask & PRE else 0, 0, 1 if mask == 7 else 0))
        res[mask] = (pert, _all_fields(m))
        m.close()
    for mask in (3, 7):
        _assert_same(res[0][0], res[mask][0], ("host Hz", mask))
        _assert_same(res[0][1], res[mask][1], ("set_depth's Hz", mask))
    assert not np.array_equal(res[7][0]["t"], res[7][1]["t"])


def test_host_write_of_hz_between_steps(monkeypatch):
    """Whole steps with Hz scaled by the host after the first: the next step's
    predictor reads the stored Hz (mask 7 equals mask 3 and 0 bitwise), its
    set_depth makes the grid valid and the step after it forms Hz again."""
    cfg = _cfg("basin", 70, 10, 88)
    outs = []
    for mask in (0, 3, 7):
        m = _model(cfg, monkeypatch, mask)
        m.step(1)
        m.sync()
        n1 = m.tracer_hstg()[2]
        assert n1 == ((1, 1, 1) if mask == 7 else (1, 1, 0) if mask == 3 else (0, 0, 0))
        m.put("Hz", 1.01 * m.get("Hz"))
        assert m.tracer_hstg()[1] is False
        m.step(1)
        m.sync()
        mk, valid, n2 = m.tracer_hstg()
        assert valid and n2[2] == n1[2] and (n2[0] > n1[0] if mask & PRE else n2[0] == 0), (n1, n2)
        m.step(1)
        m.sync()
        n3 = m.tracer_hstg()[2]
        assert (n3[2] > n2[2] if mask == 7 else n3[2] == 0), (n2, n3)
        outs.append(_all_fields(m))
        m.close()
    for out in outs[1:]:
        _assert_same(outs[0], out, "host Hz between steps")


# ---- 7. one tracer ----
def test_one_tracer_takes_the_per_level_kernels(monkeypatch):
    cfg = oracle.filament_cfg(LLm=21, MMm=9, N=10, sizex=200.0 * 21, sizey=50.0 * 9, np_xi=1, np_eta=1)
    assert cfg.NT == 1
    outs = []
    for mask in (0, None):
        m = _model(cfg, monkeypatch, mask)
        m.step(3)
        m.sync()
        assert m.tracer_hstg() == (_default(cfg.N) if mask is None else mask, True, (0, 0, 0))
        outs.append(_all_fields(m))
        m.close()
    _assert_same(outs[0], outs[1], "NT = 1")
