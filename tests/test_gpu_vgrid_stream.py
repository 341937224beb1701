"""Hz and z_w formed inside k_omega_seg, k_set_huv1_chain, k_uv2_fused,
k_visc3d_stg and k_t3dmix_stg (ROMS_GPU_VGRID2) against the streamed arrays
(ROMS_GPU_VGRID2=0): bitwise equal fields.

The five kernels form a column's (or a staged window's) Hz and z_w from z_sd,
h, hinv and Cs_w with set_depth's own expressions (VGrid, roms_dev.h) while
the stored arrays are set_depth's own, under the validity flag ROMS_GPU_VGRID
obeys.  Every comparison runs the default mask, every kernel (31) and the
streaming forms (0); the outputs are bitwise equal and the default is within
RTOL_ROUTINE of the oracle.  Every state has a non-zero free surface.
  * routine level, on the closed KPP basin after 4 oracle steps with the
    model's own set_depth first, at the depths and widths that switch a path
    of each kernel (named at the cases);
  * whole steps, every field of romsgpu.FIELDS (the predictor's
    k_omega_seg<true> through c2 / c3 -> t; the doubly periodic wrap must
    carry z_sd);
  * 2 x 2 subdomains;
  * validity: a host-written Hz sends every kernel back to the stored arrays
    until the next set_depth.
Wi's error is taken relative to We's interior maximum, as test_gpu_depths
does on this basin: where the Courant split leaves Wi zero it is
cancellation noise of We.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_lmd_lean import _restore, _snapshot, _tindex
from test_gpu_multirank import _case, run_decomposed
from test_gpu_parity import RTOL_ROUTINE, interior, relerr
from test_gpu_vgrid import _cfg

pytestmark = pytest.mark.gpu

ALL, DEFAULT = 31, 31   # kVg2All, kVg2Default (roms_dev.h)
VARIANTS = (None, ALL, 0)   # the default mask, every kernel, the streaming forms
UV_OUT = ["u", "v", "FlxU", "FlxV"]
UV2_OUT = ["u", "v", "ubar", "vbar", "FlxU", "FlxV"]
# routine -> (time indices, outputs)
ROUTINES = {"omega": ("nstp", ["We", "Wi"]), "set_HUV1": ("nstp", UV_OUT), "step3d_uv2": ("nrhs", UV2_OUT),
            "visc3d": ("nrhs", ["u", "v", "rufrc", "rvfrc"]), "t3dmix": ("nrhs", ["t"])}


def _basin(N, LLm, MMm):
    cfg = _cfg("basin", N, LLm)
    cfg.MMm = MMm
    return cfg


def _model(cfg, monkeypatch, vgrid2=None, env=None):
    """A model of cfg under ROMS_GPU_VGRID2=vgrid2 (None: unset, the default)."""
    if vgrid2 is None:
        monkeypatch.delenv("ROMS_GPU_VGRID2", raising=False)
    else:
        monkeypatch.setenv("ROMS_GPU_VGRID2", str(vgrid2))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")   # whole steps keep Hz_u, Hz_v readable
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    for k in (env or {}):
        monkeypatch.delenv(k)
    assert m.vgrid2() == (DEFAULT if vgrid2 is None else vgrid2, True)   # init ran set_depth
    return m


def _state(cfg, mixing=False):
    """The oracle of cfg after 4 steps and a copy of its state; mixing: smooth
    non-zero visc2_r, visc2_p, diff2 (the closed basin has none of its own)."""
    o = oracle.Oracle(cfg)
    o.init()
    o.step(4)
    if mixing:
        for n, amp in (("visc2_r", 40.0), ("visc2_p", 40.0), ("diff2", 15.0)):
            a = o.field(n)
            jj, ii = np.meshgrid(np.arange(a.shape[-2]), np.arange(a.shape[-1]), indexing="ij")
            a[...] = amp * (1.0 + 0.5 * np.sin(0.37 * ii) * np.cos(0.23 * jj))
    state = _snapshot(o)
    assert np.max(np.abs(state["zeta"])) > 0.0
    return o, state


def _run(m, o, state, routine, tix):
    for n, a in state.items():
        m.put(n, a)
    m.set_tindex(*tix, nfast=o.nfast())
    assert m.vgrid2()[1] is False   # the host wrote Hz
    m.set_depth()
    assert m.vgrid2()[1] is True
    assert m.vgrid_mismatch() == (0, 0, 0)
    getattr(m, routine)()
    m.sync()
    return {n: m.get(n) for n in ROUTINES[routine][1]}


def _check(cfg, routines, monkeypatch, env=None, mixing=False, omega_seg=None):
    """Each routine from the same state on one model per variant: bitwise equal
    among the variants, the default within RTOL_ROUTINE of the oracle."""
    o, state = _state(cfg, mixing)
    models = [_model(cfg, monkeypatch, v, env) for v in VARIANTS]
    try:
        if omega_seg is not None:
            assert models[0].horizontal_path()["omega_seg"] is omega_seg
        for routine in routines:
            which, names = ROUTINES[routine]
            tix, _ = _tindex(o, which)
            _restore(o, state)
            o.set_tindex(tix)
            o.call("set_depth")
            o.call(routine)
            outs = [_run(m, o, state, routine, tix) for m in models]
            ref = {n: interior(o.field(n), cfg.LLm, cfg.MMm) for n in set(names) | {"We"}}
            bad = []
            for n in names:
                a = interior(outs[0][n], cfg.LLm, cfg.MMm)
                if n == "Wi":
                    e = float(np.abs(a - ref[n]).max()) / float(np.abs(ref["We"]).max())
                else:
                    e = relerr(a, ref[n])
                print("N=%d %dx%d %s %s: relerr %.3e" % (cfg.N, cfg.LLm, cfg.MMm, routine, n, e))
                if not (e <= RTOL_ROUTINE):
                    bad.append((routine, n, e))
            assert not bad, bad
            for v, out in zip(VARIANTS[1:], outs[1:]):
                for n in names:
                    assert np.array_equal(outs[0][n], out[n]), (routine, v, n)
    finally:
        for m in models:
            m.close()


# ---- 1. routine level ----
OMEGA_CASES = [
    # N, LLm, MMm, environment, segment form
    (5, 40, 32, None, True), (12, 40, 32, None, True), (50, 40, 32, None, True), (63, 40, 32, None, True),
    (64, 40, 32, None, True),     # the 16-column blocks start
    (88, 40, 32, None, True),     # 11-row segments
    (100, 40, 32, None, True), (101, 40, 32, None, True),   # uneven partition
    (104, 40, 32, None, True),    # every register row full
    (105, 40, 32, None, False),   # the two-pass k_omega, unchanged
    (100, 40, 6, None, True), (100, 70, 6, None, True),     # partial 16- and 64-column blocks
    (100, 31, 6, None, False),    # too narrow for the segment form
    (12, 70, 6, None, True),
    (100, 40, 32, {"ROMS_GPU_OMEGA_CW": "32"}, True), (100, 70, 6, {"ROMS_GPU_OMEGA_CW": "64"}, True),
    (100, 40, 32, {"ROMS_GPU_OMEGA_CW": "64"}, True),
]


@pytest.mark.parametrize("N,LLm,MMm,env,seg", OMEGA_CASES,
                         ids=["%d-%dx%d%s" % (c[0], c[1], c[2], "-cw" + c[3]["ROMS_GPU_OMEGA_CW"] if c[3] else "")
                              for c in OMEGA_CASES])
def test_omega_bitwise(N, LLm, MMm, env, seg, monkeypatch):
    _check(_basin(N, LLm, MMm), ["omega"], monkeypatch, env=env, omega_seg=seg)


# chain segments of set_HUV1 / step3d_uv2 (k_chain.h chain_kl): N = 5 KL 5 with three empty lanes; 18 KL 5 with a
# short last segment 5/5/5/3; 21 KL 13 with two empty segments 13/8/0/0; 52 KL 13 full; 53 KL 25 with one empty
# segment 25/25/3/0; 99 KL 25 with a short last segment; 100 FULL; 101 the one-lane fallbacks, unchanged
@pytest.mark.parametrize("N,LLm", [(5, 40), (18, 40), (21, 40), (52, 40), (53, 40), (99, 40), (100, 40), (101, 40),
                                   (18, 70), (53, 70), (100, 70)])
def test_set_huv1_and_uv2_bitwise(N, LLm, monkeypatch):
    _check(_basin(N, LLm, 32 if LLm == 40 else 14), ["set_HUV1", "step3d_uv2"], monkeypatch)


# the staged windows: N = 2 (one level ahead is the last), 3, 12, 100; 70 columns (a partial second tile) and
# 30 rows (not a multiple of the tiles' 4)
@pytest.mark.parametrize("N,LLm,MMm", [(2, 40, 32), (3, 40, 32), (12, 40, 32), (100, 40, 32), (12, 70, 30),
                                       (100, 70, 14)])
def test_visc3d_and_t3dmix_bitwise(N, LLm, MMm, monkeypatch):
    cfg = _basin(N, LLm, MMm)
    assert cfg.NT == 2
    _check(cfg, ["visc3d", "t3dmix"], monkeypatch, mixing=True)


# ---- 2. whole steps ----
@pytest.mark.parametrize("case,N", [("basin", 20), ("basin", 100), ("pipes", None), ("filament", None)])
def test_whole_steps_bitwise(case, N, monkeypatch):
    cfg = _cfg(case, N)
    outs = []
    for v in VARIANTS:
        m = _model(cfg, monkeypatch, v)
        m.step(3)
        m.sync()
        assert m.vgrid2() == (DEFAULT if v is None else v, True)
        assert m.vgrid_mismatch() == (0, 0, 0)
        outs.append({n: m.get(n) for n in romsgpu.FIELDS})
        m.close()
    assert np.max(np.abs(outs[0]["zeta"])) > 0.0
    for out in outs[1:]:
        for n in romsgpu.FIELDS:
            assert np.array_equal(outs[0][n], out[n], equal_nan=True), n


# ---- 3. decomposed ----
def test_decomposed_2x2_bitwise(monkeypatch):
    case = _case("basin_flux")
    fields = ("zeta", "ubar", "vbar", "u", "v", "t", "Hz", "z_w", "FlxU", "FlxV", "We", "Wi", "rufrc", "rvfrc",
              "Akv", "Akt")
    runs = []
    for v in VARIANTS:
        if v is None:
            monkeypatch.delenv("ROMS_GPU_VGRID2", raising=False)
        else:
            monkeypatch.setenv("ROMS_GPU_VGRID2", str(v))
        parts, _ = run_decomposed(case, 2, 2, 3, fields=fields, probe=lambda m: (m.vgrid2(), m.vgrid_mismatch()))
        runs.append(parts)
    for rank in range(4):
        on = runs[0][rank]
        assert np.max(np.abs(on[4]["zeta"])) > 0.0
        for v, parts in zip(VARIANTS, runs):
            mask = DEFAULT if v is None else v
            assert parts[rank][5] == ((mask, True), (0, 0, 0)), (rank, v, parts[rank][5])
            for n in fields:
                assert np.array_equal(on[4][n], parts[rank][4][n]), (rank, v, n)


# ---- 4. validity ----
def test_host_written_hz_turns_the_grid_off(monkeypatch):
    """After the host writes Hz (and, so that omega's result depends on the
    stored grid at all, a z_w stretched unevenly over the levels) omega and
    set_HUV1 follow the stored arrays under every mask; after set_depth they
    give the base results again."""
    cfg = _basin(18, 40, 32)
    o, state = _state(cfg)
    tix, _ = _tindex(o, "nstp")
    names = ["We", "Wi"] + UV_OUT
    res = {}
    for v in VARIANTS:
        m = _model(cfg, monkeypatch, v)
        mask = DEFAULT if v is None else v

        def both():
            for n in UV_OUT:   # set_HUV1 works in place
                m.put(n, state[n])
            m.omega()
            m.sync()
            out = {n: m.get(n) for n in ("We", "Wi")}
            m.set_HUV1()
            m.sync()
            out.update({n: m.get(n) for n in UV_OUT})
            return out

        for n, a in state.items():
            m.put(n, a)
        m.set_tindex(*tix, nfast=o.nfast())
        m.set_depth()
        assert m.vgrid2() == (mask, True)
        base = both()
        m.put("Hz", 1.5 * m.get("Hz"))
        assert m.vgrid2() == (mask, False)
        zw = m.get("z_w")
        m.put("z_w", zw * (1.0 + 0.3 * np.linspace(0.0, 1.0, zw.shape[0]) ** 2)[:, None, None])
        pert = both()
        m.set_depth()
        assert m.vgrid2() == (mask, True)
        assert m.vgrid_mismatch() == (0, 0, 0)
        again = both()
        m.close()
        res[v] = (base, pert, again)
    for n in names:
        for v in VARIANTS[:2]:
            for q in range(3):
                assert np.array_equal(res[v][q][n], res[0][q][n]), (v, q, n)
        assert np.array_equal(res[None][0][n], res[None][2][n]), n
    assert not np.array_equal(res[None][0]["We"], res[None][1]["We"])
    assert not np.array_equal(res[None][0]["FlxU"], res[None][1]["FlxU"])
