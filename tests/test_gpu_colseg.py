"""GPU parity of the segment-partitioned column solvers (k_colseg.h), which
replace the sequential Thomas sweeps for deep grids (N > 63: the C3 workload;
forced on at N = 50 here): the predictor's tracer and momentum columns
(pre_step3d), the corrector's momentum columns (step3d_uv1) and the tracer
corrector (step3d_t).  Their elimination order differs from the reference's, so the
bound is the north_star floating-point tolerance rather than bit equality:
1e-12 relative per routine call, field RMS < 1e-10 over a run.

Cases: the closed basin with nonlinear EOS at N = 50 (C2 depth) and with
LMD/KPP + surface fluxes at N = 100 (C3 depth), on small horizontal grids so
the oracle finishes in seconds.  Each routine is also compared with the
library's own sequential path (ROMS_GPU_COLSEG=0) on the same state.
"""
import os

import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, basin_cfg, check_fields, copy_state, interior, relerr

pytestmark = pytest.mark.gpu


def seg_cfg(case):
    if case == "n50":
        return basin_cfg(nonlin=True, LLm=40, MMm=24, N=50)
    c = basin_cfg(nonlin=True, LLm=24, MMm=20, N=100)
    c.lmd, c.surf_flux = oracle.LMD_ALL, 1
    return c


def make_model(cfg, colseg):
    old = os.environ.get("ROMS_GPU_COLSEG")
    os.environ["ROMS_GPU_COLSEG"] = str(colseg)
    try:
        return romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                       nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                       sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd,
                                       surf_flux=bool(cfg.surf_flux))
    finally:
        if old is None:
            del os.environ["ROMS_GPU_COLSEG"]
        else:
            os.environ["ROMS_GPU_COLSEG"] = old


# ru/rv after pre_step3d and step3d_uv1 are dead in the reference (the next
# read is preceded by prsgrd's assignment, prsgrd.F:293), so the segment
# solvers do not store them; their effect is checked through u, v, rufrc, rvfrc
ROUTINES = [("pre_step3d", "pred", ["t", "u", "v"]),
            ("step3d_uv1", "corr", ["u", "v", "rufrc", "rvfrc"]),
            ("step3d_t", "corr", ["t"])]


@pytest.mark.parametrize("case", ["n50", "n100"])
@pytest.mark.parametrize("routine,mode,outs", ROUTINES, ids=[r[0] for r in ROUTINES])
def test_seg_routine_parity(case, routine, mode, outs):
    cfg = seg_cfg(case)
    o = oracle.Oracle(cfg)
    o.init()
    o.step(3)
    iic, kstp, knew, nstp, nrhs, nnew = o.tindex()
    if mode == "corr":
        nrhs, nnew = 3, 3 - nstp
    else:
        nrhs, nnew = nstp, 3
    o.set_tindex([iic, kstp, knew, nstp, nrhs, nnew])
    # level-varying mixing and implicit vertical fluxes, so every per-level
    # input of the column solves is distinct (without LMD, Akv/Akt are the
    # constant background and Wi stays zero in these cases)
    rng = np.random.default_rng(11)
    for name in ("Akv", "Akt"):
        a = o.field(name)
        a[...] = a * (1.0 + 0.5 * rng.random(a.shape))
    we, wi = o.field("We"), o.field("Wi")
    wi[...] = wi + 0.01 * float(np.abs(we).max()) * rng.standard_normal(wi.shape)
    res = {}
    for colseg in (1, 0):
        m = make_model(cfg, colseg)
        copy_state(o, m)
        m.set_tindex(iic, kstp, knew, nstp, nrhs, nnew, nfast=o.nfast())
        getattr(m, routine)()
        m.sync()
        res[colseg] = {n: interior(m.get(n), cfg.LLm, cfg.MMm) for n in outs}
        m.close()
    o.call(routine)
    for n in outs:
        ref = interior(o.field(n), cfg.LLm, cfg.MMm)
        assert relerr(res[0][n], ref) <= RTOL_ROUTINE, (n, "sequential")
        e = relerr(res[1][n], ref)
        assert e <= RTOL_ROUTINE, (n, e)
        assert e > 0.0 or np.array_equal(res[1][n], ref)


@pytest.mark.parametrize("case", ["n50", "n100"])
def test_seg_run_rms(case):
    cfg = seg_cfg(case)
    o = oracle.Oracle(cfg)
    o.init()
    m = make_model(cfg, 1)
    o.step(30)
    m.step(30)
    check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms")
    m.close()


def _run_colreg(cfg, mask, nsteps):
    old = os.environ.get("ROMS_GPU_COLREG")
    os.environ["ROMS_GPU_COLREG"] = str(mask)
    try:
        m = make_model(cfg, 0)
    finally:
        if old is None:
            del os.environ["ROMS_GPU_COLREG"]
        else:
            os.environ["ROMS_GPU_COLREG"] = old
    m.step(nsteps)
    out = {n: m.get(n) for n in ("zeta", "ubar", "vbar", "u", "v", "t", "ru", "rv", "rufrc", "rvfrc", "FlxU", "We")}
    m.close()
    return out


@pytest.mark.parametrize("lmd", [0, oracle.LMD_ALL])
def test_register_column_kernels_bitwise(lmd):
    """The N = 50 register-resident column solver (k_pre_tracer_v_reg:
    ROMS_GPU_COLREG bit 2) keeps the sequential LDS solver's expressions
    and order: 12 steps equal the LDS form bitwise."""
    cfg = seg_cfg("n50")
    cfg.lmd, cfg.surf_flux = lmd, int(lmd != 0)
    a = _run_colreg(cfg, 0, 12)
    b = _run_colreg(cfg, 2, 12)
    for n in a:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.parametrize("case", ["n50", "n100"])
@pytest.mark.parametrize("switch", ["ROMS_GPU_PREUV_LDS", "ROMS_GPU_OMEGA_SEG", "ROMS_GPU_UV1_LDS", "ROMS_GPU_OMEGA_HB"])
def test_seg_variants_bitwise(case, switch, monkeypatch):
    """Variants that keep the reference's operations and order, so 6 steps
    equal the plain forms bitwise:
    - k_pre_uv_seg<true> (ROMS_GPU_PREUV_LDS, default) forms the predictor's
      cf_stp*u(nstp) + cf_bak*u(indx) and u(indx) = Hz*u(nstp) in its spline
      phase and keeps them in LDS instead of reloading u and Hz later;
    - k_omega_seg (ROMS_GPU_OMEGA_SEG, default) reads each input once and runs
      the partial sums of the divergence as one chain through the waves;
    - k_uv1_seg<true> (ROMS_GPU_UV1_LDS, default) keeps the spline phase's Hz
      pairs in LDS for the viscosity rows and chains the rufrc sum through
      the waves in k order;
    - k_omega_seg<true> (ROMS_GPU_OMEGA_HB, default) forms pre_step3d's
      Hz_bak/Hz_fwd in the predictor's omega with k_pre_tracer_h1's
      expression, the tracer kernel loading them instead."""
    cfg = seg_cfg(case)
    out = []
    for env in ("0", "1"):
        monkeypatch.setenv(switch, env)
        m = make_model(cfg, 1)
        m.step(6)
        out.append({n: m.get(n) for n in ("zeta", "ubar", "vbar", "u", "v", "t", "rufrc", "rvfrc")})
        m.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), n


@pytest.mark.parametrize("lmd", [0, oracle.LMD_ALL])
def test_seg_buffer_forms_bitwise(lmd, monkeypatch):
    """Segment solvers with buffer loads (the default; k_pre_tracer_segb,
    k_step3d_t_segb, k_uv1_segb, k_pre_uv_segb: the lane's column and the
    level offset in one VGPR) keep the expressions and their order: 6 steps
    at N = 100, with and without KPP, equal the pointer forms
    (ROMS_GPU_SEG_BUF=0) bitwise."""
    cfg = seg_cfg("n100")
    cfg.lmd, cfg.surf_flux = lmd, int(lmd != 0)
    out = []
    for env in ("0", None):
        if env is None:
            monkeypatch.delenv("ROMS_GPU_SEG_BUF")
        else:
            monkeypatch.setenv("ROMS_GPU_SEG_BUF", env)
        m = make_model(cfg, 1)
        m.step(6)
        out.append({n: m.get(n) for n in ("zeta", "ubar", "vbar", "u", "v", "t", "rufrc", "rvfrc")})
        m.close()
    for o in out[1:]:
        for n in out[0]:
            assert np.array_equal(out[0][n], o[n]), n


def _omega_cfg(case):
    if case == "n50":
        return seg_cfg("n50")
    c = basin_cfg(nonlin=True, LLm=40, MMm=16, N=100)   # >= 32 columns wide: the segment form runs
    c.lmd, c.surf_flux = oracle.LMD_ALL, 1
    return c


@pytest.mark.parametrize("case", ["n50", "n100"])
def test_omega_blocks(case, monkeypatch):
    """k_omega_seg on 64-, 32- and 16-column blocks (ROMS_GPU_OMEGA_CW): the
    k-order chain of partial sums keeps the reference's order, so 6 whole
    steps (predictor omega with Hz_bak/Hz_fwd, corrector, closing omega) are
    equal across block widths bitwise."""
    cfg = _omega_cfg(case)
    names = ("zeta", "ubar", "vbar", "u", "v", "t", "We", "Wi", "rufrc", "rvfrc")
    runs = {}
    for cw in ("64", "32", "16"):
        monkeypatch.setenv("ROMS_GPU_OMEGA_CW", cw)
        m = make_model(cfg, 1)
        m.step(6)
        runs[cw] = {n: m.get(n) for n in names}
        m.close()
    for cw in ("32", "16"):
        for n in names:
            assert np.array_equal(runs["64"][n], runs[cw][n]), (cw, n)
