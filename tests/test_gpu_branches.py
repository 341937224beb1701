"""Routine parity on states that take every data-dependent branch.

The depth, width and subdomain sweeps pin which kernel form runs; the states
of tests/branch_states.py pin which branch inside the kernel runs
(tests/test_branch_states.py asserts, on the oracle alone, the share of points
in each arm).  Here: one routine call per state on the oracle and on the GPU
from identical fields and time indices, within RTOL_ROUTINE of the oracle --
whole interiors, and whole arrays with their ghost rows where the state is
about an edge.  No point is left out: every branch here is continuous across
its threshold (cff at cw_min and at cutoff*cw_max, We -> 0 as cw_max -> 0+,
Flather's q -> 0 at 1 - 1/sqrt(2), the min of the drag), so a comparison that
flips by an ulp on one side moves the result by an ulp.

  omega           the four regimes of the Courant split in k_omega (two-pass,
                  width < 32), k_omega_seg on 64-column blocks (N = 21) and on
                  16-column blocks (N = 64); We and Wi relative to the larger
                  of their maxima (Wi is the larger one here)
  consumers       pre_step3d, step3d_uv1, step3d_t with that We / Wi pair
  linear drag     pre_step3d through roms_gpu_init with Zob = 0 (from_case
                  cannot set it): r_D and the u, v it feeds
  Flather         step2d at iif = 1, 2 with ndtfast = 4, three sets of open sides
  cext            pre_step3d and step3d_uv2 with boundary data of both signs
  KPP             over the linear EOS and over the split EOS without salinity
                  (rho_eos -> bvf, lmd_vmix at both time indices, 12 whole
                  steps); a surface layer inside the top cell (N = 12, 100);
                  a layer base where swr_frac is exactly zero

What the cases catch, tried on a scratch copy of the kernels, and the
measured errors: DESIGN.md section 4, "Branch coverage".
"""
import numpy as np
import pytest

import branch_states as bs
import oracle
import romsgpu
from test_gpu_depths import depth_model
from test_gpu_lmd import LMD_OUT
from test_gpu_obc import full
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, check_fields, copy_state, interior
from test_gpu_register import host_model

pytestmark = pytest.mark.gpu


def judge(tag, errs, tol=RTOL_ROUTINE):
    for n, e in errs.items():
        print("%s %s %.3e" % (tag, n, e))
    bad = [(n, e) for n, e in errs.items() if not e <= tol]
    assert not bad, (tag, bad)


def interior_errors(o, m, cfg, outs):
    return check_fields(o, m, outs, cfg.LLm, cfg.MMm, float("inf"))


def whole_errors(o, m, outs):
    return {n: full(m.get(n), o.field(n)) for n in outs}


def obc_model(cfg):
    return romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                   nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex,
                                   sizey=cfg.sizey, lmd=cfg.lmd, obc=cfg.obc, v_sponge=cfg.v_sponge,
                                   island=bool(cfg.island), curvgrid=bool(cfg.curvgrid))


def hand_over(o, m, tix, iif=1):
    copy_state(o, m)
    m.set_tindex(*tix, iif=iif, nfast=o.nfast())


# (Lm, Mm, N) -> omega in the segment form
OMEGA_FORMS = {(24, 10, 12): False, (40, 16, 21): True, (40, 16, 64): True}


@pytest.mark.parametrize("size", list(OMEGA_FORMS), ids=lambda s: "%dx%dx%d" % s)
def test_omega_four_regimes(size):
    cfg, o, tix = bs.omega_state(*size)
    m = depth_model(cfg)
    try:
        assert m.horizontal_path()["omega_seg"] == OMEGA_FORMS[size]
        hand_over(o, m, tix)
        o.call("omega")
        m.omega()
        m.sync()
        ref = {n: interior(o.field(n), cfg.LLm, cfg.MMm) for n in ("We", "Wi")}
        scale = max(float(np.abs(a).max()) for a in ref.values())
        errs = {n: float(np.abs(interior(m.get(n), cfg.LLm, cfg.MMm) - ref[n]).max()) / scale for n in ref}
    finally:
        m.close()
    judge("omega %dx%dx%d" % size, errs)


CONSUMERS = [("pre_step3d", "pred", ["t", "u", "v", "r_D"]), ("step3d_uv1", "corr", ["u", "v", "rufrc", "rvfrc"]),
             ("step3d_t", "corr", ["t"])]


@pytest.mark.parametrize("routine,mode,outs", CONSUMERS, ids=[c[0] for c in CONSUMERS])
def test_omega_consumers(routine, mode, outs):
    cfg, o, tix = bs.omega_state(40, 16, 21)
    o.call("omega")
    tix = bs.set_mode(o, mode)
    m = depth_model(cfg)
    try:
        hand_over(o, m, tix)
        o.call(routine)
        getattr(m, routine)()
        m.sync()
        errs = interior_errors(o, m, cfg, outs)
    finally:
        m.close()
    judge(routine + " after the four-regime omega", errs)


def test_linear_drag_through_roms_gpu_init():
    cfg, o, tix = bs.drag_state()
    m, host = host_model(o, cfg)
    try:
        o.call("pre_step3d")
        m.pre_step3d()
        m.sync()
        errs = interior_errors(o, m, cfg, ["r_D", "u", "v", "t"])
    finally:
        m.close()
    judge("pre_step3d with linear drag", errs)


@pytest.mark.parametrize("obc", [15, 5, 10])
def test_flather_high_courant(obc):
    cfg, o, tix = bs.flather_state(obc)
    m = obc_model(cfg)
    errs = {}
    try:
        copy_state(o, m)
        for iif in (1, 2):
            fast = bs.fast_indices(tix, iif)
            o.set_tindex(fast)
            o.L.or_set_iif(o.h, iif)
            m.set_tindex(*fast, iif=iif, nfast=o.nfast())
            o.call("step2d")
            m.step2d()
            m.sync()
            for n, e in whole_errors(o, m, ["zeta", "ubar", "vbar", "DU_avg1", "DV_avg1", "Zt_avg1"]).items():
                errs["iif=%d %s" % (iif, n)] = e
    finally:
        m.close()
    judge("step2d ndtfast=%d obc=%d" % (cfg.ndtfast, obc), errs)


CEXT = [("pre_step3d", "pred", ["u", "v", "t"]), ("step3d_uv2", "corr", ["u", "v", "ubar", "vbar", "FlxU", "FlxV"])]


@pytest.mark.parametrize("routine,mode,outs", CEXT, ids=[c[0] for c in CEXT])
def test_cext_both_signs(routine, mode, outs):
    cfg, o, tix = bs.cext_state(mode)
    m = obc_model(cfg)
    try:
        hand_over(o, m, tix, iif=2)
        o.call(routine)
        getattr(m, routine)()
        m.sync()
        errs = whole_errors(o, m, outs)
    finally:
        m.close()
    judge(routine + " with boundary data of both signs", errs)


@pytest.mark.parametrize("eos", ["linear", "nosalt"])
def test_kpp_eos_routines(eos):
    rho_out = (["rho"] if eos == "linear" else ["rho1", "qp1"]) + ["rhoA", "rhoS", "bvf"]
    errs = {}
    for mode in ("pred", "corr"):
        cfg, o, tix = bs.kpp_eos_state(eos, mode)
        tind = tix[4]
        m = depth_model(cfg)
        try:
            hand_over(o, m, tix)
            o.call("rho_eos", tind)
            m.rho_eos(tind)
            m.sync()
            for n, e in interior_errors(o, m, cfg, rho_out).items():
                errs["%s rho_eos %s" % (mode, n)] = e
            hand_over(o, m, tix)     # lmd_vmix from the oracle's bvf on both sides
            o.call("lmd_vmix", tind)
            m.lmd_vmix(tind)
            m.sync()
            for n, e in interior_errors(o, m, cfg, LMD_OUT).items():
                errs["%s lmd_vmix %s" % (mode, n)] = e
        finally:
            m.close()
    judge("KPP " + eos, errs)


@pytest.mark.parametrize("eos", ["linear", "nosalt"])
def test_kpp_eos_12_steps(eos):
    cfg = bs.kpp_eos_state(eos, "pred")[0]
    o = oracle.Oracle(cfg)
    o.init()
    o.step(12)
    m = depth_model(cfg)
    try:
        m.step(12)
        m.sync()
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC + LMD_OUT, cfg.LLm, cfg.MMm, float("inf"), kind="rms")
    finally:
        m.close()
    judge("KPP %s 12 steps rms" % eos, errs, RMS_RUN)


@pytest.mark.parametrize("state,N", [("top", 12), ("top", 100), ("swr", 12)])
def test_kpp_layer_ends(state, N):
    cfg, o, tix = (bs.kpp_top_state if state == "top" else bs.kpp_swr_state)(N)
    m = depth_model(cfg)
    try:
        hand_over(o, m, tix)
        o.call("lmd_vmix", tix[3])
        m.lmd_vmix(tix[3])
        m.sync()
        errs = interior_errors(o, m, cfg, LMD_OUT)
    finally:
        m.close()
    judge("lmd_vmix %s N=%d" % (state, N), errs)
