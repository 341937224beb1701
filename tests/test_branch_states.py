"""The states of tests/branch_states.py do what they are for -- on the CPU
oracle alone, so this file needs no GPU.

For every state: the share of points in each arm of its branch, from a numpy
restatement of the branch condition on the routine's inputs (printed, and
asserted against the share the state is built for); where the restatement
also yields the output (omega's We / Wi, the linear drag's r_D, the linear
EOS's bvf) it is compared with the oracle's to 1e-14 relative, a second,
independent reference for those lines; and every field is finite after the
routine.  tests/test_gpu_branches.py then runs the HIP kernels on the same
states.
"""
import numpy as np
import pytest

import branch_states as bs
import oracle
import romsgpu

RESTATED = 1e-14


def all_finite(o):
    bad = [n for n in romsgpu.FIELDS if not np.isfinite(o.field(n)).all()]
    assert not bad, bad


@pytest.fixture
def show(capsys):
    """print() past pytest's capture: the shares are this file's report."""
    def _show(*a):
        with capsys.disabled():
            print(*a)
    return _show


def shares(show, tag, d):
    show(tag, "  ".join("%s %.1f%%" % (k, 100.0 * float(v)) for k, v in d.items()))


OMEGA_SIZES = [(24, 10, 12), (40, 16, 21), (40, 16, 64)]


@pytest.mark.parametrize("size", OMEGA_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_omega_takes_all_four_regimes(size, show):
    cfg, o, tix = bs.omega_state(*size)
    We, Wi, reg = bs.omega_split(o, cfg, tix)
    o.call("omega")
    part = {"cw < cw_min": np.mean(reg[1:cfg.N] == 1), "cw < cutoff*cw_max": np.mean(reg[1:cfg.N] == 2),
            "cff = cw_max*cw": np.mean(reg[1:cfg.N] == 3), "cw_max <= 0": np.mean(reg[1:cfg.N] == 4)}
    shares(show, "omega %dx%dx%d:" % size, part)
    assert all(v >= 0.02 for v in part.values()), part
    I = bs.box(cfg)
    we, wi = o.field("We")[I], o.field("Wi")[I]
    scale = max(np.abs(we).max(), np.abs(wi).max())
    err = max(np.abs(We - we).max(), np.abs(Wi - wi).max()) / scale
    show("omega restated: %.2e of max(|We|, |Wi|) = %.3e; max|Wi| / max|We| = %.2f"
          % (err, scale, np.abs(wi).max() / np.abs(we).max()))
    assert err <= RESTATED
    assert np.all(we[reg == 4] == 0.0) and np.abs(wi[reg == 4]).max() > 0.1 * scale
    all_finite(o)


def test_omega_consumers_stay_finite(show):
    """pre_step3d, step3d_uv1 and step3d_t with We / Wi as omega makes them
    from the scaled fluxes (implicit rows far from diagonal dominance): the
    oracle's outputs are finite at the full flux factor."""
    for routine, mode in (("pre_step3d", "pred"), ("step3d_uv1", "corr"), ("step3d_t", "corr")):
        cfg, o, tix = bs.omega_state(40, 16, 21)
        o.call("omega")
        bs.set_mode(o, mode)
        o.call(routine)
        all_finite(o)
        show(routine, {n: "%.3e" % np.abs(o.field(n)).max() for n in ("u", "v", "t")})


def test_linear_drag_clamp_binds_and_does_not(show):
    cfg, o, tix = bs.drag_state()
    r_D, binds = bs.drag_clamp(o, cfg)
    o.call("pre_step3d")
    part = {"rdrg (clamp idle)": np.mean(~binds), "0.8*Hz/dt (clamp binds)": np.mean(binds)}
    shares(show, "linear drag, rdrg = %g:" % cfg.rdrg, part)
    assert all(v >= 0.2 for v in part.values()), part
    got = o.field("r_D")[0][bs.box(cfg)]
    assert np.abs(got - r_D).max() <= RESTATED * np.abs(r_D).max()
    all_finite(o)


@pytest.mark.parametrize("obc", [15, 5, 10])
def test_flather_edges_on_both_sides_of_the_threshold(obc, show):
    cfg, o, tix = bs.flather_state(obc)
    for side, cx in bs.flather_cx(o, cfg).items():
        part = {"cx <= %.4f" % bs.K_FL: np.mean(cx <= bs.K_FL), "cx > %.4f" % bs.K_FL: np.mean(cx > bs.K_FL)}
        shares(show, "Flather obc=%d %s (cx %.3f .. %.3f):" % (obc, side, cx.min(), cx.max()), part)
        assert all(v >= 0.2 for v in part.values()), (side, part)
    for iif in (1, 2):
        o.set_tindex(bs.fast_indices(tix, iif))
        o.L.or_set_iif(o.h, iif)
        o.call("step2d")
        all_finite(o)
    assert np.abs(o.field("ubar")).max() > 1e-4


@pytest.mark.parametrize("routine,mode", [("pre_step3d", "pred"), ("step3d_uv2", "corr")])
def test_cext_boundary_data_of_both_signs(routine, mode, show):
    cfg, o, tix = bs.cext_state(mode)
    o.call(routine)
    for side, part in bs.cext_arms(o, cfg, tix).items():
        shares(show, "cext %s %s:" % (routine, side), part)
        assert part["data in"] >= 0.2 and part["data out"] >= 0.2, (side, part)
        assert part["ran bry arm"] > 0.0 and part["ran ubind arm"] > 0.0, (side, part)
    all_finite(o)


@pytest.mark.parametrize("eos", ["linear", "nosalt"])
@pytest.mark.parametrize("mode", ["pred", "corr"])
def test_kpp_eos_variants(eos, mode, show):
    cfg, o, tix = bs.kpp_eos_state(eos, mode)
    assert (cfg.nonlin_eos, cfg.salinity, cfg.NT) == ((0, 1, 2) if eos == "linear" else (1, 0, 1))
    tind = tix[4]
    o.call("rho_eos", tind)
    if eos == "linear":
        ref = bs.linear_bvf(o, cfg, tind)
        assert np.abs(o.field("bvf")[bs.box(cfg)] - ref).max() <= RESTATED * np.abs(ref).max()
    else:
        # rho_eos.F:198, 213-215: without SALINITY the split EOS keeps Ts = 34.5,
        # so rho1 = rho - rho0 is sea water's (fresh water at 4..14 degC: -28)
        rho1 = o.field("rho1")[bs.box(cfg)]
        assert -3.0 < rho1.min() and rho1.max() < 0.5, (rho1.min(), rho1.max())
    o.call("lmd_vmix", tind)
    all_finite(o)
    show("KPP %s %s: hbls %.1f .. %.1f m" % ((eos, mode) + (o.field("hbls")[0][bs.box(cfg)].min(),
                                                            o.field("hbls")[0][bs.box(cfg)].max())))
    o.step(12)
    all_finite(o)


@pytest.mark.parametrize("N", [12, 100])
def test_kpp_layer_ends_inside_the_top_cell(N, show):
    cfg, o, tix = bs.kpp_top_state(N)
    o.call("lmd_vmix", tix[3])
    kbls, _ = bs.kpp_base(o, cfg)
    part = {"kbls == N": np.mean(kbls == N), "kbls < N": np.mean(kbls < N)}
    shares(show, "KPP heating N=%d:" % N, part)
    assert part["kbls == N"] >= 0.05
    all_finite(o)


def test_kpp_layer_reaches_zero_short_wave(show):
    cfg, o, tix = bs.kpp_swr_state()
    o.call("lmd_vmix", tix[3])
    kbls, swr = bs.kpp_base(o, cfg)
    part = {"swr_frac(kbls-1) <= 0": np.mean(swr <= 0.0), "> 0": np.mean(swr > 0.0)}
    shares(show, "KPP mixed columns: hbls up to %.0f m;" % o.field("hbls")[0][bs.box(cfg)].max(), part)
    assert part["swr_frac(kbls-1) <= 0"] >= 0.05 and part["> 0"] >= 0.05
    all_finite(o)


def _open_side_cases():
    import test_gpu_open_sides as sweep
    return sweep, sweep.SWEEP, sweep.SWEEP_IDS


@pytest.mark.parametrize("obc,size", _open_side_cases()[1], ids=_open_side_cases()[2])
def test_open_side_twin_takes_every_arm(obc, size):
    """The oracle's half of tests/test_gpu_open_sides.py, for every set of open
    sides at both sizes: the twin state takes every arm of step2d's and the
    3-D routines' boundary code on every open side (asserted inside the
    helpers), the oracle's outputs are finite, the sponge band lies along
    the open sides alone, and in the 12-step run every open side moves and
    every closed side stays a wall."""
    sweep = _open_side_cases()[0]
    sweep.stage(obc, size, "corr", False)
    for iif in (1, 2):
        sweep.oracle_step2d(obc, size, iif)
    for routine, (mode, outs) in sweep.ROUTINES3D.items():
        for tuned in (False, True):
            cfg, o, tix, ub = sweep.oracle_3d_arms(obc, size, routine, tuned)
            o.call(routine)
            sweep.all_finite(o, outs)
    cfg = bs.flather_cfg(obc, ndtfast=30, **sweep.size_kw(size))
    cfg.v_sponge = sweep.V_SPONGE
    o = oracle.Oracle(cfg)
    o.init()
    sweep.check_sponge(cfg, o)
    cfg = sweep.run_cfg(obc, size)
    o = oracle.Oracle(cfg)
    o.init()
    first = {n: o.field(n).copy() for n in sweep.STATE}
    o.step(sweep.RUN_STEPS)
    all_finite(o)
    sweep.check_sides_moved(cfg, first, o.field)
