"""The numpy restatement of the baroclinic pressure fluxes (tests/pflx_ref.py) held to checks that do not depend on
it.  The recipe that compiles reference routines for the oracle is frozen, so the restatement cannot be pinned to a
compiled calc_pressure_flux; these properties stand in:

* constant density: every dR is 0 and P is the hydrostatic line, to (N+2) ulp of max|P| (one rounding a level and
  the top);
* timescale = dt (alpha = 1): the slow parts are the whole signal and the fluxes vanish, exactly;
* u - Uflx carries no depth-integrated transport when FlxU is set_HUV's of u: the baroclinic property the filters
  rely on, to rounding;
* p_fast read one cell off in i, or up summed top-down, changes up on the test state: the device comparison of
  tests/test_gpu_pflx.py (np.array_equal against this restatement) can see those mistakes."""
import numpy as np
import pytest

import branch_states as bs
import pflx_ref as pr
from test_uvdiag_ref import slot, small_basin, started

STATIC = ("pm", "pn", "ptide", "dn_u", "dm_v", "umask", "vmask", "rmask")
LEVELS = ("z_r", "z_w", "Hz", "rho1", "qp1", "rho", "FlxU", "FlxV")


def pflx_state(o, cfg, tix):
    """What the restatement reads of the corrector's entry state (host layout, copies)."""
    s = {n: o.field(n)[0].copy() for n in STATIC}
    s.update({n: o.field(n).copy() for n in LEVELS})
    for c in "uv":
        s[c + "_rhs"] = slot(o.field(c), cfg.N, tix[4]).copy()
    return s


def alpha_of(cfg, timescale=0.0):
    return cfg.dt / (timescale if timescale > 0 else pr.TIMESCALE)


def restated(cfg, s, st, timescale=0.0, **kw):
    return pr.corrector(s, st, cfg.LLm, cfg.MMm, cfg.rho0, bool(cfg.nonlin_eos), bool(cfg.pot_tides),
                        alpha_of(cfg, timescale), **kw)


@pytest.fixture(scope="module")
def basin():
    cfg = small_basin()
    o = started(cfg)
    tix = bs.set_mode(o, "corr")
    return cfg, pflx_state(o, cfg, tix)


def test_constant_density_gives_the_hydrostatic_line(basin):
    cfg, s0 = basin
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    R0 = 3.25
    for split in (True, False):
        s = dict(s0, rho1=np.full_like(s0["rho1"], R0), qp1=np.zeros_like(s0["qp1"]), rho=np.full_like(s0["rho"], R0))
        P = pr.pressure(s, L, M, cfg.rho0, split, False)
        r, c = slice(1, M + 2), slice(1, L + 2)
        zw = s["z_w"][N][r, c]
        tol = (N + 2) * np.spacing(np.abs(P).max())
        for k in range(N):
            want = pr.G * zw + (pr.G / cfg.rho0) * R0 * (zw - s["z_r"][k][r, c])
            err = np.abs(P[k][r, c] - want).max()
            print("split %d level %d: %.3e of %.3e" % (split, k + 1, err, tol))
            assert err <= tol
        z = P.copy()
        z[:, r, c] = 0
        assert not z.any()


def test_pot_tides_lower_the_surface_pressure_by_g_ptide(basin):
    cfg, s0 = basin
    x = np.linspace(0.0, 1.0, cfg.LLm + 4)
    s = dict(s0, ptide=0.3 * np.sin(6.0 * x)[None, :] * np.ones((cfg.MMm + 4, 1)))
    a = pr.pressure(s, cfg.LLm, cfg.MMm, cfg.rho0, True, False)
    b = pr.pressure(s, cfg.LLm, cfg.MMm, cfg.rho0, True, True)
    r, c = slice(1, cfg.MMm + 2), slice(1, cfg.LLm + 2)
    assert np.array_equal(b[-1][r, c], a[-1][r, c] - pr.G * s["ptide"][r, c]) and not np.array_equal(a, b)


def test_alpha_one_leaves_no_fast_part(basin):
    cfg, s = basin
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    st = pr.zero_state(N, L, M)
    st["p_slow"][...] = 7.0   # forgotten at once: beta = 0 (inside the range; outside it stays)
    st["p_slow"][:, :1], st["p_slow"][:, M + 2:], st["p_slow"][:, :, :1], st["p_slow"][:, :, L + 2:] = 0, 0, 0, 0
    up, vp = restated(cfg, s, st, timescale=cfg.dt)
    P = pr.pressure(s, L, M, cfg.rho0, True, False)
    Uflx, Vflx = pr.barotropic(s, L, M)
    assert np.array_equal(st["p_slow"], P) and np.abs(P).max() > 0
    ju, iu = slice(2, M + 2), slice(2, L + 3)
    jv, iv = slice(2, M + 3), slice(2, L + 2)
    for k in range(N):
        assert np.array_equal(st["u_slow"][k][ju, iu], (s["u_rhs"][k] - Uflx)[ju, iu])
        assert np.array_equal(st["v_slow"][k][jv, iv], (s["v_rhs"][k] - Vflx)[jv, iv])
    assert np.abs(st["u_slow"]).max() > 0 and np.abs(st["v_slow"]).max() > 0
    assert not up.any() and not vp.any()


def test_baroclinic_velocity_carries_no_transport(basin):
    """With FlxU = 0.5*(Hz(i)+Hz(i-1))*dn_u*u (set_HUV), sum_k (u - Uflx)*(Hz(i-1)+Hz(i)) = 0 up to rounding.
    Roundings: three a term of FlxU, N-1 of its sum, five of the division into a velocity, two of dn_u =
    2/(pn+pn), N of sum Hz against z_w(N)-z_w(0), and per level three of the product below plus the N-1 of its sum:
    below (3N + 16) ulp of S = sum_k (|u| + |Uflx|)*(Hz(i-1)+Hz(i))."""
    cfg, s0 = basin
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    j, i, im = slice(2, M + 2), slice(2, L + 3), slice(1, L + 2)
    s = dict(s0)
    s["FlxU"] = np.zeros_like(s0["FlxU"])
    for k in range(N):
        s["FlxU"][k][j, i] = 0.5 * (s["Hz"][k][j, i] + s["Hz"][k][j, im]) * s["dn_u"][j, i] * s["u_rhs"][k][j, i]
    Uflx, _ = pr.barotropic(s, L, M)
    tot, S = np.zeros((M, L + 1)), np.zeros((M, L + 1))
    for k in range(N):
        hz = s["Hz"][k][j, im] + s["Hz"][k][j, i]
        tot = tot + (s["u_rhs"][k][j, i] - Uflx[j, i]) * hz
        S = S + (np.abs(s["u_rhs"][k][j, i]) + np.abs(Uflx[j, i])) * hz
    assert np.abs(Uflx).max() > 0
    ulps = (np.abs(tot)[S > 0] / (np.finfo(float).eps * S[S > 0])).max()
    print("residual transport: %.2f eps of S (bound %d)" % (ulps, 3 * N + 16))
    assert ulps <= 3 * N + 16


def test_the_comparison_sees_a_shifted_p_fast_and_a_top_down_sum(basin):
    cfg, s = basin
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    runs = {}
    for name, kw in (("right", {}), ("shifted", dict(p_shift=1)), ("top down", dict(top_down=True))):
        st = pr.zero_state(N, L, M)
        for _ in range(3):
            up, vp = restated(cfg, s, st, **kw)
        runs[name] = (up, vp)
    up = runs["right"][0]
    assert np.abs(up).max() > 0 and np.abs(runs["right"][1]).max() > 0
    for name in ("shifted", "top down"):
        n = int((runs[name][0] != up).sum())
        print("%s: up differs at %d of %d points" % (name, n, L * M))
        assert n > 0
    z = up.copy()
    z[2:M + 2, 2:L + 2] = 0
    assert not z.any()
