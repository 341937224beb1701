"""Tracer budget terms on the device (DIAGNOSTICS with diag_trc): k_tdiag_snap, k_tdiag_h,
k_tdiag_v with their sinks, the C entries, Model.tdiag*, the diagnostics file.

The expected values never come from the library's own terms: they are the numpy restatement tests/tdiag_ref.py over
the corrector's entry state (taken from the CPU oracle at the corrector stage, as tests/test_gpu_branches.py takes
its states), the downloaded ROMS_TDIA_SNAP and the downloaded t(nnew).  The kernels evaluate the reference's
operations in the reference's order without contraction, so all six terms are compared with np.array_equal on whole
arrays, the zeros outside the written ranges included.  The budget closure is a check of its own, independent of
the restatement.
"""
import os
import threading

import numpy as np
import pytest

import branch_states as bs
import oracle
import romsgpu
import tdiag_ref
from test_gpu_branches import hand_over
from test_gpu_depths import depth_cfg
from test_gpu_io import BASIN_LMD, FIL, read, slab
from test_gpu_multirank import run_decomposed
from test_gpu_parity import RTOL_ROUTINE, basin_cfg
from test_tdiag_ref import stirred_filament

pytestmark = pytest.mark.gpu

TERMS = ("advx", "advy", "advz", "mixx", "mixy", "mixz")
CLOSURE_ULPS = 32   # the issue's bound; the restatement alone stays within 1 ulp of it on the CPU (test_tdiag_ref.py)


def small_basin(LLm=36, MMm=11, N=5, **kw):
    c = basin_cfg(nonlin=True, LLm=LLm, MMm=MMm, N=N, NT=2, sizex=2.0e3 * LLm, sizey=2.0e3 * MMm)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def model_of(cfg):
    return romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                   nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex,
                                   sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux),
                                   island=bool(cfg.island), curvgrid=bool(cfg.curvgrid))


def slot(a, N, itrc, l):
    q = (itrc - 1) * 3 + (l - 1)
    return a[q * N:(q + 1) * N]


def corrector_state(cfg, o=None):
    """The oracle after 3 steps with the corrector's indices, and copies of what the restatement reads."""
    if o is None:
        o = oracle.Oracle(cfg)
        o.init()
        o.step(3)
    tix = bs.set_mode(o, "corr")
    E = {n: o.field(n).copy() for n in ("t", "FlxU", "FlxV", "We", "Hz", "pm", "pn", "umask", "vmask", "rmask", "z_w")}
    return o, tix, E


def sample_and_check(m, cfg, tix, E, tracers, per=False, rivers=None, closure=True):
    """After m.step3d_t() on the handed-over state: every armed tracer's six terms equal the restatement; the
    closure and the snapshot checks.  Returns {itrc: {term: array}}."""
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    nrhs, nnew = tix[4], tix[5]
    tnew_all = m.get("t")
    out = {}
    r, c = slice(2, M + 2), slice(2, L + 2)
    pm, pn = E["pm"][0], E["pn"][0]
    water = E["rmask"][0][r, c] > 0
    for itrc in tracers:
        got = {k: m.tdiag(itrc, k) for k in TERMS + ("snap",)}
        tr, te, tn = slot(E["t"], N, itrc, nrhs), slot(E["t"], N, itrc, nnew), slot(tnew_all, N, itrc, nnew)
        want = tdiag_ref.terms(tr, E["FlxU"], E["FlxV"], E["We"], E["Hz"], pm, pn, E["umask"][0], E["vmask"][0],
                               got["snap"], tn, cfg.dt, per, per, rivers=rivers, itrc=itrc, z_w=E["z_w"])
        for k in TERMS:
            assert got[k].shape == (N, M + 4, L + 4)
            if not np.array_equal(got[k], want[k]):
                bad = np.argwhere(got[k] != want[k])
                raise AssertionError("tracer %d %s: %d cells differ, first (k, j, i) index %s, max |diff| %.3e"
                                     % (itrc, k, len(bad), bad[0], np.abs(got[k] - want[k]).max()))
            assert np.abs(got[k]).max() > 0 or k in ("mixx", "mixy"), (itrc, k)
        # the snapshot is t(nnew) after the horizontal update: t_entry - dt*pm*pn*div(FX, FE)
        FX, FE = want["FX"], want["FE"]
        S = te[:, r, c] - cfg.dt * pm[r, c] * pn[r, c] * (FX[:, r, 3:L + 3] - FX[:, r, c] + FE[:, 3:M + 3, c] - FE[:, r, c])
        e = np.abs(got["snap"][:, r, c] - S).max() / np.abs(S).max()
        print("tracer %d snapshot vs t_entry - dt*pm*pn*div(FX,FE): %.3e of the field scale" % (itrc, e))
        assert e <= RTOL_ROUTINE
        assert not got["snap"][:, 0].any() and not got["snap"][:, :, 0].any()
        if closure:   # independent of the restatement: the library's own terms close the budget
            res, scale = tdiag_ref.closure_residual(got, te, tn, E["Hz"], pm, pn, cfg.dt, L, M)
            ulps = (np.abs(res) / np.spacing(scale))[:, water]
            print("tracer %d closure: %.2f ulp of the largest term" % (itrc, ulps.max()))
            assert ulps.max() <= CLOSURE_ULPS
        out[itrc] = got
    return out


def leaky_walls(cfg):
    """The oracle after 3 steps with FlxU, FlxV of the wall faces 1, Lm+1 and 1, Mm+1 set to fractions of their
    inner neighbours': a closed basin has no flux there, and the lanes that own those faces would write the same
    zeros whatever they computed.  The terms are algebra over whatever fluxes the corrector is handed."""
    o = oracle.Oracle(cfg)
    o.init()
    o.step(3)
    L, M = cfg.LLm, cfg.MMm
    fu, fv = o.field("FlxU"), o.field("FlxV")
    fu[:, 2:M + 2, L + 2] = 0.5 * fu[:, 2:M + 2, L + 1]
    fu[:, 2:M + 2, 2] = -0.25 * fu[:, 2:M + 2, 3]
    fv[:, M + 2, 2:L + 2] = 0.5 * fv[:, M + 1, 2:L + 2]
    fv[:, 2, 2:L + 2] = -0.25 * fv[:, 3, 2:L + 2]
    return o


def run_case(cfg, tracers=(1, 2), per=False, model=None, leaky=False, o=None):
    o, tix, E = corrector_state(cfg, leaky_walls(cfg) if leaky else o)
    m = model(cfg) if model else model_of(cfg)
    try:
        hand_over(o, m, tix)
        m.tdiag_begin(tracers)
        assert m.tdiag_state() == (len(tracers), False, 0, True)
        m.step3d_t()
        m.sync()
        return sample_and_check(m, cfg, tix, E, tracers, per), E
    finally:
        m.close()


def test_closed_basin():
    got, _ = run_case(small_basin())
    L, M = 36, 11
    for itrc in (1, 2):
        g = got[itrc]
        # the wall faces 1, Lm+1 and Mm+1 carry no flux (the periodic case has values there); nothing beyond
        assert np.abs(g["advx"][:, 2:M + 2, L + 1]).max() > 0 and not g["advx"][:, :, L + 2:].any()
        assert not g["advx"][:, M + 2].any() and not g["advx"][:, :, :2].any() and not g["advx"][:, :2].any()
        assert np.abs(g["advy"][:, M + 1, 2:L + 2]).max() > 0 and not g["advy"][:, :, L + 2].any()
        assert not g["advz"][-1].any() and not g["advz"][:, :, L + 2].any() and not g["advz"][:, M + 2].any()
        assert np.abs(g["mixx"]).max() > 0 and np.abs(g["mixy"]).max() > 0 and np.abs(g["mixz"]).max() > 0


def test_closed_basin_with_flux_through_the_wall_faces():
    got, _ = run_case(small_basin(), leaky=True)
    L, M = 36, 11
    for itrc in (1, 2):
        g = got[itrc]
        assert np.abs(g["advx"][:, 2:M + 2, L + 2]).min() > 0 and np.abs(g["advx"][:, 2:M + 2, 2]).min() > 0
        assert np.abs(g["advy"][:, M + 2, 2:L + 2]).min() > 0 and np.abs(g["advy"][:, 2, 2:L + 2]).min() > 0
        assert not g["advx"][:, :, L + 3].any() and not g["advy"][:, M + 3].any()


def test_one_tracer_of_two_is_armed():
    got, _ = run_case(small_basin(), tracers=(2,))
    assert list(got) == [2]


def test_periodic_filament():
    cfg, o = stirred_filament(FIL["LLm"], FIL["MMm"], FIL["N"])
    got, _ = run_case(cfg, tracers=(1,), per=True, model=lambda c: romsgpu.Model.from_case(**FIL), o=o)
    L, M = FIL["LLm"], FIL["MMm"]
    g = got[1]
    # the written ranges: faces Lm+1 and Mm+1 hold values, the lines beyond and before nothing
    assert np.abs(g["advx"][:, 2:M + 2, L + 2]).max() > 0 and not g["advx"][:, :, L + 3].any()
    assert np.abs(g["mixx"][:, 2:M + 2, L + 2]).max() > 0 and not g["advx"][:, :, :2].any() and not g["advx"][:, M + 2].any()
    assert np.abs(g["advy"][:, M + 2, 2:L + 2]).max() > 0 and not g["advy"][:, M + 3].any()
    assert not g["advy"][:, :, L + 2].any() and not g["advz"][:, :, L + 2].any() and not g["advz"][:, M + 2].any()


def test_island_masked_faces():
    _, E = run_case(small_basin(island=1))
    assert (E["rmask"][0][2:13, 2:38] == 0).any() and (E["umask"][0][2:13, 2:39] == 0).any()


def test_curvgrid():
    _, E = run_case(small_basin(curvgrid=1))
    assert np.ptp(E["pm"][0][2:13, 5]) > 0 and np.ptp(E["pn"][0][5, 2:38]) > 0


def test_rough_metrics():
    """pm and pn vary along both axes (tests/metrics.py `rough`, every entry different from its neighbours): a term
    that reads pm or pn one cell off differs from the restatement."""
    import metrics
    cfg = small_basin()
    o = oracle.Oracle(cfg)
    o.init()
    metrics.apply_grid(o, None, metrics.rough(cfg.LLm, cfg.MMm))
    o.step(3)
    _, E = run_case(cfg, o=o)
    for n in ("pm", "pn"):
        assert metrics.neighbours_differ(E[n][0], (-1, cfg.MMm + 2, -1, cfg.LLm + 2)) == 0, n


def test_surface_and_nonlocal_terms_reach_mixz():
    got, _ = run_case(small_basin(lmd=oracle.LMD_ALL, surf_flux=1))
    plain, _ = run_case(small_basin())
    assert np.abs(got[1]["mixz"]).max() > 10 * np.abs(plain[1]["mixz"]).max()


def test_rivers_on_a_u_face_and_a_v_face():
    import coasts
    import rivers
    from test_gpu_rivers_sweep import NRIV, mouths_of, sweep_model
    from test_rivers import sweep_cfg
    size = (65, 9, 6)
    cfg = sweep_cfg(*size)
    o = oracle.Oracle(cfg)
    o.init()
    land, mouths = mouths_of("specks", size)
    trc = rivers.river_tracers(NRIV)
    _, uf, vf, vol = rivers.apply_rivers(o, None, land, mouths, None, trc, coasts.VISC)
    assert (np.abs(uf) > 1e-3).any() and (np.abs(vf) > 1e-3).any()
    o.step(3)
    o, tix, E = corrector_state(cfg, o)
    m = sweep_model(cfg)
    try:
        rivers.put_rivers(m, vol, trc, uf, vf)
        hand_over(o, m, tix)
        m.tdiag_begin((1, 2))
        m.step3d_t()
        m.sync()
        got = sample_and_check(m, cfg, tix, E, (1, 2), rivers=(uf, vf, vol, trc))
        # the override matters: without it the restatement is another field at the river faces
        tr = slot(E["t"], cfg.N, 1, tix[4])
        dry = tdiag_ref.horizontal(tr, E["FlxU"], E["FlxV"], E["umask"][0], E["vmask"][0], cfg.LLm, cfg.MMm, (True,) * 4)
        assert not np.array_equal(dry["mixx"], got[1]["mixx"]) and not np.array_equal(dry["mixy"], got[1]["mixy"])
    finally:
        m.close()


@pytest.mark.parametrize("MMm", [3, 4, 5])
@pytest.mark.parametrize("LLm", [63, 64, 65])
def test_widths_and_heights(LLm, MMm):
    """Lanes own faces from the line start at i = 1, 64 per wavefront, four rows per block: face Lm+1 lands on the
    last lane (63), on the next block (64) or mid-wavefront (65); row Mm+1 is the block's last row (3), the next
    block's first (4) or second (5)."""
    got, _ = run_case(small_basin(LLm=LLm, MMm=MMm, N=4), leaky=True)
    for i in (1, 2):
        assert np.abs(got[i]["advx"][:, 2:MMm + 2, LLm + 2]).min() > 0 and np.abs(got[i]["mixx"][:, 2:MMm + 2, LLm + 2]).max() > 0
        assert np.abs(got[i]["advy"][:, MMm + 2, 2:LLm + 2]).min() > 0 and np.abs(got[i]["mixy"][:, MMm + 2, 2:LLm + 2]).max() > 0
        assert np.abs(got[i]["mixz"][:, MMm + 1, LLm + 1]).max() > 0


_PATHS = {}


def column_path_of(N):
    """(segment solvers, global column scratch) the library chooses at depth N; it depends on N alone."""
    if N not in _PATHS:
        m = romsgpu.Model.from_case(1, 16, 4, N, 2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30, sizex=32e3,
                                    sizey=8e3)
        _PATHS[N] = m.column_path()
        m.close()
    return _PATHS[N]


def switch_depths():
    """Found, not assumed: the first depth whose column scratch lives in global memory (ColGlb; the one before it
    is the last on ColLds), by bisection -- the rule is a size threshold -- and the first depth from there on at
    which the corrector takes the segment solvers: a scan in steps of 8 (a narrower run of segment depths would be
    skipped), then bisection back to its first depth."""
    lo, hi = 4, 128
    assert not column_path_of(lo)[1] and column_path_of(hi)[1]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if column_path_of(mid)[1] else (mid, hi)
    glb = hi
    b = next(N for N in range(glb, 257, 8) if column_path_of(N)[0])
    a = b - 8
    while b - a > 1 and a >= glb:
        mid = (a + b) // 2
        a, b = (a, mid) if column_path_of(mid)[0] else (mid, b)
    return glb, b


@pytest.mark.parametrize("which", ["3", "4", "last ColLds", "first ColGlb", "first segments"])
def test_depths(which):
    """N = 3, 4: the shortest spline systems.  The last depth with the column scratch in LDS (ColLds) and the first
    with it in global memory (ColGlb): k_tdiag_v follows k_step3d_t_v's switch.  The first depth at which the
    corrector's own solve is the segment form (k_step3d_t_segb_pair): k_tdiag_v then runs on ColGlb next to it, the
    path a 100-level run takes."""
    glb, seg = switch_depths()
    N = {"last ColLds": glb - 1, "first ColGlb": glb, "first segments": seg}.get(which) or int(which)
    print("depth", which, N)
    path = column_path_of(N)   # ahead of the model under test: the library keeps one model per host thread
    cfg = depth_cfg(N)
    o, tix, E = corrector_state(cfg)
    m = model_of(cfg)
    try:
        assert m.column_path() == path == (which == "first segments", N >= glb)
        hand_over(o, m, tix)
        m.tdiag_begin((1, 2))
        m.step3d_t()
        m.sync()
        sample_and_check(m, cfg, tix, E, (1, 2))
    finally:
        m.close()


def six(m, itrc):
    return {k: m.tdiag(itrc, k) for k in TERMS}


def test_means_windows_and_sampling():
    """Three steps with avg equal the recurrence navg += 1, coef = 1/navg, X_avg = X_avg*(1-coef) + X*coef over the
    three plain samples of a twin model (the library keeps one model per host thread: the twin runs in a thread
    of its own); tdiag_sample(False) freezes the window."""
    case = dict(BASIN_LMD, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)
    samples, errs = [], []

    def twin():
        try:
            m = romsgpu.Model.from_case(**case)
            m.tdiag_begin((1, 2))
            for _ in range(3):
                m.step(1)
                samples.append({i: six(m, i) for i in (1, 2)})
            m.close()
        except Exception as e:
            errs.append(repr(e))

    th = threading.Thread(target=twin)
    th.start()
    th.join(timeout=240)
    assert not errs, errs
    m = romsgpu.Model.from_case(**case)
    try:
        m.tdiag_begin((1, 2), avg=True)
        avg = None
        for n in range(1, 4):
            m.step(1)
            coef, x = 1.0 / n, samples[n - 1]
            avg = x if avg is None else {i: {k: avg[i][k] * (1 - coef) + x[i][k] * coef for k in TERMS} for i in x}
            assert m.tdiag_state()[2] == n
            for i in (1, 2):
                for k in TERMS:
                    assert np.array_equal(m.tdiag(i, k), avg[i][k]), (n, i, k)
        assert not np.array_equal(avg[1]["advx"], samples[2][1]["advx"])
        m.tdiag_sample(False)   # calc_diag off: the window is frozen
        m.step(1)
        assert m.tdiag_state() == (2, True, 3, False)
        assert np.array_equal(m.tdiag(1, "mixz"), avg[1]["mixz"])
    finally:
        m.close()


def test_file_and_window_reset(tmp_path):
    from scipy.io import netcdf_file
    case = dict(BASIN_LMD, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)
    dt = case["dt"]
    p, q = str(tmp_path / "dia_avg.nc"), str(tmp_path / "dia.nc")
    m = romsgpu.Model.from_case(**case)
    try:
        L, M, N = m.Lm, m.Mm, m.N
        m.tdiag_begin((2, 1), avg=True)
        assert m.L.roms_gpu_wrt_tdiag(p.encode(), 1, 1, 0.0, 0.0, m.t) == -4   # no sample yet
        assert b"no sample" in m.L.roms_gpu_last_error() and not os.path.exists(p)
        wins = []
        for rec, nsamp in ((1, 2), (2, 1)):
            m.step(nsamp)
            assert m.tdiag_state()[2] == nsamp
            wins.append({i: six(m, i) for i in (1, 2)})
            m.wrt_tdiag(p, rec, rec, m.time(dt), nsamp * dt)
            assert m.tdiag_state()[2] == 0   # the window is reset
        assert m.L.roms_gpu_wrt_tdiag(p.encode(), 3, 3, 0.0, 0.0, m.t) == -4
        m.io_wait()
        # the second window starts clean: one sample, equal to a plain sample of the same step
        d = read(p)
        with netcdf_file(p, "r", mmap=False) as nc:
            names = [n for n in nc.variables if "_" in n and n.split("_")[0] in ("temp", "salt")]
            assert names == [t + s for t in ("salt", "temp") for s in ("_advx", "_advy", "_advz", "_mixx", "_mixy", "_mixz")]
            v = nc.variables["temp_mixz"]
            assert (v.long_name, v.units) == (b"mixing z-flux", b"C m^3/s")
            assert nc.variables["salt_advx"].long_name == b"x-advective flux"
            assert v.dimensions == ("time", "s_rho", "eta_rho", "xi_rho") and v.shape[1:] == (N, M + 2, L + 2)
            assert nc.diagnostic_options == b"Chosen Diagnostics = , Tracers"
            assert nc.diag_avg_time == b"120.0 seconds"
            assert np.array_equal(nc.variables["ocean_time"][:], [2 * dt, 3 * dt])
        for rec, w in enumerate(wins):
            for i, t in ((1, "temp"), (2, "salt")):
                for k in TERMS:
                    assert np.array_equal(d["%s_%s" % (t, k)][rec], slab(w[i][k], "r", L, M)), (rec, t, k)
        assert not np.array_equal(d["temp_advx"][0], d["temp_advx"][1]) and np.abs(d["temp_mixz"]).max() > 0
        # without avg: the last sample, no diag_avg_time
        m.tdiag_begin((1,))
        assert m.L.roms_gpu_wrt_tdiag(q.encode(), 1, 1, 0.0, 0.0, m.t) == -4
        m.step(1)
        x = six(m, 1)
        m.wrt_tdiag(q, 1, 1, m.time(dt))
        m.io_wait()
        d = read(q)
        assert np.array_equal(d["temp_advy"][0], slab(x["advy"], "r", L, M)) and "salt_advx" not in d
        with netcdf_file(q, "r", mmap=False) as nc:
            assert not hasattr(nc, "diag_avg_time")
    finally:
        m.close()


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "rim-first"])
def test_decomposition_bitwise(overlap, monkeypatch):
    """2 x 2 ranks on one GPU: every rank's terms are bitwise the single domain's over its own faces.  rim-first
    (ROMS_GPU_OVERLAP3D=1): launch_step3d_t's run() goes over five sub-ranges, the snapshot and the vertical terms
    with it."""
    if overlap:
        monkeypatch.setenv("ROMS_GPU_OVERLAP3D", "1")
    case = dict(BASIN_LMD, N=6)
    arm = lambda m: m.tdiag_begin((1, 2), avg=True)
    probe = lambda m: ({i: six(m, i) for i in (1, 2)}, m.tdiag_state())
    m = romsgpu.Model.from_case(**case)
    arm(m)
    m.step(3)
    ref, st = probe(m)
    m.close()
    assert st == (2, True, 3, True)
    parts, _ = run_decomposed(case, 2, 2, 3, fields=("t",), probe=probe, setup=arm)
    for rank, (iSW, jSW, Lm, Mm, _, (got, st)) in enumerate(parts):
        assert st == (2, True, 3, True)
        for i in (1, 2):
            for k in TERMS:
                ni, nj = Lm + (k in ("advx", "mixx")), Mm + (k in ("advy", "mixy"))
                g = got[i][k][:, 2:nj + 2, 2:ni + 2]
                w = ref[i][k][:, jSW + 2:jSW + nj + 2, iSW + 2:iSW + ni + 2]
                assert np.array_equal(g, w), (rank, i, k, float(np.abs(g - w).max()))
                assert np.abs(g).max() > 0
                z = got[i][k].copy()
                z[:, 2:nj + 2, 2:ni + 2] = 0
                assert not z.any(), (rank, i, k)


def test_not_armed_and_disarmed_change_nothing(monkeypatch):
    case = dict(BASIN_LMD, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)

    def run(mode):
        m = romsgpu.Model.from_case(**case)
        if mode != "never":
            m.tdiag_begin((1, 2), avg=True)
        if mode == "disarmed":
            m.tdiag_begin(())
            assert m.tdiag_state() == (0, False, 0, False)
        m.step(3)
        out = (m.get("t"), m.lean_stores(), m.tracer_pair(), m.tracer_hstg())
        m.close()
        return out

    never, disarmed, armed = run("never"), run("disarmed"), run("armed")
    assert np.array_equal(never[0], armed[0]) and np.array_equal(never[0], disarmed[0])
    assert never[1:] == disarmed[1:]
    # the armed run's counters: a replayed graph counts the launches of its capture only and an armed, sampling
    # run enqueues every step, so the two are compared with every step enqueued on both sides
    monkeypatch.setenv("ROMS_GPU_NO_GRAPH", "1")
    never, armed = run("never"), run("armed")
    assert np.array_equal(never[0], armed[0])
    assert never[1:] == armed[1:], (never[1:], armed[1:])
    assert sum(never[1][1]) + sum(never[2][2]) + sum(never[3][2]) > 0   # something was counted


def test_refusals():
    m = romsgpu.Model.from_case(**dict(BASIN_LMD, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3))
    E = lambda: m.L.roms_gpu_last_error()
    I = lambda *a: (romsgpu.ctypes.c_int * len(a))(*a)
    a = np.empty(m.N * m.shape2[0] * m.shape2[1])
    try:
        assert m.L.roms_gpu_tdiag_begin(1, I(3), 0) == -1 and b"outside 1..NT" in E()
        assert m.L.roms_gpu_tdiag_begin(1, I(0), 0) == -1 and b"outside 1..NT" in E()
        assert m.L.roms_gpu_tdiag_begin(2, I(1, 1), 0) == -1 and b"repeated" in E()
        assert m.tdiag_state() == (0, False, 0, False)
        assert m.L.roms_gpu_tdiag_sample(1) == -4 and b"not armed" in E()
        assert m.L.roms_gpu_tdiag_copy_out(1, 1, a.ctypes.data, a.size) == -1 and b"not armed" in E()
        m.tdiag_begin((2,))
        # a refused call leaves the arming as it was
        assert m.L.roms_gpu_tdiag_begin(2, I(1, 1), 1) == -1 and m.L.roms_gpu_tdiag_begin(1, I(3), 1) == -1
        assert m.tdiag_state() == (1, False, 0, True)
        assert m.L.roms_gpu_tdiag_copy_out(1, 1, a.ctypes.data, a.size) == -1 and b"not armed" in E()
        assert m.L.roms_gpu_tdiag_copy_out(2, 1, a.ctypes.data, a.size - 1) == -1 and b"count" in E()
        assert m.L.roms_gpu_tdiag_copy_out(2, 8, a.ctypes.data, a.size) == -1 and b"term" in E()
        with pytest.raises(ValueError):
            m.tdiag(2, "advw")
    finally:
        m.close()
    m = romsgpu.Model.from_case(**dict(FIL, adv_isoneutral=True))
    try:
        assert m.L.roms_gpu_tdiag_begin(1, I(1), 0) == -1 and b"adv_isoneutral" in E()
    finally:
        m.close()
