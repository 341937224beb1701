"""Baroclinic pressure fluxes on the device (roms_gpu_pflx_*, k_pflx.hip) against the numpy restatement of
calc_pressure_flux and prsgrd's P (tests/pflx_ref.py, held to its own checks by tests/test_pflx_ref.py).

The corrector's entry state comes from the CPU oracle and is handed over; every m.prsgrd() with the corrector's
indices is then followed by the two launches, and up, vp, u_slow, v_slow, p_slow are compared with np.array_equal
over the whole arrays, the zeros outside the ranges included, after each of three consecutive calls (from the
second on the filters carry state)."""
import numpy as np
import pytest

import branch_states as bs
import oracle
import pflx_ref as pr
import romsgpu
from test_gpu_branches import hand_over, obc_model
from test_gpu_dropin import dropin_step
from test_gpu_io import BASIN_LMD, FIL
from test_gpu_multirank import run_decomposed
from test_gpu_obc import obc_cfg
from test_gpu_tdiag import model_of
from test_pflx_ref import alpha_of, pflx_state, restated
from test_uvdiag_ref import VISC2, small_basin, started, stirred_filament

pytestmark = pytest.mark.gpu

NAMES = ("up", "vp", "u_slow", "v_slow", "p_slow")
SMALL = dict(BASIN_LMD, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)


def five(m):
    return {n: m.pflx(n) for n in NAMES}


def same(got, want, what=""):
    for n in NAMES:
        g, w = got[n], want[n]
        assert g.shape == w.shape, (what, n)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d points differ, first index %s, max |diff| %.3e of %.3e"
                                 % (what, n, len(bad), bad[0], np.abs(g - w).max(), np.abs(w).max()))


def run_case(cfg, o=None, model=None, timescale=0.0, calls=3, handed=None):
    """Three corrector prsgrd calls on the oracle's state; returns the last five arrays and the state."""
    o = o or started(cfg)
    tix = bs.set_mode(o, "corr")
    s = pflx_state(o, cfg, tix)
    st = pr.zero_state(cfg.N, cfg.LLm, cfg.MMm)
    m = model(cfg) if model else model_of(cfg)
    try:
        if handed:
            m.set_tindex(*tix, nfast=o.nfast())
        else:
            hand_over(o, m, tix)
        m.pflx_begin(timescale)
        assert m.pflx_state() == (True, alpha_of(cfg, timescale), 0)
        for n in range(1, calls + 1):
            m.prsgrd()
            m.sync()
            up, vp = restated(cfg, s, st, timescale)
            got = five(m)
            same(got, dict(st, up=up, vp=vp), "call %d" % n)
            assert m.pflx_state()[2] == n
        assert m.pflx_path() == (0, calls)   # the grid came through a host write: the streaming form
        for n in NAMES:
            assert np.abs(got[n]).max() > 0, n
        return got, s
    finally:
        m.close()


def test_closed_basin():
    got, s = run_case(small_basin())
    # up(2,:) reads p_fast(1,:), the first column prsgrd itself writes at the wall; up(1,:) = u_fast(1,:)*.. is 0 at a
    # closed wall (u = FlxU = 0 there), so the column formed at i = 0 shows in p_slow(0,:,:) -- the edge deviation
    assert np.abs(got["up"][:, 3]).max() > 0
    assert not got["up"][:, 2].any()
    assert np.abs(got["p_slow"][:, 1:13, 1]).max() > 0


def test_other_timescale():
    run_case(small_basin(), timescale=600.0)


def test_periodic_filament():
    cfg, o = stirred_filament(FIL["LLm"], FIL["MMm"], FIL["N"])
    assert not cfg.nonlin_eos   # the branch without SPLIT_EOS, on rho
    got, _ = run_case(cfg, o=o, model=lambda c: romsgpu.Model.from_case(**FIL))
    assert np.abs(got["up"][:, 2]).max() > 0   # i = 1 of the periodic grid: p_fast(0,:) is the seam's


def test_island():
    _, s = run_case(small_basin(island=1))
    assert (s["umask"][2:13, 3:38] == 0).any()


def test_curvgrid():
    _, s = run_case(small_basin(curvgrid=1))
    assert np.ptp(s["pm"][2:13, 5]) > 0


def test_rough_metrics():
    import metrics
    cfg = small_basin(curvgrid=1)
    o = oracle.Oracle(cfg)
    o.init()
    o.field("visc2_r")[...] = VISC2
    o.field("visc2_p")[...] = VISC2
    metrics.apply_grid(o, None, metrics.rough(cfg.LLm, cfg.MMm))
    o.step(3)
    run_case(cfg, o=o)


def test_open_boundaries():
    cfg = obc_cfg(obc=15, island=0, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)
    got, _ = run_case(cfg, model=obc_model)
    assert np.abs(got["up"][:, 2]).max() > 0   # the open western edge: u(1,:) flows, up(1,:) reads p_fast(0,:)


def test_pot_tides():
    from test_gpu_register import _ptide, host_model
    cfg = small_basin(pot_tides=1)
    o = oracle.Oracle(cfg)
    o.init()
    o.field("ptide")[...] = _ptide(o)
    o.step(3)
    got, s = run_case(cfg, o=o, model=lambda c: host_model(o, c)[0], handed=True)
    st = pr.zero_state(cfg.N, cfg.LLm, cfg.MMm)
    cfg.pot_tides = 0
    for _ in range(3):
        restated(cfg, s, st)
    assert not np.array_equal(st["p_slow"], got["p_slow"])


def test_without_split_eos():
    cfg = small_basin()
    cfg.nonlin_eos = 0
    run_case(cfg)


@pytest.mark.parametrize("N", [2, 3, 5, 64])
def test_depths(N):
    run_case(small_basin(N=N) if N < 64 else small_basin(LLm=20, MMm=5, N=N))


@pytest.mark.parametrize("MMm", [3, 4, 5])
@pytest.mark.parametrize("LLm", [62, 63, 64, 65, 66])
def test_widths_and_heights(LLm, MMm):
    """64 consecutive i per wavefront from the line start at i = 1, four rows per block: the last column of p_slow
    (Lm), of u_slow (Lm+1) and the rows Mm, Mm+1 fall on either side of a wavefront and of a block."""
    run_case(small_basin(LLm=LLm, MMm=MMm, N=3), calls=2)


PATHS = []   # (formed, streamed) k_pflx_p launches of every stepped() model, in order


def stepped(case, n, arm=True, env=None, by_routine=False):
    m = romsgpu.Model.from_case(**case)
    try:
        if arm:
            m.pflx_begin()
        for _ in range(n):
            if by_routine:
                dropin_step(m, lmd=bool(case.get("lmd")))
            else:
                m.step()
        m.sync()
        PATHS.append(m.pflx_path())
        return five(m) if arm else None, {f: m.get(f) for f in ("u", "v", "t", "zeta")}, m.pflx_state()
    finally:
        m.close()


def test_formed_and_streamed_vertical_grid_give_the_same_bits(monkeypatch):
    a, _, st = stepped(SMALL, 3)
    assert st[0] and st[2] == 3
    f, s = PATHS[-1]
    assert f + s == 3 and f >= 2   # whole steps: the walks formed the grid (k_pflx_p<true>)
    monkeypatch.setenv("ROMS_GPU_VGRID", "0")
    monkeypatch.setenv("ROMS_GPU_VGRID2", "0")
    b, _, _ = stepped(SMALL, 3)
    assert PATHS[-1] == (0, 3)   # and streamed it here
    same(a, b, "VGRID=0")
    assert np.abs(a["up"]).max() > 0


def test_whole_steps_equal_steps_by_routine():
    a, fa, sa = stepped(SMALL, 4)
    b, fb, sb = stepped(SMALL, 4, by_routine=True)
    same(a, b, "by routine")
    assert sa == sb and sa[2] == 4 and np.abs(a["vp"]).max() > 0
    for n in fa:
        assert np.array_equal(fa[n], fb[n]), n


def test_not_armed_is_the_parent_behaviour(monkeypatch):
    def run(mode):
        m = romsgpu.Model.from_case(**SMALL)
        try:
            if mode != "never":
                m.pflx_begin()
            if mode == "disarmed":
                m.pflx_begin(on=False)
            if mode != "armed":
                assert m.pflx_state() == (False, 0.0, 0)
                a = np.empty(m.shape2[0] * m.shape2[1])
                assert m.L.roms_gpu_pflx_copy_out(1, a.ctypes.data, a.size) == -4
                assert b"not armed" in m.L.roms_gpu_last_error()
                with pytest.raises(romsgpu.RomsGpuError):
                    m.pflx("up")
            m.step(3)
            return {n: m.get(n) for n in ("u", "v", "t", "zeta", "rho")}
        finally:
            m.close()

    never, disarmed, armed = run("never"), run("disarmed"), run("armed")
    for n in never:
        assert np.array_equal(never[n], disarmed[n]) and np.array_equal(never[n], armed[n]), n
    monkeypatch.setenv("ROMS_GPU_NO_GRAPH", "1")
    enq = run("never")
    for n in never:
        assert np.array_equal(never[n], enq[n]), n


def test_refusals_and_copy_in():
    m = romsgpu.Model.from_case(**SMALL)
    E = lambda: m.L.roms_gpu_last_error()
    ms = (romsgpu.ctypes.c_double * 2)()
    a2 = np.zeros(m.shape2)
    a3 = np.zeros((m.N,) + m.shape2)
    try:
        assert m.L.roms_gpu_time_pflx(1, ms) == -4 and b"not armed" in E()
        assert m.L.roms_gpu_pflx_copy_in(3, a3.ctypes.data, a3.size) == -4 and b"not armed" in E()
        m.pflx_begin()
        assert m.L.roms_gpu_pflx_copy_out(0, a2.ctypes.data, a2.size) == -1 and b"ROMS_PFLX" in E()
        assert m.L.roms_gpu_pflx_copy_out(6, a2.ctypes.data, a2.size) == -1
        assert m.L.roms_gpu_pflx_copy_out(1, a2.ctypes.data, a2.size - 1) == -1 and b"count" in E()
        assert m.L.roms_gpu_pflx_copy_out(5, a2.ctypes.data, a2.size) == -1 and b"count" in E()
        assert m.L.roms_gpu_pflx_copy_in(1, a2.ctypes.data, a2.size) == -1 and b"results" in E()
        assert m.L.roms_gpu_time_pflx(0, ms) == -1
        # the predictor's prsgrd never filters
        m.t.nstp = m.t.nrhs = 1
        m.prsgrd()
        m.sync()
        assert m.pflx_state()[2] == 0 and not m.pflx("p_slow").any()
        rng = np.random.default_rng(5)
        for n in ("u_slow", "v_slow", "p_slow"):
            a = rng.standard_normal(a3.shape)
            m.pflx_set(n, a)
            assert np.array_equal(m.pflx(n), a), n
        assert m.time_pflx(2)[0] > 0
    finally:
        m.close()


def joined(parts, name, L, M, lev):
    """The ranks' arrays of `name` put together over their own ranges (this rank's 0.. or 1.. to its Lm, Mm [+1])."""
    out = np.zeros(((lev,) if lev else ()) + (M + 4, L + 4))
    i0 = j0 = 0 if name == "p_slow" else 1
    for iSW, jSW, Lm, Mm, _, got in parts:
        i1 = Lm + 1 if name == "u_slow" else Lm
        j1 = Mm + 1 if name == "v_slow" else Mm
        a = got[name]
        z = a.copy()
        z[..., j0 + 1:j1 + 2, i0 + 1:i1 + 2] = 0
        assert not z.any(), (name, iSW, jSW)
        dst = out[..., jSW + j0 + 1:jSW + j1 + 2, iSW + i0 + 1:iSW + i1 + 2]
        src = a[..., j0 + 1:j1 + 2, i0 + 1:i1 + 2]
        # where two ranks hold the same point (p_slow's column 0, u_slow's Lm+1) they hold the same bits
        seen = dst != 0
        assert np.array_equal(dst[seen], src[seen]), (name, iSW, jSW)
        dst[...] = src
    return out


@pytest.mark.parametrize("npx,npe", [(2, 2), (1, 3)])
def test_decomposition_bitwise(npx, npe):
    case = dict(BASIN_LMD, N=6)
    ref, _, st = stepped(case, 3)
    assert st[2] == 3
    parts, _ = run_decomposed(case, npx, npe, 3, fields=("zeta",), probe=five, setup=lambda m: m.pflx_begin())
    for n in NAMES:
        got = joined(parts, n, case["LLm"], case["MMm"], 0 if n in ("up", "vp") else case["N"])
        if not np.array_equal(got, ref[n]):
            bad = np.argwhere(got != ref[n])
            raise AssertionError("%s: %d points differ, first %s" % (n, len(bad), bad[0]))
        assert np.abs(got).max() > 0


# ---------------------------------------------------------------- restart
def test_restart_carries_the_filters(tmp_path):
    """Four uninterrupted steps against two steps, a restart file, a fresh model and two more: up, vp and the three
    filter states are the same bits; the file holds the three variables with the reference's dimensions."""
    from test_gpu_io import read, slab
    ref, _, _ = stepped(SMALL, 4)
    p = str(tmp_path / "rst.nc")
    b = romsgpu.Model.from_case(**SMALL)
    b.pflx_begin()
    b.step(1)
    b.wrt_rst(p, 1, 1, b.time(SMALL["dt"]))   # EXACT_RESTART: the step before ...
    b.step(1)
    b.wrt_rst(p, 2, 2, b.time(SMALL["dt"]))   # ... and the restart record
    b.io_wait()
    kept = five(b)
    L, M, N = b.Lm, b.Mm, b.N
    b.close()
    d = read(p)
    for n, g in (("u_slow", "u"), ("v_slow", "v"), ("p_slow", "r")):
        assert np.array_equal(d[n][1], slab(kept[n], g, L, M)), n
        assert np.abs(d[n][1]).max() > 0
    from scipy.io import netcdf_file
    with netcdf_file(p, "r", mmap=False) as nc:
        v = nc.variables
        assert v["u_slow"].dimensions == ("time", "s_rho", "eta_rho", "xi_u") and v["u_slow"].typecode() == "d"
        assert v["v_slow"].dimensions == ("time", "s_rho", "eta_v", "xi_rho") and v["v_slow"].typecode() == "d"
        assert v["p_slow"].dimensions == ("time", "s_rho", "eta_rho", "xi_rho") and v["p_slow"].typecode() == "d"
        assert v["u_slow"].long_name == b"time filtered u" and v["u_slow"].units == b"m/s"
        assert v["v_slow"].long_name == b"time filtered v" and v["v_slow"].units == b"m/s"
        assert v["p_slow"].long_name == b"time filtered pressure" and v["p_slow"].units == b"Pa??"
        assert v["p_slow"].shape[1:] == (N, M + 2, L + 2)
    c = romsgpu.Model.from_case(**SMALL)
    try:
        c.pflx_begin()
        c.restart(p)
        assert c.t.forw_start == 1 and c.t.iic == 2
        got0 = five(c)
        for n in ("u_slow", "v_slow", "p_slow"):   # the closed basin has no land: what was written is what is read
            assert np.array_equal(got0[n], kept[n]), n
        c.step(2)
        c.sync()
        same(five(c), ref, "restarted")
    finally:
        c.close()


def test_restart_file_without_the_filters_and_not_armed_file(tmp_path):
    """A file written while not armed has no filter variable and is today's; read while armed it gives the
    documented fallback -- u_slow = u(tindx), v_slow = v(tindx) over their write ranges, p_slow = 0 -- and a
    message that names it, while the call succeeds."""
    from test_gpu_io import read, slab
    p = str(tmp_path / "rst_plain.nc")
    b = romsgpu.Model.from_case(**SMALL)
    b.step(2)
    b.wrt_rst(p, 1, 1, b.time(SMALL["dt"]))
    b.io_wait()
    b.close()
    d = read(p)
    assert not {"u_slow", "v_slow", "p_slow"} & set(d)
    c = romsgpu.Model.from_case(**SMALL)
    try:
        c.pflx_begin()
        c.pflx_set("p_slow", np.ones((c.N,) + c.shape2))
        assert c.get_init(p, 1, 1) == 0
        msg = c.L.roms_gpu_last_error()
        assert b"u_slow (initialised to u)" in msg and b"v_slow (initialised to v)" in msg
        assert b"p_slow (initialised to 0.0)" in msg and b"WARNING" in msg
        L, M, N = c.Lm, c.Mm, c.N
        got = five(c)
        assert not got["p_slow"].any()
        for n, f in (("u_slow", "u"), ("v_slow", "v")):
            a = c.get(f)[:N]   # tindx = 1
            assert np.array_equal(slab(got[n], f, L, M), slab(a, f, L, M)) and np.abs(got[n]).max() > 0, n
            assert np.array_equal(slab(got[n], f, L, M), d[f][0]), n
            z = got[n].copy()
            slab(z, f, L, M)[...] = 0
            assert not z.any(), n
    finally:
        c.close()


# ---------------------------------------------------------------- extraction
def line_objects():
    k = np.arange(12.0)
    ang = lambda n, a0: a0 + 0.11 * np.arange(n)
    return [("grid1_south_u", 3.75 + k, np.full(12, 3.375), ang(12, 0.2), "up, vp"),
            ("grid1_west_v", np.full(8, 0.25), 0.625 + np.arange(8.0), ang(8, -0.4), "vp")]


def extract_formula(m, iobj, ipos, jpos, upe, vpe, umask, vmask):
    """extract_data.F:764-770, 815-821 over upe, vpe: (up, vp) of an object's points."""
    from test_gpu_extract import compute_coef, interp
    ipu, jpu, cfu = compute_coef(ipos + 1.0, jpos + 0.5, umask)     # absolute -> rho index -> u index
    ipv, jpv, cfv = compute_coef(ipos + 0.5, jpos + 1.0, vmask)
    li, lj, lc, cosa, sina = m.extract_coef(iobj, "u")
    assert np.array_equal(li, ipu) and np.array_equal(lj, jpu) and np.array_equal(lc, cfu, equal_nan=True)
    li, lj, lc, _, _ = m.extract_coef(iobj, "v")
    assert np.array_equal(li, ipv) and np.array_equal(lj, jpv) and np.array_equal(lc, cfv, equal_nan=True)
    ui, vi = interp(upe, ipu, jpu, cfu), interp(vpe, ipv, jpv, cfv)
    return cosa * ui - sina * vi, sina * ui + cosa * vi


def test_extraction_of_a_rotated_line_and_its_file(tmp_path):
    cfg = small_basin()
    o = started(cfg)
    tix = bs.set_mode(o, "corr")
    s = pflx_state(o, cfg, tix)
    st = pr.zero_state(cfg.N, cfg.LLm, cfg.MMm)
    objs = line_objects()
    m = model_of(cfg)
    try:
        hand_over(o, m, tix)
        m.extract_begin(cfg.N, cfg.theta_s, cfg.theta_b, cfg.hc)
        # not armed at the time the object is added: unsupported, today's message
        m.extract_add("early_south_u", objs[0][1], objs[0][2], "up", ang=objs[0][3])
        assert b"not produced here" in m.L.roms_gpu_last_error() and b"up" in m.L.roms_gpu_last_error()
        m.pflx_begin()
        info = m.extract_info(1)   # armed afterwards: it stays as it was added
        assert info["unsupported"] == ("up",) and info["vars"] == ("u",)
        with pytest.raises(romsgpu.RomsGpuError, match="scalar"):
            m.extract_add("grid1_east_r", objs[0][1], objs[0][2], "up")
        for name, ip, jp, ang, ov in objs:
            m.extract_add(name, ip, jp, ov, ang=ang)
        assert set(m.extract_info(2)["vars"]) == {"u", "v", "up", "vp"} and m.extract_info(2)["unsupported"] == ()
        assert set(m.extract_info(3)["vars"]) == {"v", "vp"}
        for _ in range(2):
            m.prsgrd()
            m.sync()
            up, vp = restated(cfg, s, st)
        m.calc_extract()
        for q, (name, ip, jp, ang, ov) in enumerate(objs):
            wu, wv = extract_formula(m, q + 2, ip, jp, up, vp, s["umask"], s["vmask"])
            if "up" in m.extract_info(q + 2)["vars"]:
                g = m.extract(q + 2, "up")
                assert np.array_equal(g, wu) and np.abs(g).max() > 0, name
            g = m.extract(q + 2, "vp")
            assert np.array_equal(g, wv) and np.abs(g).max() > 0, name
        p = str(tmp_path / "ext.nc")
        m.wrt_extract(p, 1, 1, 100.0)
        m.io_wait()
        from scipy.io import netcdf_file
        with netcdf_file(p, "r", mmap=False) as nc:
            v = nc.variables["grid1_up_south"]
            assert v.dimensions == ("time_early", "np002") and v.typecode() == "d"
            assert v.long_name == b"pressure flux" and v.units == b"W/m^2"
            assert (int(v.start), int(v.count), int(v.dsize)) == (1, 12, 12)
            assert np.array_equal(v[0], m.extract(2, "up"))
            assert nc.variables["grid1_vp_west"].dimensions == ("time_early", "np003")
            assert np.array_equal(nc.variables["grid1_vp_south"][0], m.extract(2, "vp"))
            assert "early_up_south" not in nc.variables
        # disarmed while an object still asks for up, vp: a sample refuses
        m.pflx_begin(on=False)
        with pytest.raises(romsgpu.RomsGpuError, match="disarmed"):
            m.calc_extract()
    finally:
        m.close()


def test_extraction_across_rank_edges_joins_to_the_single_domain():
    """The periodic filament, 2 x 2: lines that cross both rank edges and lie next to the seams, so that upe, vpe
    are read across the exchanged halos; the single domain is checked against the formula over its own up, vp
    (tests above hold those to the restatement), the pieces against the single domain."""
    import threading
    L, M = FIL["LLm"], FIL["MMm"]
    k, kj = np.arange(L - 1.0), np.arange(M - 1.0)
    ang = lambda n, a0: a0 + 0.07 * np.arange(n)
    objs = [("chd_mid_u", 0.75 + k, np.full(k.size, 14.75), ang(k.size, 0.5), "up, vp"),
            ("chd_west_v", np.full(kj.size, 19.75), 1.125 + kj, ang(kj.size, -1.1), "up, vp"),
            ("chd_south_u", 0.25 + k, np.full(k.size, 0.375), ang(k.size, 0.1), "up, vp")]

    def sample(mm, whole=False):
        mm.pflx_begin()
        mm.extract_begin(FIL["N"], 6.0, 2.0, 25.0)
        for name, ip, jp, a, ov in objs:
            mm.extract_add(name, ip, jp, ov, ang=a)
        mm.step(3)
        mm.calc_extract()
        out = {}
        for q in range(len(objs)):
            info = mm.extract_info(q + 1)
            out[q] = (info["start_idx"], info["np"], {v: mm.extract(q + 1, v) for v in ("up", "vp")} if info["np"] else {})
        if whole:
            def wrapped(a):
                a = a.copy()
                a[:, 0:2], a[:, L + 2:] = a[:, L:L + 2], a[:, 2:4]
                a[0:2, :], a[M + 2:, :] = a[M:M + 2, :], a[2:4, :]
                return a
            ones = np.ones((M + 4, L + 4))
            upe, vpe = wrapped(mm.pflx("up")), wrapped(mm.pflx("vp"))
            for q, (name, ip, jp, a, ov) in enumerate(objs):
                wu, wv = extract_formula(mm, q + 1, ip, jp, upe, vpe, ones, ones)
                assert np.array_equal(out[q][2]["up"], wu) and np.array_equal(out[q][2]["vp"], wv), name
                assert np.abs(wu).max() > 0 and np.abs(wv).max() > 0
        mm.close()
        return out

    ref = sample(romsgpu.Model.from_case(**FIL), whole=True)
    npx, npe = 2, 2
    parts, errs = {}, []

    def work(rank):
        try:
            h = romsgpu.comm_create_local(787, npx * npe, rank)
            parts[rank] = sample(romsgpu.Model.from_case(np_xi=npx, np_eta=npe, comm=h, rank=rank, **FIL))
            romsgpu.comm_destroy(h)
        except Exception as e:
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(npx * npe)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
    assert not errs, errs
    for q, (name, gi, gj, a, ov) in enumerate(objs):
        s0, n0, whole = ref[q]
        assert (s0, n0) == (1, gi.size)
        for v, w in whole.items():
            glob = np.full(w.shape, np.nan)
            cover = np.zeros(gi.size, int)
            for r in range(npx * npe):
                s_, n, piece = parts[r][q]
                if n:
                    glob[s_ - 1:s_ - 1 + n] = piece[v]
                    cover[s_ - 1:s_ - 1 + n] += 1
            assert (cover == 1).all(), (name, cover)
            assert np.array_equal(glob, w), (name, v)
