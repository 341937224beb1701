"""Momentum budget terms on the device (DIAGNOSTICS with diag_uv): the snapshots,
k_uvdiag_rhs, k_uvdiag_hmx, k_uvdiag_cpl with their sinks, the C entries, Model.uvdiag*, the diagnostics file.

The expected values never come from the library's own terms: they are the numpy restatement tests/uvdiag_ref.py over
the corrector's entry state (taken from the CPU oracle at the corrector stage, as tests/test_gpu_branches.py takes
its states) and the ru, rv, u, v(nnew) downloaded between the library's own prsgrd, step3d_uv1, visc3d and
step3d_uv2.  The kernels evaluate the reference's operations in the reference's order without contraction, so all
fourteen terms are compared with np.array_equal on whole arrays, the zeros outside the ranges included.  The budget
closure is a check of its own, independent of the restatement.
"""
import os
import threading

import numpy as np
import pytest

import branch_states as bs
import oracle
import romsgpu
import uvdiag_ref as ur
from test_gpu_branches import hand_over, obc_model
from test_gpu_depths import depth_cfg, depth_model
from test_gpu_io import BASIN_LMD, FIL, read, slab
from test_gpu_multirank import run_decomposed
from test_gpu_obc import obc_cfg
from test_gpu_parity import RTOL_ROUTINE
from test_gpu_tdiag import column_path_of, model_of, switch_depths
from test_uvdiag_ref import (CLOSURE_ULPS, edges_of, entry_state, inner, restated, small_basin, stages, started,
                             stirred_filament)

pytestmark = pytest.mark.gpu

TERMS = ur.TERMS
SMALL = dict(BASIN_LMD, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)


def fourteen(m):
    return {c: {k: m.uvdiag(c, k) for k in TERMS} for c in "uv"}


def gpu_stages(m, cfg, tix, s):
    def call(name):
        getattr(m, name)()
        m.sync()
    return stages(call, m.get, cfg, tix, s)


def check(m, cfg, s, fin, vis2=True, closure=True):
    """Every term equals the restatement over s; each is non-zero somewhere; the library's own terms close the budget."""
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    want = restated(cfg, s)
    got = fourteen(m)
    for comp in "uv":
        for k in TERMS:
            g, w = got[comp][k], want[comp][k]
            assert g.shape == (N, M + 4, L + 4)
            if not np.array_equal(g, w):
                bad = np.argwhere(g != w)
                raise AssertionError("%s_%s: %d points differ, first (k, j, i) index %s, max |diff| %.3e of %.3e"
                                     % (comp, k, len(bad), bad[0], np.abs(g - w).max(), np.abs(w).max()))
            assert np.abs(g).max() > 0 or (k == "hmx" and not vis2), (comp, k)
        assert np.array_equal(m.uvdiag(comp, "prev"), ur.clip(s[comp + "_prev"], comp, L, M, edges_of(cfg))), comp
        if closure:
            r, c = inner(cfg, comp)
            water = s[comp + "mask"][r, c] > 0
            if not water.any():   # MMm = 3: no v row away from the walls
                continue
            res, sc = ur.closure_residual(got[comp], s[comp + "_prev"], fin[0 if comp == "u" else 1], s["Hz2"], cfg.dt, comp)
            ulps = (np.abs(res) / np.spacing(sc))[:, r, c][:, water].max()
            print("%s closure: %.2f ulp of the largest term" % (comp, ulps))
            assert ulps <= CLOSURE_ULPS
    return got


def run_case(cfg, o=None, model=None, avg=False, closure=True, before=None):
    o = o or started(cfg)
    tix = bs.set_mode(o, "corr")
    s = entry_state(o, cfg, tix)
    m = model(cfg) if model else model_of(cfg)
    try:
        if before:
            before(m)
        hand_over(o, m, tix)
        m.uvdiag_begin(avg=avg)
        assert m.uvdiag_state() == (True, avg, 0, True)
        fin = gpu_stages(m, cfg, tix, s)
        assert m.uvdiag_state() == (True, avg, 1 if avg else 0, True)
        return check(m, cfg, s, fin, closure=closure), s
    finally:
        m.close()


def test_closed_basin():
    got, s = run_case(small_basin())
    L, M = 36, 11
    # the first u column and the first v row of the closed grid hold nothing (wrt_diag_uv zeroes them)
    for k in TERMS:
        assert not got["u"][k][:, :, :3].any() and not got["v"][k][:, :3].any()
        assert np.abs(got["u"][k][:, 2:M + 2, 3]).max() > 0 and np.abs(got["v"][k][:, 3, 2:L + 2]).max() > 0


def test_means_sink_first_sample_equals_the_store_sink():
    a, _ = run_case(small_basin())
    b, _ = run_case(small_basin(), avg=True)
    for c in "uv":
        for k in TERMS:
            assert np.array_equal(a[c][k], b[c][k]), (c, k)


def test_periodic_filament():
    cfg, o = stirred_filament(FIL["LLm"], FIL["MMm"], FIL["N"])
    got, _ = run_case(cfg, o=o, model=lambda c: romsgpu.Model.from_case(**FIL))
    L, M = FIL["LLm"], FIL["MMm"]
    for k in TERMS:   # istrU = jstrV = 1 on the periodic grid
        assert np.abs(got["u"][k][:, 2:M + 2, 2]).max() > 0 and np.abs(got["v"][k][:, 2, 2:L + 2]).max() > 0
        assert not got["u"][k][:, :, L + 2:].any() and not got["v"][k][:, M + 2:].any()


def test_island():
    _, s = run_case(small_basin(island=1))
    assert (s["umask"][2:13, 3:38] == 0).any() and (s["pmask"][2:13, 2:38] == 0).any()


def test_curvgrid():
    _, s = run_case(small_basin(curvgrid=1))
    assert np.ptp(s["pm"][2:13, 5]) > 0 and np.abs(s["dndx"]).max() > 0


def test_rough_metrics():
    """pm, pn and f vary along both axes (tests/metrics.py `rough`, every entry different from its neighbours), with
    the curvature terms on: a term that reads a metric one cell off, or dm_p for dm_v, differs from the restatement."""
    import metrics
    from test_uvdiag_ref import VISC2
    cfg = small_basin(curvgrid=1)
    o = oracle.Oracle(cfg)
    o.init()
    o.field("visc2_r")[...] = VISC2
    o.field("visc2_p")[...] = VISC2
    metrics.apply_grid(o, None, metrics.rough(cfg.LLm, cfg.MMm))
    o.step(3)
    _, s = run_case(cfg, o=o)
    R = metrics.ranges(cfg.LLm, cfg.MMm)
    for n in ("fomn", "dndx", "dmde", "dm_r", "dn_r", "dm_p", "dn_p", "dn_u", "dm_v"):
        assert metrics.neighbours_differ(s[n], R[n]) == 0, n


def test_open_boundaries():
    cfg = obc_cfg(obc=15, island=0, LLm=36, MMm=11, N=5, sizex=72e3, sizey=22e3)
    run_case(cfg, model=obc_model)


def test_rivers():
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
    # the closure leaves river faces out (step3d_uv2 sets them): the term comparisons cover them
    run_case(cfg, o=o, model=sweep_model, before=lambda m: rivers.put_rivers(m, vol, trc, uf, vf), closure=False)


@pytest.mark.parametrize("MMm,N", [(3, 3), (4, 4), (5, 5)])
@pytest.mark.parametrize("LLm", [63, 64, 65])
def test_widths_heights_and_shallow_depths(LLm, MMm, N):
    """64 consecutive i per wavefront from the line start at i = 1, four rows per block: column Lm lands on the last
    lane but one (63), the last lane (64) or the next block (65); row Mm in the block's third or fourth row or the
    next block.  N = 3 has no fourth-order vertical face, N = 4 one."""
    run_case(small_basin(LLm=LLm, MMm=MMm, N=N))


def uv1_ru(cfg, forced):
    """ru, rv after the library's prsgrd and step3d_uv1 on the oracle's corrector state, and the oracle's own."""
    o = started(cfg, visc2=0.0)
    tix = bs.set_mode(o, "corr")
    m = depth_model(cfg, forced=forced)
    try:
        hand_over(o, m, tix)
        m.uvdiag_begin()
        m.prsgrd()
        m.step3d_uv1()
        m.sync()
        got = (m.get("ru"), m.get("rv"), m.column_path())
    finally:
        m.close()
    o.call("prsgrd")
    o.call("step3d_uv1")
    return got, (o.field("ru").copy(), o.field("rv").copy())


@pytest.mark.parametrize("which", ["last ColLds", "first ColGlb", "first segments"])
def test_depths(which):
    """Either side of the column scratch switch (k_uv1 on ColLds, on ColGlb) and the first depth at which step3d_uv1
    is the segment form, found at run time: there the final ru comes from the segment solver's sampling
    instantiation and must agree with the oracle's."""
    glb, seg = switch_depths()
    N = {"last ColLds": glb - 1, "first ColGlb": glb, "first segments": seg}[which]
    print("depth", which, N)
    path = column_path_of(N)
    cfg = depth_cfg(N)
    o = started(cfg)
    tix = bs.set_mode(o, "corr")
    s = entry_state(o, cfg, tix)
    m = model_of(cfg)
    try:
        assert m.column_path() == path == (which == "first segments", N >= glb)
        hand_over(o, m, tix)
        m.uvdiag_begin()
        fin = gpu_stages(m, cfg, tix, s)
        check(m, cfg, s, fin)
    finally:
        m.close()
    if which == "first segments":
        o.call("prsgrd")
        o.call("step3d_uv1")
        r, c = slice(2, cfg.MMm + 2), slice(2, cfg.LLm + 2)
        for n in ("ru", "rv"):
            ref = o.field(n)[:, r, c]
            e = np.abs(s[n + "_fin"][:, r, c] - ref).max() / np.abs(ref).max()
            print("final %s, segment form vs oracle: %.3e" % (n, e))
            assert e <= RTOL_ROUTINE


@pytest.mark.parametrize("off", [(), ("ROMS_GPU_SEG_BUF",), ("ROMS_GPU_SEG_BUF", "ROMS_GPU_UV1_LDS")],
                         ids=["k_uv1_segb", "k_uv1_seg<true>", "k_uv1_seg<false>"])
def test_segment_form_stores_the_column_forms_final_ru(off, monkeypatch):
    """A depth at which both forms run (the segment form forced): the ru, rv the sampling instantiations store agree
    with what uv1_col stores, and both with the oracle's.  The three segment kernels are reached by switching the
    buffer form and the LDS form off."""
    cfg = depth_cfg(44)   # four segments of 11 rows when forced, k_uv1 on ColLds otherwise
    (ru_c, rv_c, path_c), (ru_o, rv_o) = uv1_ru(cfg, forced=False)
    for name in off:
        monkeypatch.setenv(name, "0")
    (ru_s, rv_s, path_s), _ = uv1_ru(cfg, forced=True)
    assert not path_c[0] and path_s[0]
    r, c = slice(2, cfg.MMm + 2), slice(2, cfg.LLm + 2)
    for a, b, ref in ((ru_s, ru_c, ru_o), (rv_s, rv_c, rv_o)):
        scale = np.abs(ref[:, r, c]).max()
        assert np.abs(a - b)[:, r, c].max() / scale <= RTOL_ROUTINE
        assert np.abs(a - ref)[:, r, c].max() / scale <= RTOL_ROUTINE
        assert np.abs(a[:, r, c]).max() > 0


def test_means_windows_sampling_and_once_per_sample():
    """Three steps with avg equal the recurrence navg += 1, coef = 1/navg, X_avg = X_avg*(1-coef) + X*coef over the
    three plain samples of a twin model (the library keeps one model per host thread: the twin runs in a thread of
    its own); uvdiag_sample(False) freezes the window; a second visc3d or step3d_uv2 before the next step3d_uv1
    leaves the terms alone."""
    samples, errs = [], []

    def twin():
        try:
            m = romsgpu.Model.from_case(**SMALL)
            m.uvdiag_begin()
            for _ in range(3):
                m.step(1)
                samples.append(fourteen(m))
            m.close()
        except Exception as e:
            errs.append(repr(e))

    th = threading.Thread(target=twin)
    th.start()
    th.join(timeout=240)
    assert not errs, errs
    m = romsgpu.Model.from_case(**SMALL)
    try:
        m.uvdiag_begin(avg=True)
        avg = None
        for n in range(1, 4):
            m.step(1)
            coef, x = 1.0 / n, samples[n - 1]
            avg = x if avg is None else {c: {k: avg[c][k] * (1 - coef) + x[c][k] * coef for k in TERMS} for c in x}
            assert m.uvdiag_state()[2] == n
            got = fourteen(m)
            for c in "uv":
                for k in TERMS:
                    assert np.array_equal(got[c][k], avg[c][k]), (n, c, k)
        assert not np.array_equal(avg["u"]["adv"], samples[2]["u"]["adv"])
        # once per sample: the hooks of a repeated visc3d / step3d_uv2 leave the means alone
        before = fourteen(m)
        m.visc3d()
        m.step3d_uv2()
        m.sync()
        after = fourteen(m)
        for c in "uv":
            for k in ("hmx", "cpl", "pgr"):
                assert np.array_equal(before[c][k], after[c][k]), (c, k)
        m.uvdiag_sample(False)   # calc_diag off: the window is frozen
        m.step(1)
        assert m.uvdiag_state() == (True, True, 3, False)
        assert np.array_equal(m.uvdiag("v", "vmx"), after["v"]["vmx"])
    finally:
        m.close()


def test_file_alone_and_with_tracers(tmp_path):
    from scipy.io import netcdf_file
    dt = SMALL["dt"]
    p, q = str(tmp_path / "dia_avg.nc"), str(tmp_path / "dia.nc")
    m = romsgpu.Model.from_case(**SMALL)
    try:
        L, M, N = m.Lm, m.Mm, m.N
        m.uvdiag_begin(avg=True)
        assert m.L.roms_gpu_wrt_diag(p.encode(), 1, 1, 0.0, 0.0, m.t) == -4   # no sample yet
        assert b"no complete sample" in m.L.roms_gpu_last_error() and not os.path.exists(p)
        wins = []
        for rec, nsamp in ((1, 2), (2, 1)):
            m.step(nsamp)
            assert m.uvdiag_state()[2] == nsamp
            wins.append(fourteen(m))
            m.wrt_diag(p, rec, rec, m.time(dt), nsamp * dt)
            assert m.uvdiag_state()[2] == 0   # the window is reset
        assert m.L.roms_gpu_wrt_diag(p.encode(), 3, 3, 0.0, 0.0, m.t) == -4
        m.io_wait()
        d = read(p)
        with netcdf_file(p, "r", mmap=False) as nc:
            names = [n for n in nc.variables if n[:2] in ("u_", "v_")]
            assert names == [c + "_" + k for c in "uv" for k in TERMS]
            v = nc.variables["u_cpl"]
            assert (v.long_name, v.units) == (b"2D/3D coupling", b"m^2/s^2")
            assert nc.variables["v_pgr"].long_name == b"Hydrostatic Presssure Gradient"
            assert v.dimensions == ("time", "s_rho", "eta_rho", "xi_u") and v.shape[1:] == (N, M + 2, L + 1)
            w = nc.variables["v_adv"]
            assert w.dimensions == ("time", "s_rho", "eta_v", "xi_rho") and w.shape[1:] == (N, M + 1, L + 2)
            assert nc.diagnostic_options == b"Chosen Diagnostics = Momentum"
            assert nc.diag_avg_time == b"120.0 seconds"
            assert np.array_equal(nc.variables["ocean_time"][:], [2 * dt, 3 * dt])
        for rec, wdw in enumerate(wins):
            for c in "uv":
                for k in TERMS:
                    assert np.array_equal(d["%s_%s" % (c, k)][rec], slab(wdw[c][k], c, L, M)), (rec, c, k)
        assert not np.array_equal(d["u_adv"][0], d["u_adv"][1]) and np.abs(d["v_vmx"]).max() > 0
        # together with armed tracers, without avg: the last sample of both, the tracers' variables after ours
        m.uvdiag_begin()
        m.tdiag_begin((1,), avg=True)
        m.step(1)
        assert m.L.roms_gpu_wrt_diag(q.encode(), 1, 1, 0.0, 0.0, m.t) == -1 and b"do_avg" in m.L.roms_gpu_last_error()
        m.tdiag_begin((1,))
        assert m.L.roms_gpu_wrt_diag(q.encode(), 1, 1, 0.0, 0.0, m.t) == -4   # the tracers have no sample
        m.step(1)
        x, tx = fourteen(m), m.tdiag(1, "advx")
        m.wrt_diag(q, 1, 1, m.time(dt))
        m.io_wait()
        d = read(q)
        assert np.array_equal(d["u_dis"][0], slab(x["u"]["dis"], "u", L, M))
        assert np.array_equal(d["temp_advx"][0], slab(tx, "r", L, M))
        with netcdf_file(q, "r", mmap=False) as nc:
            assert not hasattr(nc, "diag_avg_time")
            assert nc.diagnostic_options == b"Chosen Diagnostics = Momentum, Tracers"
            names = [n for n in nc.variables if "_" in n and n.split("_")[0] in ("u", "v", "temp")]
            assert names[:14] == [c + "_" + k for c in "uv" for k in TERMS] and names[14] == "temp_advx"
    finally:
        m.close()


def test_decomposition_bitwise():
    """2 x 2 ranks on one GPU: every rank's means are bitwise the single domain's over its own points; the rank
    boundaries keep the fourth-order form."""
    case = dict(BASIN_LMD, N=6)
    arm = lambda m: m.uvdiag_begin(avg=True)
    probe = lambda m: (fourteen(m), m.uvdiag_state())
    m = romsgpu.Model.from_case(**case)
    arm(m)
    m.step(3)
    ref, st = probe(m)
    m.close()
    assert st == (True, True, 3, True)
    parts, _ = run_decomposed(case, 2, 2, 3, fields=("u",), probe=probe, setup=arm)
    for rank, (iSW, jSW, Lm, Mm, _, (got, st)) in enumerate(parts):
        assert st == (True, True, 3, True)
        for c in "uv":
            i0 = 2 if (c == "u" and iSW == 0) else 1     # istrU on the western ranks
            j0 = 2 if (c == "v" and jSW == 0) else 1     # jstrV on the southern ranks
            for k in TERMS:
                g = got[c][k][:, j0 + 1:Mm + 2, i0 + 1:Lm + 2]
                w = ref[c][k][:, jSW + j0 + 1:jSW + Mm + 2, iSW + i0 + 1:iSW + Lm + 2]
                assert np.array_equal(g, w), (rank, c, k, float(np.abs(g - w).max()))
                assert np.abs(g).max() > 0 or k == "hmx"
                z = got[c][k].copy()
                z[:, j0 + 1:Mm + 2, i0 + 1:Lm + 2] = 0
                assert not z.any(), (rank, c, k)


def test_armed_disarmed_and_never_armed_leave_the_same_fields(monkeypatch):
    def run(mode):
        m = romsgpu.Model.from_case(**SMALL)
        if mode != "never":
            m.uvdiag_begin(avg=True)
        if mode == "disarmed":
            m.uvdiag_begin(on=False)
            assert m.uvdiag_state() == (False, False, 0, False)
        m.step(3)
        out = {n: m.get(n) for n in ("u", "v", "t", "zeta")}
        m.close()
        return out

    never, disarmed, armed = run("never"), run("disarmed"), run("armed")
    for n in never:
        assert np.array_equal(never[n], armed[n]) and np.array_equal(never[n], disarmed[n]), n
    # and with every step enqueued on both sides
    monkeypatch.setenv("ROMS_GPU_NO_GRAPH", "1")
    never, armed = run("never"), run("armed")
    for n in never:
        assert np.array_equal(never[n], armed[n]), n


def test_refusals():
    m = romsgpu.Model.from_case(**SMALL)
    E = lambda: m.L.roms_gpu_last_error()
    a = np.empty(m.N * m.shape2[0] * m.shape2[1])
    ms = (romsgpu.ctypes.c_double * 4)()
    try:
        assert m.uvdiag_state() == (False, False, 0, False)
        assert m.L.roms_gpu_uvdiag_sample(1) == -4 and b"not armed" in E()
        assert m.L.roms_gpu_uvdiag_copy_out(0, 1, a.ctypes.data, a.size) == -4 and b"not armed" in E()
        assert m.L.roms_gpu_wrt_diag(b"x.nc", 1, 1, 0.0, 0.0, m.t) == -4 and b"not armed" in E()
        assert m.L.roms_gpu_time_uvdiag(1, m.t, ms) == -4 and b"not armed" in E()
        m.step(1)
        m.uvdiag_begin()
        assert m.L.roms_gpu_uvdiag_copy_out(2, 1, a.ctypes.data, a.size) == -1 and b"comp" in E()
        assert m.L.roms_gpu_uvdiag_copy_out(0, 0, a.ctypes.data, a.size) == -1 and b"term" in E()
        assert m.L.roms_gpu_uvdiag_copy_out(0, 9, a.ctypes.data, a.size) == -1 and b"term" in E()
        assert m.L.roms_gpu_uvdiag_copy_out(1, 1, a.ctypes.data, a.size - 1) == -1 and b"count" in E()
        assert m.L.roms_gpu_time_uvdiag(0, m.t, ms) == -1 and b"bad arguments" in E()
        assert m.L.roms_gpu_wrt_diag(b"x.nc", 1, 1, 0.0, 0.0, m.t) == -4 and b"no complete sample" in E()
        # a sample that step3d_uv2 has not closed is not writable
        m.prsgrd()
        m.step3d_uv1()
        m.sync()
        assert m.L.roms_gpu_wrt_diag(b"x.nc", 1, 1, 0.0, 0.0, m.t) == -4 and b"no complete sample" in E()
        assert m.uvdiag_state() == (True, False, 0, True)
        assert not os.path.exists("x.nc")
        with pytest.raises(ValueError):
            m.uvdiag("u", "advx")
        ts = m.time_uvdiag(2)
        assert len(ts) == 4 and all(t > 0 for t in ts)
    finally:
        m.close()
