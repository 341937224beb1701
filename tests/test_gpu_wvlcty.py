"""True vertical velocity w on the device (wvlcty.F):
k_wvlcty with its two sinks, Model.wvlcty, history and averages files.

The expected values never come from the library's w: they are the numpy
restatement of wvlcty_tile (tests/wvlcty_ref.py, pinned bit for bit to the
reference's own routine by tests/test_wvlcty_ref.py) over arrays downloaded
with Model.get after the step.  The kernel evaluates the reference's
operations in the reference's order without contraction, so every comparison
is np.array_equal.  Model.wvlcty() holds 0 wherever wvlcty_tile writes nothing,
and so does the restatement: whole arrays are compared, which also shows that
nothing outside the computed range and its copies was written.
"""
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import romsgpu
import wvlcty_ref
from test_gpu_avg import ALIGN, Recurrence, check, sample
from test_gpu_io import BASIN_LMD, FIL, join, read, slab

pytestmark = pytest.mark.gpu

W = romsgpu.WRT
HERE = os.path.dirname(os.path.abspath(__file__))
# a plain closed basin: T and S, nonlinear EOS, no KPP
BASIN = dict(case_id=1, LLm=36, MMm=11, N=5, NT=2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30, sizex=72e3,
             sizey=22e3)
# the history file whose bytes the commit before ROMS_WRT_W wrote (tests/golden/his_no_w_sha256.json)
TINY = dict(case_id=0, LLm=32, MMm=24, N=16, NT=1, salinity=False, nonlin_eos=False, dt=5.0, ndtfast=60, sizex=12.8e3,
            sizey=3.2e3)


def periodic(case):
    return case["case_id"] == 0


def w_and_ref(case, steps=3):
    m = romsgpu.Model.from_case(**case)
    m.step(steps)
    w = m.wvlcty()
    ref = wvlcty_ref.of_model(m, periodic(case))
    extra = dict(rmask=m.get("rmask")[0], pm=m.get("pm")[0], pn=m.get("pn")[0])
    m.close()
    return w, ref, extra


@pytest.mark.parametrize("name", ["filament", "basin_lmd", "basin_curvgrid", "basin_island"])
def test_kernel_equals_the_restatement(name):
    """FIL: both ranges widened, no copies.  Closed basin: four edges, four corners.  curvgrid: pm(j), pn(i) not
    uniform.  island: land inside -- the reference multiplies by no mask and neither may the kernel."""
    case = dict(filament=FIL, basin_lmd=BASIN_LMD, basin_curvgrid=dict(BASIN_LMD, curvgrid=True),
                basin_island=dict(BASIN_LMD, island=True))[name]
    w, ref, x = w_and_ref(case)
    assert w.shape == (case["N"], case["MMm"] + 4, case["LLm"] + 4)
    assert np.array_equal(w, ref)
    assert np.abs(w).max() > 0
    L, M = case["LLm"], case["MMm"]
    if periodic(case):   # the rim 0 and Lm+1 / Mm+1 is computed, rows -1 and Lm+2 untouched
        assert np.abs(w[:, 1:M + 3, 1]).max() > 0 and not w[:, :, 0].any() and not w[:, 0].any()
    else:
        assert np.array_equal(w[:, 1, 1], w[:, 2, 2]) and np.array_equal(w[:, M + 2, L + 2], w[:, M + 1, L + 1])
    if name == "basin_curvgrid":
        assert np.ptp(x["pm"][2:M + 2, 5]) > 0 and np.ptp(x["pn"][5, 2:L + 2]) > 0
    if name == "basin_island":
        assert (x["rmask"][2:M + 2, 2:L + 2] == 0).any()


def test_rough_metrics():
    """pm and pn vary along both axes (tests/metrics.py `rough`, put into the model after init): a pm or pn read one
    cell off, or one for the other, differs from the restatement, which the reference's routine pins on random planes."""
    import metrics
    import oracle
    from test_gpu_parity import basin_cfg
    case = dict(BASIN_LMD, curvgrid=True)
    cfg = basin_cfg(nonlin=True, LLm=case["LLm"], MMm=case["MMm"], N=case["N"], sizex=case["sizex"], sizey=case["sizey"])
    cfg.lmd, cfg.surf_flux, cfg.curvgrid = oracle.LMD_ALL, 1, 1
    o = oracle.Oracle(cfg)
    o.init()
    m = romsgpu.Model.from_case(**case)
    try:
        planes = metrics.apply_grid(o, m, metrics.rough(cfg.LLm, cfg.MMm))
        m.step(3)
        w = m.wvlcty()
        ref = wvlcty_ref.of_model(m, False)
        for n in ("pm", "pn"):
            assert np.array_equal(m.get(n)[0], planes[n])
            assert metrics.neighbours_differ(planes[n], (-1, cfg.MMm + 2, -1, cfg.LLm + 2)) == 0, n
    finally:
        m.close()
    assert np.array_equal(w, ref) and np.abs(w).max() > 0


@pytest.mark.parametrize("N", [3, 4, 5])
def test_level_counts_of_the_rolling_window(N):
    """The one-sided ends with one (N = 3), two (4) and three (5) levels of the four-point middle loop
    k = N-1..2 between them.  N = 3 is the smallest depth the model runs; the kernel's window of four Wrk values
    is first full at k = 3, so at N = 3 the only middle level is also the last one emitted inside the walk."""
    w, ref, _ = w_and_ref(dict(BASIN, N=N))
    assert np.array_equal(w, ref) and np.abs(w).max() > 0


@pytest.mark.parametrize("LLm", [64, 65, 36])
def test_widths_against_the_wavefront(LLm):
    """Lanes are 64 consecutive i from the line start at i = 1 (tile_i0), four rows per block.  LLm = 64: the
    eastern edge column i = Lm sits on the last lane of the first wavefront; 65: on the first lane of the next
    block; 36: mid-wavefront.  That lane also writes the copy at Lm+1 and, in the first and last row, a corner."""
    w, ref, _ = w_and_ref(dict(BASIN, LLm=LLm, sizex=2e3 * LLm))
    assert np.array_equal(w, ref) and np.abs(w[:, 2:-2, LLm + 2]).max() > 0


def test_host_pitch_and_odd_plane(monkeypatch):
    """ROMS_GPU_PITCH=0 on the 37 x 27 x 5 shape: rows of Lm+4 doubles, an odd plane, slot nstp = 2 on an odd double."""
    monkeypatch.setenv("ROMS_GPU_PITCH", "0")
    m = romsgpu.Model.from_case(**ALIGN)
    slots = []
    for _ in range(2):
        m.step(1)
        slots.append(m.t.nstp)
        assert np.array_equal(m.wvlcty(), wvlcty_ref.of_model(m, False))
    m.close()
    assert 2 in slots


def interp_like_w(om):
    """omega (0:N) to rho levels with wvlcty's own weights."""
    N = om.shape[0] - 1
    out = np.empty_like(om[1:])
    out[N - 1] = 0.375 * om[N] + 0.75 * om[N - 1] - 0.125 * om[N - 2]
    for k in range(N - 1, 1, -1):
        out[k - 1] = 0.5625 * (om[k] + om[k - 1]) - 0.0625 * (om[k + 1] + om[k - 2])
    out[0] = -0.125 * om[2] + 0.75 * om[1] + 0.375 * om[0]
    return out


@pytest.mark.parametrize("case", [FIL, BASIN_LMD], ids=["filament", "basin_lmd"])
def test_slot_is_nstp_and_w_is_not_omega(case):
    """Negative controls (both hold on the CPU oracle for these cases after 3 steps): the restatement with
    u, v(nnew) is another field from the second step on, and so is pm*pn*(We+Wi) brought to rho levels."""
    m = romsgpu.Model.from_case(**case)
    L, M = m.Lm, m.Mm
    differs, not_omega = [], []
    for _ in range(3):
        m.step(1)
        w = m.wvlcty()
        assert np.array_equal(w, wvlcty_ref.of_model(m, periodic(case)))
        differs.append(not np.array_equal(slab(w, "r", L, M), slab(wvlcty_ref.of_model(m, periodic(case), "nnew"), "r", L, M)))
        om = interp_like_w(m.get("pm")[0] * m.get("pn")[0] * (m.get("We") + m.get("Wi")))
        not_omega.append(not np.array_equal(slab(w, "r", L, M), slab(om, "r", L, M)))
        assert np.abs(w).max() > 0
    m.close()
    assert all(differs[1:]) and all(not_omega), (differs, not_omega)


def test_averages_windows_file_and_the_other_means(tmp_path):
    p = str(tmp_path / "avg_w.nc")
    case, dt = BASIN_LMD, BASIN_LMD["dt"]
    mask = romsgpu.WRT_DEFAULT | W["W"]
    m = romsgpu.Model.from_case(**case)
    m.avg_begin(mask)
    assert m.avg_state() == (0, 0.0, mask)
    rec, wins, others = Recurrence(), [], []
    for r, nsamp in ((1, 4), (2, 2)):
        for n in range(nsamp):
            m.step(1)
            time = m.time(dt)
            m.calc_avg(time)
            x = sample(m, mask)
            x["w"] = wvlcty_ref.of_model(m, False)
            rec.add(x, time)
            wavg = rec.avg.pop("w")   # check() knows the other fields only
            check(m, rec, "window %d sample %d" % (r, n + 1))
            rec.avg["w"] = wavg
            assert np.array_equal(m.avg("w"), wavg), (r, n)
        if r == 1:
            others = {k: m.avg(k) for k in ("zeta", "ubar", "vbar", "u", "v", "temp", "salt")}
        m.wrt_avg(p, r, r, nsamp * dt)
        assert m.avg_state()[0] == 0
        wins.append(dict(rec.avg))
        rec = Recurrence()   # the second window starts clean: its first sample does not read the old mean
    m.io_wait()
    L, M, N = m.Lm, m.Mm, m.N
    m.close()
    d = read(p)
    from scipy.io import netcdf_file
    with netcdf_file(p, "r", mmap=False) as nc:
        v = nc.variables["w"]
        assert (v.long_name, v.units) == (b"averaged vertical velocity", b"meter second-1")
        assert v.dimensions == ("time", "s_rho", "eta_rho", "xi_rho") and v.shape[1:] == (N, M + 2, L + 2)
    for r, avg in enumerate(wins):
        assert np.array_equal(d["w"][r], slab(avg["w"], "r", L, M)), r
        assert np.array_equal(d["u"][r], slab(avg["u"], "u", L, M)), r
    assert not np.array_equal(d["w"][0], d["w"][1]) and np.abs(d["w"]).max() > 0
    # the other means are bitwise what they are without the W bit
    m = romsgpu.Model.from_case(**case)
    m.avg_begin(romsgpu.WRT_DEFAULT)
    m.step_avg(4, dt)
    for k, a in others.items():
        assert np.array_equal(m.avg(k), a), k
    with pytest.raises(romsgpu.RomsGpuError):
        m.avg("w")   # not in the mask
    m.close()


def test_w_alone_can_be_armed():
    m = romsgpu.Model.from_case(**BASIN)
    m.avg_begin(W["W"])
    assert m.avg_state()[2] == W["W"]
    rec = Recurrence()
    for _ in range(2):
        m.step(1)
        m.calc_avg(m.time(BASIN["dt"]))
        rec.add(dict(w=wvlcty_ref.of_model(m, False)), m.time(BASIN["dt"]))
        assert np.array_equal(m.avg("w"), rec.avg["w"])
    m.close()


def test_history_file_holds_w_where_the_reference_defines_it(tmp_path):
    p, q = str(tmp_path / "his_w.nc"), str(tmp_path / "his_plain.nc")
    case = BASIN_LMD
    m = romsgpu.Model.from_case(**case)
    m.step(3)
    m.wrt_his(p, 1, 1, m.time(case["dt"]), mask=romsgpu.WRT_ALL)
    w = m.wvlcty()
    assert np.array_equal(w, wvlcty_ref.of_model(m, False))
    m.io_wait()
    L, M, N = m.Lm, m.Mm, m.N
    m.close()
    d = read(p)
    assert np.array_equal(d["w"][0], slab(w, "r", L, M))
    from scipy.io import netcdf_file
    with netcdf_file(p, "r", mmap=False) as nc:
        names = list(nc.variables)
        v = nc.variables["w"]
        assert (v.long_name, v.units) == (b"vertical velocity", b"meter second-1")
        assert v.dimensions == ("time", "s_rho", "eta_rho", "xi_rho") and v.shape[1:] == (N, M + 2, L + 2)
    # def_vars_ocean_vars (basic_output.F:808-830): omega, w, AKv
    assert names[names.index("omega"):names.index("omega") + 3] == ["omega", "w", "AKv"]
    # without the bit: no w, and the bytes the commit before this feature wrote for the same run
    m = romsgpu.Model.from_case(**TINY)
    m.step(3)
    m.wrt_his(q, 1, 1, m.time(TINY["dt"]), mask=romsgpu.WRT_DEFAULT | W["R"] | W["O"] | W["Akv"])
    m.io_wait()
    m.close()
    assert "w" not in read(q)
    want = json.load(open(os.path.join(HERE, "golden", "his_no_w_sha256.json")))
    raw = open(q, "rb").read()
    assert (len(raw), hashlib.sha256(raw).hexdigest()) == (want["bytes"], want["sha256"])


def _partitioned(case, tmp_path, tag):
    dt = case["dt"]
    mask = romsgpu.WRT_DEFAULT | W["W"]
    single = str(tmp_path / ("single_%s.nc" % tag))
    m = romsgpu.Model.from_case(**case)
    m.avg_begin(mask)
    m.step_avg(3, dt)
    m.wrt_avg(single, 1, 1, 3 * dt)
    m.io_wait()
    m.close()
    npx, npe = 2, 2
    paths = [str(tmp_path / ("avg_%s.%d.nc" % (tag, r))) for r in range(npx * npe)]
    errs = []

    def work(rank):
        try:
            h = romsgpu.comm_create_local(781 if periodic(case) else 782, npx * npe, rank)
            mm = romsgpu.Model.from_case(np_xi=npx, np_eta=npe, comm=h, rank=rank, **case)
            mm.avg_begin(mask)
            mm.step_avg(3, dt)
            mm.wrt_avg(paths[rank], 1, 1, 3 * dt)
            mm.io_wait()
            mm.close()
            romsgpu.comm_destroy(h)
        except Exception as e:
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(npx * npe)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
    assert not errs, errs
    joined, ref = join(paths), read(single)
    for name in ("zeta", "u", "v", "temp", "w"):
        assert np.array_equal(joined[name], ref[name]), name
    assert np.abs(ref["w"]).max() > 0


@pytest.mark.parametrize("case", [FIL, BASIN_LMD], ids=["filament", "basin_lmd"])
def test_partitioned_averages_of_w_join_to_the_single_domain(case, tmp_path):
    """2 x 2 ranks: at an interior rank edge nothing outside istr..iend is written in a closed direction, the
    widened rows of a periodic one come from exchanged halos, and the file ranges join without a seam."""
    _partitioned(case, tmp_path, "fil" if periodic(case) else "basin")


def test_the_step_is_untouched():
    def run(armed):
        m = romsgpu.Model.from_case(**FIL)
        if armed:
            m.avg_begin(romsgpu.WRT_DEFAULT | W["W"])
        for _ in range(6):
            m.step(1)
            if armed:
                m.calc_avg(m.time(FIL["dt"]))
                m.wvlcty()
        out = {k: m.get(k) for k in ("zeta", "u", "v", "t", "FlxU", "FlxV")}
        m.close()
        return out

    a, b = run(True), run(False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_errors():
    m = romsgpu.Model.from_case(**BASIN)
    a = np.empty(m.N * m.shape2[0] * m.shape2[1])
    assert m.L.roms_gpu_wvlcty_copy_out(a.ctypes.data, a.size) == -4
    assert b"nothing was computed" in m.L.roms_gpu_last_error()
    m.step(1)
    m.wvlcty()
    assert m.L.roms_gpu_wvlcty_copy_out(a.ctypes.data, a.size - 1) == -1
    m.close()
