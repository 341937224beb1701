"""Time-averaged output on the device (calc_avg_ocean_vars / wrt_avg_ocean_vars,
basic_output.F:421-515, 1036-1118).

The expected values never come from the library's own averaging: they are the
recurrence  navg += 1; coef = 1/navg; avg = avg*(1-coef) + x*coef  in numpy
over states downloaded with Model.get after each step (paths the parity tests
pin to the oracle).  The kernel evaluates the same two multiplies and one add
in the same order without contraction, so every comparison is np.array_equal
over the reference's write ranges (dimensions.F:40-45).
"""
import os
import threading

import numpy as np
import pytest

import romsgpu
from test_gpu_io import BASIN_LMD, FIL, PASSIVE, join, read, slab

pytestmark = pytest.mark.gpu

W = romsgpu.WRT
ALIGN = dict(case_id=1, LLm=37, MMm=27, N=5, NT=2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30,
             sizex=74e3, sizey=54e3)   # (Lm+4)*(Mm+4) = 1271 and N odd: slot 2 sits on an odd double at ROMS_GPU_PITCH=0
GRID = dict(zeta="r", ubar="u", vbar="v", u="u", v="v", t="r", rho="r", omega="r", Akv="r", Akt="r", Aks="r",
            hbls="r", hbbl="r")


def sample(m, mask=romsgpu.WRT_DEFAULT, slot="nstp"):
    """What calc_avg samples after a step: zeta/ubar/vbar(knew), u/v/t(nstp), the rest as they stand."""
    t, N = m.t, m.N
    s = t.nstp if slot == "nstp" else t.nnew
    x = dict(zeta=m.get("zeta")[t.knew - 1:t.knew], ubar=m.get("ubar")[t.knew - 1:t.knew],
             vbar=m.get("vbar")[t.knew - 1:t.knew], u=m.get("u")[(s - 1) * N:s * N], v=m.get("v")[(s - 1) * N:s * N])
    tr = m.get("t").reshape(m.NT, 3, N, *m.shape2)[:, s - 1]
    for q in range(m.NT):
        x["t%d" % q] = tr[q]
    if mask & W["R"]:
        x["rho"] = m.get("rho1") - m.get("qp1") * m.get("z_r")   # SPLIT_EOS (basic_output.F:1084-1085)
    if mask & W["O"]:
        x["omega"] = m.get("We") + m.get("Wi")
    if mask & W["Akv"]:
        x["Akv"] = m.get("Akv")
    if mask & W["Akt"]:
        x["Akt"] = m.get("Akt")[:N + 1]
    if mask & W["Aks"]:
        x["Aks"] = m.get("Akt")[N + 1:]
    if mask & W["Hbls"]:
        x["hbls"] = m.get("hbls")
    if mask & W["Hbbl"]:
        x["hbbl"] = m.get("hbbl")
    return x


class Recurrence:
    """calc_avg_ocean_vars in numpy."""

    def __init__(self):
        self.navg, self.t_avg, self.avg = 0, 0.0, {}

    def add(self, x, time):
        self.navg += 1
        coef = 1.0 / self.navg
        self.t_avg = self.t_avg * (1.0 - coef) + time * coef
        for k, v in x.items():
            self.avg[k] = v * coef if self.navg == 1 else self.avg[k] * (1.0 - coef) + v * coef

    def reset(self):
        self.navg = 0


def got(m, key):
    if key[0] == "t" and key[1:].isdigit():
        return m.avg("t", int(key[1:])), "r"
    return m.avg(key), GRID[key]


def check(m, rec, what=""):
    for key, want in rec.avg.items():
        a, g = got(m, key)
        assert a.shape == want.shape, (what, key, a.shape, want.shape)
        assert np.array_equal(slab(a, g, m.Lm, m.Mm), slab(want, g, m.Lm, m.Mm)), (what, key)
    navg, t_avg, _ = m.avg_state()
    assert navg == rec.navg and t_avg == rec.t_avg, (what, navg, t_avg, rec.navg, rec.t_avg)


def test_filament_default_mask_equals_numpy_recurrence():
    m = romsgpu.Model.from_case(**FIL)
    m.avg_begin()
    assert m.avg_state() == (0, 0.0, romsgpu.WRT_DEFAULT)
    rec, wrong = Recurrence(), Recurrence()
    differs = []
    for n in range(5):
        m.step(1)
        time = m.time(FIL["dt"])
        m.calc_avg(time)
        rec.add(sample(m), time)
        check(m, rec, "sample %d" % (n + 1))
        # negative control: u taken from slot nnew is another average
        wrong.add(dict(u=sample(m, slot="nnew")["u"]), time)
        differs.append(not np.array_equal(slab(m.avg("u"), "u", m.Lm, m.Mm), slab(wrong.avg["u"], "u", m.Lm, m.Mm)))
    m.close()
    assert all(differs[1:]), differs


@pytest.mark.parametrize("case", [BASIN_LMD, PASSIVE], ids=["basin_lmd", "basin_nt4"])
def test_basin_kpp_full_mask(case):
    m = romsgpu.Model.from_case(**case)
    m.avg_begin(romsgpu.WRT_ALL)
    assert m.avg_state()[2] == romsgpu.WRT_ALL
    rec = Recurrence()
    for n in range(4):
        m.step(1)
        time = m.time(case["dt"])
        m.calc_avg(time)
        rec.add(sample(m, romsgpu.WRT_ALL), time)
        check(m, rec, "sample %d" % (n + 1))
    assert set(rec.avg) == {"zeta", "ubar", "vbar", "u", "v", "rho", "omega", "Akv", "Akt", "Aks", "hbls", "hbbl"} | \
        {"t%d" % q for q in range(case["NT"])}
    # every tracer's average is its own, and "temp"/"salt" name the first two
    for q in range(1, case["NT"]):
        assert not np.array_equal(m.avg("t", q), m.avg("t", 0))
    assert np.array_equal(m.avg("temp"), m.avg("t", 0)) and np.array_equal(m.avg("salt"), m.avg("t", 1))
    assert np.abs(rec.avg["rho"]).max() > 0 and np.abs(rec.avg["omega"]).max() > 0 and rec.avg["hbls"].max() > 0
    m.close()


def _align_run(monkeypatch, pitch0):
    if pitch0:
        monkeypatch.setenv("ROMS_GPU_PITCH", "0")
    else:
        monkeypatch.delenv("ROMS_GPU_PITCH", raising=False)
    m = romsgpu.Model.from_case(**ALIGN)
    mask = romsgpu.WRT_DEFAULT | W["R"] | W["O"] | W["Akt"]
    m.avg_begin(mask)
    rec = Recurrence()
    slots = []
    for n in range(3):
        m.step(1)
        slots.append(m.t.nstp)
        time = m.time(ALIGN["dt"])
        m.calc_avg(time)
        rec.add(sample(m, mask), time)
        check(m, rec, "pitch0=%s sample %d" % (pitch0, n + 1))
    out = {k: slab(got(m, k)[0], got(m, k)[1], m.Lm, m.Mm) for k in rec.avg}
    m.close()
    assert 2 in slots   # the slot that is only 8-byte aligned at the host pitch was sampled
    return out


def test_alignment_paths_agree(monkeypatch):
    """Default pitch: every pointer 16-byte aligned (double2 sweep).  ROMS_GPU_PITCH=0 with an odd plane and odd N:
    slot nstp = 2 of u, v, t starts on an odd double (8-byte sweep).  Both equal numpy, hence each other."""
    a = _align_run(monkeypatch, False)
    b = _align_run(monkeypatch, True)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_windows_and_the_averages_file(tmp_path):
    p = str(tmp_path / "fil_avg.nc")
    dt = FIL["dt"]
    mask = romsgpu.WRT_DEFAULT | W["O"]
    m = romsgpu.Model.from_case(**FIL)
    m.avg_begin(mask)
    rec = Recurrence()
    wins = []
    pm, pn = m.get("pm"), m.get("pn")
    for r, nsamp in ((1, 3), (2, 2)):
        for _ in range(nsamp):
            m.step(1)   # in the second window: steps and samples while the writer drains record 1
            time = m.time(dt)
            m.calc_avg(time)
            rec.add(sample(m, mask), time)
        m.wrt_avg(p, r, r, nsamp * dt)
        assert m.avg_state()[0] == 0
        wins.append((dict(rec.avg), rec.t_avg, m.t.iic))
        rec = Recurrence()   # restarted from nothing: no leak across the reset
    m.io_wait()
    L, M = m.Lm, m.Mm
    m.close()
    d = read(p)
    assert d["_attrs"]["type"] == b"ROMS averages file"
    assert d["_attrs"]["averaging_timescale"] == b"15.0 seconds"
    with_names = {}
    from scipy.io import netcdf_file
    with netcdf_file(p, "r", mmap=False) as nc:
        for k, v in nc.variables.items():
            if k not in ("ocean_time", "time_step"):
                with_names[k] = (v.long_name, getattr(v, "units", b""))
    assert set(with_names) == {"zeta", "ubar", "vbar", "u", "v", "temp", "omega"}
    assert all(ln.startswith(b"averaged ") for ln, _ in with_names.values()), with_names
    assert with_names["zeta"] == (b"averaged free-surface elevation", b"meter")
    assert with_names["temp"][0] == b"averaged potential temperature"
    assert d["ocean_time"].tolist() == [wins[0][1], wins[1][1]]
    assert wins[0][1] == pytest.approx(2 * dt) and wins[1][1] == pytest.approx(4.5 * dt)
    for r, (avg, _, iic) in enumerate(wins):
        assert d["time_step"][r].tolist() == [iic, r + 1, r + 1, 0, 0, 0]
        assert np.array_equal(d["zeta"][r], slab(avg["zeta"][0], "r", L, M))
        assert np.array_equal(d["ubar"][r], slab(avg["ubar"][0], "u", L, M))
        assert np.array_equal(d["vbar"][r], slab(avg["vbar"][0], "v", L, M))
        assert np.array_equal(d["u"][r], slab(avg["u"], "u", L, M))
        assert np.array_equal(d["v"][r], slab(avg["v"], "v", L, M))
        assert np.array_equal(d["temp"][r], slab(avg["t0"], "r", L, M))
        assert np.array_equal(d["omega"][r], slab((avg["omega"] * pm[0]) * pn[0], "r", L, M))   # basic_output.F:482
    assert not np.array_equal(d["u"][0], d["u"][1])


def test_partitioned_averages_join_to_single_domain(tmp_path):
    dt = FIL["dt"]
    single = str(tmp_path / "single_avg.nc")
    m = romsgpu.Model.from_case(**FIL)
    m.avg_begin()
    m.step_avg(3, dt)
    m.wrt_avg(single, 1, 1, 3 * dt)
    m.io_wait()
    m.close()
    npx, npe = 2, 2
    paths = [str(tmp_path / ("avg.%d.nc" % r)) for r in range(npx * npe)]
    errs = []

    def work(rank):
        try:
            h = romsgpu.comm_create_local(778, npx * npe, rank)
            mm = romsgpu.Model.from_case(np_xi=npx, np_eta=npe, comm=h, rank=rank, **FIL)
            mm.avg_begin()
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
    a = read(paths[3])["_attrs"]
    assert list(a["partition"])[:2] == [3, 4] and a["type"] == b"ROMS averages file"
    joined = join(paths)
    ref = read(single)
    assert ref["ocean_time"].tolist() == [2 * dt]
    for name in ("zeta", "ubar", "vbar", "u", "v", "temp"):
        assert np.array_equal(joined[name], ref[name]), name


def test_errors(tmp_path):
    p = str(tmp_path / "none.nc")
    m = romsgpu.Model.from_case(**FIL)
    with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
        m.calc_avg(5.0)
    m.avg_begin()
    with pytest.raises(romsgpu.RomsGpuError, match="no sample"):
        m.wrt_avg(p, 1, 1, 5.0)
    m.io_wait()
    assert not os.path.exists(p)
    assert m.avg_state() == (0, 0.0, romsgpu.WRT_DEFAULT)
    with pytest.raises(romsgpu.RomsGpuError):
        m.avg("salt")
    with pytest.raises(romsgpu.RomsGpuError):
        m.avg("rho")   # not in the mask
    # bits the configuration cannot serve are dropped: no salinity, no LMD here
    m.avg_begin(romsgpu.WRT_ALL)
    assert m.avg_state()[2] == romsgpu.WRT_ALL & ~(W["Aks"] | W["Hbls"] | W["Hbbl"])
    m.avg_begin(0)
    assert m.avg_state() == (0, 0.0, 0)
    with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
        m.calc_avg(5.0)
    m.close()


def test_the_step_is_untouched():
    def run(armed):
        m = romsgpu.Model.from_case(**FIL)
        if armed:
            m.avg_begin(romsgpu.WRT_ALL)
        for _ in range(6):
            m.step(1)
            if armed:
                m.calc_avg(m.time(FIL["dt"]))
        out = {k: m.get(k) for k in ("zeta", "u", "v", "t")}
        m.close()
        return out

    a, b = run(True), run(False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
