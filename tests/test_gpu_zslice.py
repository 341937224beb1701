"""Z-level slices on the device (calc_zslice / sigma_to_z / calc_average /
wrt_zslice, zslice_output.F).

The expected values never come from the library's own slicing: `restate` is
sigma_to_z in numpy over Model.get downloads of z_r, z_w, rmask and u, v, t in
slot nnew -- the reference's expressions in its order, one ufunc per operation
(no contraction), IEEE division -- so every comparison is np.array_equal over
cells 1..Mm x 1..Lm.  It also returns each cell's class, from which the tests
assert that the masked cases reach every branch of the classification.
"""
import os
import threading

import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_io import FIL, join, read, slab
from test_gpu_lmd import lmd_basin_cfg

pytestmark = pytest.mark.gpu

T, U, V = romsgpu.ZSL_T, romsgpu.ZSL_U, romsgpu.ZSL_V
MASKED, ABOVE, TOP, BELOW, BOTTOM, INTERIOR, TIE = range(7)
CLASS_NAMES = ("masked", "above surface", "top half-layer", "below bottom", "bottom half-layer", "interior", "interior tie")


def _model(case, N=5):
    """Pipes_ana / Rivers_ana as test_gpu_lmd_lean builds them, at 37 x 27: odd, no multiple of a wave or tile."""
    if case == "filament":
        return romsgpu.Model.from_case(**FIL)
    if case == "basin":   # the N = 2 model of test_gpu_lmd_lean
        cfg = lmd_basin_cfg(surf_flux=1, LLm=40, MMm=32, N=N)
    else:
        cfg = (oracle.pipes_cfg if case == "pipes" else oracle.rivers_cfg)(LLm=37, MMm=27, N=N, np_xi=1, np_eta=1)
    return romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                   nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex,
                                   sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))


def inner(a, m):
    return a[..., 2:m.Mm + 2, 2:m.Lm + 2]


def zz_of(m, g, zr=None, zw=None):
    """zz(0:N+1) of calc_zslice at rho, u or v points, on cells 1..Mm x 1..Lm."""
    zr = m.get("z_r") if zr is None else zr
    zw = m.get("z_w") if zw is None else zw
    N = m.N
    if g == "r":
        zz = np.concatenate([zw[0:1] - zw[N], zr - zw[N], (zw[N] - zw[N])[None]])
    else:
        ax = -1 if g == "u" else -2
        zrn, zwn = np.roll(zr, 1, axis=ax), np.roll(zw, 1, axis=ax)   # a(i-1,j) / a(i,j-1)
        if g == "u":
            surf = 0.5 * (zwn[N] + zw[N])
            z0 = 0.5 * (zwn[0] + zw[0]) - surf
        else:
            surf = 0.5 * (zw[N] + zwn[N])
            z0 = 0.5 * (zw[0] + zwn[0]) - surf
        zz = np.concatenate([z0[None], 0.5 * (zr + zrn) - surf, (surf - surf)[None]])
    return inner(zz, m)


def restate(var, zz, rmask, zlev):
    """sigma_to_z for one depth: (values, classes) on the arrays' cells."""
    N = var.shape[0]
    dpth = zz[N + 1] - zz[0]
    cls = np.full(dpth.shape, -1)
    out = np.zeros(dpth.shape)
    todo = np.ones(dpth.shape, bool)

    def take(cond, c):
        hit = todo & cond
        cls[hit] = c
        todo[hit] = False
        return hit

    take(rmask < 0.5, MASKED)
    take(dpth * (zlev - zz[N + 1]) > 0.0, ABOVE)
    top = take(dpth * (zlev - zz[N]) > 0.0, TOP)
    take(dpth * (zz[0] - zlev) > 0.0, BELOW)
    bot = take(dpth * (zz[1] - zlev) > 0.0, BOTTOM)
    with np.errstate(all="ignore"):
        vtop = var[N - 1] + (zlev - zz[N]) * (var[N - 1] - var[N - 2]) / (zz[N] - zz[N - 1])
        vbot = var[0] - (zz[1] - zlev) * (var[1] - var[0]) / (zz[2] - zz[1])
        out[top] = vtop[top]
        out[bot] = vbot[bot]
        for k in range(N - 1, 0, -1):   # the first k from above wins: at an exact tie the higher k
            prod = (zz[k + 1] - zlev) * (zlev - zz[k])
            hit = take(prod >= 0.0, INTERIOR)
            cls[hit & (prod == 0.0)] = TIE
            vin = (var[k - 1] * (zz[k + 1] - zlev) + var[k] * (zlev - zz[k])) / (zz[k + 1] - zz[k])
            out[hit] = vin[hit]
    assert not todo.any()
    return out, cls


def fields(m, slot="nnew"):
    """name -> (grid, var(N, Mm, Lm)) of what calc_zslice samples: u, v, t in slot nnew."""
    s, N = (m.t.nnew if slot == "nnew" else m.t.nstp), m.N
    tr = m.get("t").reshape(m.NT, 3, N, *m.shape2)[:, s - 1]
    out = dict(u=("u", inner(m.get("u")[(s - 1) * N:s * N], m)), v=("v", inner(m.get("v")[(s - 1) * N:s * N], m)))
    for q in range(m.NT):
        out["t%d" % (q + 1)] = ("r", inner(tr[q], m))
    return out


def expected(m, depths, slot="nnew"):
    """name -> (slices (ndep, Mm, Lm), classes) by the restatement."""
    zz = {g: zz_of(m, g) for g in "ruv"}
    rm = inner(m.get("rmask")[0], m)
    out = {}
    for name, (g, var) in fields(m, slot).items():
        r = [restate(var, zz[g], rm, z) for z in depths]
        out[name] = (np.stack([x[0] for x in r]), np.stack([x[1] for x in r]))
    return out


def got(m, name):
    return inner(m.zslice("t", int(name[1:])) if name[0] == "t" else m.zslice(name), m)


def fixture_depths(m):
    """The fixture depths, chosen from the downloaded z: above the surface, in every column's top half-layer, two
    mid-depths, zz(2) of one wet column not on the rim (an exact tie), between the shallowest bottom and the
    shallowest lowest level, and below every bottom.  Returns (depths, (jc, ic)) in cells-1.. indices."""
    zz = zz_of(m, "r")
    wet = inner(m.get("rmask")[0], m) >= 0.5
    N = m.N
    hmax = (zz[N + 1] - zz[0])[wet].max()
    cand = np.argwhere(wet[1:-1, 1:-1]) + 1
    jc, ic = cand[len(cand) // 2]
    tie = zz[2][jc, ic]
    d = [1.0, 0.5 * zz[N][wet].max(), -0.3 * hmax, tie, 0.5 * (zz[0][wet].max() + zz[1][wet].max()), -0.7 * hmax, -2.0 * hmax]
    return [float(x) for x in d], (int(jc), int(ic))


def check(m, want, what=""):
    for name, (val, _) in want.items():
        a = got(m, name)
        assert a.shape == val.shape and np.isfinite(val).all(), (what, name)
        assert np.array_equal(a, val), (what, name, int(np.count_nonzero(a != val)))


def class_counts(want, name="t1"):
    return [int(np.count_nonzero(want[name][1] == c)) for c in range(7)]


@pytest.mark.parametrize("case,N", [("rivers", 5), ("pipes", 5), ("filament", 12), ("basin", 2)])
def test_snapshot_equals_numpy_restatement(case, N):
    m = _model(case, N)
    assert m.N == N
    if N == 2:   # the single bracket: the initial grid under seeded fields in every slot, no step at this depth
        rng = np.random.default_rng(2)
        for name in ("u", "v", "t"):
            a = m.get(name)
            m.put(name, a + rng.uniform(-1.0, 1.0, a.shape))
    else:
        m.step(3)
    depths, (jc, ic) = fixture_depths(m)
    tracers = tuple(range(1, m.NT + 1))
    m.zslice_begin(depths, T | U | V, tracers)
    assert m.zslice_state() == (0, T | U | V, len(depths), False)
    m.calc_zslice()
    want = expected(m, depths)
    counts = class_counts(want)
    print(case, N, dict(zip(CLASS_NAMES, counts)))
    check(m, want, case)
    assert np.abs(want["u"][0]).max() > 0 and np.abs(want["t1"][0]).max() > 0
    # the tie column: the depth is its zz(2) exactly, and the value is the higher-k bracket's formula
    zz, var = zz_of(m, "r"), fields(m)["t1"][1]
    k = min(2, N - 1)   # at N = 2 the depth is zz(N): no top half-layer (not > 0), the single bracket k = 1
    assert want["t1"][1][3, jc, ic] == TIE
    zl = depths[3]
    hk = (var[k - 1, jc, ic] * (zz[k + 1, jc, ic] - zl) + var[k, jc, ic] * (zl - zz[k, jc, ic])) / (zz[k + 1, jc, ic] - zz[k, jc, ic])
    assert got(m, "t1")[3, jc, ic] == hk
    if case in ("rivers", "pipes"):   # every branch of the classification holds a cell
        assert all(c > 0 for c in counts), dict(zip(CLASS_NAMES, counts))
    # negative controls: slot nstp in place of nnew is another slice, and so is a field sliced as another's
    if N > 2:
        wrong = expected(m, depths, slot="nstp")
        assert not np.array_equal(got(m, "u"), wrong["u"][0]) or not np.array_equal(got(m, "t1"), wrong["t1"][0])
    assert not np.array_equal(got(m, "u"), want["v"][0])
    # cells outside 1..Lm x 1..Mm are never written
    full = m.zslice("u")
    assert not full[:, :2].any() and not full[:, -2:].any() and not full[:, :, :2].any() and not full[:, :, -2:].any()
    m.close()


@pytest.mark.parametrize("ndep", [1, 32])
def test_one_and_thirty_two_unsorted_repeated_depths(ndep):
    m = _model("rivers")
    m.step(3)
    base, _ = fixture_depths(m)
    rng = np.random.default_rng(5)
    depths = [base[2]] if ndep == 1 else [float(x) for x in rng.permutation((base * 5)[:32])]   # four chunks of the search
    assert len(depths) == ndep and (ndep == 1 or len(set(depths)) < ndep)
    m.zslice_begin(depths, T | U | V, (2, 1))   # the tracers in another order: q follows `tracers`
    m.calc_zslice()
    want = expected(m, depths)
    assert np.array_equal(got(m, "t1"), want["t2"][0]) and np.array_equal(got(m, "t2"), want["t1"][0])
    assert np.array_equal(inner(m.zslice("temp"), m), want["t1"][0]) and np.array_equal(inner(m.zslice("salt"), m), want["t2"][0])
    assert np.array_equal(got(m, "u"), want["u"][0]) and np.array_equal(got(m, "v"), want["v"][0])
    m.close()


def test_running_mean_equals_numpy_recurrence(tmp_path):
    p = str(tmp_path / "win.nc")
    m = _model("rivers")
    m.step(3)
    depths, _ = fixture_depths(m)
    m.zslice_begin(depths, T | U | V, (1, 2), avg=True)
    for window in range(2):
        avg, navg = {}, 0
        for n in range(4 if window == 0 else 2):
            m.step(1)
            m.calc_zslice()
            navg += 1
            coef = 1.0 / navg
            for name, (x, _) in expected(m, depths).items():
                avg[name] = x * coef if navg == 1 else avg[name] * (1.0 - coef) + x * coef
            assert m.zslice_state()[0] == navg
            check(m, {k: (v, None) for k, v in avg.items()}, "window %d sample %d" % (window, navg))
        m.wrt_zslice(p, window + 1, window + 1, m.time(20.0))
        assert m.zslice_state() == (0, T | U | V, len(depths), True)   # the next window starts fresh
    m.io_wait()
    m.close()


def test_streaming_path_equals_vgrid_path():
    m = _model("pipes")
    m.step(3)
    depths, _ = fixture_depths(m)
    m.zslice_begin(depths, T | U | V, (1, 2))
    assert m.vgrid()[1]
    m.calc_zslice()
    a = {k: m.zslice(*k) for k in (("u",), ("v",), ("t", 1), ("t", 2))}
    m.put("z_r", m.get("z_r"))   # a host write of z_r ends VGrid's validity: the kernel streams z_r, z_w
    assert not m.vgrid()[1]
    m.calc_zslice()
    for k, v in a.items():
        assert np.array_equal(m.zslice(*k), v), k
    check(m, expected(m, depths), "streaming")
    m.close()


def test_the_slices_file(tmp_path):
    p, p2 = str(tmp_path / "zsl_avg.nc"), str(tmp_path / "zsl.nc")
    m = _model("rivers")
    m.step(2)
    depths, _ = fixture_depths(m)
    L, M = m.Lm, m.Mm
    m.zslice_begin(depths, T | U | V, (1, 2), avg=True)
    recs = []
    for r in (1, 2):
        for _ in range(2):
            m.step(1)
            m.calc_zslice()
        recs.append({k: m.zslice(k) for k in ("temp", "salt", "u", "v")})
        m.wrt_zslice(p, r, r, m.time(20.0))
        recs[-1]["time"], recs[-1]["iic"] = m.time(20.0), m.t.iic
    m.io_wait()
    # a snapshot file: wrt_zslice samples by itself
    m.zslice_begin(depths[:3], T | U, (2,))
    m.step(1)
    m.wrt_zslice(p2, 1, 1, m.time(20.0))
    m.io_wait()
    snap = dict(salt=m.zslice("salt"), u=m.zslice("u"))
    want = expected(m, depths[:3])
    assert np.array_equal(inner(snap["salt"], m), want["t2"][0]) and np.array_equal(inner(snap["u"], m), want["u"][0])
    m.close()
    from scipy.io import netcdf_file
    d = read(p)
    assert d["_dims"]["depth"] == len(depths) and d["_dims"]["xi_rho"] == L + 2 and d["_dims"]["xi_u"] == L + 1 and \
        d["_dims"]["eta_rho"] == M + 2 and d["_dims"]["eta_v"] == M + 1
    assert d["depth"].tolist() == depths
    assert d["ocean_time"].tolist() == [recs[0]["time"], recs[1]["time"]]
    with netcdf_file(p, "r", mmap=False) as nc:
        meta = {k: (v.dimensions, getattr(v, "long_name", None), getattr(v, "units", None)) for k, v in nc.variables.items()}
    assert set(meta) == {"ocean_time", "time_step", "depth", "temp", "salt", "u", "v"}
    assert meta["depth"][0] == ("depth",)
    assert meta["temp"] == (("time", "depth", "eta_rho", "xi_rho"), b"averagedpotential temperature", b"Celsius")
    assert meta["salt"] == (("time", "depth", "eta_rho", "xi_rho"), b"averagedsalinity", b"PSU")
    assert meta["u"] == (("time", "depth", "eta_rho", "xi_u"), b"averaged u-momentum component", b"meter second-1")
    assert meta["v"] == (("time", "depth", "eta_v", "xi_rho"), b"averaged v-momentum component", b"meter second-1")
    for r, rec in enumerate(recs):
        assert d["time_step"][r].tolist() == [rec["iic"], r + 1, r + 1, 0, 0, 0]
        for name, g in (("temp", "r"), ("salt", "r"), ("u", "u"), ("v", "v")):
            f = d[name][r]
            assert np.array_equal(f, slab(rec[name], g, L, M)), (r, name)
            i0, j0 = (0 if g == "u" else 1), (0 if g == "v" else 1)   # cells 1..Lm x 1..Mm inside the partition range
            core = np.zeros(f.shape[1:], bool)
            core[j0:j0 + M, i0:i0 + L] = True
            assert not f[:, ~core].any() and f[:, core].any(), (r, name)
    assert not np.array_equal(d["u"][0], d["u"][1])
    d2 = read(p2)
    assert d2["depth"].tolist() == depths[:3] and set(d2) - {"_attrs", "_dims"} == {"ocean_time", "time_step", "depth", "salt", "u"}
    with netcdf_file(p2, "r", mmap=False) as nc:
        assert nc.variables["salt"].long_name == b"salinity" and nc.variables["u"].long_name == b"u-momentum component"
    assert np.array_equal(d2["salt"][0], slab(snap["salt"], "r", L, M)) and np.array_equal(d2["u"][0], slab(snap["u"], "u", L, M))


def test_partitioned_slices_join_to_single_domain(tmp_path):
    dt = FIL["dt"]
    single = str(tmp_path / "single_zsl.nc")
    m = romsgpu.Model.from_case(**FIL)
    m.step(3)
    depths, _ = fixture_depths(m)
    m.zslice_begin(depths, T | U | V, (1,))
    m.wrt_zslice(single, 1, 1, m.time(dt))
    m.io_wait()
    m.close()
    npx, npe = 2, 2
    paths = [str(tmp_path / ("zsl.%d.nc" % r)) for r in range(npx * npe)]
    errs = []

    def work(rank):
        try:
            h = romsgpu.comm_create_local(779, npx * npe, rank)
            mm = romsgpu.Model.from_case(np_xi=npx, np_eta=npe, comm=h, rank=rank, **FIL)
            mm.step(3)
            mm.zslice_begin(depths, T | U | V, (1,))
            mm.wrt_zslice(paths[rank], 1, 1, mm.time(dt))
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
    a = read(paths[3])
    assert list(a["_attrs"]["partition"])[:2] == [3, 4] and a["depth"].tolist() == depths
    joined = join(paths)
    ref = read(single)
    for name in ("temp", "u", "v"):
        assert np.abs(ref[name]).max() > 0
        assert np.array_equal(joined[name], ref[name]), name


def test_errors(tmp_path):
    p = str(tmp_path / "none.nc")
    m = romsgpu.Model.from_case(**FIL)
    for fn, args in ((m.calc_zslice, ()), (m.wrt_zslice, (p, 1, 1, 5.0)), (m.zslice, ("u",))):
        with pytest.raises(romsgpu.RomsGpuError, match="not armed|not being sliced"):
            fn(*args)
    for bad in ([], [-1.0] * 33):
        with pytest.raises(romsgpu.RomsGpuError, match="ndep"):
            m.zslice_begin(bad)
    for bad in ((0,), (m.NT + 1,), (1, m.NT + 1)):
        with pytest.raises(romsgpu.RomsGpuError, match="tracer index"):
            m.zslice_begin([-1.0], T, bad)
    with pytest.raises(romsgpu.RomsGpuError, match="nt_z"):
        m.zslice_begin([-1.0], T, ())
    assert m.zslice_state() == (0, 0, 0, False)   # a refused call arms nothing
    m.zslice_begin([-1.0, -2.0], T | U, (1,), avg=True)
    assert m.zslice_state() == (0, T | U, 2, True)
    with pytest.raises(romsgpu.RomsGpuError, match="no sample"):
        m.wrt_zslice(p, 1, 1, 5.0)
    m.io_wait()
    assert not os.path.exists(p)
    with pytest.raises(romsgpu.RomsGpuError, match="not being sliced"):
        m.zslice("v")
    with pytest.raises(romsgpu.RomsGpuError, match="no such sliced tracer"):
        m.zslice("t", 2)
    buf = np.empty(2 * m.shape2[0] * m.shape2[1] + 1)
    assert m.L.roms_gpu_zslice_copy_out(U, 0, buf.ctypes.data, buf.size) == -1
    assert b"count" in m.L.roms_gpu_last_error()
    assert m.L.roms_gpu_zslice_copy_out(U, 0, buf.ctypes.data, buf.size - 1) == 0
    m.zslice_begin([-1.0], what=0)
    assert m.zslice_state() == (0, 0, 0, False)
    with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
        m.calc_zslice()
    m.close()


def test_the_step_is_untouched():
    def run(armed):
        m = romsgpu.Model.from_case(**FIL)
        if armed:
            m.zslice_begin([-2.0, -15.0, -30.0], T | U | V, (1,), avg=True)
        for _ in range(6):
            m.step(1)
            if armed:
                m.calc_zslice()
        out = {k: m.get(k) for k in ("zeta", "u", "v", "t")}
        m.close()
        return out

    a, b = run(True), run(False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
