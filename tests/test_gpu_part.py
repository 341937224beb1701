"""Lagrangian particles on the device (particles.F):
k_particles.hip behind Model.part_begin / part_add / do_particles / particles /
wrt_part.

The expected values never come from the library: they are the numpy
restatement of do_particles (tests/part_ref.py, checked by
tests/test_part_ref.py) over arrays downloaded with Model.get after the step.
The kernels evaluate the reference's operations in the reference's order
without contraction, and compaction and packing are stable, so every
comparison is np.array_equal on the whole np x 13 list, order included.
Positions of a 2 x 2 run against the single domain are held to
test_part_ref.POS_BOUND, ten times what the restatement itself measures
(7.105e-15 basin, 1.066e-14 periodic).
"""
import threading

import numpy as np
import pytest

import part_ref
import romsgpu
from part_ref import Rank, Ranks
from test_gpu_io import read
from test_gpu_wvlcty import BASIN, TINY, periodic
from test_part_ref import CALLS, POS_BOUND, SEED, eight_list, quadrant_flow

pytestmark = pytest.mark.gpu

BLOCK = 256   # lanes per block of the per-particle kernels (k_particles.hip kPB)


def ref_rank(m, case, rank=0, npx=1, npe=1, **kw):
    per = periodic(case)
    return Rank(m.Lm, m.Mm, m.N, case["dt"], exch=part_ref.exch_flags(npx, npe, rank, per, per), mynode=rank, **kw)


def same(m, r, what=""):
    got = m.particles()
    assert got.shape == r.part.shape, (what, got.shape, r.part.shape)
    assert np.array_equal(got, r.part), (what, np.argwhere(got != r.part)[:5])
    s = m.part_state()
    assert s == r.state(), (what, s, r.state())


def call(m, r, case, step=True, what=""):
    """One step (or none), do_particles on the device and in the restatement over the downloaded fields."""
    if step:
        m.step(1)
    m.do_particles()
    part_ref.of_model(m, r)
    per = periodic(case)
    Ranks([r], 1, 1, per, per).do_particles()
    same(m, r, what)


def cloud(m, n, rng, lo=0.0):
    return rng.uniform(lo, m.Lm - lo, n), rng.uniform(lo, m.Mm - lo, n), rng.uniform(0, m.N, n)


def put_slot(m, name, plane_fn):
    """Overwrite slot nnew of u or v through roms_gpu_copy_in; plane_fn(k) -> value or plane of level k."""
    a, N, s = m.get(name), m.N, m.t.nnew
    for k in range(1, N + 1):
        a[(s - 1) * N + k - 1] = plane_fn(k)
    m.put(name, a)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK + 1])
def test_counts_against_the_wavefront_and_the_block(n, tmp_path):
    m = romsgpu.Model.from_case(**BASIN)
    m.part_begin(600)
    r = ref_rank(m, BASIN)
    px, py, pz = cloud(m, n, np.random.default_rng(SEED + n))
    m.part_add(px, py, pz)
    r.add(px, py, pz)
    same(m, r, "seeded")
    for s in range(3):
        call(m, r, BASIN, what="step %d" % s)
    assert m.part_state()["np"] == n
    m.wrt_part(str(tmp_path / "p.nc"), 1, 1, 0.0)
    m.io_wait()
    m.close()


def test_positions_that_take_every_branch():
    """px, py exactly 0 and exactly nx, ny; pz in the bottom and the top half level; N = 3, where k is clamped to
    [1, 2]; then a vertical flux written with roms_gpu_copy_in drives one particle below 0 and one above nz."""
    case = dict(BASIN, N=3)
    m = romsgpu.Model.from_case(**case)
    nx, ny, nz = m.Lm, m.Mm, m.N
    m.part_begin(64)
    r = ref_rank(m, case)
    px = [0.0, float(nx), 5.5, 7.25, 0.0, float(nx), 9.0, 11.0, 13.5, 14.5, 20.0, 21.0]
    py = [3.0, 4.0, 0.0, float(ny), 0.0, float(ny), 5.0, 6.0, 5.5, 2.5, 5.0, 5.0]
    pz = [1.2, 1.7, 0.4, 2.3, 1.5, 1.5, 0.2, nz - 0.2, 0.0, float(nz), 0.3, nz - 0.3]
    m.part_add(px, py, pz)
    r.add(px, py, pz)
    m.step(1)
    call(m, r, case, step=False, what="branches")
    # We: downwards in the lower half, upwards in the upper, at least 0.7 levels per call
    We = m.get("We")
    A = 0.7 * m.get("Hz").max() / (case["dt"] * m.get("pm")[0][3, 3] * m.get("pn")[0][3, 3])
    for k in range(nz + 1):
        We[k] = -A if k < 2 else A
    m.put("We", We)
    m.put("Wi", np.zeros_like(We))
    keep = (r.part[:, 0] == 11) | (r.part[:, 0] == 12)
    assert keep.sum() == 2
    before = dict(r.state())
    call(m, r, case, step=False, what="clamps")
    s = m.part_state()
    assert s["n_bot"] - before["n_bot"] >= 1 and s["n_sur"] - before["n_sur"] >= 1
    got = {int(p[0]): p[3] for p in m.particles()}
    assert got[11] == 0.02 and got[12] == nz - 0.02
    m.close()


def _both_orders(case, extra):
    """6 steps with 200 random particles, the cell ordering off and on; extra(m, r, tag): more calls."""
    out = []
    for sort in (False, True):
        m = romsgpu.Model.from_case(**case)
        m.part_begin(400, sort=sort)
        r = ref_rank(m, case, sort=sort)
        px, py, pz = cloud(m, 200, np.random.default_rng(SEED))
        m.part_add(px, py, pz)
        r.add(px, py, pz)
        for s in range(6):
            call(m, r, case, what="sort %d step %d" % (sort, s))
        extra(m, r, "sort %d" % sort)
        out.append(m.particles())
        m.close()
    a, b = out
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert np.array_equal(a[np.argsort(a[:, 0])], b[np.argsort(b[:, 0])])   # the same particles, another order
    return out


def test_filament_random_particles_wrap_in_both_directions():
    """Six stepped calls, then three without stepping in a constant flow written with roms_gpu_copy_in (0.4 cells
    per call towards the north-east): particles within a cell of the east and north edges wrap."""
    case = TINY

    def extra(m, r, tag):
        pm, pn = m.get("pm")[0][3, 3], m.get("pn")[0][3, 3]
        put_slot(m, "u", lambda k: 0.4 / (case["dt"] * pm))
        put_slot(m, "v", lambda k: 0.4 / (case["dt"] * pn))
        start = {int(p[0]): (p[1], p[2]) for p in m.particles()}
        moved0 = m.part_state()["n_moved"]
        for s in range(3):
            call(m, r, case, step=False, what="%s flow %d" % (tag, s))
        end = {int(p[0]): (p[1], p[2]) for p in m.particles()}
        assert sorted(end) == sorted(start) and m.part_state()["n_lost"] == 0
        assert any(end[t][0] < start[t][0] for t in end) and any(end[t][1] < start[t][1] for t in end)
        assert m.part_state()["n_moved"] > moved0

    _both_orders(case, extra)


def test_basin_random_particles_and_a_loss_at_the_wall():
    """... and a particle a tenth of a cell from the east wall, in an outflow set up by roms_gpu_copy_in of a
    constant u(nnew), is lost: n_lost counts it."""
    case = BASIN

    def extra(m, r, tag):
        n0, lost0 = m.part_state()["np"], m.part_state()["n_lost"]
        m.part_add([m.Lm - 0.1], [5.0], [2.5])
        r.add([m.Lm - 0.1], [5.0], [2.5])
        put_slot(m, "u", lambda k: 0.4 / (case["dt"] * m.get("pm")[0][3, 3]))
        call(m, r, case, step=False, what=tag + " outflow")
        s = m.part_state()
        assert s["n_lost"] >= lost0 + 1 and s["np"] <= n0
        assert m.part_state()["ntag"] == 201 and 201 not in m.particles()[:, 0]

    _both_orders(case, extra)


def test_uniform_flow_displacement_and_the_start_of_later_additions():
    """Fields written with roms_gpu_copy_in, do_particles called without stepping: constant u, v, We + Wi = 0,
    constant Hz, the basin's uniform metric.  Every increment is dt*U*pm, dt*V*pn within 16 ulp (eight weights
    that sum to 1 round by at most that); additions into px round by half an ulp of the position each.  A particle
    added before the first call starts with dm = d (it moves d), one added later from dm = 0 (it moves 1.5 d)."""
    case = BASIN
    m = romsgpu.Model.from_case(**case)
    m.step(1)
    U, V = 0.05, -0.03
    put_slot(m, "u", lambda k: U)
    put_slot(m, "v", lambda k: V)
    m.put("We", np.zeros_like(m.get("We")))
    m.put("Wi", np.zeros_like(m.get("Wi")))
    m.put("Hz", np.full_like(m.get("Hz"), 7.0))
    pm, pn = m.get("pm")[0][3, 3], m.get("pn")[0][3, 3]
    assert np.ptp(m.get("pm")[0]) == 0 and np.ptp(m.get("pn")[0]) == 0
    dx, dy = case["dt"] * U * pm, case["dt"] * V * pn
    m.part_begin(200)
    r = ref_rank(m, case)
    px, py, pz = cloud(m, 100, np.random.default_rng(SEED), lo=2.0)
    m.part_add(px, py, pz)
    r.add(px, py, pz)
    start = m.particles()
    n = 5
    for s in range(n):
        if s == 1:
            m.part_add([10.0], [5.0], [2.5])
            r.add([10.0], [5.0], [2.5])
        call(m, r, case, step=False, what="call %d" % s)
        P = m.particles()
        assert np.all(np.abs(P[:, 7] - dx) <= 16 * np.spacing(abs(dx))) and np.all(np.abs(P[:, 8] - dy) <= 16 * np.spacing(abs(dy)))
        assert np.all(P[:, 9] == 0.0)
        if s == 0:
            assert np.all(np.abs(P[:, 1] - start[:, 1] - dx) <= 16 * np.spacing(abs(dx)) + np.spacing(64.0))
        if s == 1:
            late = P[P[:, 0] == 101][0]
            assert abs(late[1] - 10.0 - 1.5 * dx) <= 24 * np.spacing(abs(dx)) + np.spacing(16.0)
            assert abs(late[2] - 5.0 - 1.5 * dy) <= 24 * np.spacing(abs(dy)) + np.spacing(8.0)
    P = m.particles()[:100]
    tol = n * (16 * np.spacing(abs(dx)) + np.spacing(64.0))
    assert np.all(np.abs(P[:, 1] - start[:, 1] - n * dx) <= tol) and np.all(np.abs(P[:, 2] - start[:, 2] - n * dy) <= tol)
    assert np.array_equal(P[:, 3], start[:, 3]) and np.array_equal(P[:, 0], start[:, 0])
    m.close()


def _flow_setup(m, case):
    """One real step, then the analytic quadrant flow in u, v(nnew) (tests/test_part_ref.py)."""
    m.step(1)
    pm, pn = m.get("pm")[0][3, 3], m.get("pn")[0][3, 3]
    u, v = quadrant_flow(m.N, m.shape2, case["dt"], pm, pn)
    put_slot(m, "u", lambda k: u[k - 1])
    put_slot(m, "v", lambda k: v[k - 1])


def _two_by_two(case, tmp_path, tag, group, stepped=False, rng_extra=0):
    """The eight-direction list on 2 x 2 ranks (threads over comm_create_local) and on the single domain.
    stepped: real steps before every call instead of the analytic flow (the fields then change per call)."""
    per = periodic(case)
    LL, MM = case["LLm"], case["MMm"]
    ext = [[part_ref.rank_extent(LL, 2, q) for q in (0, 1)], [part_ref.rank_extent(MM, 2, q) for q in (0, 1)]]
    gx, gy, gz = eight_list(LL, MM, ext[0][1][1], ext[1][1][1], per)
    if rng_extra:   # on the rank edges exactly, and about them
        rng = np.random.default_rng(SEED + 1)
        ex = np.concatenate([np.full(rng_extra, float(ext[0][1][1])), rng.uniform(1, LL - 1, rng_extra)])
        ey = np.concatenate([rng.uniform(1, MM - 1, rng_extra), np.full(rng_extra, float(ext[1][1][1]))])
        gx, gy = np.concatenate([gx, ex]), np.concatenate([gy, ey])
        gz = np.concatenate([gz, rng.uniform(0, case["N"], 2 * rng_extra)])
    # the single domain on the device
    m = romsgpu.Model.from_case(**case)
    m.part_begin(4 * gx.size)
    m.part_add(gx, gy, gz)
    if not stepped:
        _flow_setup(m, case)
    for _ in range(CALLS):
        if stepped:
            m.step(1)
        m.do_particles()
    single = m.particles(global_=True)
    sfile = str(tmp_path / ("single_%s_part.nc" % tag))
    m.wrt_part(sfile, 1, 1, 1.0)
    m.io_wait()
    assert m.part_state()["n_lost"] == 0
    m.close()
    errs, lists, fields, geo = [], {}, {}, {}
    paths = [str(tmp_path / ("%s_part.%d.nc" % (tag, q))) for q in range(4)]

    def work(rank):
        try:
            h = romsgpu.comm_create_local(group, 4, rank)
            mm = romsgpu.Model.from_case(np_xi=2, np_eta=2, comm=h, rank=rank, **case)
            geo[rank] = (mm.Lm, mm.Mm, mm.iSW, mm.jSW)
            mine = (gx >= mm.iSW) & (gx < mm.iSW + mm.Lm) & (gy >= mm.jSW) & (gy < mm.jSW + mm.Mm)
            mm.part_begin(4 * gx.size)
            mm.part_add(gx[mine] - mm.iSW, gy[mine] - mm.jSW, gz[mine])
            if not stepped:
                _flow_setup(mm, case)
            lists[rank], fields[rank] = [], []
            for _ in range(CALLS):
                if stepped:
                    mm.step(1)
                mm.do_particles()
                rr = Rank(mm.Lm, mm.Mm, mm.N, case["dt"])
                part_ref.of_model(mm, rr)
                fields[rank].append(rr.F)
                lists[rank].append((mm.particles(), mm.part_state()))
            mm.wrt_part(paths[rank], 1, 1, 1.0)
            mm.io_wait()
            mm.close()
            romsgpu.comm_destroy(h)
        except Exception as e:
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(q,)) for q in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
    assert not errs, errs
    # the multi-rank restatement over each rank's downloaded fields
    ranks = []
    for q in range(4):
        nx, ny, isw, jsw = geo[q]
        r = Rank(nx, ny, case["N"], case["dt"], exch=part_ref.exch_flags(2, 2, q, per, per), mynode=q)
        mine = (gx >= isw) & (gx < isw + nx) & (gy >= jsw) & (gy < jsw + ny)
        r.add(gx[mine] - isw, gy[mine] - jsw, gz[mine])
        ranks.append(r)
    R = Ranks(ranks, 2, 2, per, per)
    for c in range(CALLS):
        for q, r in enumerate(ranks):
            r.F = fields[q][c]
        R.do_particles()
        for q, r in enumerate(ranks):
            got, state = lists[q][c]
            assert got.shape == r.part.shape and np.array_equal(got, r.part), (tag, "call", c, "rank", q)
            assert state == r.state(), (tag, c, q, state, r.state())
    if not stepped:
        assert sum(r.count["n_moved"] for r in ranks) >= 8
    assert all(r.count["n_lost"] == 0 and r.count["n_range"] == 0 for r in ranks)
    return single, sfile, ranks, geo, paths, (gx, gy, gz)


@pytest.mark.parametrize("case", [TINY, BASIN], ids=["filament", "basin"])
def test_two_by_two_ranks_equal_the_restatement_and_join_to_the_single_domain(case, tmp_path):
    """Every rank's list equals the multi-rank restatement bit for bit after every call; the union of tags is
    the single domain's; positions agree with the single-domain device run within POS_BOUND; the partitioned
    files' tags join to the single domain's file."""
    per = periodic(case)
    name = "periodic" if per else "basin"
    single, sfile, ranks, geo, paths, (gx, gy, gz) = _two_by_two(case, tmp_path, name, 791 if per else 792)
    LL, MM = case["LLm"], case["MMm"]
    # tags of the 2 x 2 run back to list entries: rank q numbered its share in list order
    share = []
    for q in range(4):
        nx, ny, isw, jsw = geo[q]
        share.append(np.flatnonzero((gx >= isw) & (gx < isw + nx) & (gy >= jsw) & (gy < jsw + ny)))
    J = {}
    for q, r in enumerate(ranks):
        for p in r.part:
            t = int(p[0])
            J[int(share[t // part_ref.BIG_NUMBER][t % part_ref.BIG_NUMBER - 1])] = (p[1] + geo[q][2] + 0.5, p[2] + geo[q][3] + 0.5, p[3])
    assert sorted(J) == sorted(int(t) - 1 for t in single[:, 0]) == list(range(gx.size))
    worst = 0.0
    for p in single:
        g = J[int(p[0]) - 1]
        dx, dy = abs(g[0] - p[1]), abs(g[1] - p[2])
        if per:
            dx, dy = min(dx, abs(dx - LL)), min(dy, abs(dy - MM))
        worst = max(worst, dx, dy, abs(g[2] - p[3]))
    print("largest position difference, 2 x 2 against the single domain on the device (%s): %.3e" % (name, worst))
    assert worst <= POS_BOUND[name]
    # the files: the partitioned set's tags (and global positions) are those of the ranks' lists
    one = read(sfile)
    assert np.array_equal(one["particles"][0, :, :single.shape[0]], single[:, :7].T)
    tags = []
    for q, path in enumerate(paths):
        d = read(path)
        n = len(ranks[q].part)
        want = ranks[q].part[:, :7].copy()
        want[:, 1] += geo[q][2] + 0.5
        want[:, 2] += geo[q][3] + 0.5
        assert np.array_equal(d["particles"][0, :, :n], want.T) and not d["particles"][0, :, n:].any()
        assert int(d["_attrs"]["big_number"]) == part_ref.BIG_NUMBER
        tags += [int(share[int(t) // part_ref.BIG_NUMBER][int(t) % part_ref.BIG_NUMBER - 1]) for t in d["particles"][0, 0, :n]]
    assert sorted(tags) == sorted(int(t) - 1 for t in one["particles"][0, 0, :single.shape[0]])


def test_two_by_two_with_deferred_exchanges_held_back(monkeypatch, tmp_path):
    """The rhs kernel reads the halos of u, v, We, Wi, Hz, whose 3-D exchanges whole steps may defer onto the halo
    stream (ROMS_GPU_XOVERLAP=1).  With every forked exchange's unpack held back and its halo poisoned
    (ROMS_GPU_XDELAY_US) the lists still equal the restatement: do_particles joins what it reads."""
    monkeypatch.setenv("ROMS_GPU_XOVERLAP", "1")
    monkeypatch.setenv("ROMS_GPU_XDELAY_US", "300")
    _two_by_two(TINY, tmp_path, "xov", 793, stepped=True, rng_extra=24)


def test_the_particles_file(tmp_path):
    from scipy.io import netcdf_file
    p = str(tmp_path / "fil_part.nc")
    case = TINY
    m = romsgpu.Model.from_case(**case)
    npmx = 90
    m.part_begin(npmx)
    px, py, pz = cloud(m, 70, np.random.default_rng(SEED))
    m.part_add(px, py, pz)
    recs = []
    for rec in (1, 2):
        m.step(1)
        m.do_particles()
        m.wrt_part(p, rec, 2, m.time(case["dt"]))
        recs.append((m.particles(global_=True), m.particles(), m.time(case["dt"])))
    m.io_wait()
    m.close()
    with netcdf_file(p, "r", mmap=False) as nc:
        v = nc.variables["particles"]
        assert v.dimensions == ("time", "seven", "npart") and v.shape == (2, 7, npmx) and v.long_name == b"Tag/x/y/z/u/v/w"
        assert v.typecode() == "d" and nc.dimensions["npart"] == npmx and nc.dimensions["seven"] == 7
        assert nc.dimensions["time"] is None and int(nc.big_number) == 10000000
        data, times = np.array(v[:]), np.array(nc.variables["ocean_time"][:])
    for q, (glob, local, time) in enumerate(recs):
        n = glob.shape[0]
        assert np.array_equal(data[q, :, :n], glob[:, :7].T) and not data[q, :, n:].any()
        assert np.array_equal(glob[:, 1], local[:, 1] + 0.5) and np.array_equal(glob[:, 2], local[:, 2] + 0.5)
        assert times[q] == time
    assert np.all(data[:, 0, :70] >= 1) and not np.array_equal(data[0], data[1])


def test_the_step_is_untouched():
    def run(armed):
        m = romsgpu.Model.from_case(**TINY)
        if armed:
            m.part_begin(300, sort=True)
            m.part_add(*cloud(m, 200, np.random.default_rng(SEED)))
        for _ in range(6):
            m.step(1)
            if armed:
                m.do_particles()
        out = {k: m.get(k) for k in ("zeta", "u", "v", "t", "FlxU", "FlxV")}
        m.close()
        return out

    a, b = run(True), run(False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_errors(tmp_path):
    m = romsgpu.Model.from_case(**TINY)
    with pytest.raises(romsgpu.RomsGpuError, match="part_begin"):
        m.do_particles()
    m.part_begin(10)
    m.part_add([1.0] * 8, [1.0] * 8, [1.0] * 8)
    before = m.particles()
    with pytest.raises(romsgpu.RomsGpuError, match="npmx"):
        m.part_add([1.0] * 3, [1.0] * 3, [1.0] * 3)
    for bad in (([-0.1], [1.0], [1.0]), ([1.0], [m.Mm + 0.1], [1.0]), ([1.0], [1.0], [m.N + 0.5]), ([np.nan], [1.0], [1.0])):
        with pytest.raises(romsgpu.RomsGpuError, match="outside"):
            m.part_add(*bad)
    assert np.array_equal(m.particles(), before) and m.part_state()["np"] == 8 and m.part_state()["ntag"] == 8
    a = np.empty(13 * 8 - 1)
    assert m.L.roms_gpu_part_copy_out(a.ctypes.data, a.size, 0) == -1
    assert b"count" in m.L.roms_gpu_last_error()
    # a message that holds one particle: two leave to the east in one call
    m.part_begin(10, fac_y=0.12)   # int(0.12 * 10 * 13) = 15 words: one particle
    m.step(1)
    m.part_add([m.Lm - 0.1, m.Lm - 0.2, 5.0], [3.0, 4.0, 5.0], [2.5, 2.5, 2.5])
    put_slot(m, "u", lambda k: 0.4 / (TINY["dt"] * m.get("pm")[0][3, 3]))
    m.do_particles()
    s = m.part_state()
    assert s["n_overflow"] == 1 and s["n_moved"] == 1 and s["np"] == 2
    assert sorted(m.particles()[:, 0]) == [1.0, 3.0]   # the first in list order fitted
    with pytest.raises(romsgpu.RomsGpuError, match="did not fit"):
        m.do_particles()
    with pytest.raises(romsgpu.RomsGpuError, match="did not fit"):
        m.wrt_part(str(tmp_path / "never.nc"), 1, 1, 0.0)
    m.part_begin(10)   # re-arming clears it
    m.do_particles()
    assert m.part_state()["np"] == 0
    m.close()
