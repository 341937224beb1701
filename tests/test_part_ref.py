"""tests/part_ref.py, the numpy restatement of do_particles (particles.F) that
every GPU test of the particles takes its expected values from, checked on
the CPU: analytic flows, the half-level extrapolation, every leaving
direction with its adjusted coordinates, and a 2 x 2 split against the
single domain on the CPU oracle's small basin.

The eight-direction list.  The model's own currents move a particle 1e-5 to
1e-3 cells per call and, at the one interior corner of a 2 x 2 basin, in one
quadrant only, so no list reaches all eight neighbours by them within 6
calls.  The velocities are therefore analytic (`quadrant_flow`: uniform on a
level, 0.2 cells per call, the four sign pairs (+,+) (+,-) (-,+) (-,-) on
levels 1..4) with the same halos on every rank, while Hz, We, Wi, pm, pn stay
the oracle's.  `eight_list` puts particles on rho levels 1..4 a tenth of a
cell from the interior corner (one per quadrant: the four diagonal moves) and
from the two interior rank edges, jittered by default_rng(20260) within
+-0.03 cells; with periodic directions the same pattern sits at the domain's
own corner, which is a rank corner too.  test_two_by_two_* checks with the
restatement alone that all eight directions carry a particle within 6 calls
and no particle is lost.

Local coordinates round differently from global ones, so the joined 2 x 2
positions differ from the single domain's.  Measured here over 6 calls: at
most 7.105e-15 (basin, LLm = 36) and 1.066e-14 (periodic 32 x 24) in px, py,
i.e. one and one and a half ulp(LLm) = 7.1e-15, below calls x ulp(LLm); the
tests allow ten times the measured value.
"""
import numpy as np
import pytest

import oracle
import part_ref
from part_ref import Rank, Ranks

SEED = 20260
CALLS = 6
# ten times the largest |position difference| measured between the joined 2 x 2 run and the single domain
POS_BOUND = {"basin": 10 * 7.105e-15, "periodic": 10 * 1.066e-14}


def basin_cfg(LLm=36, MMm=11, N=5, dt=60.0, sizex=72e3, sizey=22e3):
    """The closed basin of tests/test_gpu_wvlcty.py (BASIN) for the oracle."""
    c = oracle.OrCfg()
    c.LLm, c.MMm, c.N, c.NT = LLm, MMm, N, 2
    c.ew_periodic = c.ns_periodic = 0
    c.salinity, c.nonlin_eos, c.lmd = 1, 1, 0
    c.case_id = oracle.CASE_BASIN
    c.dt, c.ndtfast = dt, 30
    c.theta_s, c.theta_b, c.hc, c.rho0 = 6.0, 2.0, 250.0, 1027.5
    c.rdrg, c.rdrg2, c.Zob = 0.0, 1.0e-3, 1.0e-2
    c.Akv_bak = 1.0e-4
    c.Akt_bak[0] = c.Akt_bak[1] = 1.0e-5
    c.Tcoef, c.T0, c.Scoef, c.S0 = 0.20, 1.0, 0.822, 1.0
    c.sizex, c.sizey = sizex, sizey
    c.diag_np_xi = c.diag_np_eta = 1
    return c


def quadrant_flow(N, shape2, dt, pm0, pn0, cells=0.2):
    """u, v of one time slot, (N, Mm+4, Lm+4): `cells` cells per call, signs by level (+,+) (+,-) (-,+) (-,-)."""
    u, v = np.zeros((N,) + shape2), np.zeros((N,) + shape2)
    for k in range(1, N + 1):
        u[k - 1] = (1.0 if (k - 1) % 4 < 2 else -1.0) * cells / (dt * pm0)
        v[k - 1] = (1.0 if (k - 1) % 2 == 0 else -1.0) * cells / (dt * pn0)
    return u, v


def eight_list(LL, MM, xc, yc, periodic):
    """Global (px, py, pz) of the eight-direction list (module docstring)."""
    rng = np.random.default_rng(SEED)
    near = [(-0.1, -0.1), (0.1, -0.1), (-0.1, 0.1), (0.1, 0.1),      # the corner: one per quadrant
            (-0.1, -2.3), (0.1, 2.3), (-2.3, -0.1), (2.3, 0.1)]      # the two rank edges
    pts = []
    for k in (1, 2, 3, 4):
        for ox, oy in near:
            pts.append((xc + ox, yc + oy, k - 0.5))
            if periodic:   # the same pattern about the domain's own corner
                pts.append(((ox + LL) % LL, (oy + MM) % MM, k - 0.5))
    p = np.array(pts)
    p[:, :2] += rng.uniform(-0.03, 0.03, size=(len(p), 2))
    if periodic:
        p[:, 0] %= LL
        p[:, 1] %= MM
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def uniform_rank(nx=12, ny=9, nz=6, dt=30.0, U=0.05, V=-0.03, pm=1e-3, pn=2e-3, hz=7.0, **kw):
    r = Rank(nx, ny, nz, dt, **kw)
    s2 = (ny + 4, nx + 4)
    r.fields(np.full((nz,) + s2, U), np.full((nz,) + s2, V), np.zeros((nz + 1,) + s2), np.zeros((nz + 1,) + s2),
             np.full((nz,) + s2, hz), np.full(s2, pm), np.full(s2, pn))
    return r


def test_uniform_flow_displacement():
    """Constant u = U, v = V, We + Wi = 0, uniform metric: every call's increment is dt*U*pm and dt*V*pn to
    within 16 ulp of itself (eight weights that sum to 1 round by at most that), so after n calls a particle
    has moved n increments, each of the 2n additions into px adding at most half an ulp of the position."""
    r = uniform_rank()
    rng = np.random.default_rng(SEED)
    n0 = 50
    r.add(rng.uniform(2, 9, n0), rng.uniform(3, 6, n0), rng.uniform(0, 6, n0))
    start = r.part.copy()
    dx, dy = 30.0 * 0.05 * 1e-3, 30.0 * -0.03 * 2e-3
    n = 5
    for _ in range(n):
        r.advance()
        assert np.all(np.abs(r.part[:, 7] - dx) <= 16 * np.spacing(abs(dx)))
        assert np.all(np.abs(r.part[:, 8] - dy) <= 16 * np.spacing(abs(dy)))
        assert np.all(r.part[:, 9] == 0.0)
    tol = n * (16 * np.spacing(abs(dx)) + np.spacing(16.0))
    assert np.all(np.abs(r.part[:, 1] - start[:, 1] - n * dx) <= tol)
    assert np.all(np.abs(r.part[:, 2] - start[:, 2] - n * dy) <= tol)
    assert np.array_equal(r.part[:, 3], start[:, 3]) and np.array_equal(r.part[:, 0], start[:, 0])
    assert r.state()["n_range"] == 0 and len(r.part) == n0


def test_half_level_extrapolation_is_linear_in_pz():
    """k is clamped to [1, nz-1], so z leaves [0, 1] below rho level 1 and above rho level nz: with u linear in
    the level, pu is the same linear function of pz there (slope b per level), not a constant."""
    r = uniform_rank(U=0.0, V=0.0)
    a, b = 0.3, 0.07
    for k in range(1, r.nz + 1):
        r.F["u"][k - 1] = a + b * k
    pz = np.array([0.0, 0.1, 0.25, 0.4, 0.5, 3.2, r.nz - 0.5, r.nz - 0.3, r.nz - 0.1, float(r.nz)])
    r.add(np.full(pz.size, 4.25), np.full(pz.size, 3.5), pz)
    r.rhs()
    want = a + b * (pz + 0.5)   # rho level k sits at pz = k - 0.5
    assert np.max(np.abs(r.part[:, 4] - want)) <= 8 * np.spacing(want.max())
    assert r.part[0, 4] < a + b and r.part[-1, 4] > a + b * r.nz   # beyond the end levels' values: extrapolated


def _one(r, px, py, pz=1.5):
    r.part = np.zeros((0, 13))
    r.add([px], [py], [pz])
    return r


@pytest.mark.parametrize("d,pos,want", [
    ("e", (12.25, 4.0), (0.25, 4.0)), ("w", (-0.25, 4.0), (-0.25, 4.0)),
    ("n", (5.0, 9.5), (5.0, 0.5)), ("s", (5.0, -0.5), (5.0, -0.5)),
    ("ne", (12.25, 9.5), (0.25, 0.5)), ("se", (12.25, -0.5), (0.25, -0.5)),
    ("nw", (-0.25, 9.5), (-0.25, 0.5)), ("sw", (-0.25, -0.5), (-0.25, -0.5))])
def test_each_leaving_direction(d, pos, want):
    """nx or ny is subtracted going east or north and nothing going west or south (:684-732); the receiver adds
    nx or ny to what came from its east or north (:746-838)."""
    nx, ny = 12, 9
    r = _one(uniform_rank(exch=(1, 1, 1, 1)), *pos)
    out = r.pack({q: True for q in part_ref.DIRS})
    assert [q for q in out if out[q]] == [d]
    assert (out[d][0][1], out[d][0][2]) == want and r.part[0, 3] == 10 * r.nz and r.count["n_moved"] == 1
    to = uniform_rank(exch=(1, 1, 1, 1))
    to.receive({part_ref.OPP[d]: out[d]})
    h = part_ref.OPP[d]
    back = (want[0] + (nx if "e" in h else 0), want[1] + (ny if "n" in h else 0))
    assert (to.part[0, 1], to.part[0, 2]) == back and 0 <= back[0] <= nx and 0 <= back[1] <= ny
    r.receive({})
    assert len(r.part) == 0   # the sender's copy is dead and goes


def test_the_east_branch_asks_for_the_second_neighbour_and_the_west_branch_does_not():
    """No northern neighbour: east of the rank and north of it goes east with py as it is; west of it and north
    goes into the nw message, which is never sent -- the particle is lost."""
    r = _one(uniform_rank(exch=(1, 1, 0, 0)), 12.25, 9.5)
    act = dict(w=True, e=True, s=False, n=False, sw=False, se=False, nw=False, ne=False)
    out = r.pack(act)
    assert len(out["e"]) == 1 and (out["e"][0][1], out["e"][0][2]) == (0.25, 9.5)
    r = _one(uniform_rank(exch=(1, 1, 0, 0)), -0.25, 9.5)
    out = r.pack(act)
    assert not any(out.values()) and r.count["n_lost"] == 1 and r.part[0, 3] == 10 * r.nz


def test_wrap_and_loss_at_a_closed_edge():
    """One rank, periodic in x, closed in y: a particle past the east edge comes back from the west less nx, one
    past the north wall is lost; pz == nz is not exchanged at all (:684)."""
    r = uniform_rank(exch=(1, 1, 0, 0))
    r.add([12.25, 5.0, 12.5, 3.0], [4.0, 9.25, 4.0, 3.0], [1.5, 1.5, float(r.nz), 2.5])
    r.first = False
    R = Ranks([r], 1, 1, ew_periodic=True)
    sent = r.pack({d: R.peer(0, d) is not None for d in part_ref.DIRS})
    r.receive({h: sent[part_ref.OPP[h]] for h in part_ref.DIRS if R.peer(0, h) is not None})
    assert r.state()["n_lost"] == 1 and r.state()["n_moved"] == 1
    assert r.part[:, 0].tolist() == [3.0, 4.0, 1.0]   # survivors in list order, then the arrival
    assert (r.part[2, 1], r.part[2, 2]) == (0.25, 4.0) and r.part[0, 1] == 12.5


def test_sort_is_stable_by_cell_and_drops_nothing():
    r = uniform_rank(sort=True)
    r.add([3.7, 1.2, 3.1, 1.9], [2.0, 2.0, 2.5, 2.9], [0.5, 0.5, 0.9, 0.1])
    r.order()
    assert r.part[:, 0].tolist() == [2.0, 4.0, 1.0, 3.0]


def split_run(name, sort=False):
    """6 calls of the eight-direction list on the single domain and on 2 x 2 ranks over the same fields."""
    if name == "basin":
        cfg, periodic = basin_cfg(), False
    else:
        cfg, periodic = oracle.filament_cfg(LLm=32, MMm=24, N=16, np_xi=1, np_eta=1), True
    o = oracle.Oracle(cfg)
    o.init()
    o.step(3)
    LL, MM, N = cfg.LLm, cfg.MMm, cfg.N
    F = {k: np.array(o.field(k)) for k in ("We", "Wi", "Hz")}
    pm, pn = np.array(o.field("pm")[0]), np.array(o.field("pn")[0])
    u, v = quadrant_flow(N, (MM + 4, LL + 4), cfg.dt, pm[2, 2], pn[2, 2])
    ext = [[part_ref.rank_extent(LL, 2, q) for q in (0, 1)], [part_ref.rank_extent(MM, 2, q) for q in (0, 1)]]
    xc, yc = ext[0][1][1], ext[1][1][1]
    gx, gy, gz = eight_list(LL, MM, xc, yc, periodic)
    one = Rank(LL, MM, N, cfg.dt, exch=part_ref.exch_flags(1, 1, 0, periodic, periodic), sort=sort)
    one.fields(u, v, F["We"], F["Wi"], F["Hz"], pm, pn)
    one.add(gx, gy, gz)
    ranks = []
    for q in range(4):
        jn, i_n = divmod(q, 2)
        (nx, isw), (ny, jsw) = ext[0][i_n], ext[1][jn]
        r = Rank(nx, ny, N, cfg.dt, exch=part_ref.exch_flags(2, 2, q, periodic, periodic), mynode=q, sort=sort)
        r.fields(*[part_ref.cut(a, isw, jsw, nx, ny) for a in (u, v, F["We"], F["Wi"], F["Hz"], pm, pn)])
        r.sw = (isw, jsw)
        mine = (gx >= isw) & (gx < isw + nx) & (gy >= jsw) & (gy < jsw + ny)
        r.add(gx[mine] - isw, gy[mine] - jsw, gz[mine])
        r.gid = np.flatnonzero(mine)   # the list entry behind each tag of this rank
        ranks.append(r)
    S, R = Ranks([one], 1, 1, periodic, periodic), Ranks(ranks, 2, 2, periodic, periodic)
    used = set()
    for _ in range(CALLS):
        S.do_particles()
        for q, r in enumerate(ranks):
            r.advance()
        sent = [r.pack({d: R.peer(q, d) is not None for d in part_ref.DIRS}) for q, r in enumerate(ranks)]
        for q, r in enumerate(ranks):
            used |= {d for d in part_ref.DIRS if sent[q][d]}
            r.receive({h: sent[R.peer(q, h)][part_ref.OPP[h]] for h in part_ref.DIRS if R.peer(q, h) is not None})
            if sort:
                r.order()
    return one, ranks, used


def joined(ranks):
    """{list entry: (global px, global py, pz)} of the 2 x 2 run."""
    out = {}
    for r in ranks:
        for p in r.part:
            src = ranks[int(p[0]) // part_ref.BIG_NUMBER]
            out[int(src.gid[int(p[0]) % part_ref.BIG_NUMBER - 1])] = (p[1] + r.sw[0], p[2] + r.sw[1], p[3])
    return out


@pytest.mark.parametrize("name", ["basin", "periodic"])
def test_two_by_two_reaches_all_eight_neighbours_and_joins_to_the_single_domain(name):
    """Measured: largest |difference| in px, py, pz 7.105e-15 (basin), 1.066e-14 (periodic); ten times that is allowed."""
    one, ranks, used = split_run(name)
    assert used == set(part_ref.DIRS), used
    assert all(r.count["n_lost"] == 0 and r.count["n_range"] == 0 for r in ranks + [one])
    J = joined(ranks)
    assert sorted(J) == list(range(len(one.part))) == sorted(int(t) - 1 for t in one.part[:, 0])
    LL, MM = (36, 11) if name == "basin" else (32, 24)
    worst = 0.0
    for p in one.part:
        g = J[int(p[0]) - 1]
        dx, dy = abs(g[0] - p[1]), abs(g[1] - p[2])
        if name == "periodic":   # the same point of the torus
            dx, dy = min(dx, abs(dx - LL)), min(dy, abs(dy - MM))
        worst = max(worst, dx, dy, abs(g[2] - p[3]))
    print("largest position difference, 2 x 2 against the single domain (%s): %.3e" % (name, worst))
    assert worst <= POS_BOUND[name]
    assert sum(r.count["n_moved"] for r in ranks) >= 8
