"""The coastlines of tests/coasts.py, checked on the CPU oracle alone.

tests/test_gpu_coasts.py compares the HIP kernels with the oracle on these
coasts; here stand the premises of that comparison: derive_masks restates the
oracle's own masks, every coast puts land on the edges it names (coasts.py's
docstring gives the constants and their lines), the oracle runs the coasts
finite and with a live flow, closed and with four open edges, and with the
viscosity on a wrong pmask or one wrong umask cell moves the run by more than
RMS_RUN, so a kernel that reads a mask wrongly cannot pass unnoticed.
"""
import numpy as np
import pytest

import coasts
import oracle
from branch_states import kpp_cfg
from test_gpu_obc import obc_cfg
from test_gpu_parity import PROGNOSTIC, RMS_RUN, interior, rms_abs

# the sizes of tests/test_gpu_coasts.py: (Lm, Mm, N)
SIZES = [(121, 12, 12), (65, 8, 12), (49, 12, 12), (48, 11, 12), (112, 12, 12), (61, 6, 100)]
SIZE_IDS = ["%dx%dx%d" % s for s in SIZES]


def coast_cfg(Lm, Mm, N, obc=0):
    cfg = kpp_cfg(Lm, Mm, N)
    if obc:
        cfg.obc, cfg.ubind, cfg.v_sponge = obc, 0.1, 1.0e3
    return cfg


def cell(a, i, j):
    return a[j + 1, i + 1]


# ---------------------------------------------------------- derive_masks ----
@pytest.mark.parametrize("case", ["island", "pipes", "rivers"])
def test_derive_masks_restates_the_oracle(case):
    """umask, vmask, pmask from the oracle's rmask equal the oracle's own
    (oracle_main.c setup_grid1) over the restated ranges, on the basin's
    island at 66 x 40 and on the Pipes_ana and Rivers_ana coasts; every entry
    outside the ranges keeps the value it had."""
    if case == "island":
        cfg = obc_cfg(LLm=66, MMm=40, N=4)
    else:
        cfg = (oracle.pipes_cfg if case == "pipes" else oracle.rivers_cfg)(LLm=40, MMm=36, N=4, np_xi=1, np_eta=1)
    Lm, Mm = cfg.LLm, cfg.MMm
    o = oracle.Oracle(cfg)
    o.init()
    rm = o.field("rmask")[0].copy()
    assert 0.0 < rm[2:-2, 2:-2].mean() < 1.0
    mine = [np.full(rm.shape, -7.0) for _ in range(3)]
    coasts.derive_masks(rm, *mine, Lm, Mm)
    ranges = {"umask": (slice(1, Mm + 3), slice(2, Lm + 3)), "vmask": (slice(2, Mm + 3), slice(1, Lm + 3)),
              "pmask": (slice(2, Mm + 3), slice(2, Lm + 3))}
    for (name, r), a in zip(ranges.items(), mine):
        ref = o.field(name)[0]
        assert np.array_equal(a[r], ref[r]), name
        kept = np.ones(a.shape, dtype=bool)
        kept[r] = False
        assert (a[kept] == -7.0).all() and (a[r] != -7.0).all(), name
    if case == "island":
        assert sorted(set(mine[2][ranges["pmask"]].ravel())) == [0.0, 1.0, 2.0]


def test_derive_masks_counts_with_integers():
    """A 2 x 2 of four wet cells is pmask 1, three 1, a straight pair 2, a
    diagonal pair 0, one 0, none 0 (setup_grid1.F's four-cell rule)."""
    Lm = Mm = 2
    for wet, want in ((((1, 1), (2, 1), (1, 2), (2, 2)), 1.0), (((1, 1), (2, 1), (1, 2)), 1.0),
                      (((1, 1), (2, 1)), 2.0), (((1, 1), (1, 2)), 2.0), (((1, 1), (2, 2)), 0.0),
                      (((2, 1), (1, 2)), 0.0), (((1, 1),), 0.0), ((), 0.0)):
        rm = np.zeros((Mm + 4, Lm + 4))
        for i, j in wet:
            rm[j + 1, i + 1] = 1.0
        um, vm, pk = (np.zeros_like(rm) for _ in range(3))
        coasts.derive_masks(rm, um, vm, pk, Lm, Mm)
        assert cell(pk, 2, 2) == want, (wet, cell(pk, 2, 2))


# --------------------------------------------------------------- geometry ----
def test_edge_columns_follow_the_constants():
    """The edges of coasts.edge_columns at the widest grid, against the
    columns tests/test_gpu_widths.py's docstring names."""
    e = coasts.edge_columns(121)
    assert e["tiles from i = 0"] == [48, 112] and e["tiles from i = 1"] == [64]
    assert e["strips"] == [60, 120] and e["16-column blocks"] == [16, 32, 48, 64, 80, 96, 112]


def _masks(Lm, Mm, land):
    rm = np.ones((Mm + 4, Lm + 4))
    rm[land] = 0.0
    um, vm, pk = (np.zeros_like(rm) for _ in range(3))
    coasts.derive_masks(rm, um, vm, pk, Lm, Mm)
    return rm, um, vm, pk


@pytest.mark.parametrize("name", list(coasts.COASTS))
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_coast_shares(size, name):
    """Per coast and size: pmask takes all of 0, 1 and 2 over its range, at
    least 0.4 of the interior is wet, the coast band holds at least 30 points."""
    Lm, Mm, _ = size
    rm, _, _, pk = _masks(Lm, Mm, coasts.COASTS[name](Lm, Mm))
    wet, band = rm[2:-2, 2:-2].mean(), int(coasts.coast_band(rm).sum())
    print("%s %dx%d: wet %.2f, band %d" % (name, Lm, Mm, wet, band))
    assert sorted(set(pk[2:Mm + 3, 2:Lm + 3].ravel())) == [0.0, 1.0, 2.0]
    assert wet >= 0.4
    assert band >= 30


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_specks_sit_on_every_edge(size):
    """Every column e-2 .. e+2 of every edge, and 1, 2, Lm-1, Lm, holds a
    land cell; the five columns about an edge hold every row 1 .. Mm (so rows
    1, 2, 3, Mm-1, Mm, 10 / 11 and every residue mod kBY = 4); apart from the
    bar and the diagonal pair no land cell touches another."""
    Lm, Mm, _ = size
    land = coasts.specks(Lm, Mm)
    cols = coasts.speck_columns(Lm)
    assert {1, 2, Lm - 1, Lm} <= set(cols)
    for c in cols:
        assert land[2:Mm + 2, c + 1].any(), c
    for fam, es in coasts.edge_columns(Lm).items():
        assert es or fam != "16-column blocks"
        for e in es:
            if e + 2 > Lm:
                continue   # the lattice needs the five columns inside the grid
            rows = {j for c in range(e - 2, e + 3) for j in range(1, Mm + 1) if cell(land, c, j)}
            assert rows == set(range(1, Mm + 1)), (fam, e, rows)
    lone = land.copy()
    for i, j in coasts.speck_extras(Lm, Mm):
        assert cell(land, i, j)
        lone[j + 1, i + 1] = False
    p = np.pad(lone, 1).astype(int)
    around = sum(p[dj:dj + lone.shape[0], di:di + lone.shape[1]] for dj in range(3) for di in range(3))
    assert (around[lone] == 1).all()
    assert not land[:2].any() and not land[-2:].any() and not land[:, :2].any() and not land[:, -2:].any()


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_channels_are_one_cell_wide(size):
    """Every eta channel is a wet column through the slab on an edge column
    (e or e+1) with land on both sides, umask 0 on both its flanks and vmask 1
    along it; the xi channel joins the first to the last; every step of the
    staircase leaves pmask 0 at the corner it shares with the next; the
    enclosed cell is wet with eight land neighbours."""
    Lm, Mm, _ = size
    g = coasts.channel_geometry(Lm, Mm)
    rm, um, vm, pk = _masks(Lm, Mm, coasts.channels(Lm, Mm))
    (s0, s1), edges = g["rows"], coasts.all_edges(Lm)
    assert len(g["eta"]) >= 2
    for c in g["eta"]:
        assert c in edges or c - 1 in edges
        for j in range(s0, s1 + 1):
            assert cell(rm, c, j) == 1.0
            if j != g["xi"]:
                assert cell(rm, c - 1, j) == 0.0 and cell(rm, c + 1, j) == 0.0, (c, j)
                assert cell(um, c, j) == 0.0 and cell(um, c + 1, j) == 0.0
            assert cell(vm, c, j) == 1.0
    for i in range(g["eta"][0], g["eta"][-1] + 1):
        assert cell(rm, i, g["xi"]) == 1.0
        if i > g["eta"][0]:
            assert cell(um, i, g["xi"]) == 1.0
        if i not in g["eta"]:
            assert cell(vm, i, g["xi"]) == 0.0 and cell(vm, i, g["xi"] + 1) == 0.0, i
    for (i, j), (i2, j2) in zip(g["stairs"], g["stairs"][1:]):
        assert (i2, j2) == (i + 1, j + 1) and cell(rm, i, j) == 1.0 and cell(rm, i2, j2) == 1.0
        assert cell(rm, i + 1, j) == 0.0 and cell(rm, i, j + 1) == 0.0
        assert cell(pk, i + 1, j + 1) == 0.0   # p(i+1, j+1): cells (i, j), (i+1, j), (i, j+1), (i+1, j+1)
    ie, je = g["enclosed"]
    assert cell(rm, ie, je) == 1.0
    assert sum(cell(rm, ie + di, je + dj) for di in (-1, 0, 1) for dj in (-1, 0, 1)) == 1.0
    assert cell(um, ie, je) == cell(um, ie + 1, je) == cell(vm, ie, je) == cell(vm, ie, je + 1) == 0.0


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_blocks_cover_whole_units(size):
    """Solid land over a whole tile of ranges from i = 0 and from i = 1 (all
    of the tile's columns that lie in the grid, kBY = 4 rows from a tile row
    of the ranges from j = 1; 2 rows where Mm < 10), over columns 17 .. 32 in
    every row, and over each strip's first and last owned column in the strip
    rows 3 .. Mm-1."""
    Lm, Mm, _ = size
    land = coasts.blocks(Lm, Mm)
    pieces = coasts.block_pieces(Lm, Mm)
    what = [p[0] for p in pieces]
    assert "tile of ranges from i = 0" in what and "tile of ranges from i = 1" in what
    assert "16-column block in every row" in what and "strip's first owned column" in what
    assert ("strip's last owned column" in what) == (Lm >= 60)
    for w, i0, i1, j0, j1 in pieces:
        assert 1 <= i0 <= i1 <= Lm and 1 <= j0 <= j1 <= Mm, (w, i0, i1, j0, j1)
        assert land[j0 + 1:j1 + 2, i0 + 1:i1 + 2].all(), w
        if w.endswith("tile of ranges from i = 0"):
            assert (i0 - coasts.tile_i0(0)) % 64 == 0 or i0 == 1
            assert i1 == Lm or (i1 + 1 - coasts.tile_i0(0)) % 64 == 0
            assert (j0 - 1) % 4 == 0 and j1 - j0 + 1 == (4 if Mm >= 10 else 2)
        if w.endswith("tile of ranges from i = 1"):
            assert (i0 - 1) % 64 == 0 and (i1 == Lm or i1 % 64 == 0)
        if w.startswith("16"):
            assert (i0 - 1) % 16 == 0 and i1 - i0 == 15 and (j0, j1) == (1, Mm)
        if w.startswith("strip"):
            assert i0 % 60 in (0, 1) and (j0, j1) == (3, Mm - 1)


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_walls_mix_the_masks_on_every_side(size):
    """On each of the four sides the ghost line and the first (last) interior
    line both hold land and water, in all four combinations, and the normal
    velocity's mask on the wall's own line (umask at i = 1 and Lm+1, vmask at
    j = 1 and Mm+1) and the tangential one in the ghost line take 0 and 1."""
    Lm, Mm, _ = size
    rm, um, vm, _ = _masks(Lm, Mm, coasts.walls(Lm, Mm))
    js, is_ = slice(2, Mm + 2), slice(2, Lm + 2)
    sides = {"west": (rm[js, 1], rm[js, 2], um[js, 2], vm[3:Mm + 2, 1]),
             "east": (rm[js, Lm + 2], rm[js, Lm + 1], um[js, Lm + 2], vm[3:Mm + 2, Lm + 2]),
             "south": (rm[1, is_], rm[2, is_], vm[2, is_], um[1, 3:Lm + 2]),
             "north": (rm[Mm + 2, is_], rm[Mm + 1, is_], vm[Mm + 2, is_], um[Mm + 2, 3:Lm + 2])}
    for side, (ghost, line, normal, tangential) in sides.items():
        combos = {(g, w) for g, w in zip(ghost, line)}
        assert combos == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)}, (side, combos)
        assert set(normal) == {0.0, 1.0} and set(tangential) == {0.0, 1.0}, side


@pytest.mark.parametrize("xs", [[30], [20, 40]], ids=["2x2", "3x2"])
def test_rank_edges_meet_every_case(xs):
    """coasts.rank_edges on the 60 x 24 grid of the decomposed GPU runs: each
    rank edge falls on land, beside land on either side, across a one-cell
    channel and along the flank of one on either side; the oracle runs it."""
    Lm, Mm, f = 60, 24, 12
    land = coasts.rank_edges(Lm, Mm, xs, [f])
    rm, um, vm, _ = _masks(Lm, Mm, land)
    wet = lambda i, j: cell(rm, i, j) == 1.0
    for e in xs:
        assert not wet(e, 2) and not wet(e + 1, 2)
        assert wet(e, 5) and not wet(e + 1, 5) and not wet(e, 7) and wet(e + 1, 7)
        assert all(wet(i, 10) and not wet(i, 9) and not wet(i, 11) for i in range(e - 3, e + 5))
        assert cell(um, e + 1, 10) == 1.0 and cell(vm, e, 10) == 0.0 and cell(vm, e + 1, 11) == 0.0
        assert all(wet(e, j) and not wet(e - 1, j) and not wet(e + 1, j) for j in (15, 16, 17))
        assert all(wet(e + 1, j) and not wet(e, j) and not wet(e + 2, j) for j in (19, 20, 21))
    assert not wet(2, f) and not wet(2, f + 1)
    assert wet(5, f) and not wet(5, f + 1) and not wet(7, f) and wet(7, f + 1)
    assert all(wet(10, j) and not wet(9, j) and not wet(11, j) for j in range(f - 3, f + 5))
    assert cell(vm, 10, f + 1) == 1.0 and cell(um, 10, f) == 0.0
    assert all(wet(i, f) and not wet(i, f - 1) and not wet(i, f + 1) for i in (14, 15, 16))
    o = oracle.Oracle(kpp_cfg(Lm, Mm, 10))
    o.init()
    coasts.apply_coast(o, None, land, coasts.VISC)
    o.step(5)
    assert all(np.isfinite(o.field(n)).all() for n in PROGNOSTIC)
    assert rm[2:-2, 2:-2].mean() >= 0.4


def test_random_is_a_quarter_land():
    land = coasts.random(121, 12)
    assert abs(land[2:-2, 2:-2].mean() - 0.25) < 0.03
    assert np.array_equal(land, coasts.random(121, 12))


def test_coast_band_is_two_cells_deep():
    rm = np.ones((13, 15))
    rm[6, 7] = 0.0
    band = coasts.coast_band(rm)
    want = np.zeros((9, 11), dtype=bool)
    want[2:7, 3:8] = True
    want[4, 5] = False
    assert np.array_equal(band, want)


# ------------------------------------------------------------ oracle runs ----
@pytest.mark.parametrize("name", list(coasts.COASTS))
@pytest.mark.parametrize("obc", [0, 15], ids=["closed", "open"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_oracle_runs_the_coast(size, obc, name):
    """12 oracle steps on the coast with the viscosity on, between closed
    walls and with four open edges (boundary data, v_sponge = 1e3): every
    field finite, max|u| >= 1e-2 m/s, land stays at rest."""
    Lm, Mm, N = size
    o = oracle.Oracle(coast_cfg(Lm, Mm, N, obc))
    o.init()
    masks = coasts.apply_coast(o, None, coasts.COASTS[name](Lm, Mm), coasts.VISC)
    o.step(12)
    for n in PROGNOSTIC:
        assert np.isfinite(o.field(n)).all(), n
    u = interior(o.field("u"), Lm, Mm)
    print("%s %dx%dx%d obc %d: max|u| %.3f" % (name, Lm, Mm, N, obc, np.abs(u).max()))
    assert np.abs(u).max() >= 1.0e-2
    assert not (u * (1.0 - interior(masks["umask"], Lm, Mm))).any()


# ------------------------------------------------------------ sensitivity ----
def _run(name, spoil, size=(121, 12, 12)):
    Lm, Mm, N = size
    o = oracle.Oracle(coast_cfg(Lm, Mm, N))
    o.init()
    masks = coasts.apply_coast(o, None, coasts.COASTS[name](Lm, Mm), coasts.VISC)
    spoil(o, masks)
    o.step(12)
    return {n: interior(o.field(n), Lm, Mm).copy() for n in ("zeta", "ubar", "vbar", "u", "v", "t")}


_CLEAN = {}


def _moved(name, spoil):
    if name not in _CLEAN:
        _CLEAN[name] = _run(name, lambda o, masks: None)
    got = _run(name, spoil)
    return {n: rms_abs(got[n], _CLEAN[name][n]) for n in got}


@pytest.mark.parametrize("name", list(coasts.COASTS))
def test_a_wrong_pmask_shows(name):
    """pmask forced to 1 everywhere (free slip at every corner and wall)
    moves u by more than RMS_RUN within 12 steps: with the viscosity on,
    visc3d's pmask is live on every coast."""
    def spoil(o, masks):
        o.field("pmask")[0][...] = 1.0
    e = _moved(name, spoil)
    print(name, {k: "%.2e" % v for k, v in e.items()})
    assert e["u"] > RMS_RUN


@pytest.mark.parametrize("name", list(coasts.COASTS))
def test_one_wrong_umask_cell_shows(name):
    """One wet u-point of the coast band closed (umask 1 -> 0) moves u by
    more than RMS_RUN within 12 steps."""
    def spoil(o, masks):
        Lm, Mm = o.cfg.LLm, o.cfg.MMm
        band = coasts.coast_band(masks["rmask"]) & (interior(masks["umask"], Lm, Mm) == 1.0)
        jj, ii = np.nonzero(band)
        q = len(jj) // 2
        o.field("umask")[0][jj[q] + 2, ii[q] + 2] = 0.0
    e = _moved(name, spoil)
    print(name, {k: "%.2e" % v for k, v in e.items()})
    assert e["u"] > RMS_RUN
