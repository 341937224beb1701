"""Coastline sweep: GPU parity with land at every tile, strip, block and wall edge.

The other GPU tests run three analytic land masks (the basin's island, the
Pipes_ana and the Rivers_ana coast); where those fall relative to a 64 x 4
tile, a 60-column strip or a 16-column block is an accident of the grid
size.  Here the coasts of tests/coasts.py (its docstring gives the edges and
the lines of the constants they come from; tests/test_coasts.py checks on
the CPU that the land is where it says) go into the closed split-EOS basin
with KPP and surface fluxes on 2 km cells (branch_states.kpp_cfg) with
uniform visc2_r, visc2_p = 40 and diff2 = 15 m2/s, so that pmask (visc3d) and
t3dmix are live.  The mask reads these runs pin:
  * the staged LDS windows wUM / wVM of k_pre_step3d.hip:95-96 and
    k_step3d_t.hip:69-70 (`ok ? F.umask[o] : 0.0`), 64 + 4 columns by 4 + 4
    rows about a tile of a range from i = 0 (edges 48 / 49, 112 / 113);
  * a lane's umask(i-1..i+2, j), vmask(i, j-1..j+2) and the masked curvature
    terms of the advection (k_common.h:385-392, 439-440, 683-721), their
    segment and v-tile forms at N = 88 .. 104 (k_colseg.h:455-525; 61 x 6 at
    N = 100: 16-column blocks 16 / 17, 32 / 33, 48 / 49, v-tiles of 4 rows);
  * prsgrd's mask of the clamped entry point (k_prsgrd.hip:180-202) and the
    strips' umask / vmask through buffer loads on feed lanes
    (k_prsgrd_strip.hip:93, 113; strips own 60 columns: 60 / 61, 120 / 121;
    rows 3 .. Mm-1 in chunks of 8: 10 / 11), k_tracer_strip.hip:79;
  * k_s2d_fb's e_rm[r] and window masks (k_step2d.hip:387-408, 494) and the
    wall phases' umask / vmask at the ghost line, folded (:647-660) and as
    separate launches (:739-848; 48 x 11 and 112 x 12 are the sizes at which
    s2d_edge_mode, :1029, does not fold);
  * the 3 x 3 masked smoother of hbl / bbl (k_lmd.hip:134-165, 605-606);
  * pmask in visc3d (k_step3d_uv.hip:496, 561, 688);
  * the pmask-weighted tangential gradients and the umask / vmask of the
    open edges (k_obc.hip:63-229), with land and water on one edge (walls);
  * rmask, umask, vmask re-exchanged 2K deep before a step's first fast step
    of a decomposed run (k_step2d.hip:967-971);
  * k_bulk.hip's masked stflx, sustr, svstr.
Tolerances are the project's: RTOL_ROUTINE per routine in the max norm,
RMS_RUN per run (test_gpu_parity), decompositions bitwise.  A whole run is
held to RMS_RUN twice: over the interior, and over coasts.coast_band alone
(the wet points within two cells of land) with the same rms / rms_abs, so a
one-cell error is not diluted by the open water.  Every model asserts the
paths it took (Model.horizontal_path(), column_path()) as the width sweep
does.

All cases passed as the library stood.  Measured on the MI355X: routines
<= 1.4e-16 at N = 12 (lmd_vmix's hbls) and <= 6.6e-16 at N = 100 (step3d_t's
t); whole runs bitwise equal to the oracle at N = 12 on every coast and
switch set, 1.5e-13 to 6.0e-13 at 61 x 6 x 100, the same over the coast band
(DESIGN.md section 4).

What the sweep catches, one predicate each in a scratch copy of the kernels,
run against this file, the width sweep's island family (open-*) and
test_gpu_obc.py:
  - k_pre_tracer_h1's staged umask window (k_pre_step3d.hip:95) taking its
    last column from the column before: fails 23 of the 57 new cases other than the bulk-flux run (that one ran
    against the last mutation only):
    pre_step3d's t on specks, channels, walls, random at 121 x 12 x 12 (1.8e-9
    to 5.1e-9), the whole runs of those coasts at 121 x 12, 65 x 8, 49 x 12
    (walls) and 112 x 12, closed, open and curvilinear (t 1.5e-6 to 1.6e-5, v
    to 1.8e-6). 48 x 11 (one tile, whose window ends in the outer ring), 61 x 6 x
    100 (the level-walking kernel runs there) and blocks pass. The island
    family and test_gpu_obc.py pass.
  - the prsgrd strip's umask on feed lane 62 taken from the row before
    (k_prsgrd_strip.hip:201): fails 17 whole runs, all 60 or more columns
    wide (121 x 12, 65 x 8, 112 x 12, 61 x 6 x 100 open; t to 1.6e-4 at
    112 x 12). Four of them (walls 121 x 12, specks / channels / random
    65 x 8) fail in the coast band alone (1.1e-10 to 2.9e-10) with the
    interior RMS under the bound. No routine case fails (a routine call
    never takes the strips). The island family and test_gpu_obc.py pass.
  - smooth_masks (k_lmd.hip:149) reading vmask(i, .) for vmask(i+1, .):
    fails 39 new cases: lmd_vmix on every coast at both sizes (Akv, Akt, ghat
    6e-3 to 7e-2 of the scale) and 29 whole runs (t 1.9e-7 to 2.1e-4). The
    island family's three routine cases fail too, its whole runs and
    test_gpu_obc.py pass.
  - the folded south wall's tangential umask read one column to the east
    (k_step2d.hip:647): fails exactly the walls runs that fold the walls:
    121 x 12, 65 x 8, 49 x 12, 61 x 6 x 100 closed and 121 x 12 curvilinear
    (t, v 8e-8 to 1.3e-6). 48 x 11 and 112 x 12 (separate wall launches), the
    open runs, every other coast, the island family and test_gpu_obc.py
    pass: no other test has land in a closed wall's ghost line.
  - k_visc3d_stg's pmask read one column to the west
    (k_step3d_uv.hip:688): fails all 55 single-domain cases (visc3d's u, v
    to 0.15 of the scale; whole runs u from 1e-7) and, with their sponge
    bands, the island family (6 cases) and 6 cases of test_gpu_obc.py. The
    same line in the unstaged k_visc3d (:561, ROMS_GPU_VISC_STG=0)
    fails nothing here: only test_visc3d_staged_windows_bitwise runs that
    kernel.
"""
import numpy as np
import pytest

import coasts
import oracle
import romsgpu
from branch_states import kpp_cfg
from test_gpu_depths import routine_errors
from test_gpu_multirank import check_decomposition, run_decomposed
from test_gpu_obc import obc_cfg
from test_gpu_parity import (ABSOLUTE, PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, _w, check_fields, interior, rms, rms_abs)
from test_gpu_widths import environ

pytestmark = pytest.mark.gpu

# (Lm, Mm, N) -> (closed-edge mode of the fast step between closed walls, prsgrd strips (per row, jA, jB),
# what the size is there for); omega takes k_omega_seg at every size
SIZES = {
    (121, 12, 12): (2, (3, 3, 11), "every edge up to 120 / 121; a second strip chunk of one row (row 11)"),
    (65, 8, 12): (2, (2, 3, 7), "a second tile of one column for ranges from i = 1; 64 / 65 is the last interior line"),
    (49, 12, 12): (2, (1, 3, 11), "a second tile of one column for ranges from i = 0"),
    (48, 11, 12): (1, (1, 3, 10), "east and north wall phases as separate launches"),
    (112, 12, 12): (1, (2, 3, 11), "east wall phase as a separate launch; two full tiles for ranges from i = 0"),
    (61, 6, 100): (2, (2, 3, 5), "segment solvers and v-tiles on 16-column blocks; a second strip of one column"),
}
ENV_OFF = {k: None for k in ("ROMS_GPU_COLSEG", "ROMS_GPU_COL_GLOBAL", "ROMS_GPU_PRS_STRIP", "ROMS_GPU_T_STRIP",
                             "ROMS_GPU_S2D_EDGES")}


def sid(size):
    return "%dx%dx%d" % size


def coast_cfg(size, obc=0, curv=0, bulk=0):
    cfg = kpp_cfg(*size)
    cfg.curvgrid, cfg.bulk_frc = curv, bulk
    if obc:
        cfg.obc, cfg.ubind, cfg.v_sponge = obc, 0.1, 1.0e3
    return cfg


def coast_model(cfg, size):
    """A model of cfg; asserts the column path by the depth sweep's rule and
    the horizontal path against SIZES (open edges never fold: mode 1)."""
    with environ(ENV_OFF):
        m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                    nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex,
                                    sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux), obc=cfg.obc,
                                    v_sponge=cfg.v_sponge, curvgrid=bool(cfg.curvgrid), bulk_frc=bool(cfg.bulk_frc),
                                    adv_isoneutral=bool(cfg.adv_isoneutral))
    edges, strips, _ = SIZES[size]
    # prsgrd_takes_strips (k_prsgrd.hip:379): no strips on a curvilinear grid, the tiles run every row
    want = {"edges": 1 if cfg.obc else edges, "strips": None if cfg.curvgrid else strips, "omega_seg": True}
    got, col = m.horizontal_path(), m.column_path()
    if got != want or col != (88 <= cfg.N <= 104, cfg.N >= 64):
        m.close()
        raise AssertionError("%s: horizontal_path() = %s, expected %s; column_path() = %s" % (sid(size), got, want, col))
    return m


# ------------------------------------------------------- routine parity ----
@pytest.mark.parametrize("name", list(coasts.COASTS))
@pytest.mark.parametrize("size", [(121, 12, 12), (61, 6, 100)], ids=sid)
def test_coast_routine_parity(size, name):
    """Every routine of the depth sweep's routine_list (visc3d and t3dmix
    among them, live under the viscosity) on one mid-run state of the coast
    -- 3 oracle steps on it, then perturbed Akv, Akt, Wi -- within
    RTOL_ROUTINE in the max norm: the tile kernels with their windows at
    121 x 12 (tile edges 48 / 49, 64 / 65, 112 / 113; rows of every residue
    mod 4), the segment solvers and v-tiles at 61 x 6 x 100 (block edges
    16 / 17 .. 48 / 49).  Every failing (routine, field, error) is reported
    at once."""
    cfg = coast_cfg(size)
    land = coasts.COASTS[name](cfg.LLm, cfg.MMm)
    m = coast_model(cfg, size)
    try:
        errs = routine_errors(cfg, m, setup=lambda o: coasts.apply_coast(o, None, land, coasts.VISC),
                              tag=name.encode())
    finally:
        m.close()
    tag = "%s %s" % (name, sid(size))
    for (rid, f), e in errs.items():
        print("%s %s %s %.3e" % (tag, rid, f, e))
    print("%s worst routine error %.3e" % (tag, max(errs.values())))
    bad = [(rid, f, e) for (rid, f), e in errs.items() if not e <= RTOL_ROUTINE]
    assert not bad, (tag, bad)


# ------------------------------------------------------------ whole runs ----
def band_errors(o, m, cfg, band):
    """check_fields' whole-run errors over the points of `band` alone."""
    get = lambda src, n: _w(src, src.get if src is m else src.field) if n == "w" else \
        (src.get(n) if src is m else src.field(n))
    out = {}
    for n in PROGNOSTIC + ["w"]:
        a = interior(get(m, n), cfg.LLm, cfg.MMm)[..., band]
        b = interior(get(o, n), cfg.LLm, cfg.MMm)[..., band]
        out[n] = rms_abs(a, b) if n in ABSOLUTE else rms(a, b)
    return out


def coast_run(size, name, steps=12, **switches):
    cfg = coast_cfg(size, **switches)
    o = oracle.Oracle(cfg)
    o.init()
    m = coast_model(cfg, size)
    try:
        masks = coasts.apply_coast(o, m, coasts.COASTS[name](cfg.LLm, cfg.MMm), coasts.VISC)
        o.step(steps)
        m.step(steps)
        m.sync()
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, float("inf"), kind="rms")
        band = coasts.coast_band(masks["rmask"])
        assert band.sum() >= 30
        near = band_errors(o, m, cfg, band)
    finally:
        m.close()
    tag = "%s %s %s" % (name, sid(size), switches or "closed")
    print(tag, "interior", {k: "%.2e" % v for k, v in errs.items()})
    print(tag, "band    ", {k: "%.2e" % v for k, v in near.items()})
    print("%s worst run rms %.3e, in the coast band %.3e" % (tag, max(errs.values()), max(near.values())))
    assert float(np.abs(interior(o.field("u"), cfg.LLm, cfg.MMm)).max()) >= 1.0e-2
    bad = [("interior", n, e) for n, e in errs.items() if not e <= RMS_RUN]
    bad += [("band", n, e) for n, e in near.items() if not e <= RMS_RUN]
    assert not bad, (tag, SIZES[size][2], bad)


@pytest.mark.parametrize("name", list(coasts.COASTS))
@pytest.mark.parametrize("size", list(SIZES), ids=sid)
def test_coast_run_rms(size, name):
    """12 whole steps between closed walls (graph replay, prsgrd strips, the
    staged tracer windows, k_s2d_fb with the wall phases folded, or as
    separate launches at 48 x 11 and 112 x 12): field RMS against the oracle
    below RMS_RUN over the interior and over the coast band alone.  SIZES
    names what each size is there for; the edges covered are those of
    coasts.edge_columns up to Lm, the strip rows 3 .. Mm-1 with the chunk
    edge 10 / 11, the walls' ghost lines and first interior lines."""
    coast_run(size, name)


@pytest.mark.parametrize("name", ["walls", "random", "specks"])
@pytest.mark.parametrize("size", [(121, 12, 12), (65, 8, 12), (61, 6, 100)], ids=sid)
def test_coast_run_open_edges(size, name):
    """The same with all four edges open (obc = 15: Flather / Orlanski with
    boundary data) and sponge bands of v_sponge = 1e3 m2/s on top of the
    viscosity: k_obc.hip:63-229 meets umask / vmask 0 and 1 and pmask 0, 1, 2
    on one edge (walls puts land into the ghost line and the first interior
    line in pieces), the wall phases run as the open edges' launches."""
    coast_run(size, name, obc=15)


@pytest.mark.parametrize("name", list(coasts.COASTS))
def test_coast_run_curvgrid(name):
    """The same at 121 x 12 on the analytic curvgrid = 1 grid, whose metrics
    are separable (pm = pm(j), pn = pn(i), f constant; grids that vary along
    both axes: tests/test_gpu_metrics.py): the masked
    curvature terms of k_common.h:683-721 beside land, and, prsgrd taking no
    strips on such a grid (asserted), k_prsgrd_uv's tiles with the mask of
    the clamped entry point (k_prsgrd.hip:180-202) in every row."""
    coast_run((121, 12, 12), name, curv=1)


def test_coast_run_bulk_fluxes():
    """The same at 121 x 12 under bulk_frc = 1 on the random coast:
    k_bulk.hip masks stflx, sustr and svstr with land on every tile edge."""
    coast_run((121, 12, 12), "random", bulk=1)


# -------------------------------------------------------- decomposed runs ----
RANK_GRID = (60, 24)   # 2 x 2: ranks of 30 x 12; 3 x 2: 20 x 12 -- all at least 2K + 2 = 10 wide


def rank_case(N=10):
    Lm, Mm = RANK_GRID
    return dict(case_id=1, LLm=Lm, MMm=Mm, N=N, NT=2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30,
                sizex=2.0e3 * Lm, sizey=2.0e3 * Mm, lmd=True, surf_flux=True)


def rank_setup(cfg, land):
    """setup(model) for run_decomposed / check_decomposition: every rank
    puts its window of the global mask planes and runs init_sequence."""
    o = oracle.Oracle(cfg)
    o.init()
    masks = coasts.coast_masks(o, land)
    return lambda m: coasts.put_coast(m, masks, coasts.VISC)


@pytest.mark.parametrize("npx,npe", [(2, 2), (3, 2)])
def test_coast_decomposition_bitwise(npx, npe):
    """The closed basin on 60 x 24 with coasts.rank_edges about every rank
    edge (columns 30 / 31, or 20 / 21 and 40 / 41; rows 12 / 13): the edge
    on land, beside land on either side, across a one-cell channel and along
    one's flank.  At the default exchange interval (K = 4, asserted) the
    fast steps run on subdomains widened into the halo, with rmask, umask,
    vmask exchanged 2K = 8 deep before each step's first fast step
    (k_step2d.hip:967-971): every subdomain equals the single domain bitwise."""
    Lm, Mm = RANK_GRID
    xs = [romsgpu.rank_extent(Lm, npx, r)[1] for r in range(1, npx)]
    ys = [romsgpu.rank_extent(Mm, npe, r)[1] for r in range(1, npe)]
    assert min(romsgpu.rank_extent(Lm, npx, r)[0] for r in range(npx)) >= 10
    assert min(romsgpu.rank_extent(Mm, npe, r)[0] for r in range(npe)) >= 10
    case = rank_case()
    setup = rank_setup(kpp_cfg(Lm, Mm, case["N"]), coasts.rank_edges(Lm, Mm, xs, ys))
    check_decomposition(case, npx, npe, setup=setup)
    parts, _ = run_decomposed(case, npx, npe, 1, fields=("zeta",), probe=lambda m: m.halo_exchanges(), setup=setup)
    assert {p[5][1] for p in parts} == {4}, [p[5] for p in parts]


def test_coast_decomposition_open_walls_bitwise():
    """test_gpu_multirank's basin_obc case (four open edges, the island, no
    sponge; the open edges exchange after every fast step) with walls on top:
    land and water in the ghost line and the first interior line of every
    open edge, cut by the rank edges of a 2 x 2 grid."""
    from test_gpu_multirank import _case
    case = _case("basin_obc")
    cfg = obc_cfg(obc=15, sponge=0.0, island=1, lmd=oracle.LMD_ALL, LLm=case["LLm"], MMm=case["MMm"], N=case["N"],
                  sizex=case["sizex"], sizey=case["sizey"])
    check_decomposition(case, 2, 2, setup=rank_setup(cfg, coasts.walls(case["LLm"], case["MMm"])))

