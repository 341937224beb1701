"""Width/height sweep: GPU parity at every grid size Lm x Mm that switches a
tile, strip or block path.

The horizontal size selects as many code paths as the level count does
(tests/test_gpu_depths.py), most of them in host code that picks ranges:
  * k_prsgrd_strip.hip: a wavefront owns kStripOwn = 60 of its 64 columns
    (:48, `own` :98), so the strip count changes at Lm = 60 / 61
    (prsgrd_strip_rows :300); a strip at a closed wall applies the one-sided
    extrapolations as lane shuffles (`xedge` :102, lpg / lu / lx :103); at
    Lm = 60 the only strip is the west and the east edge strip at once, at
    Lm = 61 / 62 the second strip owns one / two columns and the first needs
    no east extrapolation; at Lm = 120 the east edge strip is a full one that
    is not the west edge strip too, the one size at which `c0 + 62 > G.xhi`
    alone decides with iend + 1 on lane 62.  The strip rows are jA..jB = 3..Mm-1 between
    closed walls and 1..Mm on a periodic grid (prsgrd_strip_rows :294-299),
    in chunks of ROMS_PRS_STRIP_J = 8 rows (:53, :320): no strip row at
    Mm = 3, one at Mm = 4, one full chunk at Mm = 11, a second chunk of one
    row at Mm = 12;
  * k_step2d.hip s2d_edge_mode (:1029): the closed walls fold into k_s2d_fb
    unless the east wall's column starts a tile of its own, (Lm + 16) % 64
    == 0 (:1036; tiles start at tile_i0(istrR) = -15, roms_dev.h:277), or the
    north wall's row does, (Mm + 1) % 4 == 0 (:1038);
  * k_vertical.hip omega_takes_seg (:652): k_omega_seg from 32 columns on,
    the two-pass k_omega below;
  * roms_dev.h grid_of (:278) with tile_i0 (:277): the 64 x 4 tiles (kBX,
    kBY :268) of ranges that start at i = 1 change count at Lm = 64 / 65,
    those that start at i = 0 at Lm = 48 / 49 and 112 / 113 (grid_of and the
    LDS windows of k_pre_tracer_h1, k_step3d_t_h1, k_kpp_int, k_visc3d_stg,
    k_t3dmix_stg);
  * the 16-column blocks of the segment solvers (k_colseg.h seg_grid_of
    :481, kSegCW), their v-tile form (kVTX x kVTY = 16 x 4, :452, :489) and
    the chain kernels (k_chain.h kChainCW :22, chain_grid_of :44) change
    count at Lm = 16 / 17, 32 / 33, ...;
  * roms_gpu_init accepts Lm >= 2, Mm >= 2 (roms_shim.cpp:742): on the
    smallest grids the two walls are closer together than the radius-2
    stencils are wide.
SIZES holds one size on each side of every switch.  Every model asserts the
path the library reports (Model.horizontal_path(), filled by the host
functions the launchers call) against the value its table entry names, so a
size that silently stops exercising its switch fails.

Cases: the closed split-EOS basin with KPP and surface fluxes at N = 12
(every size) and at N = 100 (segment solvers, k_omega_seg on 16-column
blocks), the doubly periodic Filament (periodic images in the fast step,
strips with no edge) and the open basin with the island, all on 2 km cells
(Filament: the reference's 200 m x 50 m) so the flow stays comparable.  Per
size: every routine against the CPU oracle on one mid-run state within
RTOL_ROUTINE (routine_errors of the depth sweep), and 12 whole steps (graph
replay, strips, folded walls) within RMS_RUN.  A routine call to prsgrd
never takes the strips (they carry the momentum r.h.s. of the next routine),
so the whole run is what pins the strips to the oracle.  The grids with Lm
or Mm <= 5 have test functions of their own.  test_width_variants_bitwise
tells which form is wrong when a strip size fails against the oracle.

What the sweep catches, tried in a scratch copy of the kernels (predicates
only), 12 whole steps of every size above:
  * k_prsgrd_strip's `own` as `lane <= 60` (a strip's last column keeps stale
    ru, rv) fails every size 60 or more columns wide that has a strip row,
    in all four families (16 sizes, field RMS 7e-4 .. 0.7); every other size
    passes.  The strip-against-tile tests catch this one too.
  * `xedge` as `c0 + 61 > G.xhi` (an east edge strip whose extrapolated
    column iend + 1 sits on lane 62 skips the wall's shuffles) fails exactly
    120 x 9 (RMS 1.2e-7), a width no other test of the suite runs: the strip
    tests' widths are 150, 64, 130, 70, 100 and 125, the whole runs' 64, 100,
    128, 192, 512 and 1024, and at Lm = 60 the west wall sets xedge anyway.
    (`c0 + 62 >= G.xhi`, the error in the other direction, changes no
    number: xedge then shuffles where no clamp binds, each lane from itself.)
  * s2d_edge_mode without its east-wall term (the fold taken although the
    wall's column starts a tile) fails exactly 112 x 12, at the path
    assertion (edges 2 for 1) and in the numbers (RMS 1.8e-8).  48 x 11
    passes it: there the north wall still blocks the fold, which is why the
    table pairs the east wall alone with a height that folds.
All sizes passed as the library stood; measured errors: DESIGN.md section 4.
"""
import contextlib
import os

import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_depths import depth_model, routine_errors
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, basin_cfg, check_fields

pytestmark = pytest.mark.gpu

# (Lm, Mm) -> (closed-edge mode of the fast step: 0 none / 1 separate edge
# launches / 2 folded, prsgrd strips (per row, jA, jB) or None, omega in the
# segment form, what the size is there for)
SIZES = {
    (2, 2): (2, None, False, "the smallest grid roms_gpu_init accepts: walls two cells apart, no strip row"),
    (3, 3): (1, None, False, "Mm = 3: no strip row (3..2), the tiles run alone; north wall not folded"),
    (5, 4): (2, (1, 3, 3), False, "Mm = 4: one strip row; the strip owns 5 columns, west and east edge at once"),
    (2, 12): (2, (1, 3, 11), False, "two columns between the walls over a second row chunk"),
    (60, 2): (2, None, True, "Mm = 2 on a full strip's width: tiles alone, walls two rows apart"),
    (16, 6): (2, (1, 3, 5), False, "one full 16-column block; k_omega"),
    (17, 9): (2, (1, 3, 8), False, "a second 16-column block of one column"),
    (31, 3): (1, None, False, "last width of the two-pass k_omega; Mm = 3: north wall alone blocks the fold"),
    (32, 10): (2, (1, 3, 9), True, "first width of k_omega_seg; two full 16-column blocks"),
    (33, 13): (2, (1, 3, 12), True, "a third 16-column block of one column; second row chunk of two rows"),
    (48, 11): (1, (1, 3, 10), True, "east and north walls both block the fold; one tile for ranges from i = 0; "
                                    "Mm = 11: exactly one row chunk"),
    (49, 12): (2, (1, 3, 11), True, "second tile of one column for ranges from i = 0; Mm = 12: second chunk of one row"),
    (60, 4): (2, (1, 3, 3), True, "one full strip, the west and the east edge strip at once; one strip row"),
    (61, 12): (2, (2, 3, 11), True, "second strip owns one column (lane 2), the first needs no east extrapolation"),
    (62, 4): (2, (2, 3, 3), True, "second strip owns two columns; one strip row"),
    (64, 11): (1, (2, 3, 10), True, "one full tile for ranges from i = 1; north wall alone blocks the fold"),
    (65, 8): (2, (2, 3, 7), True, "second tile of one column for ranges from i = 1"),
    (112, 12): (1, (2, 3, 11), True, "east wall alone blocks the fold; two full tiles for ranges from i = 0"),
    (113, 6): (2, (2, 3, 5), True, "third tile of one column for ranges from i = 0"),
    (120, 9): (2, (2, 3, 8), True, "two full strips: the east edge strip is not the west one, and the wall's "
                                   "extrapolated column iend + 1 sits on its last feed lane but one (62)"),
    (121, 10): (2, (3, 3, 9), True, "third strip owns one column; the widest grid of the sweep"),
}
# N = 100: the segment solvers' 16-column blocks and v-tiles, k_omega_seg on 16-column blocks
SIZES_N100 = {
    (16, 4): (2, (1, 3, 3), False, "one full 16-column block; k_omega (two-pass) at the segment depth"),
    (17, 5): (2, (1, 3, 4), False, "a second block of one column"),
    (33, 3): (1, None, True, "k_omega_seg with a third block of one column; one v-tile row of 3 rows"),
    (61, 6): (2, (2, 3, 5), True, "four blocks, the last of 13 columns; two v-tile rows; a second strip of one column"),
}
# doubly periodic: no edge (mode 0), every row 1..Mm in strips, no edge strip
SIZES_FILAMENT = {
    (4, 4): (0, (1, 1, 4), False, "tiny periodic grid: the halo images are the interior itself"),
    (60, 7): (0, (1, 1, 7), True, "one full strip whose feed lanes read the periodic halo"),
    (61, 9): (0, (2, 1, 9), True, "second strip of one column; a second row chunk of one row"),
    (64, 6): (0, (2, 1, 6), True, "one full tile"),
    (65, 8): (0, (2, 1, 8), True, "second tile of one column; exactly one row chunk"),
}
# all four edges open, an island: the edges never fold (mode 1)
SIZES_OPEN = {
    (17, 12): (1, (1, 3, 11), False, "a second 16-column block of one column beside an open edge"),
    (61, 10): (1, (2, 3, 9), True, "second strip of one column at the open east edge"),
    (65, 14): (1, (2, 3, 13), True, "second tile of one column at the open east edge"),
}
FAMILIES = {"kpp": SIZES, "n100": SIZES_N100, "filament": SIZES_FILAMENT, "open": SIZES_OPEN}


def is_tiny(size):
    return min(size) <= 5


def params(tiny, only=None):
    return [pytest.param(fam, size, id="%s-%dx%d" % ((fam,) + size))
            for fam, table in FAMILIES.items() for size in table
            if is_tiny(size) == tiny and (only is None or fam in only)]


def width_cfg(family, size):
    Lm, Mm = size
    if family == "filament":
        return oracle.filament_cfg(LLm=Lm, MMm=Mm, N=10, sizex=200.0 * Lm, sizey=50.0 * Mm, np_xi=1, np_eta=1)
    c = basin_cfg(nonlin=True, LLm=Lm, MMm=Mm, N={"kpp": 12, "n100": 100, "open": 10}[family],
                  sizex=2.0e3 * Lm, sizey=2.0e3 * Mm)
    if family == "open":
        c.obc, c.ubind, c.v_sponge, c.island, c.lmd = 15, 0.1, 1.0, 1, oracle.LMD_ICELAND
    else:
        c.lmd, c.surf_flux = oracle.LMD_ALL, 1
    return c


@contextlib.contextmanager
def environ(env):
    """The variables of env set (a value of None: unset) for the block."""
    old = {k: os.environ.pop(k, None) for k in env}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def width_model(family, size, env=None, want=None):
    """A model of the family at the size (env: ROMS_GPU_* switches for its
    init); asserts the column path by the depth sweep's rule and the
    horizontal path against the table entry (or `want`)."""
    cfg = width_cfg(family, size)
    with environ(env or {}):
        if family in ("kpp", "n100"):
            m = depth_model(cfg)
        else:
            m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                        nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                        sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, obc=cfg.obc,
                                        v_sponge=cfg.v_sponge, island=bool(cfg.island))
    edges, strips, seg, _ = FAMILIES[family][size]
    want = want or {"edges": edges, "strips": strips, "omega_seg": seg}
    got, col = m.horizontal_path(), m.column_path()
    if got != want or (cfg.N < 64 and col != (False, False)):
        m.close()
        raise AssertionError("%s %dx%d: horizontal_path() = %s, expected %s; column_path() = %s"
                             % ((family,) + size + (got, want, col)))
    return cfg, m


def routine_parity(family, size):
    cfg, m = width_model(family, size)
    try:
        errs = routine_errors(cfg, m)
    finally:
        m.close()
    tag = "%s %dx%d" % ((family,) + size)
    for (rid, f), e in errs.items():
        print("%s %s %s %.3e" % (tag, rid, f, e))
    print("%s worst routine error %.3e" % (tag, max(errs.values())))
    bad = [(rid, f, e) for (rid, f), e in errs.items() if not e <= RTOL_ROUTINE]
    assert not bad, (tag, FAMILIES[family][size][3], bad)


_RUN_REF = {}   # one entry: the configuration last asked for


def run_ref(cfg):
    key = bytes(cfg)
    if key not in _RUN_REF:
        o = oracle.Oracle(cfg)
        o.init()
        o.step(12)
        _RUN_REF.clear()
        _RUN_REF[key] = o
    return _RUN_REF[key]


def run_rms(family, size):
    cfg, m = width_model(family, size)
    try:
        o = run_ref(cfg)
        m.step(12)
        m.sync()
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, float("inf"), kind="rms")
    finally:
        m.close()
    tag = "%s %dx%d" % ((family,) + size)
    print(tag, {k: "%.2e" % v for k, v in errs.items()})
    print("%s worst run rms %.3e" % (tag, max(errs.values())))
    bad = [(n, e) for n, e in errs.items() if not e <= RMS_RUN]
    assert not bad, (tag, FAMILIES[family][size][3], bad)


@pytest.mark.parametrize("family,size", params(tiny=False))
def test_width_routine_parity(family, size):
    """Each routine at the size within RTOL_ROUTINE of the oracle (the table
    entry names the paths); every failing (routine, field, error) is reported
    at once."""
    routine_parity(family, size)


@pytest.mark.parametrize("family,size", params(tiny=False))
def test_width_run_rms(family, size):
    """12 whole steps at the size (graph replay, strips, folded walls): field
    RMS against the oracle below RMS_RUN, every failing field reported at once."""
    run_rms(family, size)


@pytest.mark.parametrize("family,size", params(tiny=True))
def test_tiny_routine_parity(family, size):
    """test_width_routine_parity on the grids with Lm or Mm <= 5."""
    routine_parity(family, size)


@pytest.mark.parametrize("family,size", params(tiny=True))
def test_tiny_run_rms(family, size):
    """test_width_run_rms on the grids with Lm or Mm <= 5."""
    run_rms(family, size)


BITWISE_FIELDS = ("zeta", "ubar", "vbar", "u", "v", "t", "FlxU", "FlxV", "We", "rufrc", "rvfrc", "Hz", "Akt")
# variant -> (environment, the path entry it changes)
VARIANTS = {
    "prs_tiles": ({"ROMS_GPU_PRS_STRIP": "0"}, {"strips": None}),
    "tracer_strips": ({"ROMS_GPU_T_STRIP": "1"}, {}),   # opt-in (roms_shim.cpp P.t_strip), same 60-column ownership
    "edge_launches": ({"ROMS_GPU_S2D_EDGES": "1"}, {"edges": 1}),
}
_DEFAULT_RUN = {}   # one entry: the size last asked for


def run_bits(size, env, want):
    env = dict({k: None for k in ("ROMS_GPU_PRS_STRIP", "ROMS_GPU_T_STRIP", "ROMS_GPU_S2D_EDGES")}, **env)
    _, m = width_model("kpp", size, env, want)
    try:
        m.step(4)
        m.sync()
        return {f: m.get(f) for f in BITWISE_FIELDS}
    finally:
        m.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", [s for s in SIZES if s[0] in (60, 61, 62) and s[1] in (4, 12)],
                         ids=lambda s: "%dx%d" % s)
def test_width_variants_bitwise(size, variant):
    """4 whole steps at the strip sizes with the prsgrd tiles, the tracer
    strips or the separate edge launches: the bits of the defaults."""
    if size not in _DEFAULT_RUN:
        _DEFAULT_RUN.clear()
        _DEFAULT_RUN[size] = run_bits(size, {}, None)
    ref = _DEFAULT_RUN[size]
    env, change = VARIANTS[variant]
    edges, strips, seg, _ = SIZES[size]
    want = dict({"edges": edges, "strips": strips, "omega_seg": seg}, **change)
    got = run_bits(size, env, want)
    assert all(np.isfinite(ref[f]).all() for f in BITWISE_FIELDS)
    bad = [(f, float(np.nanmax(np.abs(got[f] - ref[f])))) for f in BITWISE_FIELDS if not np.array_equal(got[f], ref[f])]
    assert not bad, (size, variant, bad)
