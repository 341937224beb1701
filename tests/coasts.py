"""Coastlines placed on the tile, strip, block and wall edges of the kernels.

Every land mask of the analytic cases is one of three shapes (the basin's
island, the Pipes_ana coast, the Rivers_ana coast), and where those fall
relative to a 64 x 4 tile, a 60-column strip or a 16-column block is an
accident of the grid size.  Almost every kernel of the hot path reads rmask,
umask, vmask or pmask through a staged window, a feed lane or a clamped
stencil, and a window loaded one cell short changes no number unless land
lies within two cells of the window's edge.  The builders below put land
there on purpose; apply_coast puts a coast into an oracle and a model after
init, and tests/test_coasts.py (CPU) and tests/test_gpu_coasts.py (GPU) run
them.  In the style of tests/branch_states.py: made from the CPU oracle
alone, with numpy restatements beside.

All arrays are on the (Mm+4, Lm+4) layout, cell (i, j) at [j+1, i+1].

The horizontal edges, taken from the constants of the code (an edge e is the
last column of a unit, e+1 the first of the next; edge_columns):
  * 64-column tiles (kBX, roms_dev.h:331) start at tile_i0(i0)
    (roms_dev.h:340): i0 rounded down to i = 1 mod 16.  Ranges from
    istrR = 0 (and -1) start at -15: edges 48, 112, ...; ranges from
    istr = 1 and istrU = 2 start at 1: edges 64, 128, ...
  * a prsgrd / tracer strip owns kStripOwn = 60 columns
    (k_prsgrd_strip.hip:48): edges 60, 120, ...
  * the 16-column blocks of the segment solvers (kSegCW, roms_dev.h:373,
    ROMS_SEG_CW :371), of k_omega_seg above N = 63 and of the chain kernels
    (kChainCW, k_chain.h:22) start at tile_i0 too: edges 16, 32, ...
The rows: tiles are kBY = 4 rows (roms_dev.h:331) from j0 = 0 or 1, so every
residue mod 4 starts a tile of some range; the strips run rows jA = 3 ..
Mm-1 between closed walls in chunks of ROMS_PRS_STRIP_J = 8
(k_prsgrd_strip.hip:53): the first chunk ends at row 10, the second starts
at row 11; the staged tracer blocks are ROMS_T_HSTG_ROWS = 8 rows
(k_common.h:307).

  specks    isolated single land cells on the lattice (j - 2 i) mod 5 = 0 in
            the columns e-2 .. e+2 of every edge, and in columns 1, 2, Lm-1,
            Lm: every five neighbouring columns hold every row 1 .. Mm once
            (rows 1, 2, 3, Mm-1, Mm, 10 / 11 and every residue mod 4 among
            them), no two cells touch, not even at a corner.  Isolated
            cells leave pmask at 1 everywhere, so a two-cell bar and a
            diagonal pair stand between the edges (columns 7 .. 11).
  channels  a slab of land with one-cell-wide wet channels through it along
            eta, each on an edge column (e and e+1 in turn), one along xi
            that joins them, a diagonal staircase of wet cells (pmask 0 at
            every step) and one wet cell enclosed on all eight sides
  blocks    solid land over a whole 64-column tile of either origin (4 tile
            rows; 2 where Mm < 10, a whole tile being most of such a grid),
            over a whole 16-column block in every row, and over a strip's
            first and last owned columns
  walls     land in the ghost line and in the first and last interior line
            of all four sides, in pieces of period 6, so one edge shows
            ghost land beside water, land on both lines, interior land
            beside a wet ghost cell and open water
  random    25 % land from a fixed seed
"""
import numpy as np

from test_gpu_parity import PROGNOSTIC, RTOL_ROUTINE, interior, relerr

MASKS = ("rmask", "umask", "vmask", "pmask")
MASKED = (("zeta", "rmask"), ("ubar", "umask"), ("vbar", "vmask"), ("u", "umask"), ("v", "vmask"))
MIXING = ("visc2_r", "visc2_p", "diff2")
VISC = (40.0, 40.0, 15.0)     # visc2_r, visc2_p [m2/s], diff2: stable on 2 km cells at dt = 60 s (nu dt / dx2 = 6e-4)

K_BX, K_BY = 64, 4            # roms_dev.h:331
K_ROW_ALIGN = 16              # tile_i0, roms_dev.h:340
K_STRIP_OWN = 60              # k_prsgrd_strip.hip:48
K_STRIP_J, K_STRIP_JA = 8, 3  # k_prsgrd_strip.hip:53; prsgrd_strip_rows' first row between closed walls
K_BLOCK = 16                  # kSegCW roms_dev.h:373, kChainCW k_chain.h:22


def tile_i0(i0):
    """roms_dev.h:340."""
    return i0 - ((i0 - 1) & (K_ROW_ALIGN - 1))


def edge_columns(Lm):
    """{family: [e, ..]}: the last columns e <= Lm of the units of each family."""
    def ends(first, width):
        return [e for e in range(first + width - 1, Lm + 1, width) if e >= 1]
    return {"tiles from i = 0": ends(tile_i0(0), K_BX), "tiles from i = 1": ends(tile_i0(1), K_BX),
            "strips": ends(1, K_STRIP_OWN), "16-column blocks": ends(tile_i0(1), K_BLOCK)}


def all_edges(Lm):
    return sorted({e for es in edge_columns(Lm).values() for e in es})


def empty(Lm, Mm):
    return np.zeros((Mm + 4, Lm + 4), dtype=bool)


# ---------------------------------------------------------------- masks ----
def derive_masks(rmask, umask, vmask, pmask, Lm, Mm):
    """setup_grid1.F's umask, vmask and pmask from rmask, in place, over the
    ranges oracle_main.c setup_grid1 and host_init.cpp fill between closed or
    open walls: u at i = 1..Lm+1, j = 0..Mm+1; v at i = 0..Lm+1, j = 1..Mm+1;
    p at i = 1..Lm+1, j = 1..Mm+1 (3 or 4 wet cells: 1; a straight pair: 2;
    a diagonal pair, one or none: 0).  Every other entry stays."""
    J, I = slice(1, Mm + 3), slice(2, Lm + 3)        # j = 0..Mm+1, i = 1..Lm+1
    Iw = slice(1, Lm + 2)                            # i - 1
    umask[J, I] = rmask[J, I] * rmask[J, Iw]
    J, I = slice(2, Mm + 3), slice(1, Lm + 3)        # j = 1..Mm+1, i = 0..Lm+1
    Js = slice(1, Mm + 2)                            # j - 1
    vmask[J, I] = rmask[J, I] * rmask[Js, I]
    J, I = slice(2, Mm + 3), slice(2, Lm + 3)        # j = 1..Mm+1, i = 1..Lm+1
    wet = (rmask > 0.5).astype(int)
    a, b, c, d = wet[J, Iw], wet[J, I], wet[Js, Iw], wet[Js, I]
    n = a + b + c + d
    straight = (a * c + b * d + a * b + c * d) > 0
    pmask[J, I] = np.where(n >= 3, 1.0, np.where((n == 2) & straight, 2.0, 0.0))


def coast_band(rmask):
    """The wet interior points (Mm, Lm) within two cells of land: the
    8-neighbourhood of the land, taken twice."""
    near = np.asarray(rmask) < 0.5
    for _ in range(2):
        p = np.pad(near, 1)
        near = np.zeros_like(near)
        for dj in range(3):
            for di in range(3):
                near |= p[dj:dj + near.shape[0], di:di + near.shape[1]]
    return (near & (np.asarray(rmask) > 0.5))[2:-2, 2:-2]


# ------------------------------------------------------------- builders ----
def speck_columns(Lm):
    """The columns specks targets: e-2 .. e+2 of every edge, and 1, 2, Lm-1, Lm."""
    cols = {1, 2, Lm - 1, Lm}
    for e in all_edges(Lm):
        cols |= set(range(e - 2, e + 3))
    return sorted(c for c in cols if 1 <= c <= Lm)


def speck_extras(Lm, Mm):
    """((i, j), ..): the bar (pmask 2) and the diagonal pair (pmask 0) of specks."""
    j = Mm // 2
    return ((7, j), (8, j + 1), (10, j), (11, j))


def specks(Lm, Mm):
    land = empty(Lm, Mm)
    for i in speck_columns(Lm):
        for j in range(1, Mm + 1):
            if (j - 2 * i) % 5 == 0:
                land[j + 1, i + 1] = True
    for i, j in speck_extras(Lm, Mm):
        land[j + 1, i + 1] = True
    return land


def channel_geometry(Lm, Mm):
    """The slab's rows (s0, s1) and columns (c0, c1), the eta channels'
    columns, the xi channel's row, the staircase cells and the enclosed cell."""
    s0, s1 = (3, Mm - 2) if Mm >= 8 else (2, Mm - 1)
    c0, c1 = 3, Lm - 2
    eta = []
    for q, e in enumerate(all_edges(Lm)):
        c = e + q % 2
        if c0 < c < c1 and (not eta or c - eta[-1] >= 2):
            eta.append(c)
    xi = s0 + (s1 - s0 + 1) // 2
    stairs = [(4 + q, s0 + q) for q in range(min(s1 - s0 + 1, 6))]
    return dict(rows=(s0, s1), cols=(c0, c1), eta=eta, xi=xi, stairs=stairs, enclosed=(12, s0 + 1))


def channels(Lm, Mm):
    g = channel_geometry(Lm, Mm)
    (s0, s1), (c0, c1) = g["rows"], g["cols"]
    land = empty(Lm, Mm)
    land[s0 + 1:s1 + 2, c0 + 1:c1 + 2] = True
    for c in g["eta"]:
        land[s0 + 1:s1 + 2, c + 1] = False
    if g["eta"]:
        land[g["xi"] + 1, g["eta"][0] + 1:g["eta"][-1] + 2] = False
    for i, j in g["stairs"] + [g["enclosed"]]:
        land[j + 1, i + 1] = False
    return land


def block_pieces(Lm, Mm):
    """[(what, i0, i1, j0, j1), ..]: the solid pieces of blocks, clipped to the grid."""
    rows = K_BY if Mm >= 10 else K_BY // 2
    j0 = 1 + K_BY if Mm >= 2 * K_BY else 1      # a tile row of the ranges from j = 1
    out = []
    for origin in (0, 1):
        first = tile_i0(origin)
        # the first tile of the origin that lies inside the grid for the most part
        t0 = first if first >= 1 or first + K_BX - 1 >= Lm // 2 else first + K_BX
        out.append(("tile of ranges from i = %d" % origin, max(t0, 1), min(t0 + K_BX - 1, Lm), j0, j0 + rows - 1))
        if t0 + 2 * K_BX - 1 <= Lm:
            out.append(("second tile of ranges from i = %d" % origin, t0 + K_BX, t0 + 2 * K_BX - 1, j0, j0 + rows - 1))
    out.append(("16-column block in every row", K_BLOCK + 1, 2 * K_BLOCK, 1, Mm))
    for s in range(0, Lm, K_STRIP_OWN):
        out.append(("strip's first owned column", s + 1, s + 1, K_STRIP_JA, Mm - 1))
        if s + K_STRIP_OWN <= Lm:
            out.append(("strip's last owned column", s + K_STRIP_OWN, s + K_STRIP_OWN, K_STRIP_JA, Mm - 1))
    return out


def blocks(Lm, Mm):
    land = empty(Lm, Mm)
    for _, i0, i1, j0, j1 in block_pieces(Lm, Mm):
        land[j0 + 1:j1 + 2, i0 + 1:i1 + 2] = True
    return land


def walls(Lm, Mm):
    """Along each side, with p the index along it: the ghost line is land
    where p mod 6 is 0, 1 or 2, the first (last) interior line where it is 2
    or 3."""
    land = empty(Lm, Mm)
    pi, pj = np.arange(-1, Lm + 3), np.arange(-1, Mm + 3)
    gi, gj = (pi % 6 <= 2) & (pi >= 1) & (pi <= Lm), (pj % 6 <= 2) & (pj >= 1) & (pj <= Mm)
    ni, nj = ((pi % 6 == 2) | (pi % 6 == 3)) & (pi >= 1) & (pi <= Lm), \
             ((pj % 6 == 2) | (pj % 6 == 3)) & (pj >= 1) & (pj <= Mm)
    land[1, gi] = land[Mm + 2, gi] = True          # j = 0, Mm+1
    land[gj, 1] = land[gj, Lm + 2] = True          # i = 0, Lm+1
    land[2, ni] = land[Mm + 1, ni] = True          # j = 1, Mm
    land[nj, 2] = land[nj, Lm + 1] = True          # i = 1, Lm
    return land


def random(Lm, Mm, seed=20):
    land = empty(Lm, Mm)
    land[2:Mm + 2, 2:Lm + 2] = np.random.default_rng(seed).random((Mm, Lm)) < 0.25
    return land


def rank_edges(Lm, Mm, xs, ys):
    """Land about the rank edges of a decomposed grid: xs the last columns,
    ys the last rows of the ranks that have a neighbour beyond.  About a
    column e (rows from the south wall; about a row f the same along xi,
    columns from the west wall): the edge on land (e and e+1 land, rows 2 ..
    3), beside land on either side (e+1 alone row 5, e alone row 7), across
    a one-cell channel along xi (rows 9 and 11 land over e-3 .. e+4, row 10
    wet), along a one-cell channel's flank (column e wet between land at e-1
    and e+1, rows 15 .. 17; column e+1 wet between e and e+2, rows 19 .. 21;
    about a row: columns 14 .. 16 only).  The grid must keep the two families
    apart: Mm >= 22, every e >= 20 and every f within 9 .. Mm-5."""
    land = empty(Lm, Mm)

    def about(e, put):
        for a, s in ((e, 2), (e + 1, 2), (e, 3), (e + 1, 3), (e + 1, 5), (e, 7)):
            put(a, s)
        for a in range(e - 3, e + 5):
            put(a, 9)
            put(a, 11)

    def put_x(i, j):
        land[j + 1, i + 1] = True

    def put_y(j, i):
        land[j + 1, i + 1] = True

    for e in xs:
        assert e >= 20 and e + 4 <= Lm and Mm >= 22
        about(e, put_x)
        for j in (15, 16, 17):
            put_x(e - 1, j)
            put_x(e + 1, j)
        for j in (19, 20, 21):
            put_x(e, j)
            put_x(e + 2, j)
    for f in ys:
        assert 9 <= f <= Mm - 5
        about(f, put_y)
        for i in (14, 15, 16):
            put_y(f - 1, i)
            put_y(f + 1, i)
    return land


COASTS = {"specks": specks, "channels": channels, "blocks": blocks, "walls": walls, "random": random}


# ------------------------------------------------------------- applying ----
def coast_masks(o, land):
    """The oracle's four mask planes with `land` added to rmask and the other
    three restated from it (copies)."""
    rm, um, vm, pk = (o.field(n)[0].copy() for n in MASKS)
    rm[land] = 0.0
    derive_masks(rm, um, vm, pk, o.cfg.LLm, o.cfg.MMm)
    return dict(zip(MASKS, (rm, um, vm, pk)))


def put_coast(m, masks, visc=None):
    """Model side of apply_coast: this rank's window of the global mask planes
    (the whole of them on a single domain), the masked rest state, the mixing
    coefficients, then the rest-state sequence (Model.init_sequence)."""
    win = (slice(m.jSW, m.jSW + m.Mm + 4), slice(m.iSW, m.iSW + m.Lm + 4))
    for n in MASKS:
        m.put(n, masks[n][win])
    for n, mk in MASKED:
        m.put(n, m.get(n) * masks[mk][win])
    if visc is not None:
        for n, add in zip(MIXING, visc):
            m.put(n, m.get(n) + add)
    m.init_sequence()


def apply_coast(o, m, land, visc=None):
    """Put the coast into the oracle o and the model m (None: the oracle
    alone) after init and before any step: rmask, the three masks restated
    from it, zeta, ubar, vbar, u, v times their masks, with visc = (visc2_r,
    visc2_p, diff2) those added uniformly to the mixing coefficients (the
    closed basin has none of its own, so that pmask and t3dmix are live; a
    sponge keeps its bands), then the rest-state sequence of main.F:244-288
    on both sides.  Asserts that both sides agree at step 0; returns the
    mask planes."""
    cfg = o.cfg
    masks = coast_masks(o, land)
    for n in MASKS:
        o.field(n)[0][...] = masks[n]
    for n, mk in MASKED:
        o.field(n)[...] *= masks[mk]
    if visc is not None:
        for n, add in zip(MIXING, visc):
            o.field(n)[...] += add
    for routine in ("set_depth", "set_HUV", "omega"):
        o.call(routine)
    o.call("rho_eos", o.tindex()[4])
    if m is not None:
        put_coast(m, masks, visc)
        m.sync()
        bad = []
        we = float(np.abs(interior(o.field("We"), cfg.LLm, cfg.MMm)).max())
        for n in PROGNOSTIC + ["rho"] + list(MASKS) + list(MIXING):
            a, b = interior(m.get(n), cfg.LLm, cfg.MMm), interior(o.field(n), cfg.LLm, cfg.MMm)
            # Wi to We's maximum, as the sweeps' routine_errors: at rest it is cancellation noise of We
            e = float(np.abs(a - b).max()) / max(we, 1e-300) if n == "Wi" else relerr(a, b)
            if not e <= RTOL_ROUTINE:
                bad.append((n, e))
        assert not bad, ("step 0", bad)
    return masks
