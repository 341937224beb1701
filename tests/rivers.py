"""River mouths placed on the tile, strip, block, wall and rank edges of the kernels.

The analytic Rivers_ana case has one river whose mouth cells lie in a
straight coast with water to the north only: v faces of positive sign, river
index 1, one wet neighbour per mouth, dx = dy.  The builders below put
mouths into the coasts of tests/coasts.py so that every arm of the river
hooks (step2d_FB.F:531-554, pre_step3d4S.F:493-522, step3d_uv2.F:689-717,
compute_horiz_tracer_fluxes.h:217-246) is taken: u and v faces of both
signs, several rivers, mouths with 1 to 4 wet neighbours, faces on both
sides of every tile, strip and block edge of coasts.edge_columns, in the
ghost line and the first interior line of the walls, and on either side of a
rank cut.  tests/test_rivers.py (CPU) checks that the faces are where this
says, tests/test_gpu_rivers_sweep.py (GPU) runs them against the oracle.

All arrays are on the (Mm+4, Lm+4) layout, cell (i, j) at [j+1, i+1]; a u
face (i, j) lies between the cells (i-1, j) and (i, j), a v face between
(i, j-1) and (i, j).  A face value is 10 * river + signed fraction of the
river's discharge: positive towards larger i or j.  A builder returns
(land, rfrc, ridx): the land to add to the case's rmask, and on the mouth
cells the share of their river's discharge and the river's number.
"""
import numpy as np

import coasts

RIV_EPS = 1e-3     # a face is one where |riv_flx| > 1e-3 (step2d_FB.F:534)


def _wet(land):
    return np.where(land, 0.0, 1.0)


# --------------------------------------------------------- calc_river_flux ----
def calc_river_flux(rmask, rfrc, ridx):
    """river_frc.F:242-279 restated: every mouth cell (rfrc > 0) of i = 0 ..
    Lm+1, j = 0 .. Mm+1 shares rfrc equally among its wet neighbours, the
    count of them an integer; the four assignments in the reference's order
    (west, east, south, north; j outer, i inner), so a face written twice
    keeps the later value.  ValueError where the reference raises 'river grid
    position error': no wet neighbour, or a wet mouth.  Returns riv_uflx,
    riv_vflx."""
    rmask = np.asarray(rmask, dtype=np.float64)
    Mm, Lm = rmask.shape[0] - 4, rmask.shape[1] - 4
    uf, vf = np.zeros_like(rmask), np.zeros_like(rmask)
    for j in range(0, Mm + 2):
        for i in range(0, Lm + 2):
            f = float(rfrc[j + 1, i + 1])
            if not f > 0:
                continue
            w, e, s, n = rmask[j + 1, i], rmask[j + 1, i + 2], rmask[j, i + 1], rmask[j + 2, i + 1]
            faces = int(w + e + s + n)
            if faces == 0 or rmask[j + 1, i + 1] > 0:
                raise ValueError("river grid position error at i = %d, j = %d" % (i, j))
            k = 10 * int(ridx[j + 1, i + 1])
            if w > 0:
                uf[j + 1, i + 1] = -f / faces + k
            if e > 0:
                uf[j + 1, i + 2] = f / faces + k
            if s > 0:
                vf[j + 1, i + 1] = -f / faces + k
            if n > 0:
                vf[j + 2, i + 1] = f / faces + k
    return uf, vf


def mouth_faces(rmask, rfrc):
    """{(i, j): wet neighbours} of every mouth cell, as calc_river_flux counts them."""
    out = {}
    for jj, ii in zip(*np.nonzero(np.asarray(rfrc) > 0)):
        out[int(ii) - 1, int(jj) - 1] = int(rmask[jj, ii - 1] + rmask[jj, ii + 1] + rmask[jj - 1, ii] + rmask[jj + 1, ii])
    return out


def split(flx):
    """(is a face, river index, signed fraction) of a plane of face values, with the hooks' arithmetic."""
    flx = np.asarray(flx, dtype=np.float64)
    on = np.abs(flx) > RIV_EPS
    idx = np.where(on, np.rint(flx / 10), 0).astype(int)
    return on, idx, np.where(on, flx - 10 * idx, 0.0)


def census(uflx, vflx, nriv):
    """What a pair of face planes holds: {"class": {(dir, sign): faces} for
    dir 0 (u) and 1 (v) and sign -1 and +1, "river": {r: faces} for r = 1 ..
    nriv, "fraction": {|fraction| rounded to 12 digits: faces}}."""
    out = {"class": {(d, s): 0 for d in (0, 1) for s in (-1, 1)}, "river": {r: 0 for r in range(1, nriv + 1)},
           "fraction": {}}
    for d, flx in enumerate((uflx, vflx)):
        on, idx, frac = split(flx)
        for s in (-1, 1):
            out["class"][d, s] = int(np.count_nonzero(on & (np.sign(frac) == s)))
        for r in np.unique(idx[on]):
            out["river"][int(r)] = out["river"].get(int(r), 0) + int(np.count_nonzero(on & (idx == r)))
        for a in np.abs(frac[on]):
            key = round(float(a), 12)
            out["fraction"][key] = out["fraction"].get(key, 0) + 1
    return out


def class_masks(uflx, vflx):
    """{(dir, sign): boolean plane of the faces of that class}."""
    out = {}
    for d, flx in enumerate((uflx, vflx)):
        on, _, frac = split(flx)
        for s in (-1, 1):
            out[d, s] = on & (np.sign(frac) == s)
    return out


# ---------------------------------------------------------------- builders ----
def deal(land, cells, nriv, rmask0=None):
    """(land, rfrc, ridx) with the rivers 1 .. nriv dealt in turn to `cells`
    ((i, j), in the order given; those without a wet neighbour are left
    out), each mouth taking 1 / (its river's mouth count).  rmask0: the
    case's own rmask (all water when None)."""
    rmask = _wet(land) if rmask0 is None else np.where(land, 0.0, rmask0)
    cells = [(i, j) for i, j in cells
             if rmask[j + 1, i] + rmask[j + 1, i + 2] + rmask[j, i + 1] + rmask[j + 2, i + 1] > 0]
    assert len(cells) >= nriv, (len(cells), nriv)
    rfrc, ridx = np.zeros(land.shape), np.zeros(land.shape, dtype=int)
    count = [len(cells[r::nriv]) for r in range(nriv)]
    for q, (i, j) in enumerate(cells):
        assert land[j + 1, i + 1]
        ridx[j + 1, i + 1] = q % nriv + 1
        rfrc[j + 1, i + 1] = 1.0 / count[q % nriv]
    return land, rfrc, ridx


def _interior_cells(land):
    """The land cells of 1 .. Lm, 1 .. Mm as (i, j), column by column."""
    Mm, Lm = land.shape[0] - 4, land.shape[1] - 4
    return [(i, j) for i in range(1, Lm + 1) for j in range(1, Mm + 1) if land[j + 1, i + 1]]


def speck_mouths(Lm, Mm, nriv, more_land=None):
    """coasts.specks with every land cell a mouth.  An isolated speck has
    four wet neighbours: a u face and a v face of each sign, a quarter of the
    mouth's share through each; the bar's two cells have three, and so have
    the specks of the first and last interior line, whose ghost neighbour is
    made land here (a face in a closed wall carries nothing into the basin:
    the fast step's hook starts at istrU and jstrV).  more_land: land to add
    before the mouths are dealt, those it buries left out."""
    land = coasts.specks(Lm, Mm)
    cells = _interior_cells(land)
    for i, j in cells:
        for gi, gj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
            if gi in (0, Lm + 1) or gj in (0, Mm + 1):
                land[gj + 1, gi + 1] = True
    if more_land is not None:
        land = land | more_land
    return deal(land, cells, nriv)


def spit_cells(land):
    """((i, j), (i, j')): the body and the tip of a one-cell-wide spit of two
    cells to add to `land`: it hangs from a straight rim along xi into open
    water three cells wide and three deep, southward or northward.  The body
    then has two wet neighbours, the tip three."""
    Mm, Lm = land.shape[0] - 4, land.shape[1] - 4
    L = lambda i, j: bool(land[j + 1, i + 1])
    for step in (-1, 1):
        for j in range(4, Mm - 2):
            for i in range(3, Lm - 1):
                if not all(L(a, j) for a in (i - 1, i, i + 1)):
                    continue
                rows = [j + step * q for q in (1, 2, 3)]
                if all(1 <= r <= Mm for r in rows) and not any(L(a, r) for a in (i - 1, i, i + 1) for r in rows):
                    return (i, rows[0]), (i, rows[1])
    raise AssertionError("no room for a spit")


def block_mouths(Lm, Mm, nriv, more_land=None, spit=None):
    """coasts.blocks and a spit (spit_cells).  The mouths: every land cell of
    a straight rim, one wet neighbour each -- to the west, east, south or
    north of it by the side of the block it is on -- and the spit's body (two
    wet neighbours, a u face of each sign) and tip (three).  more_land: land
    to add first; spit: the spit's cells where more_land holds one already."""
    land = coasts.blocks(Lm, Mm)
    if more_land is not None:
        land = land | more_land
    spit = spit_cells(land) if spit is None else spit
    for i, j in spit:
        land[j + 1, i + 1] = True
    rmask = _wet(land)
    cells = [c for c, n in mouth_faces(rmask, land & _inside(Lm, Mm)).items() if n == 1]
    # the rim cells beside the spit's body lost their place on a straight rim; keep those whose wet
    # neighbour is an interior cell
    keep = []
    for i, j in sorted(cells):
        (wi, wj), = [(a, b) for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)) if rmask[b + 1, a + 1] > 0]
        if 1 <= wi <= Lm and 1 <= wj <= Mm:
            keep.append((i, j))
    return deal(land, keep + list(spit), nriv)


def _inside(Lm, Mm):
    m = np.zeros((Mm + 4, Lm + 4), dtype=bool)
    m[2:Mm + 2, 2:Lm + 2] = True
    return m


def wall_mouths(Lm, Mm, nriv=3):
    """coasts.walls.  The mouths: the ghost-line land cells beside a wet cell
    of the first (last) interior line -- i = 0 flowing into i = 1, likewise
    at Lm+1, j = 0 and Mm+1: the face at i = 1 lies outside istrU .. iend (at
    j = 1 outside jstrV .. jend), so the fast step and the predictor skip it
    while the corrector (from istr, jstr) and the tracer fluxes do not -- and
    every land cell of the first and last interior lines, flowing inward,
    along the wall, and out into a wet ghost cell."""
    land = coasts.walls(Lm, Mm)
    cells = []
    for i in range(1, Lm + 1):
        cells += [(i, 0)] if land[1, i + 1] and not land[2, i + 1] else []
        cells += [(i, Mm + 1)] if land[Mm + 2, i + 1] and not land[Mm + 1, i + 1] else []
    for j in range(1, Mm + 1):
        cells += [(0, j)] if land[j + 1, 1] and not land[j + 1, 2] else []
        cells += [(Lm + 1, j)] if land[j + 1, Lm + 2] and not land[j + 1, Lm + 1] else []
    rim = [(i, j) for i, j in _interior_cells(land) if i in (1, Lm) or j in (1, Mm)]
    return deal(land, cells + rim, nriv)


def rank_mouths(Lm, Mm, xs, ys, nriv=3):
    """coasts.rank_edges(Lm, Mm, xs, ys) and four cells at the walls.  About
    every cut column e: (e, 7), a mouth in the last owned column of one rank
    whose eastern face u(e+1) is the first u point of the next; (e+1, 5), its
    mirror image, whose western face u(e+1) is its own rank's first u point
    and carries water into the rank before; (e-1, 16) and (e+1, 16) into the
    one-cell channel at e, (e, 20) and (e+2, 20) into the one at e+1.  About
    every cut row f the same along eta: (7, f), (5, f+1), (15, f-1),
    (15, f+1).  At the walls: (1, 4), (Lm, 4), (4, 1), (4, Mm) with a wet
    ghost cell beside them -- the face u(1, 4) is at a rank's istr but not
    its istrU."""
    land = coasts.rank_edges(Lm, Mm, xs, ys)
    cells = []
    for e in xs:
        cells += [(e, 7), (e + 1, 5), (e - 1, 16), (e + 1, 16), (e, 20), (e + 2, 20)]
    for f in ys:
        cells += [(7, f), (5, f + 1), (15, f - 1), (15, f + 1)]
    walls = [(1, 4), (Lm, 4), (4, 1), (4, Mm)]
    for i, j in walls:
        assert not land[j:j + 3, i:i + 3].any(), (i, j)
        land[j + 1, i + 1] = True
    return deal(land, cells + walls, nriv)


def both_mouths(Lm, Mm, nriv):
    """(land, speck mouths, block mouths): one land that holds the specks and
    the blocks with their spit, and the (rfrc, ridx) of speck_mouths and of
    block_mouths on it -- for a change of faces in mid-run."""
    specks = speck_mouths(Lm, Mm, nriv)[0]
    land = block_mouths(Lm, Mm, nriv, specks)[0]
    ls, sf, si = speck_mouths(Lm, Mm, nriv, land)
    lb, bf, bi = block_mouths(Lm, Mm, nriv, land, spit_cells(coasts.blocks(Lm, Mm) | specks))
    assert np.array_equal(ls, land) and np.array_equal(lb, land)
    return land, (sf, si), (bf, bi)


def receiving(cls, d, s):
    """The cells the faces `cls` of class (d, s) flow into."""
    return cls if s > 0 else np.roll(cls, -1, axis=1 - d)


def fed_cells(uflx, vflx, nriv):
    """{r: the interior cells that river r's faces flow into and no other river's}."""
    planes = [split(f) for f in (uflx, vflx)]

    def fed(which):
        cells = np.zeros(uflx.shape, dtype=bool)
        for d, (on, idx, frac) in enumerate(planes):
            for s in (-1, 1):
                cells |= receiving(on & which(idx) & (np.sign(frac) == s), d, s)
        cells[:2] = cells[-2:] = False
        cells[:, :2] = cells[:, -2:] = False
        return cells

    return {r: fed(lambda idx, r=r: idx == r) & ~fed(lambda idx, r=r: (idx != r) & (idx > 0)) for r in range(1, nriv + 1)}


def own_water(dS, fed, r):
    """Whose water came in, from a twin run in which river r alone is 1 PSU
    saltier: dS (N, Mm+4, Lm+4) is the twin's salinity less the run's.  The
    basin's salinity (35 +- 0.25) is farther from every river's than the
    rivers' are from one another, so a cell's salinity by itself is nearest
    the saltiest river's whichever river feeds it; the twin's change is the
    fraction of river r's water in a cell.  Returns (the largest change in
    the cells river r alone feeds, the largest in the cells another river
    alone feeds): the first is that river's water, the second what 20 steps
    of advection at a Courant number of 1e-3 and of diffusion at diff2 dt /
    dx2 = 2e-4 carry over from a neighbouring mouth -- a small part of the
    first; rivers told apart wrongly would swap the two."""
    own = float(np.abs(dS[:, fed[r]]).max())
    other = max(float(np.abs(dS[:, fed[q]]).max()) for q in fed if q != r)
    return own, other


# ---------------------------------------------------------------- applying ----
def river_tracers(nriv):
    """riv_trc (nriv, 2), distinct per river and per tracer: T = 15 + 5 r, S = 1 + 2 r (the basin: 4 to 14, 35)."""
    r = np.arange(1, nriv + 1, dtype=np.float64)
    return np.stack([15.0 + 5.0 * r, 1.0 + 2.0 * r], axis=1)


def river_volumes(o, uflx, vflx, nriv, speed=0.03):
    """riv_vol (nriv,), distinct per river: the discharge at which the
    river's fastest face flows at speed * (1 + r / (4 nriv)) [m/s] over the
    rest depth (h of the two cells; a mouth's own h is as defined as a wet
    cell's in the analytic basin)."""
    h, dn_u, dm_v = o.field("h")[0], o.field("dn_u")[0], o.field("dm_v")[0]
    vol = np.full(nriv, np.inf)
    for flx, dn, sh in ((uflx, dn_u, (0, 1)), (vflx, dm_v, (1, 0))):
        on, idx, frac = split(flx)
        depth = 0.5 * (h + np.roll(h, sh, axis=(0, 1)))
        for jj, ii in zip(*np.nonzero(on)):
            r = idx[jj, ii] - 1
            if dn[jj, ii] > 0:     # a face of the outer ghost lines has no metric, and no hook reads it
                vol[r] = min(vol[r], dn[jj, ii] * depth[jj, ii] / abs(frac[jj, ii]))
    assert np.isfinite(vol).all(), vol
    return vol * speed * (1.0 + np.arange(1, nriv + 1) / (4.0 * nriv))


def put_rivers(m, vol, trc, uflx, vflx):
    """Model side of apply_rivers: this rank's window of the global face
    planes, halo included (the whole of them on a single domain)."""
    win = (slice(m.jSW, m.jSW + m.Mm + 4), slice(m.iSW, m.iSW + m.Lm + 4))
    m.set_river_frc(vol, trc, uflx[win], vflx[win])


def apply_rivers(o, m, land, mouths, vol, trc, visc=None):
    """coasts.apply_coast(o, m, land, visc), then the faces of calc_river_flux
    on the resulting rmask with mouths = (rfrc, ridx) into the oracle
    (set_river_faces) and the model (set_river_frc; m None: the oracle
    alone).  vol None: river_volumes.  Returns (masks, riv_uflx, riv_vflx,
    vol)."""
    masks = coasts.apply_coast(o, m, land, visc)
    uflx, vflx = calc_river_flux(masks["rmask"], *mouths)
    nriv = int(np.max(mouths[1]))
    if vol is None:
        vol = river_volumes(o, uflx, vflx, nriv)
    o.set_river_faces(vol, trc, uflx, vflx)
    if m is not None:
        put_rivers(m, vol, trc, uflx, vflx)
    return masks, uflx, vflx, vol
