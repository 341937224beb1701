"""A numpy restatement of the tracer budget terms of the corrector: DIAGNOSTICS with diag_trc, non-isoneutral build
(diagnostics.F:608-661 diag_t_adv_hc4, step3d_t_ISO.F:236-248, 909-917, 1102-1134, compute_horiz_tracer_fluxes.h:45-114,
146-196, 217-246 with UPSTREAM_TS, compute_vert_tracer_fluxes.h:37-71).

Pure functions of their arguments.  Arrays are (N, Mm+4, Lm+4) or (Mm+4, Lm+4) in the layout of Model.get: index
[k-1, j+1, i+1] holds (i, j, k); w-point arrays have N+1 planes, plane k at [k].  Every operation is the reference's,
in its order, in float64: the results are meant to be compared bit for bit.  Outside the written ranges the terms
are 0.

The edge rule of the elementary differences is that of compute_horiz_tracer_fluxes.h:50-84, 131-165: on a physical,
non-periodic edge of the whole grid the difference one face outside is a copy of the first one inside; on a
periodic side or a rank boundary nothing is copied.  `edges` = (west, east, south, north) says which sides of the
rank are such physical edges.  edge_rule="as_written" gives what diag_t_adv_hc4 does in eta (:645-646: the north flag
decides the south copy and vice versa), for the negative control; in xi the two forms differ only in the slice
lengths of :627-628 (equal on a square grid).
"""
import numpy as np

C6_UP = 0.1666666666666666    # compute_horiz_tracer_fluxes.h:106
C6_C4 = 0.1666666666666667    # diagnostics.F:635
RIV_EPS = 1e-3


def _pos(a):
    return np.where(a > 0.0, a, 0.0)


def _neg(a):
    return np.where(a < 0.0, a, 0.0)


def _nint(x):
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


def _xi_terms(T, um, Fl, Lm, Mm, lo_copy, hi_copy):
    """(adv, FX) over faces i = 1..Lm+1, j = 1..Mm of the arrays' last axis; 0 elsewhere."""
    g = np.zeros_like(T)
    g[..., 1:] = (T[..., 1:] - T[..., :-1]) * um[..., 1:]     # grd(i), i = 0..Lm+2 at column i+1
    if lo_copy:
        g[..., 1] = g[..., 2]                                   # FX(istr-1) = FX(istr)
    if hi_copy:
        g[..., Lm + 3] = g[..., Lm + 2]                         # FX(iend+2) = FX(iend+1)
    adv, FX = np.zeros_like(T), np.zeros_like(T)
    c = slice(2, Lm + 3)                                        # faces i = 1..Lm+1
    cm1, cp1 = slice(1, Lm + 2), slice(3, Lm + 4)
    r = slice(2, Mm + 2)                                        # rows j = 1..Mm
    t0, t1, F = T[:, r, c], T[:, r, cm1], Fl[:, r, c]
    e0, e1, e2 = g[:, r, cm1], g[:, r, c], g[:, r, cp1]
    curv_m, curv_0 = e1 - e0, e2 - e1                           # curv(i-1), curv(i)
    FX[:, r, c] = 0.5 * (t0 + t1) * F - C6_UP * (curv_m * _pos(F) + curv_0 * _neg(F))
    g2_0, g2_m = e2 + e1, e1 + e0                               # grd(i) after :629-632, grd(i-1)
    adv[:, r, c] = 0.5 * (t0 + t1 - C6_C4 * (g2_0 - g2_m)) * F
    return adv, FX


def _river_faces(FX, flx, Hz, z_w, riv_vol, riv_trc, itrc, shift, rng):
    """compute_horiz_tracer_fluxes.h:217-246 on the faces of `rng` = (rows, cols); shift: (dj, di) to the cell behind."""
    N = Hz.shape[0]
    rows, cols = rng
    for jj in range(rows.start, rows.stop):
        for ii in range(cols.start, cols.stop):
            f = flx[jj, ii]
            if not abs(f) > RIV_EPS:
                continue
            jb, ib = jj - shift[0], ii - shift[1]
            riv_depth = 0.5 * (z_w[N, jb, ib] - z_w[0, jb, ib] + z_w[N, jj, ii] - z_w[0, jj, ii])
            iriver = _nint(f / 10)
            vel = riv_vol[iriver - 1] * (f - 10 * iriver) / riv_depth
            FX[:, jj, ii] = riv_trc[iriver - 1, itrc - 1] * 0.5 * (Hz[:, jb, ib] + Hz[:, jj, ii]) * vel


def horizontal(t_rhs, FlxU, FlxV, umask, vmask, Lm, Mm, edges, rivers=None, itrc=1, Hz=None, z_w=None,
               edge_rule="intended"):
    """dict(advx, advy, mixx, mixy, FX, FE).  rivers: None or (riv_uflx, riv_vflx, riv_vol, riv_trc(nriv, NT)); it
    needs Hz and z_w."""
    west, east, south, north = edges
    advx, FX = _xi_terms(t_rhs, umask, FlxU, Lm, Mm, west, east)
    sw = lambda a: np.swapaxes(a, -1, -2)
    s_copy, n_copy = (south, north) if edge_rule == "intended" else (north, south)
    advy, FE = _xi_terms(sw(t_rhs), sw(vmask), sw(FlxV), Mm, Lm, s_copy, n_copy)
    advy, FE = np.ascontiguousarray(sw(advy)), np.ascontiguousarray(sw(FE))
    if rivers is not None:
        uf, vf, vol, trc = rivers
        _river_faces(FX, uf, Hz, z_w, vol, np.asarray(trc), itrc, (0, 1), (slice(2, Mm + 2), slice(2, Lm + 3)))
        _river_faces(FE, vf, Hz, z_w, vol, np.asarray(trc), itrc, (1, 0), (slice(2, Mm + 3), slice(2, Lm + 2)))
    return dict(advx=advx, advy=advy, mixx=FX - advx, mixy=FE - advy, FX=FX, FE=FE)


def spline_flux(t_rhs, Hz, We, Lm, Mm):
    """FC(1:N) of compute_vert_tracer_fluxes.h:37-71 (SPLINE_TS, natural b.c.) as N planes, FC(N) = 0, over
    i = 1..Lm, j = 1..Mm; 0 elsewhere."""
    N = t_rhs.shape[0]
    box = (slice(2, Mm + 2), slice(2, Lm + 2))
    t = [None] + [t_rhs[k][box] for k in range(N)]          # t[k], k = 1..N
    H = [None] + [Hz[k][box] for k in range(N)]
    W = [We[k][box] for k in range(N + 1)]                   # We(k), k = 0..N
    FC = [None] * (N + 1)
    CF = [None] * (N + 2)
    CF[1] = np.ones_like(t[1])
    FC[0] = 2.0 * t[1]
    for k in range(1, N):
        cff = 1. / (2. * H[k] + H[k + 1] * (2. - CF[k]))
        CF[k + 1] = cff * H[k]
        FC[k] = cff * (3. * (H[k] * t[k + 1] + H[k + 1] * t[k]) - H[k + 1] * FC[k - 1])
    FC[N] = (2. * t[N] - FC[N - 1]) / (1. - CF[N])
    for k in range(N - 1, -1, -1):
        FC[k] = FC[k] - CF[k + 1] * FC[k + 1]
        FC[k + 1] = FC[k + 1] * W[k + 1]
    FC[N] = np.zeros_like(t[1])
    FC[0] = np.zeros_like(t[1])
    out = np.zeros_like(t_rhs)
    for k in range(1, N + 1):
        out[k - 1][box] = FC[k]
    return out


def vertical(t_rhs, We, Hz, pm, pn, S, t_new, dt, Lm, Mm):
    """dict(advz, mixz, zflx): step3d_t_ISO.F:911-914, 1104-1132.  S: t(nnew) between the horizontal and the vertical
    update (VFlxD's first content); t_new: t(nnew) as the implicit solve leaves it."""
    N = t_rhs.shape[0]
    box = (slice(2, Mm + 2), slice(2, Lm + 2))
    advz = spline_flux(t_rhs, Hz, We, Lm, Mm)
    zflx, mixz = np.zeros_like(t_rhs), np.zeros_like(t_rhs)
    pmn = pm[box] * pn[box]
    z = None
    for k in range(N):
        D = (S[k][box] - Hz[k][box] * t_new[k][box]) / dt
        z = D / pmn if k == 0 else D / pmn + z
        zflx[k][box] = z
        mixz[k][box] = z - advz[k][box]
    return dict(advz=advz, mixz=mixz, zflx=zflx)


def terms(t_rhs, FlxU, FlxV, We, Hz, pm, pn, umask, vmask, S, t_new, dt, ew_periodic, ns_periodic, edges=None,
          rivers=None, itrc=1, z_w=None, edge_rule="intended"):
    """All six terms.  edges: the rank's physical edges (west, east, south, north); None: a single rank, physical
    wherever the direction is not periodic."""
    Mm, Lm = t_rhs.shape[1] - 4, t_rhs.shape[2] - 4
    if edges is None:
        edges = (not ew_periodic, not ew_periodic, not ns_periodic, not ns_periodic)
    edges = (edges[0] and not ew_periodic, edges[1] and not ew_periodic, edges[2] and not ns_periodic,
             edges[3] and not ns_periodic)
    out = horizontal(t_rhs, FlxU, FlxV, umask, vmask, Lm, Mm, edges, rivers, itrc, Hz, z_w, edge_rule)
    out.update(vertical(t_rhs, We, Hz, pm, pn, S, t_new, dt, Lm, Mm))
    return out


def closure_residual(d, t_entry, t_new, Hz, pm, pn, dt, Lm, Mm):
    """(residual, scale) of Hz*t_new = t_entry(nnew) - dt*pm*pn*[di(advx+mixx) + dj(advy+mixy) + dk(advz+mixz)] over
    i = 1..Lm, j = 1..Mm; scale: the largest magnitude among the identity's terms in the cell."""
    r, c = slice(2, Mm + 2), slice(2, Lm + 2)
    fx, fe, fz = d["advx"] + d["mixx"], d["advy"] + d["mixy"], d["advz"] + d["mixz"]
    dx = fx[:, r, 3:Lm + 3] - fx[:, r, c]
    dy = fe[:, 3:Mm + 3, c] - fe[:, r, c]
    dz = fz[:, r, c].copy()
    dz[1:] -= fz[:-1, r, c]
    k = dt * pm[r, c] * pn[r, c]
    lhs = Hz[:, r, c] * t_new[:, r, c]
    res = lhs - (t_entry[:, r, c] - k * (dx + dy + dz))
    parts = [lhs, t_entry[:, r, c], k * fx[:, r, 3:Lm + 3], k * fx[:, r, c], k * fe[:, 3:Mm + 3, c], k * fe[:, r, c],
             k * fz[:, r, c]]
    scale = np.max(np.abs(np.stack(parts)), axis=0)
    return res, scale
