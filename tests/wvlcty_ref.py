"""wvlcty_tile (wvlcty.F:18-192) restated in numpy: the true vertical velocity
w at rho points, the expected value of every test of the device kernel.

Arrays are the (levels, Mm+4, Lm+4) C views Model.get returns of the
reference's (-1:Lm+2, -1:Mm+2, levels) arrays: cell (i, j) is [.., j+1, i+1].
Every statement keeps the reference's operand order (numpy evaluates left to
right and never contracts a*b+c), so results are compared bit for bit.
tests/test_wvlcty_ref.py pins this file to the reference's own routine through
tests/golden/wvlcty_golden.npz.
"""
import numpy as np


def ranges(Lm, Mm, ew_periodic, ns_periodic):
    """imin, imax, jmin, jmax of a rank that owns the whole grid (wvlcty.F:46-59): istr..iend, one row more on
    each side in a periodic direction only (there istrR = istr-2, so max(istrR, istr-1) = istr-1)."""
    return ((0, Lm + 1) if ew_periodic else (1, Lm)) + ((0, Mm + 1) if ns_periodic else (1, Mm))


def wvlcty(FlxU, FlxV, u, v, z_r, pm, pn, ew_periodic, ns_periodic, out=None, edges=None, rng=None):
    """u, v: the (N, ..) slot nstp.  out: the (N, Mm+4, Lm+4) array written into (zeros by default); cells outside
    the computed range and its copies keep what they held.  edges: (west, east, south, north) physical edges of
    the rank (default: every side of a direction that is not periodic); rng: (imin, imax, jmin, jmax) of a rank
    that owns a part of the grid (default: ranges())."""
    N, M4, L4 = FlxU.shape
    Lm, Mm = L4 - 4, M4 - 4
    if N < 2:
        raise ValueError("wvlcty: N < 2 has no defined formula")
    imin, imax, jmin, jmax = rng or ranges(Lm, Mm, ew_periodic, ns_periodic)
    if edges is None:
        edges = (not ew_periodic, not ew_periodic, not ns_periodic, not ns_periodic)
    west, east, south, north = edges
    w = np.zeros((N, M4, L4)) if out is None else out

    def at(a, di=0, dj=0):   # a(i+di, j+dj [, k]) over imin..imax, jmin..jmax
        return a[..., jmin + 1 + dj:jmax + 2 + dj, imin + 1 + di:imax + 2 + di]

    # Wrk(0) = 0; Wrk(k) = Wrk(k-1) - pm*pn*(FlxU(i+1)-FlxU(i)+FlxV(j+1)-FlxV(j))
    mn = at(pm) * at(pn)
    Wrk = [np.zeros_like(mn)]
    for k in range(1, N + 1):
        Wrk.append(Wrk[k - 1] - mn * (at(FlxU[k - 1], 1, 0) - at(FlxU[k - 1]) + at(FlxV[k - 1], 0, 1) - at(FlxV[k - 1])))
    W = [None] * (N + 1)
    W[N] = +0.375 * Wrk[N] + 0.75 * Wrk[N - 1] - 0.125 * Wrk[N - 2]
    for k in range(N - 1, 1, -1):
        W[k] = +0.5625 * (Wrk[k] + Wrk[k - 1]) - 0.0625 * (Wrk[k + 1] + Wrk[k - 2])
    W[1] = -0.125 * Wrk[2] + 0.75 * Wrk[1] + 0.375 * Wrk[0]
    # the motion along s-surfaces: Wxi at u points imin..imax+1, Weta at v points jmin..jmax+1
    for k in range(1, N + 1):
        uk, vk, zk = u[k - 1], v[k - 1], z_r[k - 1]
        Wxi0 = at(uk) * (at(zk) - at(zk, -1, 0)) * (at(pm) + at(pm, -1, 0))
        Wxi1 = at(uk, 1, 0) * (at(zk, 1, 0) - at(zk)) * (at(pm, 1, 0) + at(pm))
        Weta0 = at(vk) * (at(zk) - at(zk, 0, -1)) * (at(pn) + at(pn, 0, -1))
        Weta1 = at(vk, 0, 1) * (at(zk, 0, 1) - at(zk)) * (at(pn, 0, 1) + at(pn))
        at(w[k - 1])[...] = W[k] + 0.25 * (Wxi0 + Wxi1 + Weta0 + Weta1)
    # gradient boundary copies (wvlcty.F:138-191): physical edges of non-periodic directions only
    J, I = slice(jmin + 1, jmax + 2), slice(imin + 1, imax + 2)
    if not ew_periodic:
        if west:
            w[:, J, imin] = w[:, J, imin + 1]
        if east:
            w[:, J, imax + 2] = w[:, J, imax + 1]
    if not ns_periodic:
        if south:
            w[:, jmin, I] = w[:, jmin + 1, I]
        if north:
            w[:, jmax + 2, I] = w[:, jmax + 1, I]
        if not ew_periodic:
            if west and south:
                w[:, jmin, imin] = w[:, jmin + 1, imin + 1]
            if west and north:
                w[:, jmax + 2, imin] = w[:, jmax + 1, imin + 1]
            if east and south:
                w[:, jmin, imax + 2] = w[:, jmin + 1, imax + 1]
            if east and north:
                w[:, jmax + 2, imax + 2] = w[:, jmax + 1, imax + 1]
    return w


def of_model(m, per, slot="nstp"):
    """The restatement over the arrays Model.get downloads from a single-rank model after a step; per: the case is
    doubly periodic (Filament), else closed on every side (the basin)."""
    N = m.N
    s = m.t.nstp if slot == "nstp" else m.t.nnew
    return wvlcty(m.get("FlxU"), m.get("FlxV"), m.get("u")[(s - 1) * N:s * N], m.get("v")[(s - 1) * N:s * N],
                  m.get("z_r"), m.get("pm")[0], m.get("pn")[0], per, per)
