"""A numpy restatement of the momentum budget terms of the corrector: DIAGNOSTICS with diag_uv, the
IMPLICIT_BOTTOM_DRAG branch (prsgrd.F:458-465, compute_horiz_rhs_uv_terms.h:1-36, diagnostics.F:238-439
set_diags_u_4th_adv / set_diags_v_4th_adv, step3d_uv1.F:141-144, 207-216, 282-291, visc3d_S.F:50-131,
step3d_uv2.F:244-278, 400-409).

Pure functions of their arguments.  Arrays are (N, Mm+4, Lm+4) or (Mm+4, Lm+4) in the layout of Model.get: index
[k-1, j+1, i+1] holds (i, j, k); w-point arrays have N+1 planes, plane k at [k].  Every operation is the reference's,
in its order, in float64: the results are meant to be compared bit for bit.  All terms are m2/s2; the u terms live
at i = istrU..Lm, j = 1..Mm, the v terms at i = 1..Lm, j = jstrV..Mm, and are 0 elsewhere (`clip`).

`edges` = (west, east, south, north) says which sides of the rank are physical, non-periodic edges of the whole grid.
There istrU (jstrV) is 2, and there the first and the last advective flux are the second-order form; on a periodic
side or a rank boundary they stay fourth order (the reference tests *_msg_exch instead: on a closed single-rank grid
the two rules coincide).  order4_at_walls=True keeps the fourth-order form everywhere, for the negative control.
"""
import numpy as np

INV24 = 1.0 / 24.0   # diagnostics.F:248


def X(a, di=0, dj=0):
    """a(i+di, j+dj) at (i, j); what wraps around lies outside every range a term is kept on."""
    return np.roll(a, (-dj, -di), axis=(-2, -1))


def f4(a, b, c, d):
    """-a + 7*b - c + 7*d, left to right."""
    return -a + 7.0 * b - c + 7.0 * d


def dxdyi(pm, pn):
    """dxdyi_u, dxdyi_v (diagnostics.F:211-214)."""
    return (0.25 * (X(pn, -1) + pn) * (X(pm, -1) + pm), 0.25 * (X(pn, 0, -1) + pn) * (X(pm, 0, -1) + pm))


def clip(a, comp, Lm, Mm, edges):
    """0 outside the component's range."""
    west, east, south, north = edges
    out = np.zeros_like(a)
    if comp == "u":
        r, c = slice(2, Mm + 2), slice(3 if west else 2, Lm + 2)
    else:
        r, c = slice(3 if south else 2, Mm + 2), slice(2, Lm + 2)
    out[..., r, c] = a[..., r, c]
    return out


def pgr(ru, rv, pm, pn, umask, vmask):
    """prsgrd.F:462-463 over ru, rv as the corrector's prsgrd leaves them."""
    du, dv = dxdyi(pm, pn)
    return ru * du * umask, rv * dv * vmask


def cor(u, v, Hz, fomn, dndx, dmde, pm, pn, uv_cor=True, curv=False):
    """compute_horiz_rhs_uv_terms.h:4-14, 32-33 over u, v(nrhs); curv: CURVGRID && UV_ADV."""
    du, dv = dxdyi(pm, pn)
    if not uv_cor and not curv:
        return np.zeros_like(u), np.zeros_like(v)
    vv, uu = v + X(v, 0, 1), u + X(u, 1)
    if curv:
        ct = 0.5 * (vv * dndx - uu * dmde)
        cff = 0.5 * Hz * (fomn + ct if uv_cor else ct)
    else:
        cff = 0.5 * Hz * fomn
    UFx, VFe = cff * vv, cff * uu
    return 0.5 * (UFx + X(UFx, -1)) * du, -0.5 * (VFe + X(VFe, 0, -1)) * dv


def _vertical(adv, W, q, dxy):
    """adv - dxdyi*(FZ4(k) - FZ4(k-1)) (diagnostics.F:311-335): W(0:N) the face's We+Wi sum, q(1:N) the velocity."""
    N = q.shape[0]
    FZ = np.zeros_like(W)
    for k in range(1, N):   # w-level k between rho levels k and k+1, q(k) at [k-1]
        if k == 1 or k == N - 1:
            FZ[k] = 0.25 * W[k] * (q[k - 1] + q[k])
        else:
            FZ[k] = INV24 * W[k] * f4(q[k - 2], q[k - 1], q[k + 1], q[k])
    out = adv.copy()
    for k in range(1, N + 1):
        out[k - 1] = out[k - 1] - dxy * (FZ[k] - FZ[k - 1])
    return out


def adv_u(u, FlxU, FlxV, We, Wi, pm, pn, Lm, Mm, edges, order4_at_walls=False):
    """set_diags_u_4th_adv over the corrector's FlxU, FlxV, We, Wi and u(nrhs)."""
    west, east, south, north = edges
    du, _ = dxdyi(pm, pn)
    fu, fv = FlxU + X(FlxU, 1), X(FlxV, -1) + FlxV
    FX4 = INV24 * fu * f4(X(u, -1), u, X(u, 2), X(u, 1))                  # east of u(i,j): at rho point i
    FY4 = INV24 * fv * f4(X(u, 0, -2), X(u, 0, -1), X(u, 0, 1), u)        # south of u(i,j)
    if not order4_at_walls:
        x2, y2 = 0.25 * fu * (u + X(u, 1)), 0.25 * fv * (u + X(u, 0, -1))
        for on, col in ((west, 2), (east, Lm + 1)):                        # i = iwest, ieast
            if on:
                FX4[..., col] = x2[..., col]
        for on, row in ((south, 2), (north, Mm + 2)):                      # j = jsouth, jnorth+1
            if on:
                FY4[:, row] = y2[:, row]
    adv = -du * (FX4 - X(FX4, -1) + X(FY4, 0, 1) - FY4)
    return _vertical(adv, X(We, -1) + We + X(Wi, -1) + Wi, u, du)


def adv_v(v, FlxU, FlxV, We, Wi, pm, pn, Lm, Mm, edges, order4_at_walls=False):
    """set_diags_v_4th_adv."""
    west, east, south, north = edges
    _, dv = dxdyi(pm, pn)
    fu, fv = X(FlxU, 0, -1) + FlxU, FlxV + X(FlxV, 0, 1)
    FX4 = INV24 * fu * f4(X(v, -2), X(v, -1), X(v, 1), v)                  # west of v(i,j)
    FY4 = INV24 * fv * f4(X(v, 0, -1), v, X(v, 0, 2), X(v, 0, 1))          # north of v(i,j): at rho point j
    if not order4_at_walls:
        x2, y2 = 0.25 * fu * (X(v, -1) + v), 0.25 * fv * (v + X(v, 0, 1))
        for on, col in ((west, 2), (east, Lm + 2)):                        # i = iwest, ieast+1
            if on:
                FX4[..., col] = x2[..., col]
        for on, row in ((south, 2), (north, Mm + 1)):                      # j = jsouth, jnorth
            if on:
                FY4[:, row] = y2[:, row]
    adv = -dv * (X(FX4, 1) - FX4 + FY4 - X(FY4, 0, -1))
    return _vertical(adv, X(We, 0, -1) + X(Wi, 0, -1) + We + Wi, v, dv)


def dis(r_fin, dxy, mask, p, c, a):
    """step3d_uv1.F:211-214: r_fin the final right-hand side."""
    return r_fin * dxy * mask - p - c - a


def vmx(q_new, q_prev, r_fin, dxy, dt):
    """step3d_uv1.F:215-216: q_new the Hz*u the implicit solve leaves, q_prev u(nnew) on entry."""
    return (q_new - q_prev) / dt - r_fin * dxy


def hmx(u, v, Hz, pm, pn, dm_r, dn_r, dm_p, dn_p, visc2_r, visc2_p, pmask):
    """visc3d_S.F:55-91, 122-127 over u, v(nstp)."""
    du, dv = dxdyi(pm, pn)
    cff = 0.5 * Hz * visc2_r * (dn_r * pm * ((pn + X(pn, 1)) * X(u, 1) - (X(pn, -1) + pn) * u)
                                - dm_r * pn * ((pm + X(pm, 0, 1)) * X(v, 0, 1) - (X(pm, 0, -1) + pm) * v))
    UFx, VFe = cff * dn_r * dn_r, -cff * dm_r * dm_r
    cff = 0.125 * (X(Hz, -1) + Hz + X(Hz, -1, -1) + X(Hz, 0, -1)) * visc2_p * (
        0.25 * (X(pm, -1) + pm + X(pm, -1, -1) + X(pm, 0, -1)) * dn_p
        * ((X(pn, 0, -1) + pn) * v - (X(pn, -1, -1) + X(pn, -1)) * X(v, -1))
        + 0.25 * (X(pn, -1) + pn + X(pn, -1, -1) + X(pn, 0, -1)) * dm_p
        * ((X(pm, -1) + pm) * u - (X(pm, -1, -1) + X(pm, 0, -1)) * X(u, 0, -1))) * pmask
    UFe, VFx = cff * dm_p * dm_p, cff * dn_p * dn_p
    hu = 0.5 * du * ((X(pn, -1) + pn) * (UFx - X(UFx, -1)) + (X(pm, -1) + pm) * (X(UFe, 0, 1) - UFe))
    hv = 0.5 * dv * ((X(pn, 0, -1) + pn) * (X(VFx, 1) - VFx) + (X(pm, 0, -1) + pm) * (VFe - X(VFe, 0, -1)))
    return hu, hv


def cpl(q_in, Hz, dn, avg1, mask, dt, comp, neighbour=-1):
    """step3d_uv2.F:244-278 (400-409 for v): q_in u(nnew) entering step3d_uv2, Hz the one it sees; dn: dn_u (dm_v),
    avg1: DU_avg1 (DV_avg1).  neighbour=+1 takes the Hz pair of the wrong side, for the negative control."""
    N = q_in.shape[0]
    Hm = X(Hz, neighbour, 0) if comp == "u" else X(Hz, 0, neighbour)
    CF = 0.5 * (Hz[N - 1] + Hm[N - 1])
    DC = q_in[N - 1].copy()
    for k in range(N - 1, 0, -1):
        CF = CF + 0.5 * (Hz[k - 1] + Hm[k - 1])
        DC = DC + q_in[k - 1]
    with np.errstate(all="ignore"):
        DC0 = (DC * dn - avg1) / (CF * dn)
    return -DC0 * mask * 0.5 * (Hz + Hm) / dt


TERMS = ("pgr", "cor", "adv", "dis", "hmx", "vmx", "cpl")   # ipgr .. icoup, diagnostics.F:56-63


def terms(s, Lm, Mm, edges, dt, uv_cor=True, curv=False, uv_vis2=True, order4_at_walls=False):
    """All 14 terms as {"u": {term: array}, "v": {...}}, clipped to their ranges.  s: dict of
      u_rhs, v_rhs, u_stp, v_stp   u, v(nrhs) and u, v(nstp) of the corrector
      FlxU, FlxV, We, Wi, Hz       the corrector's (Hz as step3d_uv1 and visc3d see it)
      ru_pgr, rv_pgr               ru, rv after prsgrd
      ru_fin, rv_fin               the final right-hand side of step3d_uv1
      u_prev, v_prev               u, v(nnew) entering step3d_uv1
      u_uv1, v_uv1                 u, v(nnew) leaving step3d_uv1
      u_in2, v_in2, Hz2            u, v(nnew) entering step3d_uv2 and the Hz it sees
      DU_avg1, DV_avg1, pm, pn, fomn, dndx, dmde, umask, vmask, pmask, dm_r, dn_r, dm_p, dn_p, dn_u, dm_v,
      visc2_r, visc2_p             (Mm+4, Lm+4)"""
    pm, pn = s["pm"], s["pn"]
    du, dv = dxdyi(pm, pn)
    out = {"u": {}, "v": {}}
    out["u"]["pgr"], out["v"]["pgr"] = pgr(s["ru_pgr"], s["rv_pgr"], pm, pn, s["umask"], s["vmask"])
    out["u"]["cor"], out["v"]["cor"] = cor(s["u_rhs"], s["v_rhs"], s["Hz"], s["fomn"], s["dndx"], s["dmde"], pm, pn,
                                           uv_cor, curv)
    out["u"]["adv"] = adv_u(s["u_rhs"], s["FlxU"], s["FlxV"], s["We"], s["Wi"], pm, pn, Lm, Mm, edges, order4_at_walls)
    out["v"]["adv"] = adv_v(s["v_rhs"], s["FlxU"], s["FlxV"], s["We"], s["Wi"], pm, pn, Lm, Mm, edges, order4_at_walls)
    for c, d, m in (("u", du, s["umask"]), ("v", dv, s["vmask"])):
        o = out[c]
        o["dis"] = dis(s["r%s_fin" % c], d, m, o["pgr"], o["cor"], o["adv"])
        o["vmx"] = vmx(s["%s_uv1" % c], s["%s_prev" % c], s["r%s_fin" % c], d, dt)
    if uv_vis2:
        out["u"]["hmx"], out["v"]["hmx"] = hmx(s["u_stp"], s["v_stp"], s["Hz"], pm, pn, s["dm_r"], s["dn_r"], s["dm_p"],
                                               s["dn_p"], s["visc2_r"], s["visc2_p"], s["pmask"])
    else:
        out["u"]["hmx"], out["v"]["hmx"] = np.zeros_like(s["Hz"]), np.zeros_like(s["Hz"])
    out["u"]["cpl"] = cpl(s["u_in2"], s["Hz2"], s["dn_u"], s["DU_avg1"], s["umask"], dt, "u")
    out["v"]["cpl"] = cpl(s["v_in2"], s["Hz2"], s["dm_v"], s["DV_avg1"], s["vmask"], dt, "v")
    return {c: {k: clip(out[c][k], c, Lm, Mm, edges) for k in TERMS} for c in ("u", "v")}


def closure_residual(t, q_prev, q_final, Hz2, dt, comp):
    """(Hz_u*u_final - (u_prev + dt*sum of the seven terms), largest |term|*dt or |u_prev| per point): q_final the
    u(nnew) step3d_uv2's coupling leaves, Hz2 the Hz it sees."""
    Hm = X(Hz2, -1, 0) if comp == "u" else X(Hz2, 0, -1)
    total = t["pgr"] + t["cor"] + t["adv"] + t["dis"] + t["vmx"] + t["hmx"] + t["cpl"]
    res = 0.5 * (Hz2 + Hm) * q_final - (q_prev + dt * total)
    scale = np.abs(q_prev)
    for k in TERMS:
        scale = np.maximum(scale, np.abs(t[k]) * dt)
    return res, scale
