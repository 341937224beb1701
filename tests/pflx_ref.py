"""numpy restatement of the baroclinic pressure fluxes, written from the Fortran: the hydrostatic pressure P of
prsgrd.F:160-226 and calc_pressure_flux of calc_pflx_mod.F:107-168, on arrays in the host layout ((levels,) Mm+4,
Lm+4: index (i, j) at [j+1, i+1]).

Every recurrence and every sum over the levels is an explicit k loop in the reference's order (np.sum adds pairwise:
it is used for neither Uflx nor up); the horizontal directions are whole-array operations, each numpy operation one
rounding, in the reference's operand order.

Ranges, the reference's: p_slow 0..nx x 0..ny, u_slow 1..nx+1 x 1..ny, v_slow 1..nx x 1..ny+1, up and vp 1..nx x 1..ny,
zero elsewhere; nothing is masked; dzt is not formed.  One deviation, shared with the device: P is formed at i = 0
on every rank, the western edge included, where prsgrd leaves it unwritten and calc_pressure_flux reads it
anyway."""
import numpy as np

G, QP2 = 9.81, 0.0000172   # scalars.F: g; eos_vars.F: qp2
TIMESCALE = 86400.0        # calc_pflx.opt


def pressure(s, L, M, rho0, split, tides, g=G, qp2=QP2):
    """P(0:nx, 0:ny, 1:N) of prsgrd.F:160-226 as (N, Mm+4, Lm+4), zero outside."""
    r, c = slice(1, M + 2), slice(1, L + 2)
    zr = s["z_r"][:, r, c]
    N = zr.shape[0]
    zwN = s["z_w"][N][r, c]
    OneFifth, OneTwelfth = 0.2, 1. / 12.
    grho = g / rho0
    HalfGRho = 0.5 * grho
    if split:
        rho1, qp1 = s["rho1"][:, r, c], s["qp1"][:, r, c]
        rho = [None] * (N + 1)
    else:
        rho = [None] + [a for a in s["rho"][:, r, c]]
    Z = lambda k: zr[k - 1]       # level k, 1-based as in the Fortran
    dZ, dR = [None] * (N + 1), [None] * (N + 1)
    for k in range(1, N):
        dZ[k] = Z(k + 1) - Z(k)
        if split:
            dpth = -0.5 * (Z(k + 1) + Z(k))
            dR[k] = rho1[k] - rho1[k - 1] + (qp1[k] - qp1[k - 1]) * dpth * (1. - qp2 * dpth)
        else:
            dR[k] = rho[k + 1] - rho[k]
    dR[N], dR[0], dZ[N], dZ[0] = dR[N - 1], dR[1], dZ[N - 1], dZ[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(N, 0, -1):    # in place: dZ(k-1), dR(k-1) are still the elementary differences
            cff = 2. * dZ[k] * dZ[k - 1]
            dZ[k] = cff / (dZ[k] + dZ[k - 1])
            cfr = 2. * dR[k] * dR[k - 1]
            dR[k] = np.where(cfr > 0., cfr / (dR[k] + dR[k - 1]), 0.)
            if split:
                dpth = -Z(k)
                dR[k] = dR[k] - qp1[k - 1] * dZ[k] * (1. - 2. * qp2 * dpth)
                rho[k] = rho1[k - 1] + qp1[k - 1] * dpth * (1. - qp2 * dpth)
    P = [None] * (N + 1)
    P[N] = g * zwN + grho * (rho[N] + 0.5 * (rho[N] - rho[N - 1]) * (zwN - Z(N)) / (Z(N) - Z(N - 1))) * (zwN - Z(N))
    if tides:
        P[N] = P[N] - g * s["ptide"][r, c]
    for k in range(N - 1, 0, -1):
        P[k] = P[k + 1] + HalfGRho * ((rho[k + 1] + rho[k]) * (Z(k + 1) - Z(k))
                                      - OneFifth * ((dR[k + 1] - dR[k]) * (Z(k + 1) - Z(k)
                                                                           - OneTwelfth * (dZ[k + 1] + dZ[k]))
                                                    - (dZ[k + 1] - dZ[k]) * (rho[k + 1] - rho[k]
                                                                             - OneTwelfth * (dR[k + 1] + dR[k]))))
    out = np.zeros((N, M + 4, L + 4))
    for k in range(1, N + 1):
        out[k - 1][r, c] = P[k]
    return out


def zero_state(N, L, M):
    return {n: np.zeros((N, M + 4, L + 4)) for n in ("u_slow", "v_slow", "p_slow")}


def barotropic(s, L, M):
    """Uflx (1..nx+1 x 1..ny), Vflx (1..nx x 1..ny+1) of calc_pflx_mod.F:111-131 as velocities, (Mm+4, Lm+4)."""
    N = s["Hz"].shape[0]
    zw, pm, pn = s["z_w"], s["pm"], s["pn"]
    ju, iu = slice(2, M + 2), slice(2, L + 3)          # u points
    jv, iv = slice(2, M + 3), slice(2, L + 2)          # v points
    iw = slice(1, L + 2)                               # i-1 of iu
    js = slice(1, M + 2)                               # j-1 of jv
    U = np.zeros((M, L + 1))
    V = np.zeros((M + 1, L))
    for k in range(1, N + 1):                          # sum(.., dim=3): from 0, k = 1..N in turn
        U = U + s["FlxU"][k - 1][ju, iu]
        V = V + s["FlxV"][k - 1][jv, iv]
    U = U * (pn[ju, iu] + pn[ju, iw]) / (zw[N][ju, iu] - zw[0][ju, iu] + zw[N][ju, iw] - zw[0][ju, iw])
    V = V * (pm[jv, iv] + pm[js, iv]) / (zw[N][jv, iv] - zw[0][jv, iv] + zw[N][js, iv] - zw[0][js, iv])
    Uflx, Vflx = np.zeros((M + 4, L + 4)), np.zeros((M + 4, L + 4))
    Uflx[ju, iu], Vflx[jv, iv] = U, V
    return Uflx, Vflx


def flux(s, st, P, L, M, alpha, p_shift=0, top_down=False):
    """One call of calc_pressure_flux(P): advances st (u_slow, v_slow, p_slow, in place) and returns up, vp.
    p_shift, top_down: deliberate mistakes for the tests that show the comparison sees them -- p_fast read p_shift
    cells off in i, up and vp summed k = N..1."""
    beta = 1 - alpha
    N = P.shape[0]
    Uflx, Vflx = barotropic(s, L, M)
    jp, ip = slice(1, M + 2), slice(1, L + 2)          # p_slow 0..nx x 0..ny
    ju, iu = slice(2, M + 2), slice(2, L + 3)
    jv, iv = slice(2, M + 3), slice(2, L + 2)
    j, i = slice(2, M + 2), slice(2, L + 2)            # up, vp 1..nx x 1..ny
    jm, im = slice(1, M + 1), slice(1, L + 1)          # j-1, i-1
    up, vp = np.zeros((M + 4, L + 4)), np.zeros((M + 4, L + 4))
    p_fast, u_fast, v_fast = (np.zeros((M + 4, L + 4)) for _ in range(3))
    terms_u, terms_v = [], []
    for k in range(N):
        st["p_slow"][k][jp, ip] = beta * st["p_slow"][k][jp, ip] + alpha * P[k][jp, ip]
        p_fast[jp, ip] = P[k][jp, ip] - st["p_slow"][k][jp, ip]
        st["u_slow"][k][ju, iu] = beta * st["u_slow"][k][ju, iu] + alpha * (s["u_rhs"][k][ju, iu] - Uflx[ju, iu])
        u_fast[ju, iu] = s["u_rhs"][k][ju, iu] - Uflx[ju, iu] - st["u_slow"][k][ju, iu]
        st["v_slow"][k][jv, iv] = beta * st["v_slow"][k][jv, iv] + alpha * (s["v_rhs"][k][jv, iv] - Vflx[jv, iv])
        v_fast[jv, iv] = s["v_rhs"][k][jv, iv] - Vflx[jv, iv] - st["v_slow"][k][jv, iv]
        pf = np.roll(p_fast, p_shift, axis=1) if p_shift else p_fast
        Hz = s["Hz"][k]
        terms_u.append(u_fast[j, i] * 0.25 * (pf[j, im] + pf[j, i]) * (Hz[j, im] + Hz[j, i]))
        terms_v.append(v_fast[j, i] * 0.25 * (pf[jm, i] + pf[j, i]) * (Hz[jm, i] + Hz[j, i]))
    for k in (range(N - 1, -1, -1) if top_down else range(N)):
        up[j, i] = up[j, i] + terms_u[k]
        vp[j, i] = vp[j, i] + terms_v[k]
    return up, vp


def corrector(s, st, L, M, rho0, split, tides, alpha, **kw):
    """What the corrector's prsgrd adds while calc_pflx is on: P of the state s, then calc_pressure_flux(P)."""
    return flux(s, st, pressure(s, L, M, rho0, split, tides), L, M, alpha, **kw)
