"""States that take the data-dependent branches of the hot path.

The per-routine GPU tests feed the kernels mid-run states of the analytic
cases; on those states several branches that depend on the data run in one
arm only ("Branch coverage").  Each builder below makes,
from the CPU oracle alone, a state whose data reach the other arms, and
returns (cfg, oracle, time indices) with the indices already set in the
oracle.  Beside each builder stands a short numpy restatement of the branch
condition from the routine's inputs, which tests/test_branch_states.py uses
to assert what share of the points runs each arm (and, where the restatement
also yields the output, to check the oracle's own lines a second time).
tests/test_gpu_branches.py runs the HIP kernels on the same states.

  omega_state    omega.F's Courant split: cw < cw_min, cw < cutoff*cw_max, the
                 rest, and cw_max <= 0 (We = 0), reached by scaling the
                 horizontal fluxes column by column over 4.5 decades
  drag_state     linear bottom drag (Zob = 0) with rdrg inside the range of
                 the 0.8*Hz/dt clamp
  flather_state  Flather's correction for cx > 1 - 1/sqrt(2): a mid-run
                 state of the open basin handed to a model with ndtfast = 4
                 (whole runs at that ndtfast blow up), on 2.3 km curvilinear
                 cells so that every edge has points on both sides
  cext_state     boundary data of both signs on every side of u3dbc / v3dbc
  twin_state     a perturbed twin of flather_state for any set of open sides
                 and any small size: noise on every time level, land on one
                 cell of every edge, boundary velocities of both signs; with
                 it the restatements of every data-dependent arm of the
                 boundary routines (normal_arms, tangential_arms, tracer_arms,
                 mask_arms, ub_arms) that tests/test_ref_pin_obc.py (against
                 the reference) and tests/test_gpu_open_sides.py (the HIP
                 kernels) assert before they compare
  kpp_eos_state  KPP over the linear EOS, and over the split EOS without
                 salinity
  kpp_top_state  surface heating and weak wind: the boundary layer ends
                 inside the top cell
  kpp_swr_state  well-mixed columns under cooling and wind: the boundary
                 layer reaches levels where swr_frac is exactly zero
  bulk_state     the bulk fluxes under the analytic atmosphere and under one
                 that reaches the other arms of calc_all_bulk_forces: stable
                 and unstable air, calm, every Charnock range, no rain, a
                 coast, water at and below the -1.8 degC of SEA_ICE_NOFLUX
"""
import functools

import numpy as np

import oracle
import romsgpu
from test_gpu_obc import obc_cfg
from test_gpu_parity import basin_cfg

G = 9.81
K_FL = 0.292893218813452      # u2dbc_im.F:36, 1 - 1/sqrt(2)
FLUX_DECADES = 4.5            # omega_state: 10**(FLUX_DECADES*rand) per column


def _started(cfg, steps=3):
    o = oracle.Oracle(cfg)
    o.init()
    o.step(steps)
    return o


def set_mode(o, mode):
    """Predictor (nrhs = nstp, nnew = 3) or corrector (nrhs = 3, nnew = 3 - nstp) indices."""
    iic, kstp, knew, nstp = o.tindex()[:4]
    tix = [iic, kstp, knew, nstp, 3, 3 - nstp] if mode == "corr" else [iic, kstp, knew, nstp, nstp, 3]
    o.set_tindex(tix)
    return tix


def box(cfg):
    """Index of the interior points (1..Lm, 1..Mm) of a (.., Mm+4, Lm+4) array."""
    return (Ellipsis, slice(2, cfg.MMm + 2), slice(2, cfg.LLm + 2))


def kpp_cfg(LLm, MMm, N, nonlin=True, NT=2, salinity=1):
    """The closed basin with KPP and surface fluxes on 2 km cells (the depth
    and width sweeps' case)."""
    c = basin_cfg(nonlin=nonlin, LLm=LLm, MMm=MMm, N=N, NT=NT, sizex=2.0e3 * LLm, sizey=2.0e3 * MMm)
    c.salinity = salinity
    c.lmd, c.surf_flux = oracle.LMD_ALL, 1
    return c


# ---------------------------------------------------------------- omega ----
def omega_state(LLm, MMm, N, decades=FLUX_DECADES):
    cfg = kpp_cfg(LLm, MMm, N)
    o = _started(cfg)
    rng = np.random.default_rng(5)
    for name in ("FlxU", "FlxV"):
        f = o.field(name)
        f *= 10.0 ** (decades * rng.random(f.shape[1:]))[None] * (1.0 + 0.5 * rng.standard_normal(f.shape))
    return cfg, o, set_mode(o, "pred")


def omega_split(o, cfg, tix):
    """omega.F:60-160 from FlxU, FlxV, Hz, z_w, swflx and the metrics, in the
    reference's operation order: (We, Wi, regime) on the interior, regime
    1..4 at the w-points k = 1..N-1 (0 at k = 0 and N)."""
    N, I = cfg.N, box(cfg)
    IX, JX = (Ellipsis, I[1], slice(3, cfg.LLm + 3)), (Ellipsis, slice(3, cfg.MMm + 3), I[2])
    FU, FV, Hz, zw = o.field("FlxU"), o.field("FlxV"), o.field("Hz"), o.field("z_w")
    dtau = cfg.dt if tix[4] == 3 else 0.6 * cfg.dt     # iic is past forw_start
    pos, neg = lambda x: np.maximum(x, 0.0), lambda x: np.minimum(x, 0.0)
    W, CX = np.zeros((N + 1,) + zw[0][I].shape), np.zeros((N + 2,) + zw[0][I].shape)
    for k in range(1, N + 1):
        W[k] = W[k - 1] - FU[k - 1][IX] + FU[k - 1][I] - FV[k - 1][JX] + FV[k - 1][I]
        CX[k] = pos(FU[k - 1][IX]) - neg(FU[k - 1][I]) + pos(FV[k - 1][JX]) - neg(FV[k - 1][I])
    W[N] = W[N] + o.field("swflx")[0][I] * o.field("dm_r")[0][I] * o.field("dn_r")[0][I]
    wrk = W[N] / (zw[N][I] - zw[0][I])
    cx0 = dtau * o.field("pm")[0][I] * o.field("pn")[0][I]
    We, Wi, reg = np.zeros_like(W), np.zeros_like(W), np.zeros(W.shape, dtype=int)
    for k in range(N - 1, 0, -1):
        w = W[k] - wrk * (zw[k][I] - zw[0][I])
        cw_max = 1.0 * np.minimum(Hz[k - 1][I], Hz[k][I]) - np.maximum(CX[k], CX[k + 1]) * cx0
        cw, cw_min = np.abs(w) * cx0, cw_max * 0.6
        r = np.where(cw_max <= 0.0, 4, np.where(cw < cw_min, 1, np.where(cw < 1.4 * cw_max, 2, 3)))
        with np.errstate(all="ignore"):
            cff = np.where(r == 1, cw_max * cw_max,
                           np.where(r == 2, cw_max * cw_max + 0.625 * ((cw - cw_min) * (cw - cw_min)), cw_max * cw))
            we = np.where(r == 4, 0.0, cw_max * cw_max * w / cff)
        We[k], Wi[k], reg[k] = we, np.where(r == 4, w, w - we), r
    return We, Wi, reg


# ----------------------------------------------------------- linear drag ----
RDRG = 2.5   # [m/s]; 0.8*Hz(k=1)/dt spans 0.35 .. 9.7 on this basin at dt = 60 s


def drag_state():
    cfg = basin_cfg(nonlin=True)
    cfg.Zob, cfg.rdrg = 0.0, RDRG
    o = _started(cfg)
    return cfg, o, set_mode(o, "pred")


def drag_clamp(o, cfg):
    """compute_rd_bott_drag.h without Zob: (r_D, clamp binds) on the interior."""
    lim = 0.8 * o.field("Hz")[0][box(cfg)] / cfg.dt
    return np.minimum(cfg.rdrg, lim), lim < cfg.rdrg


# --------------------------------------------------------------- Flather ----
FLATHER_NDTFAST = 4
FLATHER_CELL = 2.3e3


def flather_cfg(obc, ndtfast=FLATHER_NDTFAST, LLm=48, MMm=40, N=12):
    return obc_cfg(obc=obc, curv=1, ndtfast=ndtfast, LLm=LLm, MMm=MMm, N=N, sizex=FLATHER_CELL * LLm,
                   sizey=FLATHER_CELL * MMm)


def flather_state(obc, **size):
    """Three steps at ndtfast = 30, then every field handed to a model of the
    same grid with ndtfast = 4: one state for single step2d calls, not a run.
    The indices returned are those after the three steps; step2d's callers
    advance kstp / knew themselves (fast_indices).  size: LLm, MMm, N other
    than 48 x 40 x 12, the cells staying 2.3 km."""
    donor = _started(flather_cfg(obc, ndtfast=30, **size))
    cfg = flather_cfg(obc, **size)
    o = oracle.Oracle(cfg)
    o.init()
    for name in romsgpu.FIELDS:
        o.field(name)[...] = donor.field(name)
    tix = donor.tindex()
    o.set_tindex(tix)
    return cfg, o, tix


def fast_indices(tix, iif):
    """Indices of fast step iif = 1, 2, .. after the state's (step2d_FB.F's kstp / knew rotation)."""
    iic, kstp, knew, nstp = tix[:4]
    for _ in range(iif):
        kstp, knew = knew, knew % 4 + 1
    return [iic, kstp, knew, nstp, 3, 3 - nstp]


def flather_cx(o, cfg):
    """cx of u2dbc / v2dbc (u2dbc_im.F:31-34) along each open side."""
    L, M = cfg.LLm, cfg.MMm
    h, pm, pn = o.field("h")[0], o.field("pm")[0], o.field("pn")[0]
    dtf = cfg.dt / cfg.ndtfast

    def cx(a, b, p):
        cff = 0.5 * (h[a] + h[b])
        return dtf * cff * np.sqrt(G / cff) * 0.5 * (p[a] + p[b])

    js, is_ = slice(2, M + 2), slice(2, L + 2)
    sides = {"west": (1, cx((js, 1), (js, 2), pm)), "east": (2, cx((js, L + 1), (js, L + 2), pm)),
             "south": (4, cx((1, is_), (2, is_), pn)), "north": (8, cx((M + 1, is_), (M + 2, is_), pn))}
    return {s: c for s, (bit, c) in sides.items() if cfg.obc & bit}


# ------------------------------------------------------------------ cext ----
CEXT_FIELDS = {"west": "u_west", "east": "u_east", "south": "v_south", "north": "v_north"}


def cext_state(mode, obc=15):
    """The open basin after three steps with a sign-changing wave added to the
    normal-velocity boundary data of every side (amplitude twice the data's)."""
    cfg = obc_cfg(obc=obc)
    o = _started(cfg)
    for q, name in enumerate(CEXT_FIELDS.values()):
        a = o.field(name).reshape(cfg.N, -1)
        m, k = np.arange(a.shape[1])[None, :], np.arange(cfg.N)[:, None]
        a += 2.0 * np.abs(a).max() * np.sin(2.0 * np.pi * 3.0 * m / a.shape[1] + 0.4 * k + q)
    return cfg, o, set_mode(o, mode)


def cext_arms(o, cfg, tix):
    """Per side, over the edge's normal-velocity points: the shares whose
    boundary data flow in / out (the test of u3dbc_im.F:96-97 and its three
    twins), and the shares that ran either arm, i.e. where the Orlanski
    inflow flag cx < 0 (u3dbc_im.F:80-92) was also set.  Call after the
    routine: the flag needs the interior u, v (nnew) it has just formed."""
    N, L, M = cfg.N, cfg.LLm, cfg.MMm
    nstp, nnew = tix[3], tix[5]
    lev = lambda a, l: a[(l - 1) * N:l * N]
    u, v = o.field("u"), o.field("v")
    js, is_ = slice(2, M + 2), slice(2, L + 2)
    pick = {"west": (u, (js, 3), (js, 4), 1.0), "east": (u, (js, L + 1), (js, L), -1.0),
            "south": (v, (3, is_), (4, is_), 1.0), "north": (v, (M + 1, is_), (M, is_), -1.0)}
    out = {}
    for side, (a, i1, i2, sgn) in pick.items():
        i1, i2 = (Ellipsis,) + i1, (Ellipsis,) + i2
        dft = lev(a, nstp)[i1] - lev(a, nnew)[i1]
        dfx = lev(a, nnew)[i1] - lev(a, nnew)[i2]
        inflow = dft * dfx < 0.0
        data_in = sgn * o.field(CEXT_FIELDS[side]).reshape(N, -1)[:, 1:-1] > 0.0
        out[side] = {"data in": data_in.mean(), "data out": (~data_in).mean(),
                     "ran bry arm": (inflow & data_in).mean(), "ran ubind arm": (inflow & ~data_in).mean()}
    return out


# ------------------------------------------------------------------ twin ----
SIDES = ("west", "east", "south", "north")
OPEN = {"west": 1, "east": 2, "south": 4, "north": 8}
TWIN_SIZE = dict(LLm=24, MMm=20, N=6)        # the grid of the reference libraries (oracle/ref/build_ref.sh)
TWIN_STATE = ("zeta", "ubar", "vbar", "u", "v", "t")
TWIN_MASKS = ("rmask", "umask", "vmask", "pmask")
TWIN_BRY = ["%s_%s" % (v, e) for v in TWIN_STATE for e in SIDES]
EPS = 1.0e-33


def twin_land(LLm, MMm):
    """One land cell on every edge, with its ghost neighbour: (i, j) in Fortran indices."""
    return {"west": [(0, 7), (1, 7)], "east": [(LLm, 11), (LLm + 1, 11)], "south": [(9, 0), (9, 1)],
            "north": [(15, MMm), (15, MMm + 1)]}


def open_sides(cfg):
    return [s for s, bit in OPEN.items() if cfg.obc & bit]


def ub_arrays(cfg):
    """Binding coefficients below 0, inside (0, 1) and above 1 on every edge, on the points 0:Mm+1 / 0:Lm+1."""
    x = lambda n, ph: 0.5 + 1.5 * np.sin(np.arange(n) * 0.37 + ph)
    return [x(cfg.MMm + 2, 0.0), x(cfg.MMm + 2, 1.0), x(cfg.LLm + 2, 2.0), x(cfg.LLm + 2, 3.0)]


def lev(a, l, N):
    return a[(l - 1) * N:l * N]


def line(a, normal, c, m):
    """a (.., Mm+4, Lm+4) on the line of normal index c ('x': i = c, 'y': j = c) at the along-edge indices m."""
    return a[..., m + 1, c + 1] if normal == "x" else a[..., c + 1, m + 1]


def build_twin(obc, LLm=TWIN_SIZE["LLm"], MMm=TWIN_SIZE["MMm"], N=TWIN_SIZE["N"]):
    """(cfg, oracle, time indices, snapshot of every array the boundary routines touch) for the open sides obc.
    flather_state at this size with seeded noise of the fields' own size on every time level, an offset on
    u and v that differs between the time levels, land on one cell of every edge and a sign-changing wave
    on the boundary velocities.  The snapshot is never written; callers restore the oracle from it."""
    cfg, o, tix = flather_state(obc, LLm=LLm, MMm=MMm, N=N)
    rng = np.random.default_rng(100 + obc)
    for name in TWIN_STATE:
        a = o.field(name)
        amp = max(float(np.abs(a).max()), 0.05) * (0.1 if name == "t" else 1.0)
        a += amp * rng.standard_normal(a.shape)
        if name in ("u", "v"):
            # a smooth offset that differs between the time levels: along every edge the change in time
            # outweighs the gradients in places and not in others, so the cy clamp binds at both ends
            J, I = np.meshgrid(np.arange(a.shape[-2]), np.arange(a.shape[-1]), indexing="ij")
            for l in range(3):
                lev(a, l + 1, cfg.N)[...] += 2.0 * amp * np.cos(2.1 * l + 0.15 * J + 0.1 * I)
    rm = o.field("rmask")[0]
    for side in twin_land(LLm, MMm).values():
        for i, j in side:
            rm[j + 1, i + 1] = 0.0
    um, vm, pm_ = o.field("umask")[0], o.field("vmask")[0], o.field("pmask")[0]
    um[:, 1:] = rm[:, 1:] * rm[:, :-1]
    vm[1:, :] = rm[1:, :] * rm[:-1, :]
    pm_[1:, 1:] = rm[1:, 1:] * rm[1:, :-1] * rm[:-1, 1:] * rm[:-1, :-1]
    for name, m in (("zeta", rm), ("ubar", um), ("vbar", vm), ("u", um), ("v", vm), ("t", rm)):
        o.field(name)[...] *= m
    for q, side in enumerate(SIDES):                # boundary velocities of both signs, as cext_state
        for comp in ("u", "v"):
            a = o.field("%s_%s" % (comp, side)).reshape(cfg.N, -1)
            m, k = np.arange(a.shape[1])[None, :], np.arange(cfg.N)[:, None]
            a += 2.0 * max(float(np.abs(a).max()), 0.01) * np.sin(2.0 * np.pi * 3.0 * m / a.shape[1] + 0.4 * k + q)
    snap = {n: o.field(n).copy() for n in TWIN_STATE + TWIN_MASKS + tuple(TWIN_BRY) + ("h", "pm", "pn")}
    for a in snap.values():
        a.setflags(write=False)
    return cfg, o, tix, snap


twin_state = functools.lru_cache(maxsize=None)(build_twin)      # one oracle per (obc, size), shared: restore before use


def twin_restore(o, snap):
    for n, a in snap.items():
        o.field(n)[...] = a


def all_taken(arms, where):
    missing = [(where, k) for k, v in arms.items() if not bool(np.any(v))]
    assert not missing, missing


# The arm restatements read a dict S: the arrays handed to the routine under their field names, and
# cfg, tix (iic, kstp, knew, nstp, nrhs, nnew) and ub (ub_arrays, or None for ub_tune off).
def mask_arms(S, name, normal, c, m):
    w = line(S[name][0], normal, c, m)
    return {"wet edge point": w == 1.0, "dry edge point": w == 0.0}


def ub_arms(S, side, m):
    if S["ub"] is None:
        return {}
    b = S["ub"][SIDES.index(side)][m]
    return {"ub < 0": b < 0.0, "0 < ub < 1": (b > 0.0) & (b < 1.0), "ub > 1": b > 1.0}


def normal_arms(S, comp, side):
    """Orlanski radiation of the normal component (u on west / east, v on south / north)."""
    cfg, N = S["cfg"], S["cfg"].N
    nstp, nnew = S["tix"][3], S["tix"][5]
    normal, nal, nmax = ("x", cfg.MMm, cfg.LLm) if comp == "u" else ("y", cfg.LLm, cfg.MMm)
    low = side in ("west", "south")
    b, i1, i2 = (1, 2, 3) if low else (nmax + 1, nmax, nmax - 1)
    m, m1 = np.arange(1, nal + 1), np.arange(1, nal + 2)
    old, new = lev(S[comp], nstp, N), lev(S[comp], nnew, N)
    gi = (line(old, normal, i1, m1) - line(old, normal, i1, m1 - 1)) * line(S["pmask"][0], normal, i1, m1)
    dft = line(old, normal, i1, m) - line(new, normal, i1, m)
    dfx = line(new, normal, i1, m) - line(new, normal, i2, m)
    first = dft * (gi[:, :-1] + gi[:, 1:]) > 0.0
    dfy = np.where(first, gi[:, :-1], gi[:, 1:])
    cff = np.maximum(dfx * dfx + dfy * dfy, EPS)
    raw = dft * dfy
    inflow = dft * dfx < 0.0
    data = S["%s_%s" % (comp, side)].reshape(N, -1)[:, 1:-1]
    data_in = data > 0.0 if low else data < 0.0
    arms = {"outflow": ~inflow, "inflow, boundary data bind": inflow & data_in, "inflow, ubind binds": inflow & ~data_in,
            "first tangential gradient": first, "second tangential gradient": ~first,
            "cy clamped at +cff": ~inflow & (raw > cff), "cy clamped at -cff": ~inflow & (raw < -cff),
            "cy inside": ~inflow & (np.abs(raw) <= cff)}
    arms.update(mask_arms(S, comp + "mask", normal, b, m))
    arms.update(ub_arms(S, side, m))
    return arms


def tangential_arms(S, comp, side, fast=False):
    """The tangential component (u on south / north, v on west / east): radiates for cx > 0, binds otherwise."""
    cfg, N = S["cfg"], S["cfg"].N
    normal, nal, nmax = ("y", cfg.LLm, cfg.MMm) if comp == "u" else ("x", cfg.MMm, cfg.LLm)
    other = "v" if comp == "u" else "u"
    low = side in ("west", "south")
    m = np.arange(2, nal + 1)
    if fast:
        vel = S[other + "bar"][S["tix"][1] - 1]
    else:
        vel = lev(S[other], S["tix"][4], N)
    c = 1 if low else nmax + 1
    s = line(vel, normal, c, m) + line(vel, normal, c, m - 1)
    cx_pos = (-s if low else s) > 0.0
    arms = {"radiates (cx > 0)": cx_pos, "binds (cx <= 0)": ~cx_pos}
    arms.update(mask_arms(S, comp + "mask", normal, 0 if low else nmax + 1, m))
    if not fast:
        arms.update(ub_arms(S, side, m))
    return arms


def tracer_arms(S, side):
    cfg, N = S["cfg"], S["cfg"].N
    normal, nal, nmax = ("x", cfg.MMm, cfg.LLm) if side in ("west", "east") else ("y", cfg.LLm, cfg.MMm)
    low = side in ("west", "south")
    m = np.arange(1, nal + 1)
    vel = line(lev(S["u" if normal == "x" else "v"], S["tix"][4], N), normal, 1 if low else nmax + 1, m)
    cx_pos = (-vel if low else vel) > 0.0
    arms = {"radiates (cx > 0)": cx_pos, "binds (cx <= 0)": ~cx_pos}
    arms.update(mask_arms(S, "rmask", normal, 0 if low else nmax + 1, m))
    arms.update(ub_arms(S, side, m))
    return arms


# ------------------------------------------------------------------- KPP ----
KPP_SIZE = (40, 16)


def kpp_eos_state(eos, mode, N=12):
    """eos 'linear': KPP over the linear EOS with T and S; 'nosalt': over the
    split EOS with NT = 1 and no salinity."""
    if eos == "linear":
        cfg = kpp_cfg(*KPP_SIZE, N, nonlin=False)
    else:
        cfg = kpp_cfg(*KPP_SIZE, N, NT=1, salinity=0)
    o = _started(cfg)
    return cfg, o, set_mode(o, mode)


def linear_bvf(o, cfg, tind):
    """rho_eos.F's bvf over the linear EOS, k = 0..N, on the interior."""
    N, I = cfg.N, box(cfg)
    t, zr = o.field("t"), o.field("z_r")
    T = t[(tind - 1) * N:tind * N][I]
    rho = cfg.Tcoef * cfg.T0 - cfg.Tcoef * T
    if cfg.salinity:
        rho = (cfg.Tcoef * cfg.T0 - cfg.Scoef * cfg.S0) - cfg.Tcoef * T
        rho = rho + cfg.Scoef * t[(3 + tind - 1) * N:(3 + tind) * N][I]
    rho = rho * o.field("rmask")[0][I]
    bvf = np.zeros((N + 1,) + rho.shape[1:])
    bvf[1:N] = (G / cfg.rho0) * (rho[:-1] - rho[1:]) / (zr[1:][I] - zr[:-1][I])
    bvf[N], bvf[0] = bvf[N - 1], bvf[1]
    return bvf


def _settle(o, tind, calls):
    """lmd_vmix averages the new boundary-layer depths with the previous
    ones (lmd_kpp.F:330-335): repeat it until they follow the forcing."""
    for _ in range(calls):
        o.L.or_lmd_vmix(o.h, tind)


def kpp_top_state(N=12):
    """Net surface heating (stflx > 0, a quarter of it short-wave) under a
    tenth of the wind stress: the surface layer shoals into the top cell."""
    cfg = kpp_cfg(*KPP_SIZE, N)
    o = _started(cfg)
    tix = set_mode(o, "pred")
    o.field("srflx")[...] = 1.0e-4
    o.field("stflx")[0][...] = 3.0e-4
    o.field("sustr")[...] *= 0.1
    _settle(o, tix[3], 6)
    return cfg, o, tix


def kpp_swr_state(N=12):
    """Every column well mixed (T and S of the top level at all levels, bvf
    from rho_eos), ten times the wind stress and ten times the cooling: the
    surface layer deepens to the levels under a cell thicker than 460 m,
    where lmd_swr_frac.F:60-75 has set both short-wave bands to exactly 0."""
    cfg = kpp_cfg(*KPP_SIZE, N)
    o = _started(cfg)
    tix = set_mode(o, "pred")
    t = o.field("t")
    tv = t.reshape(cfg.NT, 3, N, t.shape[-2], t.shape[-1])
    tv[...] = tv[:, :, N - 1:N]
    o.L.or_rho_eos(o.h, tix[3])
    o.field("stflx")[0][...] = -1.0e-3
    o.field("sustr")[...] *= 10.0
    _settle(o, tix[3], 8)
    return cfg, o, tix


def kpp_base(o, cfg):
    """From the depths lmd_vmix left: kbls of lmd_kpp.F:348-352 per interior
    column (N: the layer ends inside the top cell) and swr_frac(kbls-1)."""
    N, I = cfg.N, box(cfg)
    zw, hbl, sw = o.field("z_w"), o.field("hbls")[0][I], o.field("swr_frac")
    kbls = np.full(hbl.shape, N)
    for k in range(N - 1, 0, -1):
        kbls = np.where(zw[k][I] > zw[N][I] - hbl, k, kbls)
    return kbls, np.take_along_axis(sw[I], (kbls - 1)[None], 0)[0]


# ------------------------------------------------------------------ bulk ----
BULK_SIZE = dict(LLm=24, MMm=20, N=6)        # the grid of the reference libraries (oracle/ref/build_ref.sh)
BULK_ATM = ("uwnd", "vwnd", "tair", "qair", "prate", "lwrad", "swrad")
BULK_OUT = ("sustr", "svstr", "sustr_r", "svstr_r", "stflx", "swflx", "srflx")
T_ICE = -1.8                                  # bulk_frc.F:790


def bulk_state(kind, mode="nstp"):
    """The closed basin with BULK_FRC and KPP after four steps, nrhs = nstp
    or 3.  kind 'analytic': the atmosphere of or_ana_forces as it stands.
    kind 'arms': air 6 degC colder to 6 degC warmer than the sea across the
    basin, dry to humid northwards, no wind at all over the southern
    quarter and up to 26 m/s in the north, rain over the eastern half only,
    a block of land, and a patch of surface water at -1.9 degC with one
    cell at -1.8 exactly."""
    from test_gpu_bulk import bulk_cfg
    cfg = bulk_cfg(**BULK_SIZE)
    o = _started(cfg, steps=4)
    tix = o.tindex()
    tix[4] = tix[3] if mode == "nstp" else 3
    o.set_tindex(tix)
    if kind == "analytic":
        return cfg, o, tix
    ny2, nx2, N = cfg.MMm + 4, cfg.LLm + 4, cfg.N
    fy, fx = np.meshgrid(np.arange(ny2) / (ny2 - 1.0), np.arange(nx2) / (nx2 - 1.0), indexing="ij")
    t = o.field("t").reshape(cfg.NT, 3, N, ny2, nx2)
    t[0, :, N - 1, 14:17, 18:21] = -1.9
    t[0, :, N - 1, 15, 19] = T_ICE
    rm = o.field("rmask")[0]
    rm[8:12, 10:14] = 0.0
    o.field("umask")[0][:, 1:] = rm[:, 1:] * rm[:, :-1]
    o.field("vmask")[0][1:, :] = rm[1:, :] * rm[:-1, :]
    windy = fy > 0.25
    sst = t[0, tix[4] - 1, N - 1]
    o.field("tair")[0][...] = sst + 6.0 * np.cos(2.0 * np.pi * fx)
    o.field("qair")[0][...] = 0.004 + 0.012 * fy
    o.field("uwnd")[0][...] = np.where(windy, 26.0 * fy, 0.0)
    o.field("vwnd")[0][...] = np.where(windy, 3.0 * np.sin(2.0 * np.pi * fx), 0.0)
    o.field("prate")[0][...] = np.where(fx > 0.5, 0.6, 0.0)
    o.field("lwrad")[0][...] = 280.0 + 80.0 * fy
    o.field("swrad")[0][...] = 200.0 * fx
    return cfg, o, tix


def bulk_arms(o, cfg, tix):
    """The data-dependent arms of calc_all_bulk_forces that follow from its
    inputs alone, over the extended bounds 0:Lm+1 x 0:Mm+1: the sign of the
    bulk Richardson number (bulk_frc.F:600-606), the Charnock ranges of
    delW (:626-632), the current-feedback threshold (:844), rain, land,
    and the sea-ice test (:790)."""
    N, ny2, nx2 = cfg.N, cfg.MMm + 4, cfg.LLm + 4
    E = (slice(1, ny2 - 1), slice(1, nx2 - 1))
    f = lambda n: o.field(n)[0][E]
    sst = o.field("t").reshape(cfg.NT, 3, N, ny2, nx2)[0, tix[4] - 1, N - 1][E]
    tair, q = f("tair"), f("qair")
    wspd = np.sqrt(f("uwnd") * f("uwnd") + f("vwnd") * f("vwnd"))
    patm = 1010.0
    es = (1.0007 + 3.46e-6 * patm) * 6.1121 * np.exp(17.502 * sst / (240.97 + sst)) * 0.98
    qsea = 0.62197 * (es / (patm - 0.378 * es))
    buoy = (sst - tair) + 0.61 * (tair + 273.16) * (qsea - q)      # Ri = -g*ZW*buoy/(TairK*delW**2)
    delw = np.sqrt(wspd * wspd + 0.5 * 0.5)
    wet = f("rmask") == 1.0
    return {"unstable (Ri < 0)": buoy > 0.0, "stable (Ri >= 0)": buoy <= 0.0,
            "calm and unstable": (wspd == 0.0) & (buoy > 0.0), "calm and stable": (wspd == 0.0) & (buoy <= 0.0),
            "delW <= 10": delw <= 10.0, "10 < delW <= 18": (delw > 10.0) & (delw <= 18.0), "delW > 18": delw > 18.0,
            "wspd > 3 (current feedback)": wspd > 3.0, "wspd <= 3": wspd <= 3.0,
            "rain": f("prate") > 0.0, "no rain": f("prate") == 0.0, "wet": wet, "land": ~wet,
            "ice: t < -1.8": wet & (sst < T_ICE), "ice: t = -1.8": wet & (sst == T_ICE), "no ice": wet & (sst > T_ICE)}


# ------------------------------------------------------------------- ISO ----
ISO_SIZE = dict(LLm=24, MMm=20, N=6)         # the grid of the reference libraries (oracle/ref/build_ref.sh)
ISO_ARRAYS = ("dRdx", "dRde", "idRz", "diff3u", "diff3v", "Akz")
ISO_LMD = 7                                   # LMD_MIXING + LMD_KPP + LMD_BKPP: idRz's hbls / hbbl arms, no ghat
ISO_SHARE = 0.01                              # every arm on at least this share of the points it is evaluated on
QP2 = 0.0000172                               # eos_vars.F:25
ISO_EPSIL = 1.0e-33                           # step3d_uv2.F:73
ISO_SQUEEZE = 3.2                             # columns squeezed down to exp(-3.2) = 4 % of their depth


def iso_cfg(obc, LLm, MMm, N, NT=2):
    """ADV_ISONEUTRAL on the closed or open basin (split EOS, KPP and BKPP without the non-local term,
    curvilinear terms on), or for obc = 'per' on the doubly periodic Filament (linear EOS, no LMD)."""
    if obc == "per":
        c = oracle.filament_cfg(LLm=LLm, MMm=MMm, N=N, NT=NT, sizex=200.0 * LLm, sizey=50.0 * MMm, np_xi=1, np_eta=1)
        c.adv_isoneutral = 1
        return c
    from test_iso import iso_cfg as basin
    c = basin(LLm=LLm, MMm=MMm, N=N, lmd=ISO_LMD, obc=obc)
    c.NT, c.salinity, c.curvgrid = NT, int(NT > 1), 1
    return c


def iso_land(LLm, MMm, per=False):
    """On every edge one land cell (with its ghost neighbour between walls) and one beside it, a row or a
    column further in: (i, j) in Fortran indices."""
    jw, je, js, jn = MMm // 3, MMm // 2 + 1, LLm // 3 + 1, 2 * LLm // 3 - 1
    on = [(1, jw), (LLm, je), (js, 1), (jn, MMm)]
    ghost = [] if per else [(0, jw), (LLm + 1, je), (js, 0), (jn, MMm + 1)]
    beside = [(2, 2 * MMm // 3), (LLm - 1, MMm // 4), (2 * LLm // 3 + 1, 2), (LLm // 5 + 1, MMm - 1)]
    return on + ghost + beside


def _wrap_all(a, per):
    import metrics
    if per[0] or per[1]:
        for plane in a:
            metrics.wrap(plane, per)


def build_iso(obc, LLm=ISO_SIZE["LLm"], MMm=ISO_SIZE["MMm"], N=ISO_SIZE["N"], NT=2):
    """(cfg, oracle, corrector's time indices, snapshot) for the open sides obc, or obc = 'per'.  The ISO basin
    (the Filament for 'per') on the metric sweep's rough planes after three steps, then, from a fixed seed:
      * every column squeezed by a smooth factor between 1 and exp(-ISO_SQUEEZE) (z_r, z_w, Hz and the fluxes
        through them), so that z_r slopes under every face and the bottom and top cells fall on both sides of
        the 50 m of idRz's blending;
      * noise on rho1 and qp1 (rho) of the size of the vertical density differences: slopes of both signs at
        every corner of a triad, dRz below zero on part of the points, either side of the limiter winning;
      * hbls and hbbl between 5 m and 1 km; noise on t, u, v, with t(nnew) = Hz*t and u, v(nnew) = Hz*u, Hz*v
        as pre_step3d and step3d_uv1 leave them;
      * land on and beside every edge (iso_land);
      * one water point at the centre with f = 0 on the points around it and rho1, qp1 (rho) uniform over the
        5 x 5 columns around it: flat and unstratified, so that epsil wins idRz's limiter there;
      * one water point a quarter of the way in with rho1 (rho) uniform along the levels of the 5 x 5 columns
        around it and growing upwards: flat and unstable, so that max(dRz, 0.) decides the limiter there
        (elsewhere dRx_max outweighs the rotational term that is left of a clamped dRz).
    The snapshot holds every field; it is never written, callers restore the oracle from it."""
    import metrics
    per = obc == "per"
    assert LLm >= 12 and MMm >= 12 and N >= 2
    cfg = iso_cfg(obc, LLm, MMm, N, NT)
    o = oracle.Oracle(cfg)
    o.init()
    metrics.apply_grid(o, None, (metrics.periodic_rough if per else metrics.rough)(LLm, MMm))
    o.step(3)
    tix = set_mode(o, "corr")
    nstp, nnew = tix[3], tix[5]
    o.L.or_rho_eos(o.h, 3)
    rng = np.random.default_rng(700 + (16 if per else obc))
    pp = (bool(cfg.ew_periodic), bool(cfg.ns_periodic))
    f = lambda n: o.field(n)
    # squeeze the columns
    i, j = np.arange(-1.0, LLm + 3)[None, :], np.arange(-1.0, MMm + 3)[:, None]
    w = (0.5 + 0.5 * np.sin(2.0 * np.pi * (i - 0.5) / LLm + 0.4)) * (0.5 + 0.5 * np.cos(2.0 * np.pi * (j - 0.5) / MMm + 1.1))
    s = np.exp(-ISO_SQUEEZE * w / w.max())
    su, sv = s.copy(), s.copy()
    su[:, 1:] = 0.5 * (s[:, 1:] + s[:, :-1])
    sv[1:, :] = 0.5 * (s[1:, :] + s[:-1, :])
    for names, fac in ((("z_r", "z_w", "Hz", "We", "Wi"), s), (("FlxU", "Hz_u", "DU_avg1", "DU_avg2"), su),
                       (("FlxV", "Hz_v", "DV_avg1", "DV_avg2"), sv)):
        for n in names:
            f(n)[...] *= fac
    # density
    for n in (("rho1", "qp1") if cfg.nonlin_eos else ("rho",)):
        a = f(n)
        amp = max(float(np.median(np.abs(a[1:] - a[:-1]))), 1e-3 * float(np.abs(a).max()), 1e-6)
        a += 0.7 * amp * rng.standard_normal(a.shape)
    # boundary layers
    for n in ("hbls", "hbbl"):
        f(n)[...] = 10.0 ** rng.uniform(0.7, 3.0, f(n).shape)
    # tracers and velocities
    t = f("t").reshape(cfg.NT, 3, N, MMm + 4, LLm + 4)
    for q in range(cfg.NT):
        t[q] += 0.1 * max(float(np.abs(t[q]).max()), 0.05) * rng.standard_normal(t[q].shape)
        t[q, nnew - 1] = f("Hz") * t[q, nstp - 1]
    for n, hz in (("u", "Hz_u"), ("v", "Hz_v")):
        a = f(n).reshape(3, N, MMm + 4, LLm + 4)
        a += max(float(np.abs(a).max()), 0.05) * rng.standard_normal(a.shape)
        a[nnew - 1] *= f(hz)
    # land
    rm = f("rmask")[0]
    for (li, lj) in iso_land(LLm, MMm, per):
        rm[lj + 1, li + 1] = 0.0
    metrics.wrap(rm, pp)
    um, vm, pm_ = f("umask")[0], f("vmask")[0], f("pmask")[0]
    um[:, 1:] = rm[:, 1:] * rm[:, :-1]
    vm[1:, :] = rm[1:, :] * rm[:-1, :]
    pm_[1:, 1:] = rm[1:, 1:] * rm[1:, :-1] * rm[:-1, 1:] * rm[:-1, :-1]
    for m in (um, vm, pm_):
        metrics.wrap(m, pp)
    for n, m in (("zeta", rm), ("ubar", um), ("vbar", vm), ("u", um), ("v", vm), ("t", rm)):
        f(n)[...] *= m
    # the flat, unstratified point
    ic, jc = iso_flat_point(LLm, MMm)
    f("f")[0][jc:jc + 3, ic:ic + 3] = 0.0
    for n in (("rho1", "qp1") if cfg.nonlin_eos else ("rho",)):
        f(n)[:, jc - 1:jc + 4, ic - 1:ic + 4] = f(n)[N - 1, jc + 1, ic + 1]
    assert rm[jc - 1:jc + 4, ic - 1:ic + 4].min() == 1.0
    # the flat, unstably stratified point: f as it is, density uniform along the levels and growing upwards
    iu, ju = iso_unstable_point(LLm, MMm)
    for n in (("rho1", "qp1") if cfg.nonlin_eos else ("rho",)):
        col = f(n)[N - 1, ju + 1, iu + 1] + (0.3 * np.arange(N) if n != "qp1" else np.zeros(N))
        f(n)[:, ju - 1:ju + 4, iu - 1:iu + 4] = col[:, None, None]
    assert rm[ju - 1:ju + 4, iu - 1:iu + 4].min() == 1.0 and abs(f("f")[0][ju + 1, iu + 1]) > 0.0
    import romsgpu as rg
    names = [n for n in rg.FIELDS + rg.ISO_FIELDS if _has_field(o, n)]
    for n in names:
        _wrap_all(f(n), pp) if f(n).ndim == 3 else None
    snap = {n: f(n).copy() for n in names}
    for a in snap.values():
        a.setflags(write=False)
    return cfg, o, tix, snap


def _has_field(o, n):
    try:
        o.field(n)
        return True
    except KeyError:
        return False


def iso_flat_point(LLm, MMm):
    """(i, j) of the flat, unstratified water point."""
    return LLm // 2, MMm // 2


def iso_unstable_point(LLm, MMm):
    """(i, j) of the flat, unstably stratified water point."""
    return LLm // 4, MMm // 2


iso_state = functools.lru_cache(maxsize=None)(build_iso)      # one oracle per case, shared: restore before use


def iso_restore(o, snap, tix):
    for n, a in snap.items():
        o.field(n)[...] = a
    o.set_tindex(tix)


def _at(a, di=0, dj=0):
    """a(i+di, j+dj) on the layout of a."""
    return np.roll(a, (-dj, -di), axis=(-2, -1))


def iso_limiter_arms(S):
    """The data-dependent arms of step3d_uv2.F:622-697 from its inputs (S: the arrays handed to the routine under
    their names, and cfg), on the interior at the w-levels 1..N-1: the clamp of dRz, which of cff*dRz, dRx_max
    and epsil wins the limiter, and the min / max arms of the blending factors cfs and cfb."""
    cfg = S["cfg"]
    N, I = cfg.N, box(cfg)
    zr, zw, fc = S["z_r"], S["z_w"], S["f"][0]
    r0g = cfg.rho0 / G
    if cfg.nonlin_eos:
        dpth = -0.5 * (zr[1:] + zr[:-1])
        raw = S["rho1"][:-1] - S["rho1"][1:] + (S["qp1"][:-1] - S["qp1"][1:]) * dpth * (1. - 2. * QP2 * dpth)
    else:
        raw = S["rho"][:-1] - S["rho"][1:]
    dRz = np.maximum(raw, 0.) + r0g * (fc * fc) * (zr[1:] - zr[:-1])
    aX, aE = np.abs(S["dRdx"]), np.abs(S["dRde"])
    mx = S["dm_u"][0] * np.maximum(aX[:-1], aX[1:])
    me = S["dn_v"][0] * np.maximum(aE[:-1], aE[1:])
    dRx_max = np.maximum(np.maximum(mx, _at(mx, 1, 0)), np.maximum(me, _at(me, 0, 1)))
    arms = {}
    if cfg.lmd:
        hs, hb = S["hbls"][0], S["hbbl"][0]
        ds, db = np.maximum(50., hs), np.maximum(50., hb)
        arms.update({"hbls > 50 m": np.broadcast_to(hs > 50., raw.shape), "hbls < 50 m": np.broadcast_to(hs < 50., raw.shape),
                     "hbbl > 50 m": np.broadcast_to(hb > 50., raw.shape), "hbbl < 50 m": np.broadcast_to(hb < 50., raw.shape)})
    else:
        ds = db = 50.
    qs, qb = (zw[N] - zw[1:N]) / ds, (zw[1:N] - zw[0]) / db
    cfs, cfb = np.minimum(1., qs), np.minimum(1., qb)
    cff = 2. * cfs * (2. - cfs) * cfb * (2. - cfb)
    a = cff * dRz
    rot = r0g * (fc * fc) * (zr[1:] - zr[:-1])
    arms.update({"dRz < 0 before its max(., 0)": raw < 0., "dRz > 0": raw > 0.,
                 "limiter: cff*dRz": (a > dRx_max) & (a > ISO_EPSIL), "limiter: dRx_max": (dRx_max >= a) & (dRx_max > ISO_EPSIL),
                 "point: epsil wins the limiter": (a <= ISO_EPSIL) & (dRx_max <= ISO_EPSIL),
                 "point: max(dRz, 0.) decides the limiter": (raw < 0.) & (a > dRx_max) & (cff * (raw + rot) < dRx_max),
                 "cfs < 1": qs < 1., "cfs = 1": qs >= 1., "cfb < 1": qb < 1., "cfb = 1": qb >= 1.})
    return {k: v[I] for k, v in arms.items()}


def iso_operator_arms(S):
    """The data-dependent arms of step3d_t_ISO.F:411-485 and :656-695 from the five arrays it is handed, on the
    interior between the levels k and k+1, k = 1..N-1: the eight sign tests of SW_TRIADS, the numbers idx and
    ide of triads they select (0..4 each), and which of the four corners wins each of the four maxima of Akz."""
    cfg = S["cfg"]
    I = box(cfg)
    X, E, d3u, d3v = S["dRdx"], S["dRde"], S["diff3u"], S["diff3v"]
    lo, up = slice(0, -1), slice(1, None)
    cx = {"dRdx(i,k) < 0": X[lo] < 0., "dRdx(i,k+1) > 0": X[up] > 0., "dRdx(i+1,k+1) < 0": _at(X, 1, 0)[up] < 0.,
          "dRdx(i+1,k) > 0": _at(X, 1, 0)[lo] > 0.}
    ce = {"dRde(j,k) < 0": E[lo] < 0., "dRde(j,k+1) > 0": E[up] > 0., "dRde(j+1,k+1) < 0": _at(E, 0, 1)[up] < 0.,
          "dRde(j+1,k) > 0": _at(E, 0, 1)[lo] > 0.}
    arms = {}
    for c in (cx, ce):
        for k, v in c.items():
            arms[k], arms["not " + k] = v, ~v
    idx, ide = sum(v.astype(int) for v in cx.values()), sum(v.astype(int) for v in ce.values())
    for q in range(5):
        arms["idx = %d" % q], arms["ide = %d" % q] = idx == q, ide == q
    fsc = S["idRz"][1:-1] * (S["z_r"][1:] - S["z_r"][:-1])
    sq = lambda a: (fsc * a) * (fsc * a)
    Hz = S["Hz"]
    with np.errstate(all="ignore"):       # Hz = 0 in ghost cells outside the interior
        cff = 2. / (Hz[1:] + Hz[:-1])
    cff2, cffX, cffE = cff * cff, S["pm"][0] * S["pm"][0], S["pn"][0] * S["pn"][0]
    # corners in the order LL, RL, LU, RU (left / right, lower / upper)
    ux = [(d3u[lo], sq(X[lo])), (_at(d3u, 1, 0)[lo], sq(_at(X, 1, 0)[lo])), (d3u[up], sq(X[up])),
          (_at(d3u, 1, 0)[up], sq(_at(X, 1, 0)[up]))]
    ve = [(d3v[lo], sq(E[lo])), (_at(d3v, 0, 1)[lo], sq(_at(E, 0, 1)[lo])), (d3v[up], sq(E[up])),
          (_at(d3v, 0, 1)[up], sq(_at(E, 0, 1)[up]))]
    with np.errstate(all="ignore"):
        maxima = {"Akz max 1 (diff3u*s2)": [d * s2 for d, s2 in ux], "Akz max 2 (diff3v*s2)": [d * s2 for d, s2 in ve],
                  "Akz max 3 (diff3u*(pm2 + cff2*s2))": [d * (cffX + cff2 * s2) for d, s2 in ux],
                  "Akz max 4 (diff3v*(pn2 + cff2*s2))": [d * (cffE + cff2 * s2) for d, s2 in ve]}
    for name, cand in maxima.items():
        c = np.stack([x[I] for x in cand])
        win, top = np.argmax(c, axis=0), c.max(axis=0)
        for q, corner in enumerate(("LL", "RL", "LU", "RU")):
            arms["%s: %s wins" % (name, corner)] = (win == q) & (top > 0.)
    return {k: (v if k.startswith("Akz") else v[I]) for k, v in arms.items()}


def iso_shares(arms, where, show=True):
    """Assert ISO_SHARE of the points on every arm (one point for the arms named 'point: ..'); returns the shares."""
    shares = {k: float(np.mean(v)) for k, v in arms.items()}
    if show:
        print("ISO arm shares %s: " % (where,) + ", ".join("%s %.3f" % kv for kv in shares.items()))
    short = [(where, k, shares[k]) for k, v in arms.items()
             if (not np.any(v) if k.startswith("point:") else shares[k] < ISO_SHARE)]
    assert not short, short
    return shares
