"""Child-boundary extraction on the device (do_extract_data of extract_data.F
with remap_src_to_grid of vertical_remapping.F).

The expected values never come from the library's own sampling: `Restate` is
compute_coef, interpolate, the rotation, get_child_thickness and
remap_src_to_grid in numpy over Model.get downloads -- the reference's
expressions in its order, one operation at a time on float64 (no contraction),
integer powers as products (x**2 = x*x, x**3 = (x*x)*x, x**4 = (x*x)*(x*x)),
IEEE division -- so the comparisons are np.array_equal.  Only cos, sin and the
child's Cs_w are taken within 4 ulp and then used as the library has them (the
libm differs).  The remap restatement also returns which of the four
integration branches every target cell took.
"""
import os
import threading

import numpy as np
import pytest
from scipy.io import netcdf_file

import romsgpu
from test_gpu_io import FIL, read
from test_gpu_zslice import _model

pytestmark = pytest.mark.gpu

F8 = np.float64
SAME, FIRST, MIDDLE, LAST = range(4)
V3 = ("u", "v", "temp", "salt")


# ---------------------------------------------------------------- objects
def masked_objects():
    """Objects for Rivers_ana / Pipes_ana at 37 x 27 (land: rows j <= 1, and rows 2, 3 outside the channel
    i = 16..22): (name, ipos, jpos, ang or None, output_vars)."""
    k = np.arange(12.0)
    si, sj = 10.25 + k, np.full(12, 3.2)      # south-like: unit steps in i, across the channel's edge, rows 3 | 4
    wi, wj = np.full(12, 5.4), 1.7 + k        # west-like: unit steps in j, from land into the water
    ang = lambda n, a0: a0 + 0.11 * np.arange(n)
    objs = [("grid1_south_r", si, sj, None, "zeta, temp, salt"),
            ("grid1_south_u", si + 0.5, sj, ang(12, 0.2), "ubar, u, up"),
            ("grid1_south_v", si, sj + 0.5, ang(12, -0.4), "vbar, v, vp"),
            ("grid1_west_r", wi, wj, None, "zeta, temp, salt"),
            ("grid1_west_u", wi + 0.5, wj, ang(12, 0.7), "ubar, u"),
            ("grid1_west_v", wi, wj + 0.5, ang(12, -1.3), "vbar, v"),
            # a cell corner of the rho grid (cfx = cfy = 0), a partly masked and a fully masked point
            ("moor1", np.array([19.5, 14.9, 4.3]), np.array([9.5, 2.8, 1.2]), np.array([0.3, -0.8, 1.9]),
             "zeta, temp, salt, ubar, vbar, u, v")]
    return objs


def open_objects(LLm=40, MMm=30):
    """Objects for Filament (no land): lines along both directions that cross every 2 x 2 rank boundary, next to
    the domain's edges too."""
    k = np.arange(LLm - 1.0)
    kj = np.arange(MMm - 1.0)
    ang = lambda n, a0: a0 + 0.07 * np.arange(n)
    # binary fractions: a rank's local position, gobj - iSW_corn, then has the single domain's fraction bit for bit
    return [("chd_south_r", 0.25 + k, np.full(k.size, 0.375), None, "zeta, temp"),
            ("chd_south_u", 0.75 + k, np.full(k.size, 0.375), ang(k.size, 0.1), "ubar, u"),
            ("chd_south_v", 0.25 + k, np.full(k.size, 0.875), ang(k.size, -0.2), "vbar, v"),
            ("chd_mid_r", 0.25 + k, np.full(k.size, 14.75), None, "zeta, temp"),
            ("chd_mid_u", 0.75 + k, np.full(k.size, 14.75), ang(k.size, 0.5), "ubar, u"),
            ("chd_mid_v", 0.25 + k, np.full(k.size, 15.25), ang(k.size, -0.6), "vbar, v"),
            ("chd_west_r", np.full(kj.size, 19.75), 0.625 + kj, None, "zeta, temp"),
            ("chd_west_u", np.full(kj.size, 20.25), 0.625 + kj, ang(kj.size, 0.9), "u"),
            ("chd_west_v", np.full(kj.size, 19.75), 1.125 + kj, ang(kj.size, -1.1), "v"),
            ("moor", np.array([20.5, 39.75, 3.125]), np.array([14.5, 29.625, 22.25]), np.array([0.3, -0.8, 1.9]),
             "zeta, temp, ubar, vbar, u, v")]


def arm(m, objs, child):
    m.extract_begin(*child)
    for name, ip, jp, ang, ov in objs:
        m.extract_add(name, ip, jp, ov, ang=ang)


def flags(ov, salinity):
    """The reference's findstr flags, reduced to what is produced."""
    f = [n for n in ("zeta", "temp", "salt", "ubar", "vbar") if n in ov]
    f += [n for n in ("u", "v") if n in ov]
    return [n for n in f if n != "salt" or salinity]


# ---------------------------------------------------------------- restatement
def compute_coef(ipos, jpos, mask):
    ip, jp = np.floor(ipos).astype(int), np.floor(jpos).astype(int)
    cfx, cfy = ipos - ip, jpos - jp
    M = lambda i, j: mask[j + 1, i + 1]
    c = np.stack([(1 - cfx) * (1 - cfy) * M(ip, jp), cfx * (1 - cfy) * M(ip + 1, jp),
                  (1 - cfx) * cfy * M(ip, jp + 1), cfx * cfy * M(ip + 1, jp + 1)])
    s = c[0] + c[1] + c[2] + c[3]
    with np.errstate(all="ignore"):
        return ip, jp, c / s


def interp(var, ip, jp, cf):
    """interpolate_2D / _3D: var (.., Mm+4, Lm+4) -> (.., np)."""
    with np.errstate(all="ignore"):
        return (var[..., jp + 1, ip + 1] * cf[0] + var[..., jp + 1, ip + 2] * cf[1] + var[..., jp + 2, ip + 1] * cf[2] +
                var[..., jp + 2, ip + 2] * cf[3])


def pw(x, n):
    return x if n == 1 else x * x if n == 2 else (x * x) * x if n == 3 else (x * x) * (x * x)


def gauss(M, b):
    for i in range(3, 0, -1):
        for j in range(i):
            ratio = M[j][i] / M[i][i]
            for k in range(i + 1):
                M[j][k] = M[j][k] - ratio * M[i][k]
            b[j] = b[j] - ratio * b[i]
    return b[0] / M[0][0]


def edge_value(H, A):
    """One boundary extrapolation of calc_interface_values; H, A counted from the edge."""
    h_b, h_t = F8(0.0), H[0]
    iH = F8(1.0) / (h_t - h_b)
    M = [[None] * 4 for _ in range(4)]
    B = [None] * 4
    for k in range(4):
        for kk in range(4):
            M[k][kk] = (F8(1.0) / F8(kk + 1)) * iH * (pw(h_t, kk + 1) - pw(h_b, kk + 1))
        h_b = h_b + H[k]
        h_t = h_t + H[k + 1]
        iH = F8(1.0) / (h_t - h_b)
        B[k] = A[k]
    return gauss(M, B)


def interface_values(H, A):
    N = len(H)
    bot, top = edge_value(H, A), edge_value(H[::-1], A[::-1])
    n = N + 1
    cp, dp = [None] * n, [None] * n
    cp[0], dp[0] = F8(0.0) / F8(1.0), bot / F8(1.0)
    for k in range(1, N):   # the reference's k = 2..n-1
        h0, h1 = H[k - 1], H[k]
        s = h0 + h1
        alpha, beta = (h1 * h1) / (s * s), (h0 * h0) / (s * s)
        s4 = (s * s) * (s * s)
        d1 = 2 * (h1 * h1) * (h1 * h1 + 2 * (h0 * h0) + 3 * h0 * h1) / s4
        d2 = 2 * (h0 * h0) * (h0 * h0 + 2 * (h1 * h1) + 3 * h0 * h1) / s4
        d = d1 * A[k - 1] + d2 * A[k]
        den = F8(1.0) - alpha * cp[k - 1]
        cp[k] = beta / den
        dp[k] = (d - alpha * dp[k - 1]) / den
    iv = [None] * n
    iv[N] = top
    for k in range(N - 1, -1, -1):
        iv[k] = dp[k] - cp[k] * iv[k + 1]
    return iv


def integrate(a0, a1, a2, z0, z1):
    one_third = F8(0.3333333333)
    return a0 * (z1 - z0) + F8(0.5) * a1 * (z1 * z1 - z0 * z0) + one_third * a2 * ((z1 * z1) * z1 - (z0 * z0) * z0)


def remap_column(H, t, Ht):
    """remap_src_to_grid for one column (float64 scalars): (t_tgt, branch of every target cell)."""
    N, Nc = len(H), len(Ht)
    iv = interface_values(H, t)
    tdt, tds = F8(0.0), F8(0.0)
    for k in range(Nc):
        tdt = tdt + Ht[k]
    for k in range(N):
        tds = tds + H[k]
    a0, a1, a2, tts = [], [], [], F8(0.0)
    for k in range(N):
        a0.append(iv[k])
        a1.append(6 * t[k] - 4 * iv[k] - 2 * iv[k + 1])
        a2.append(3 * (iv[k] + iv[k + 1] - 2 * t[k]))
        tts = tts + t[k] * H[k]
    Ho = [H[k] * (tdt / tds) for k in range(N)]
    hst = F8(0.0)
    for k in range(N):
        hst = hst + Ho[k]
    Ho[N - 1] = Ho[N - 1] + tdt - hst
    z = [F8(0.0)]
    for k in range(N):
        z.append(z[k] + Ho[k])
    istart, iend = [1] * Nc, [1] * Nc
    fstart, fend = [F8(0.0)] * Nc, [F8(0.0)] * Nc
    cth, csh, idx = Ht[0], Ho[0], 1
    for kn in range(Nc - 1):
        while cth > csh and idx < N:   # idx < N: the library's clamp (the reference has none)
            idx += 1
            csh = csh + Ho[idx - 1]
        iend[kn] = idx
        istart[kn + 1] = idx
        fend[kn] = (cth - z[idx - 1]) / Ho[idx - 1]
        fstart[kn + 1] = fend[kn]
        cth = cth + Ht[kn + 1]
    iend[Nc - 1], fend[Nc - 1] = N, F8(1.0)
    tmp, branch, tt = [], [], F8(0.0)
    for k in range(Nc):
        di, br = F8(0.0), set()
        for i in range(istart[k], iend[k] + 1):
            q = i - 1
            if istart[k] == iend[k]:
                di = integrate(a0[q], a1[q], a2[q], fstart[k], fend[k]) * H[q]
                br.add(SAME)
            elif i == istart[k] and i < iend[k]:
                di = integrate(a0[q], a1[q], a2[q], fstart[k], F8(1.0)) * H[q]
                br.add(FIRST)
            elif istart[k] < i < iend[k]:
                di = di + integrate(a0[q], a1[q], a2[q], F8(0.0), F8(1.0)) * H[q]
                br.add(MIDDLE)
            else:
                di = di + integrate(a0[q], a1[q], a2[q], F8(0.0), fend[k]) * H[q]
                br.add(LAST)
        tmp.append(di / Ht[k])
        tt = tt + tmp[k] * Ht[k]
        branch.append(br)
    diff = tt - tts
    out = [tmp[k] - diff * (tmp[k] / tt) if tt != 0.0 else F8(0.0) for k in range(Nc)]
    return np.array(out), branch


def child_thickness(h, Nc, hc, csw):
    """get_child_thickness over all points at once: (Nc, np)."""
    ds = F8(1.0) / F8(Nc)
    hinv = 1.0 / (h + hc)
    zprev = -h
    out = []
    for k in range(1, Nc + 1):
        cff_w = hc * ds * F8(k - Nc)
        z = h * (cff_w + csw[k] * h) * hinv
        out.append(z - zprev)
        zprev = z
    return np.array(out)


class Restate:
    """Everything do_extract_data computes for the armed objects, from downloads of the model's fields."""

    def __init__(self, m, objs, child, slot3="nstp", zero_ang=False, angler=None):
        self.m, self.objs, self.child = m, objs, child
        t = m.t
        N = m.N
        s3 = getattr(t, slot3)
        self.f2 = {n: m.get(n)[t.knew - 1] for n in ("zeta", "ubar", "vbar")}
        self.f3 = {n: m.get(n)[(s3 - 1) * N:s3 * N] for n in ("u", "v")}
        tr = m.get("t").reshape(m.NT, 3, N, *m.shape2)[:, s3 - 1]
        self.f3["temp"] = tr[0]
        if m.salinity and m.NT >= 2:
            self.f3["salt"] = tr[1]
        self.masks = dict(r=m.get("rmask")[0], u=m.get("umask")[0], v=m.get("vmask")[0])
        self.mismatch = m.extract_state()[1]
        if self.mismatch:
            self.hz = dict(r=m.get("Hz"))
            if m.extract_state()[4]:
                self.hz.update(u=m.get("Hz_u"), v=m.get("Hz_v"))
            self.csw = m.extract_child_cs()
        self.angler = np.zeros(m.shape2) if angler is None else angler
        self.zero_ang = zero_ang
        self.branches = set()
        self.aux = {}

    def coefs(self, q):
        """{grid: (ip, jp, cf)}, local range (i0, n) of object q (0-based) by the reference's arithmetic."""
        m = self.m
        name, gi, gj, ang, ov = self.objs[q]
        s, n = romsgpu.extract_locate(m.Lm, m.Mm, m.iSW, m.jSW, gi, gj)
        li, lj = gi[s - 1:s - 1 + n] - m.iSW, gj[s - 1:s - 1 + n] - m.jSW
        ri, rj = li + 0.5, lj + 0.5
        out = dict(r=compute_coef(ri, rj, self.masks["r"]))
        if ang is not None:
            ui = ri + 0.5
            out["u"] = compute_coef(ui, rj, self.masks["u"])
            out["v"] = compute_coef(ui - 0.5, rj + 0.5, self.masks["v"])
        return out, s, n

    def remap(self, prof, g, cf):
        Hp = interp(self.hz[g], *cf)
        h = np.zeros(Hp.shape[1])
        for k in range(Hp.shape[0]):
            h = h + Hp[k]
        with np.errstate(all="ignore"):
            Hc = child_thickness(h, self.child[0], F8(self.child[3]), self.csw)
            out = np.empty((self.child[0], prof.shape[1]))
            for p in range(prof.shape[1]):
                out[:, p], br = remap_column(list(Hp[:, p]), list(prof[:, p]), list(Hc[:, p]))
                if np.isfinite(out[:, p]).all():
                    self.branches.update(*br)
        return out, Hp, Hc

    def obj(self, q, cosa, sina):
        """name -> expected array of object q, rotation with the given cosa, sina."""
        name, gi, gj, ang, ov = self.objs[q]
        cf, s, n = self.coefs(q)
        want = flags(ov, "salt" in self.f3)
        out = {}
        if n == 0:
            return out
        if "zeta" in want:
            out["zeta"] = interp(self.f2["zeta"], *cf["r"])
        with np.errstate(all="ignore"):
            if "ubar" in want or "vbar" in want:
                ui, vi = interp(self.f2["ubar"], *cf["u"]), interp(self.f2["vbar"], *cf["v"])
                if "ubar" in want:
                    out["ubar"] = cosa * ui - sina * vi
                if "vbar" in want:
                    out["vbar"] = sina * ui + cosa * vi
            prof = {}
            for v in ("temp", "salt"):
                if v in want:
                    prof[v] = ("r", interp(self.f3[v], *cf["r"]))
            if "u" in want or "v" in want:
                ui, vi = interp(self.f3["u"], *cf["u"]), interp(self.f3["v"], *cf["v"])
                if "u" in want:
                    prof["u"] = ("u", cosa * ui - sina * vi)
                if "v" in want:
                    prof["v"] = ("v", sina * ui + cosa * vi)
        for v, (g, p) in prof.items():
            if self.mismatch:
                out[v], Hp, Hc = self.remap(p, g, cf[g])
                self.aux[(q, v)] = (p, Hp, Hc)
            else:
                out[v] = p
        return out


def ulps(a, b):
    a, b = np.asarray(a, F8), np.asarray(b, F8)
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))) if a.size else 0.0


def check_coefficients(m, R):
    """Test 1: ip, jp, coef bitwise; cosa, sina, Cs_w within 4 ulp.  Returns the library's (cosa, sina) per object."""
    cs = []
    for q, (name, gi, gj, ang, ov) in enumerate(R.objs):
        cf, s, n = R.coefs(q)
        info = m.extract_info(q + 1)
        assert (info["np"], info["start_idx"] if n else 0) == (n, s if n else 0), name
        assert info["scalar"] == (ang is None)
        ca = sa = np.ones(n)
        for g in cf:
            ip, jp, c, ca, sa = m.extract_coef(q + 1, g)
            assert np.array_equal(ip, cf[g][0]) and np.array_equal(jp, cf[g][1]), (name, g)
            assert np.array_equal(c, cf[g][2], equal_nan=True), (name, g)
        if ang is not None and n:
            with np.errstate(all="ignore"):
                angp = interp(R.angler, *cf["r"]) - ang[s - 1:s - 1 + n]
            ok = np.isfinite(angp)
            assert ulps(ca[ok], np.cos(angp[ok])) <= 4 and ulps(sa[ok], np.sin(angp[ok])) <= 4, name
            assert np.isnan(ca[~ok]).all() and np.isnan(sa[~ok]).all()
        cs.append((ca, sa))
    return cs


def child_cs(Nc, theta_s, theta_b):
    ds = 1.0 / Nc
    out = np.zeros(Nc + 1)
    out[0] = -1.0
    for k in range(1, Nc):
        sc = ds * (k - Nc)
        csrf = (1.0 - np.cosh(theta_s * sc)) / (np.cosh(theta_s) - 1.0) if theta_s > 0 else -sc * sc
        out[k] = (np.exp(theta_b * csrf) - 1.0) / (1.0 - np.exp(-theta_b)) if theta_b > 0 else csrf
    return out


def compare_all(m, R, cs, equal=True):
    """Every variable of every object against the restatement; returns the names compared."""
    seen, nan_pts = [], 0
    for q in range(len(R.objs)):
        exp = R.obj(q, *cs[q])
        info = m.extract_info(q + 1)
        assert set(info["vars"]) == set(exp) or info["np"] == 0, (R.objs[q][0], info, set(exp))
        for v, e in exp.items():
            got = m.extract(q + 1, v)
            assert got.shape == e.shape, (R.objs[q][0], v, got.shape, e.shape)
            nan_pts += int(np.isnan(got).any())
            if equal:
                assert np.array_equal(got, e, equal_nan=True), (R.objs[q][0], v, np.nanmax(np.abs(got - e)))
            seen.append((q, v, got, e))
    return seen


PARENT = dict(rivers=(6.0, 6.0, 25.0), pipes=(6.0, 6.0, 25.0), filament=(6.0, 2.0, 25.0))


def masked_model(case, child_of):
    m = _model(case, 5)
    child = child_of(m)
    arm(m, masked_objects(), child)
    m.step(3)
    return m, child


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("case", ["rivers", "pipes"])
def test_coefficients_and_no_mismatch(case):
    m, child = masked_model(case, lambda mm: (mm.N,) + PARENT[case])
    objs = masked_objects()
    assert m.extract_state() == (7, False, 5, 75, False)
    m.calc_extract()
    R = Restate(m, objs, child)
    cs = check_coefficients(m, R)
    # the masks put the special points where the objects expect them
    ncorner = []
    for q in range(len(objs)):
        ip, jp, _ = R.coefs(q)[0]["r"]
        ncorner += [int(4 - (R.masks["r"][jp[p] + 1:jp[p] + 3, ip[p] + 1:ip[p] + 3] > 0.5).sum()) for p in range(ip.size)]
    assert 4 in ncorner and any(0 < c < 4 for c in ncorner) and 0 in ncorner
    ip, jp, c = R.coefs(6)[0]["r"]
    assert (objs[6][1][0] + 0.5 == ip[0]) and (objs[6][2][0] + 0.5 == jp[0]) and c[0, 0] == 1.0 and (c[1:, 0] == 0).all()
    assert np.isnan(m.extract_coef(7, "r")[2][:, 2]).all()
    seen = compare_all(m, R, cs)
    assert {v for _, v, _, _ in seen} == {"zeta", "ubar", "vbar", "u", "v", "temp", "salt"}
    assert all(g.shape == ((5, g.shape[-1]) if v in V3 else (g.shape[-1],)) for _, v, g, _ in seen)
    # the fully masked point is NaN, the wet ones are numbers
    moor = {v: g for q, v, g, _ in seen if q == 6}
    assert np.isnan(moor["temp"][:, 2]).all() and np.isnan(moor["zeta"][2]) and np.isfinite(moor["temp"][:, 0]).all()
    # negative controls: the other slot, u against v, no rotation
    other = Restate(m, objs, child, slot3="nnew")
    wet = np.isfinite(moor["temp"][0])
    assert not np.array_equal(other.obj(6, *cs[6])["u"][:, wet], moor["u"][:, wet])
    assert not np.array_equal(moor["u"][:, wet], moor["v"][:, wet])
    unrot = R.obj(6, np.ones(3), np.zeros(3))
    assert not np.array_equal(unrot["u"][:, wet], moor["u"][:, wet]) and np.abs(moor["u"][:, wet]).max() > 0
    m.close()


@pytest.mark.parametrize("case,nchd", [("rivers", 1), ("rivers", 2), ("rivers", 3), ("rivers", 8), ("pipes", 3),
                                       ("pipes", 8)])
def test_mismatch_masked(case, nchd):
    child = (nchd, 5.0, 1.5, 40.0)
    m, _ = masked_model(case, lambda mm: child)
    objs = masked_objects()
    assert m.extract_state() == (7, True, nchd, 75, True)
    assert ulps(m.extract_child_cs(), child_cs(nchd, 5.0, 1.5)) <= 4
    m.calc_extract()
    R = Restate(m, objs, child)
    cs = check_coefficients(m, R)
    seen = compare_all(m, R, cs)
    assert all(g.shape[0] == nchd for _, v, g, _ in seen if v in V3)
    want = {1: {MIDDLE, FIRST, LAST}, 2: {MIDDLE}, 3: {FIRST, LAST}, 8: {SAME}}[nchd]
    assert want <= R.branches, R.branches
    # the fully masked point: NaN, nothing faults; the wet points: numbers
    moor = {v: g for q, v, g, _ in seen if q == 6}
    assert all(np.isnan(moor[v][:, 2]).all() and np.isfinite(moor[v][:, 0]).all() for v in V3)
    # conservation, independent of the remap's restatement: sum(t_tgt*Hz_chd) == sum(t_src*Hz_par) on wet points
    for (q, v), (p, Hp, Hc) in R.aux.items():
        if v != "temp":
            continue
        got = m.extract(q + 1, v)
        ok = np.isfinite(got).all(axis=0)
        a, b = (got * Hc).sum(axis=0)[ok], (p * Hp).sum(axis=0)[ok]
        assert ok.any() and np.max(np.abs(a - b) / np.abs(b)) <= 1e-12, (q, v)
    m.close()


def test_all_four_branches_occur_over_the_child_counts():
    """The restatement's branch report over Nc = 1, 2, 3, 8 on one parent column (no device needed beyond import)."""
    H = [F8(x) for x in (3.0, 2.5, 2.0, 1.5, 1.0)]
    t = [F8(x) for x in (4.0, 5.0, 7.0, 8.0, 8.5)]
    seen = set()
    for nc in (1, 2, 3, 8):
        out, br = remap_column(H, t, [F8(10.0 / nc)] * nc)
        seen.update(*br)
        assert abs(sum(out) * (10.0 / nc) - sum(a * b for a, b in zip(H, t))) < 1e-12 * 60
    assert seen == {SAME, FIRST, MIDDLE, LAST}


def test_constant_profile_stays_constant():
    m = _model("rivers", 5)
    arm(m, masked_objects(), (8, 5.0, 1.5, 40.0))
    m.step(2)
    t = m.get("t")
    t[:] = 7.25
    m.put("t", t)
    m.calc_extract()
    for q in (0, 3, 6):
        got = m.extract(q + 1, "temp")
        ok = np.isfinite(got)
        assert ok.any() and np.max(np.abs(got[ok] - 7.25)) <= 1e-12 * 7.25
    m.close()


def test_filament_same_count_other_stretching():
    m = romsgpu.Model.from_case(**FIL)
    child = (12, 4.0, 2.0, 25.0)
    objs = open_objects()
    arm(m, objs, child)
    m.step(3)
    assert m.extract_state()[1:3] == (True, 12)
    m.calc_extract()
    R = Restate(m, objs, child)
    cs = check_coefficients(m, R)
    seen = compare_all(m, R, cs)
    assert {v for _, v, _, _ in seen} == {"zeta", "ubar", "vbar", "u", "v", "temp"}
    assert all(np.isfinite(g).all() for _, _, g, _ in seen)
    assert "salt" not in m.extract_info(1)["vars"]
    # the timing entry runs the same two launches and leaves the same results
    ms = m.time_calc_extract(2)
    assert ms[0] > 0 and ms[1] > 0
    compare_all(m, R, cs)
    m.close()


def test_angler_enters_the_rotation():
    m = _model("rivers", 5)
    jj, ii = np.meshgrid(np.arange(m.shape2[0]), np.arange(m.shape2[1]), indexing="ij")
    angler = 0.01 * ii + 0.02 * jj
    objs = masked_objects()
    m.extract_begin(5, *PARENT["rivers"], angler=angler)
    for name, ip, jp, ang, ov in objs:
        m.extract_add(name, ip, jp, ov, ang=ang)
    m.step(2)
    m.calc_extract()
    R = Restate(m, objs, (5,) + PARENT["rivers"], angler=angler)
    cs = check_coefficients(m, R)
    compare_all(m, R, cs)
    plain = np.cos(-objs[6][3])
    assert not np.allclose(cs[6][0][:2], plain[:2])
    m.close()


def test_hz_u_hz_v_are_set_huvs_of_the_step_just_taken():
    m = _model("rivers", 5)
    arm(m, masked_objects(), (3, 5.0, 1.5, 40.0))
    assert m.extract_state()[4]
    m.step(2)
    before = m.get("Hz")
    m.step(1)
    after, hu, hv = m.get("Hz"), m.get("Hz_u"), m.get("Hz_v")
    L, M = m.Lm, m.Mm
    c = (slice(None), slice(2, M + 2), slice(2, L + 2))      # cells 1..Mm x 1..Lm
    w = (slice(None), slice(2, M + 2), slice(1, L + 1))      # i - 1
    s = (slice(None), slice(1, M + 1), slice(2, L + 2))      # j - 1
    assert np.array_equal(hu[c], 0.5 * (before[c] + before[w]))
    assert np.array_equal(hv[c], 0.5 * (before[c] + before[s]))
    assert not np.array_equal(hu[c], 0.5 * (after[c] + after[w])) and not np.array_equal(hv[c], 0.5 * (after[c] + after[s]))
    m.close()


def write_objects_file(path, objs):
    with netcdf_file(path, "w", version=2) as nc:
        nc.createDimension("two", 2)
        nc.createDimension("three", 3)
        for name, ip, jp, ang, ov in objs:
            d = "n_" + name
            nc.createDimension(d, ip.size)
            v = nc.createVariable(name, "d", ("two" if ang is None else "three", d))
            v[0], v[1] = ip, jp
            if ang is not None:
                v[2] = ang
            v.output_vars = ov


def test_the_extraction_file(tmp_path):
    m = _model("rivers", 5)
    objs = masked_objects()
    objs.insert(2, ("grid2_off_r", np.array([-4.0, -3.0]), np.array([5.0, 5.0]), None, "zeta, temp"))   # np = 0
    src, p = str(tmp_path / "objects.nc"), str(tmp_path / "ext.nc")
    write_objects_file(src, objs)
    with netcdf_file(src, "r", mmap=False) as nc:   # an object's index is its variable's place in the file
        order = list(nc.variables)
    objs.sort(key=lambda o: order.index(o[0]))
    iu, iv, ioff = (1 + [o[0] for o in objs].index(n) for n in ("grid1_south_u", "grid1_south_v", "grid2_off_r"))
    m.extract_begin(3, 5.0, 1.5, 40.0)
    assert m.extract_objects_file(src) == 8
    msg = m.L.roms_gpu_last_error()
    assert b"not produced here" in msg and b"grid1_south_u: up" in msg and b"grid1_south_v: vp" in msg
    info = m.extract_info(iu)
    assert info["unsupported"] == ("up",) and set(info["vars"]) == {"ubar", "u"}
    assert m.extract_info(iv)["unsupported"] == ("vp",) and m.extract_info(ioff)["np"] == 0
    m.step(2)
    snaps = []
    for rec in (1, 2):
        m.wrt_extract(p, rec, rec, 100.0 * rec)
        snaps.append({(q, v): m.extract(q + 1, v) for q in range(8) for v in m.extract_info(q + 1)["vars"]
                      if m.extract_info(q + 1)["np"]})
        m.step(1)
    m.io_wait()
    d = read(p)
    dims = d["_dims"]
    assert dims["time_" + objs[0][0].split("_")[0]] is None and dims["s_rho"] == 3
    for q, (name, ip, jp, ang, ov) in enumerate(objs):
        lab = "np%03d" % (q + 1)
        if name == "grid2_off_r":
            assert lab not in dims
        else:
            assert dims[lab] == ip.size, lab
    assert not any(k.startswith("grid2") for k in d)
    assert d["grid1_time"].tolist() == [100.0, 200.0] and d["moor1_time"].tolist() == [100.0, 200.0]
    names = {k for k in d if not k.startswith("_")}
    assert names == {"grid1_time", "moor1_time", "grid1_zeta_south", "grid1_temp_south", "grid1_salt_south",
                     "grid1_ubar_south", "grid1_u_south", "grid1_vbar_south", "grid1_v_south", "grid1_zeta_west",
                     "grid1_temp_west", "grid1_salt_west", "grid1_ubar_west", "grid1_u_west", "grid1_vbar_west",
                     "grid1_v_west", "moor1_zeta", "moor1_temp", "moor1_salt", "moor1_ubar", "moor1_vbar", "moor1_u",
                     "moor1_v"}
    file_name = lambda q, v: objs[q][0].split("_")[0] + "_" + v + ("_" + objs[q][0].split("_")[1] if "_" in objs[q][0] else "")
    for rec in (0, 1):
        for (q, v), a in snaps[rec].items():
            assert np.array_equal(d[file_name(q, v)][rec], a, equal_nan=True), (q, v, rec)
    with netcdf_file(p, "r", mmap=False) as nc:
        v = nc.variables["grid1_temp_west"]
        lab = lambda n: "np%03d" % (1 + [o[0] for o in objs].index(n))
        assert v.dimensions == ("time_grid1", "s_rho", lab("grid1_west_r")) and v.typecode() == "d"
        assert (int(v.start), int(v.count), v.dname, int(v.dsize)) == (1, 12, b"n_grid1_west_r", 12)
        assert v.long_name == b"potential temperature" and v.units == b"Celsius"
        v = nc.variables["grid1_ubar_south"]
        assert v.dimensions == ("time_grid1", lab("grid1_south_u")) and v.long_name == b"vertically averaged u-momentum component"
        assert v.units == b"meter second-1"
        assert nc.variables["moor1_zeta"].dimensions == ("time_grid1", lab("moor1"))
        t = nc.variables["grid1_time"]
        assert t.long_name == b"Time since 2000" and t.units == b"second" and t.dimensions == ("time_grid1",)
    m.close()


def test_partitioned_pieces_join_to_the_single_domain():
    objs = open_objects()
    child = (7, 4.0, 2.0, 25.0)

    def sample(mm):
        arm(mm, objs, child)
        mm.step(3)
        mm.calc_extract()
        out = {}
        for q in range(len(objs)):
            info = mm.extract_info(q + 1)
            out[q] = (info["start_idx"], info["np"], {v: mm.extract(q + 1, v) for v in info["vars"]} if info["np"] else {})
        mm.close()
        return out

    ref = sample(romsgpu.Model.from_case(**FIL))
    npx, npe = 2, 2
    parts, errs = {}, []

    def work(rank):
        try:
            h = romsgpu.comm_create_local(781, npx * npe, rank)
            parts[rank] = sample(romsgpu.Model.from_case(np_xi=npx, np_eta=npe, comm=h, rank=rank, **FIL))
            romsgpu.comm_destroy(h)
        except Exception as e:
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(npx * npe)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
    assert not errs, errs
    for q, (name, gi, gj, ang, ov) in enumerate(objs):
        s0, n0, whole = ref[q]
        assert (s0, n0) == (1, gi.size)
        for v, a in whole.items():
            glob = np.full(a.shape, np.nan)
            cover = np.zeros(gi.size, int)
            for r in range(npx * npe):
                s, n, piece = parts[r][q]
                if n:
                    glob[..., s - 1:s - 1 + n] = piece[v]
                    cover[s - 1:s - 1 + n] += 1
            assert (cover == 1).all(), (name, cover)
            assert np.array_equal(glob, a), (name, v, np.nanmax(np.abs(glob - a)))


def test_errors(tmp_path):
    p = str(tmp_path / "none.nc")
    m = _model("basin", 2)   # N = 2 < 5
    k = np.arange(4.0)
    for fn, args in ((m.calc_extract, ()), (m.wrt_extract, (p, 1, 1, 5.0))):
        with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
            fn(*args)
    with pytest.raises(romsgpu.RomsGpuError, match="extract_begin"):
        m.extract_add("a_b_r", 3.2 + k, 4.1 + k, "zeta")
    m.extract_begin(4, 5.0, 1.5, 40.0)
    with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
        m.calc_extract()
    with pytest.raises(romsgpu.RomsGpuError, match="scalar"):
        m.extract_add("a_b_r", 3.2 + k, 4.1 + k, "zeta, ubar")
    with pytest.raises(romsgpu.RomsGpuError, match="scalar"):
        m.extract_add("a_b_r", 3.2 + k, 4.1 + k, "temp, v")
    with pytest.raises(romsgpu.RomsGpuError, match="N >= 5"):
        m.extract_add("a_b_r", 3.2 + k, 4.1 + k, "zeta, temp")
    with pytest.raises(romsgpu.RomsGpuError, match="N >= 5"):
        m.extract_add("a_b_u", 3.2 + k, 4.1 + k, "ubar", ang=0.1 * k)   # 'u' inside 'ubar'
    assert m.extract_state() == (0, True, 4, 0, False)   # a refused call arms nothing
    with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
        m.wrt_extract(p, 1, 1, 5.0)
    m.io_wait()
    assert not os.path.exists(p)
    assert m.extract_add("a_b_r", 3.2 + k, 4.1 + k, "zeta") == 1   # 2-D variables need no remap
    with pytest.raises(romsgpu.RomsGpuError, match="no sample"):
        m.extract(1, "zeta")
    m.calc_extract()
    assert m.extract(1, "zeta").shape == (4,)
    with pytest.raises(romsgpu.RomsGpuError, match="not extracted"):
        m.extract(1, "temp")
    with pytest.raises(romsgpu.RomsGpuError, match="no such object"):
        m.extract(2, "zeta")
    buf = np.empty(5)
    assert m.L.roms_gpu_extract_copy_out(1, 1, buf.ctypes.data, 5) == -1 and b"count" in m.L.roms_gpu_last_error()
    assert m.L.roms_gpu_extract_copy_out(1, 3, buf.ctypes.data, 4) == -1 and b"one ROMS_EXT" in m.L.roms_gpu_last_error()
    assert m.L.roms_gpu_extract_copy_out(1, 1, buf.ctypes.data, 4) == 0
    with pytest.raises(romsgpu.RomsGpuError):
        m.extract_objects_file(str(tmp_path / "absent.nc"))
    assert m.extract_state()[0] == 1
    m.extract_begin(2, 1.0, 1.0, 1.0)   # begin clears and disarms
    assert m.extract_state() == (0, True, 2, 0, False)
    with pytest.raises(romsgpu.RomsGpuError, match="not armed"):
        m.calc_extract()
    m.close()


def test_arming_after_a_step_waits_for_fresh_hz_u_hz_v():
    m = romsgpu.Model.from_case(**FIL)
    m.step(2)   # whole steps without an armed object do not store Hz_u, Hz_v
    objs = open_objects()
    arm(m, objs, (7, 4.0, 2.0, 25.0))
    with pytest.raises(romsgpu.RomsGpuError, match="stale"):
        m.calc_extract()
    with pytest.raises(romsgpu.RomsGpuError, match="no sample"):
        m.extract(2, "u")
    m.step(1)
    m.calc_extract()
    R = Restate(m, objs, (7, 4.0, 2.0, 25.0))
    compare_all(m, R, check_coefficients(m, R))
    # without the remap nothing reads them: no wait
    arm(m, objs, (12,) + PARENT["filament"])
    assert m.extract_state()[1:5:3] == (False, False)
    m.calc_extract()
    m.close()


def test_the_step_is_untouched():
    def run(armed):
        m = romsgpu.Model.from_case(**FIL)
        if armed:
            arm(m, open_objects(), (7, 4.0, 2.0, 25.0))
        for _ in range(6):
            m.step(1)
            if armed:
                m.calc_extract()
        out = {k: m.get(k) for k in ("zeta", "u", "v", "t")}
        m.close()
        return out

    a, b = run(True), run(False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
