"""ADV_ISONEUTRAL in the oracle against the reference's own routines.

oracle/ref/build_ref.sh compiles prsgrd.F, step3d_uv2.F and step3d_t_ISO.F from the reference tree, unchanged, with
ADV_ISONEUTRAL (and with it SW_TRIADS and STABILIZE) at 24 x 20 x 6, nt = 2: the basin with MASKING, SALINITY, the
split EOS, LMD_KPP and LMD_BKPP, closed (iso0) and open on E+S (iso6), W+N (iso9) and all sides (iso15), so that every
side copies LapT and zeroes it, and the SW and NE corners lie between one of each; and the doubly periodic Filament set with
the linear EOS and no LMD (isoper), which reaches the rho arm of dRz and the /50. arms of cfs and cfb.  Each stage
hands one state to the reference routine and to its restatement (or_prsgrd / or_step3d_uv2 / or_step3d_t with
oracle/oracle_iso.c) and compares every element of every array the routine can write, ghost rows and corners
included, bit for bit: + - * / sqrt abs min max in IEEE double on both sides, no contraction, so a difference is a
difference in evaluation order or in the arm taken.  No tolerance, no exception: flang evaluates f**2 as f*f.

The state is branch_states.iso_state.  From the arrays handed to the reference each stage first asserts that every
data-dependent arm is taken on at least 1 % of the points it is evaluated on (one point each for epsil winning the
limiter and for max(dRz, 0.) deciding it), and prints the shares.

The reference reads private scratch that it never wrote.  Which results that touches is not taken from a reading of
the code: every stage runs the reference twice, with the scratch filled with two different values, and the
elements that differ between the runs are the undefined ones.  For prsgrd that set must be exactly dRdx at
i = istr and i = iend+1 (all j = jstr..jend, all k) and dRde at j = jstr and j = jend+1 (all i = istr..iend, all k)
on non-periodic edges -- rx(istr-1), rx(iend+2), which the extrapolation of prsgrd.F:256-268 does not set; the
oracle continues the extrapolation there, see oracle_iso.c -- and empty for isoper.  step3d_uv2 and step3d_t show no
undefined output at all, apart from Akz itself, which is a scratch array: the routine writes it on the interior at
the w-levels 1..N-1 and nowhere else, and that is where it is compared.

Not marked gpu.  Skips only where neither the libraries nor the reference tree exist.
"""
import numpy as np
import pytest

import branch_states as bs
import oracle.ref as ref

SIZE = bs.ISO_SIZE
FILLS = (1.0e3, -7.5e5)
TIME_LEVELS = ("u", "v", "ubar", "vbar", "t", "zeta")

pytestmark = pytest.mark.skipif(not (ref.have_tree() or all(ref.available(v) for v in ref.ISO_VARIANTS)),
                                reason="neither oracle/_ref libraries nor a reference tree")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def differ(a, b):
    assert a.shape == b.shape
    return bits(a) != bits(b)


def where(mask):
    """The first few (k, j, i) Fortran indices of a mask on the (levels, Mm+4, Lm+4) layout."""
    return [(int(k), int(j) - 1, int(i) - 1) for k, j, i in np.argwhere(mask)[:8]]


def setup(variant):
    """iso_state restored in its oracle, and the library: (cfg, o, r, snap)."""
    assert ref.available(variant)
    obc = "per" if variant == "isoper" else ref.ISO[variant]
    cfg, o, tix, snap = bs.iso_state(obc, **SIZE)
    bs.iso_restore(o, snap, tix)
    r = ref.RefLib(variant)
    assert (r.LLm, r.MMm, r.N, r.NT) == (SIZE["LLm"], SIZE["MMm"], SIZE["N"], 2) and r.LLm != r.MMm
    return cfg, o, r, snap


def inputs(o, cfg):
    """What the oracle holds now, as the reference is about to be handed it."""
    S = {n: o.field(n).copy() for n in ("z_r", "z_w", "Hz", "f", "pm", "pn", "dm_u", "dn_v") + bs.ISO_ARRAYS}
    for n in (("rho1", "qp1", "hbls", "hbbl") if cfg.nonlin_eos else ("rho",)):
        S[n] = o.field(n).copy()
    S["cfg"] = cfg
    return S


def run_twice(o, r, stage, get):
    """The reference stage on the oracle's present state with the scratch filled with each of FILLS:
    (results of the first run, {name: mask of the elements that follow the fill})."""
    runs = []
    for v in FILLS:
        r.load(o)
        r.iso_fill(v)
        for call in stage:
            r.iso_call(call)
        runs.append(get())
    return runs[0], {n: differ(runs[0][n], runs[1][n]) for n in runs[0]}


def ocean(r, names):
    out = r.ocean()
    return {n: out[n] for n in names}


def compare(o, got, skip=None):
    bad = {}
    for n, a in got.items():
        d = differ(a, o.field(n))
        if skip is not None and n in skip:
            d &= ~skip[n]
        if d.any():
            bad[n] = (int(d.sum()), where(d))
    assert not bad, bad


def to_prsgrd(variant):
    return setup(variant)


def to_uv2(variant):
    cfg, o, r, snap = setup(variant)
    o.call("prsgrd")
    return cfg, o, r, snap


def to_t(variant):
    cfg, o, r, snap = to_uv2(variant)
    o.call("step3d_uv2")
    return cfg, o, r, snap


def test_libraries():
    """Sizes, open sides, periodicity, EOS and boundary layers are what the tests assume; across the four basin
    libraries every side is open (LapT copied) and closed (LapT zeroed), every corner lies between two open and
    between two closed sides, and the south-west and north-east corners between one of each, either way round."""
    opened = {s: set() for s in bs.SIDES}
    kinds = {}
    for v in ref.ISO_VARIANTS:
        assert ref.available(v)
        r = ref.RefLib(v)
        assert r.obc == ref.ISO[v] and r.per == ((v == "isoper"),) * 2
        assert r.split_eos == r.kpp == (v != "isoper")
        if v != "isoper":
            for s in bs.SIDES:
                opened[s].add(bool(r.obc & bs.OPEN[s]))
            for ew, ns in (("west", "south"), ("east", "south"), ("west", "north"), ("east", "north")):
                kinds.setdefault((ew, ns), set()).add((bool(r.obc & bs.OPEN[ew]), bool(r.obc & bs.OPEN[ns])))
    assert all(k == {True, False} for k in opened.values()), opened
    assert all({(True, True), (False, False)} <= k for k in kinds.values()), kinds
    every = {(True, True), (True, False), (False, True), (False, False)}
    assert kinds[("west", "south")] == every and kinds[("east", "north")] == every, kinds


@pytest.mark.parametrize("variant", ref.ISO_VARIANTS)
def test_state_conditions(variant):
    """The four conditions on the state: land on and beside every edge, the flat point is water, f = 0 around it,
    the inputs are finite, and the metrics differ cell by cell (the rough planes)."""
    cfg, o, r, snap = setup(variant)
    L, M = cfg.LLm, cfg.MMm
    rm = snap["rmask"][0]
    I = rm[2:M + 2, 2:L + 2]
    assert (I[:, 0] == 0).any() and (I[:, -1] == 0).any() and (I[0] == 0).any() and (I[-1] == 0).any()
    assert (I[:, 1] == 0).any() and (I[:, -2] == 0).any() and (I[1] == 0).any() and (I[-2] == 0).any()
    ic, jc = bs.iso_flat_point(L, M)
    assert rm[jc + 1, ic + 1] == 1.0 and snap["f"][0][jc + 1, ic + 1] == 0.0
    iu, ju = bs.iso_unstable_point(L, M)
    assert rm[ju + 1, iu + 1] == 1.0 and snap["f"][0][ju + 1, iu + 1] != 0.0
    assert all(np.isfinite(a).all() for a in snap.values())
    for n in ("pm", "pn"):
        a = snap[n][0][2:M + 2, 2:L + 2]
        assert (a[:, 1:] != a[:, :-1]).all() and (a[1:] != a[:-1]).all()


@pytest.mark.parametrize("variant", ref.ISO_VARIANTS)
def test_prsgrd_slopes(variant):
    """The corrector prsgrd: dRdx, dRde, whole arrays, outside the cells the reference leaves undefined -- and that
    set is exactly the two edge rows of each on non-periodic edges."""
    cfg, o, r, snap = to_prsgrd(variant)
    L, M, N = cfg.LLm, cfg.MMm, cfg.N
    stage = (ref.ISO_PRSGRD, ref.ISO_EXCH_SLOPES)      # the exchange is step3d_uv1's (step3d_uv1.F:529-532)
    got, undefined = run_twice(o, r, stage, lambda: {n: r.iso_get(n) for n in ("dRdx", "dRde")})
    want = {n: np.zeros((N, M + 4, L + 4), dtype=bool) for n in got}
    if variant != "isoper":
        want["dRdx"][:, 2:M + 2, [2, L + 2]] = True          # i = istr, iend+1; j = jstr..jend
        want["dRde"][:, [2, M + 2], 2:L + 2] = True          # j = jstr, jend+1; i = istr..iend
    for n in got:
        extra, missing = undefined[n] & ~want[n], want[n] & ~undefined[n]
        assert not extra.any() and not missing.any(), (n, "further undefined", where(extra), "defined after all", where(missing))
    o.call("prsgrd")
    compare(o, got, skip=undefined)
    for n in got:
        assert differ(got[n], snap[n]).any() and np.isfinite(o.field(n)).all(), n


@pytest.mark.parametrize("variant", ref.ISO_VARIANTS)
def test_step3d_uv2(variant):
    """step3d_uv2 from the oracle's slopes: diff3u, diff3v, idRz and u, v, FlxU, FlxV, ubar, vbar, whole arrays."""
    cfg, o, r, snap = to_uv2(variant)
    bs.iso_shares(bs.iso_limiter_arms(inputs(o, cfg)), ("step3d_uv2", variant))
    names3 = ("diff3u", "diff3v", "idRz", "FlxU", "FlxV")

    def get():
        out = {n: r.iso_get(n) for n in names3}
        out.update(ocean(r, ("u", "v", "ubar", "vbar")))
        return out
    got, undefined = run_twice(o, r, (ref.ISO_UV2,), get)
    assert not any(m.any() for m in undefined.values()), {n: where(m) for n, m in undefined.items() if m.any()}
    o.call("step3d_uv2")
    compare(o, got)
    I = bs.box(cfg)
    for n in ("diff3u", "diff3v", "idRz"):
        assert np.isfinite(got[n]).all() and (got[n][I] > 0.).any() and differ(got[n], snap[n]).any(), n
    ic, jc = bs.iso_flat_point(cfg.LLm, cfg.MMm)
    assert (got["idRz"][1:cfg.N, jc + 1, ic + 1] > 1.0e30).all()          # epsil in the denominator


@pytest.mark.parametrize("variant", ref.ISO_VARIANTS)
def test_step3d_t(variant):
    """step3d_t from the oracle's five arrays: t(nnew) of both tracers (every time level and ghost row of t is
    compared) and Akz where the routine writes it."""
    cfg, o, r, snap = to_t(variant)
    L, M, N = cfg.LLm, cfg.MMm, cfg.N
    bs.iso_shares(bs.iso_operator_arms(inputs(o, cfg)), ("step3d_t", variant))
    before = o.field("t").copy()
    got, undefined = run_twice(o, r, (ref.ISO_T,), lambda: dict(ocean(r, ("t",)), Akz=r.iso_get("Akz")))
    assert not undefined["t"].any(), where(undefined["t"])
    written = np.zeros((N + 1, M + 4, L + 4), dtype=bool)
    written[1:N, 2:M + 2, 2:L + 2] = True
    extra, missing = ~undefined["Akz"] & ~written, undefined["Akz"] & written
    assert not extra.any() and not missing.any(), (where(extra), where(missing))
    o.call("step3d_t")
    compare(o, got, skip={"Akz": ~written})
    nnew = o.tindex()[5]
    t0, t1 = (a.reshape(cfg.NT, 3, N, M + 4, L + 4)[:, nnew - 1] for a in (before, got["t"]))
    wet = snap["rmask"][0][2:M + 2, 2:L + 2] == 1.0
    moved = differ(t0, t1)[..., 2:M + 2, 2:L + 2]
    assert moved[..., wet].all()
    assert np.isfinite(got["t"]).all() and np.isfinite(got["Akz"][written]).all()
    assert (got["Akz"][1:N, 2:M + 2, 2:L + 2] > 0.).mean() > 0.5
