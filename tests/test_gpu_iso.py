"""ADV_ISONEUTRAL on the device: every intermediate of the operator, whole arrays, at the sizes that switch a path.

tests/test_ref_pin_iso.py pins the oracle's three ISO routines to the reference's own, bit for bit.  Here the HIP
kernels (k_iso.hip, the corrector k_prsgrd, k_step3d_uv2 and k_step3d_t_v<.., true>) are held to both, stage by
stage: prsgrd -> dRdx, dRde; step3d_uv2 -> diff3u, diff3v, idRz; step3d_t -> Akz, t(nnew), each stage from the same
inputs copied in (the six arrays travel through the field ids ROMS_dRdx .. ROMS_Akz).

  * The six ISO arrays must equal the oracle's bit for bit, ghost rows included: sqrt, /, min, max are IEEE on both
    sides and k_iso.hip's header claims the oracle's bits.
  * What follows a column solve (t, u, v, ubar, vbar, FlxU, FlxV) is held to RTOL_ROUTINE of the field's maximum
    over the whole array, as everywhere else; the measured worst case is printed.
  * Against the reference's own routines (the libraries of oracle/ref, where present): the same six arrays bit for
    bit -- dRdx, dRde outside the cells the reference leaves undefined, Akz where the routine writes it -- and
    t whole, bit for bit as well; u, v, ubar, vbar, FlxU, FlxV within RTOL_ROUTINE.

The states: branch_states.iso_state at 24 x 20 x 6 for every library, with the arm shares asserted first; the same
builder at 40 x 16 with N = 2 (one interior w-level: k = 0, k < N and k = N in three consecutive passes), 3, 63
(the LDS column form at its 64 KiB limit), 64 and 88 (k_step3d_t_v<ColGlb, true>, at 88 beside the other routines'
segment solvers), the column path asserted; mid-run states at LLm = 62 .. 66 x 5 and 65 x 3, 4, 5 (N = 5), where the
64 x 4 tiles meet each launch's own origin; the coastline sweep's specks, channels and walls at 121 x 12; NT = 1
(no salinity, split EOS) and NT = 4.  Every one of these also runs whole steps against the oracle, and one of each
family 12 steps within RMS_RUN.  Decompositions 3 x 2 (uneven), 2 x 2 on the Filament and 2 x 1 on the open basin
equal the single domain bitwise from perturbed fields, the six arrays included.
"""
import functools

import numpy as np
import pytest

import branch_states as bs
import oracle
import oracle.ref as ref
import romsgpu
import test_ref_pin_iso as pin
from test_gpu_obc import full
from test_gpu_parity import PROGNOSTIC, RMS_RUN, RTOL_ROUTINE, check_fields, copy_state

pytestmark = pytest.mark.gpu

SIX = tuple(romsgpu.ISO_FIELDS)
STAGES = (("prsgrd", ("dRdx", "dRde")),
          ("step3d_uv2", ("diff3u", "diff3v", "idRz", "u", "v", "ubar", "vbar", "FlxU", "FlxV")),
          ("step3d_t", ("Akz", "t")))


def iso_model(cfg, **kw):
    """A model of cfg with every switch of it; asserts the column path by the depth sweep's rule: the segment
    solvers at N = 88 .. 104, global column scratch (k_step3d_t_v<ColGlb, true> under ISO, k_step3d_t.hip:813-816)
    from N = 64 up, the LDS form below."""
    per = cfg.case_id == oracle.CASE_FILAMENT
    m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex,
                                sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=False if per else bool(cfg.surf_flux),
                                obc=cfg.obc, v_sponge=cfg.v_sponge, island=bool(cfg.island),
                                curvgrid=bool(cfg.curvgrid), adv_isoneutral=bool(cfg.adv_isoneutral), **kw)
    got, want = m.column_path(), (88 <= cfg.N <= 104, cfg.N >= 64)
    if got != want:
        m.close()
        raise AssertionError("N = %d: column_path() = %s, expected %s" % (cfg.N, got, want))
    return m


def hand_over(o, m, tix):
    copy_state(o, m)
    for n in SIX:
        m.put(n, o.field(n))
    m.set_tindex(*tix, nfast=o.nfast())


def run_stages(o, m, tix, before=None):
    """The three routines on the oracle and on the device from the oracle's present state, every stage from the
    oracle's arrays: {routine: {name: (device array, oracle array)}}.  before(routine) runs ahead of each stage."""
    out = {}
    hand_over(o, m, tix)
    for routine, names in STAGES:
        if before is not None:
            before(routine)
        o.call(routine)
        getattr(m, routine)()
        m.sync()
        out[routine] = {n: (m.get(n), o.field(n).copy()) for n in names}
        for n in names:
            m.put(n, o.field(n))
    return out


def judge(tag, out):
    """The six arrays bitwise, the rest within RTOL_ROUTINE, whole arrays; every figure printed first."""
    bad = []
    for routine, res in out.items():
        for n, (a, b) in res.items():
            e, nd = full(a, b), int(pin.differ(a, b).sum())
            print("%s %s %s: %d of %d elements differ, max error / max %.3e" % (tag, routine, n, nd, a.size, e))
            assert np.isfinite(a).all(), (tag, routine, n)
            if (nd if n in SIX else not e <= RTOL_ROUTINE):
                bad.append((routine, n, nd, e, pin.where(pin.differ(a, b)) if a.ndim == 3 else None))
    assert not bad, (tag, bad)


def midrun_stages(o, m, cfg, tag):
    """Stage parity from the state the oracle holds after whole steps, at the corrector's indices."""
    tix = bs.set_mode(o, "corr")
    o.L.or_rho_eos(o.h, 3)
    judge(tag, run_stages(o, m, tix))


def whole_steps(cfg, tag, steps=1, prepare=None, stages=True):
    """One whole step within RTOL_ROUTINE of the oracle (interior, PROGNOSTIC), `steps` in all within RMS_RUN,
    then the three stages from the oracle's state.

    Where the segment solvers run (N = 88 .. 104) the routines upstream of the operator are not bit-exact (they
    are held to RTOL_ROUTINE, test_gpu_depths), and the operator is discontinuous in its inputs: SW_TRIADS divides
    by the number of slopes of the right sign, which jumps where a slope crosses zero.  One oracle step from t
    times (1 + 1e-16 * noise) moves t by 5e-9 of its maximum at 40 x 16 x 64 and x 88 with the switch, and by 1e-14
    without it (oracle against oracle, no device involved).  So t after a whole step is held to RTOL_ROUTINE, and
    the run to RMS_RUN, only where everything upstream is bit-exact.  At those depths every other field is held
    after one step and the operator by the stages, which are bitwise there from identical inputs; measured at
    40 x 16 x 88: t 2.5e-9 of its maximum after one step, RMS 1.8e-9 after three, inside what one ulp does to the
    oracle itself."""
    o = oracle.Oracle(cfg)
    o.init()
    m = iso_model(cfg)
    try:
        if prepare is not None:
            prepare(o, m)
        o.step(1)
        m.step(1)
        m.sync()
        e1 = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, float("inf"))
        # Wi to We's maximum, as the depth, width and coast sweeps hold it (test_gpu_depths.routine_errors): where
        # the Courant split leaves Wi zero it is cancellation noise of We
        I = (Ellipsis, slice(2, cfg.MMm + 2), slice(2, cfg.LLm + 2))
        e1["Wi"] = float(np.abs(m.get("Wi")[I] - o.field("Wi")[I]).max()) / max(float(np.abs(o.field("We")[I]).max()), 1e-300)
        print("%s one step, max relative error per field:" % tag, {k: "%.1e" % v for k, v in e1.items()})
        exact_upstream = not m.column_path()[0]
        bad = [(k, v) for k, v in e1.items() if not v <= RTOL_ROUTINE and (k != "t" or exact_upstream)]
        assert not bad, (tag, bad)
        if steps > 1 and exact_upstream:
            o.step(steps - 1)
            m.step(steps - 1)
            m.sync()
            er = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms")
            print("%s %d steps, RMS error per field:" % (tag, steps), {k: "%.1e" % v for k, v in er.items()})
        assert float(m.get("Akz").max()) > 0.0
        if stages:
            midrun_stages(o, m, cfg, tag)
    finally:
        m.close()


# ------------------------------------------------ iso_state, every library ----
@functools.lru_cache(maxsize=None)
def state_results(variant):
    """Oracle, device and (where the library is there) reference through the three stages on iso_state."""
    obc = "per" if variant == "isoper" else ref.ISO[variant]
    cfg, o, tix, snap = bs.iso_state(obc, **bs.ISO_SIZE)
    bs.iso_restore(o, snap, tix)
    have = ref.available(variant)
    r = ref.RefLib(variant) if have else None
    refs, shares = {}, {}
    calls = {"prsgrd": (ref.ISO_PRSGRD, ref.ISO_EXCH_SLOPES), "step3d_uv2": (ref.ISO_UV2,), "step3d_t": (ref.ISO_T,)}

    def before(routine):
        if routine == "step3d_uv2":
            shares[routine] = bs.iso_shares(bs.iso_limiter_arms(pin.inputs(o, cfg)), (routine, variant))
        if routine == "step3d_t":
            shares[routine] = bs.iso_shares(bs.iso_operator_arms(pin.inputs(o, cfg)), (routine, variant))
        if have:
            names = dict(STAGES)[routine]

            def get():
                oc = r.ocean()
                return {n: (r.iso_get(n) if n in ref.ISO_ARRAYS else oc[n]) for n in names}
            refs[routine] = pin.run_twice(o, r, calls[routine], get)

    m = iso_model(cfg)
    try:
        out = run_stages(o, m, tix, before)
    finally:
        m.close()
    return cfg, out, refs, shares


@pytest.mark.parametrize("variant", ref.ISO_VARIANTS)
def test_stage_parity_on_iso_state(variant):
    """Against the oracle, with the arm shares asserted from the arrays handed over."""
    cfg, out, refs, shares = state_results(variant)
    assert set(shares) == {"step3d_uv2", "step3d_t"}
    judge("iso_state %s" % variant, out)


@pytest.mark.parametrize("variant", ref.ISO_VARIANTS)
def test_kernels_against_reference_routines(variant):
    """Against the reference's own prsgrd, step3d_uv2 and step3d_t."""
    if not ref.available(variant):
        pytest.skip("no oracle/_ref library for %s" % variant)
    cfg, out, refs, shares = state_results(variant)
    L, M, N = cfg.LLm, cfg.MMm, cfg.N
    written = np.zeros((N + 1, M + 4, L + 4), dtype=bool)
    written[1:N, 2:M + 2, 2:L + 2] = True
    bad = []
    for routine, names in STAGES:
        got, undefined = refs[routine]
        for n in names:
            a = out[routine][n][0]
            d = pin.differ(a, got[n])
            skip = ~written if n == "Akz" else undefined[n]
            nd, e = int((d & ~skip).sum()), float(np.abs(np.where(skip, 0.0, a - got[n])).max()) / float(np.abs(got[n][~skip]).max())
            print("reference %s %s %s: %d elements differ, max error / max %.3e" % (variant, routine, n, nd, e))
            if (nd if n in SIX + ("t",) else not e <= RTOL_ROUTINE):
                bad.append((routine, n, nd, e))
    assert not bad, (variant, bad)


# ------------------------------------------------------------------ depths ----
DEPTHS = {2: "one interior w-level", 3: "the depth sweep's shallowest", 63: "LDS columns at the 64 KiB limit",
          64: "k_step3d_t_v<ColGlb, true>", 88: "ColGlb under ISO beside the other routines' segment solvers"}


@pytest.mark.parametrize("N", list(DEPTHS))
def test_depths(N):
    """iso_state at 40 x 16 x N through the three stages, and whole steps at that depth; iso_model asserts that
    the column scratch is global (the <ColGlb, true> form) at 64 and 88 and in LDS at 2, 3 and 63."""
    cfg, o, tix, snap = bs.iso_state(0, 40, 16, N)
    bs.iso_restore(o, snap, tix)
    m = iso_model(cfg)
    try:
        assert m.column_path() == (N == 88, N >= 64)
        judge("depth %d" % N, run_stages(o, m, tix))
    finally:
        m.close()
    whole_steps(bs.iso_cfg(0, 40, 16, N), "depth %d" % N, steps=12 if N == 64 else 3)


# ------------------------------------------------------ widths and heights ----
SIZES = [(L, 5) for L in (62, 63, 64, 65, 66)] + [(65, M) for M in (3, 4)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_widths_and_heights(size):
    whole_steps(bs.iso_cfg(0, size[0], size[1], 5), "size %dx%dx5" % size, steps=12 if size == (65, 5) else 3)


# ------------------------------------------------------------------ coasts ----
@pytest.mark.parametrize("name", ["specks", "channels", "walls"])
def test_coasts(name):
    import coasts
    from test_gpu_coasts import coast_cfg, coast_model
    size = (121, 12, 12)
    cfg = coast_cfg(size)
    cfg.adv_isoneutral = 1
    o = oracle.Oracle(cfg)
    o.init()
    m = coast_model(cfg, size)
    try:
        coasts.apply_coast(o, m, coasts.COASTS[name](size[0], size[1]), coasts.VISC)
        steps = 12 if name == "walls" else 3
        o.step(steps)
        m.step(steps)
        m.sync()
        er = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms")
        print("coast %s %d steps, RMS error per field:" % (name, steps), {k: "%.1e" % v for k, v in er.items()})
        assert float(m.get("Akz").max()) > 0.0
        midrun_stages(o, m, cfg, "coast %s" % name)
    finally:
        m.close()


# ----------------------------------------------------------- tracer counts ----
@pytest.mark.parametrize("NT", [1, 4])
def test_tracer_counts(NT):
    """NT = 1: no salinity under the split EOS; NT = 4: two passive tracers behind T and S, given T's and S's
    fields scaled so that every tracer differs.  t is compared whole, every tracer."""
    def prepare(o, m):
        t = o.field("t").reshape(NT, 3, -1)
        for q in range(2, NT):
            t[q] = (0.5 + 0.25 * q) * t[q - 2]
        m.put("t", o.field("t"))
    whole_steps(bs.iso_cfg(0, 40, 16, 6, NT=NT), "NT %d" % NT, steps=12 if NT == 4 else 3, prepare=prepare)


# ---------------------------------------------------------- decompositions ----
def _rough_start(case):
    """setup(model) for check_decomposition: seeded noise, drawn on the whole grid and cut to the rank's window,
    on t (1 % of its range), u and v, so that after a step the slopes, idRz, diff3u and diff3v differ across
    every rank edge."""
    rng = np.random.default_rng(41)
    ny2, nx2 = case["MMm"] + 4, case["LLm"] + 4
    z = {n: rng.standard_normal((lev, ny2, nx2)) for n, lev in
         (("t", 3 * case["N"] * case["NT"]), ("u", 3 * case["N"]), ("v", 3 * case["N"]))}
    if case["case_id"] == 0:
        import metrics
        for a in z.values():
            for plane in a:
                metrics.wrap(plane, (True, True))

    def setup(m):
        from test_gpu_multirank import window
        for n, amp in (("t", 0.02), ("u", 0.02), ("v", 0.02)):
            a = m.get(n)
            mask = m.get({"t": "rmask", "u": "umask", "v": "vmask"}[n])
            m.put(n, a + amp * window(z[n], m.iSW, m.jSW, m.Lm, m.Mm) * mask)
    return setup


DECOMPOSITIONS = {
    "basin-3x2": (dict(case_id=1, LLm=38, MMm=27, N=6, NT=2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30,
                       sizex=114e3, sizey=81e3, lmd=bs.ISO_LMD, surf_flux=True, adv_isoneutral=True), 3, 2),
    "filament-2x2": (dict(case_id=0, LLm=40, MMm=30, N=6, NT=1, salinity=False, nonlin_eos=False, dt=5.0, ndtfast=60,
                          sizex=8.0e3, sizey=1.5e3, adv_isoneutral=True), 2, 2),
    "open-basin-2x1": (dict(case_id=1, LLm=36, MMm=20, N=6, NT=2, salinity=True, nonlin_eos=True, dt=60.0, ndtfast=30,
                            sizex=108e3, sizey=60e3, lmd=bs.ISO_LMD, surf_flux=True, obc=15, adv_isoneutral=True), 2, 1),
}


@pytest.mark.parametrize("name", list(DECOMPOSITIONS))
def test_decompositions_bitwise(name):
    from test_gpu_multirank import FIELDS, check_decomposition
    case, npx, npe = DECOMPOSITIONS[name]
    check_decomposition(case, npx, npe, nsteps=3, fields=FIELDS + SIX, setup=_rough_start(case))


# ------------------------------------------------------------ the field ids ----
def test_iso_fields_refused_without_the_switch():
    cfg = bs.iso_cfg(0, 24, 20, 6)
    cfg.adv_isoneutral = 0
    m = iso_model(cfg)
    try:
        for n in SIX:
            assert m.L.roms_gpu_field_size(romsgpu.FIELD_ID[n]) == 0
            with pytest.raises(romsgpu.RomsGpuError):
                m.get(n)
            with pytest.raises((romsgpu.RomsGpuError, ValueError)):
                m.put(n, np.zeros((cfg.N, cfg.MMm + 4, cfg.LLm + 4)))
    finally:
        m.close()
