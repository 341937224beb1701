"""Depth sweep: GPU parity at every level count N that switches a column path.

The vertical level count selects the code path of almost every column
routine (roms_shim.cpp: colseg / col_global, roms_dev.h seg_count /
seg_rows_ok, k_chain.h chain_kl, k_vertical.hip k_omega_seg's own partition).
The other GPU tests run N = 4, 8, 10, 12, 16, 20, 32, 50 and 100; DEPTHS below
adds one depth on each side of every switch and the partitions nobody ran:
every segment at its minimum of 11 rows, every segment full (the last
segment's spline system then fills all KR = 14 register rows), mixed
partitions whose remainder split ends on a short segment, the chain kernels'
partitions with empty top lanes, and the sequential solvers' automatic
choice of global column scratch.

Case: the closed split-EOS basin with KPP and surface fluxes on 40 x 16
columns (>= 32 wide, so omega takes k_omega_seg; not a multiple of 16, so the
last 16-column block is partial).  Each routine is compared with the CPU
oracle on one mid-run state whose Akv, Akt and Wi are perturbed as in
test_gpu_colseg.test_seg_routine_parity (every implicit row then has
distinct, non-zero coefficients), within RTOL_ROUTINE; 12 whole steps within
RMS_RUN.  Every model asserts the path it took through Model.column_path().

What the sweep catches, tried in a scratch copy of k_colseg.h: seg_span's
remainder split giving one segment a row too few fails N = 21, 47, 53, 63,
87, 93 and 101 (every partition with a non-zero remainder); spline_fc_seg's
ns capped at KR - 1 fails exactly N = 52 (forced) and N = 104.  (fc[KR-1]
itself, interface N of a full last segment, is dead: the vertical fluxes at
the surface are set to zero, so a wrong value there changes nothing.)
All depths passed as the library stood; measured errors: DESIGN.md section 4.
"""
import functools
import os

import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_colseg import make_model
from test_gpu_lmd import LMD_OUT
from test_gpu_parity import (PROGNOSTIC, RMS_RUN, ROUTINE_CASES, RTOL_ROUTINE, basin_cfg, check_fields, copy_state,
                             interior, relerr)

pytestmark = pytest.mark.gpu

LLM, MMM = 40, 16

# N -> the paths it selects with the default build constants (kSegRows 13,
# kSegMaxS 8, kSegCW 16, kSegNMin 11, kChainG 4).  "omega" is k_omega_seg's
# partition: 64-column blocks of ceil(N/13) segments up to N = 63, 16-column
# blocks of a multiple of four segments above.  "chain" is the levels per
# lane of set_HUV1 / step3d_uv2's four-lane columns.
DEPTHS = {
    3: "sequential LDS; omega one segment of 3 of its 13 rows; chain KL 5: 3/0/0/0",
    5: "sequential LDS; omega one segment; chain KL 5 with three empty lanes: 5/0/0/0",
    21: "sequential LDS; omega 2 segments 11/10; first chain KL 13, two empty lanes: 13/8/0/0",
    44: "forced: 4 segments of kSegNMin = 11 rows; default sequential LDS; omega 4 x 11",
    47: "forced: 12/12/12/11, the last segment a short one; default sequential LDS",
    52: "forced: 4 segments of 13 rows, last spline system ns = 14 = KR; last chain KL 13, full lanes",
    53: "sequential LDS (segments need 8 x 11 rows); omega 5 segments; first chain KL 25, one empty lane: 25/25/3/0",
    63: "sequential LDS at exactly 64 KiB of dynamic LDS (no raised limit); omega 5 segments 13/13/13/12/12",
    64: "first depth on global column scratch (ColGlb), chosen automatically; omega 8 segments of 8 on 16-column blocks",
    87: "last depth before the segments: ColGlb; omega 8 segments 11 x 7 / 10",
    88: "8 segments of kSegNMin = 11 rows (default)",
    93: "8 segments 12 x 5 / 11 x 3 (default)",
    101: "8 segments 13 x 5 / 12 x 3 without chains: k_set_huv1, unfused step3d_uv2",
    104: "8 segments of 13 rows, last spline system ns = 14 = KR; last depth of omega's segment form",
    105: "past every special path: ColGlb, two-pass k_omega, no chains",
}
FORCED = (44, 47, 52)   # also run with ROMS_GPU_COLSEG=1
CASES = [pytest.param(N, forced, id="%d%s" % (N, "-colseg" if forced else ""))
         for N in DEPTHS for forced in ((False, True) if N in FORCED else (False,))]


def depth_cfg(N):
    c = basin_cfg(nonlin=True, LLm=LLM, MMm=MMM, N=N)
    c.lmd, c.surf_flux = oracle.LMD_ALL, 1
    return c


def depth_model(cfg, forced=False, col_global=None):
    """A model of cfg with ROMS_GPU_COLSEG=1 (forced) or unset, and
    ROMS_GPU_COL_GLOBAL as given or unset; asserts the column path the
    library reports against the dispatch rule for cfg.N."""
    keep = {k: os.environ.pop(k, None) for k in ("ROMS_GPU_COLSEG", "ROMS_GPU_COL_GLOBAL")}
    try:
        if col_global is not None:
            os.environ["ROMS_GPU_COL_GLOBAL"] = str(int(col_global))
        if forced:
            m = make_model(cfg, 1)
        else:
            m = romsgpu.Model.from_case(cfg.case_id, cfg.LLm, cfg.MMm, cfg.N, cfg.NT, salinity=bool(cfg.salinity),
                                        nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast,
                                        sizex=cfg.sizex, sizey=cfg.sizey, lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux))
    finally:
        os.environ.pop("ROMS_GPU_COL_GLOBAL", None)
        for k, v in keep.items():
            if v is not None:
                os.environ[k] = v
    N = cfg.N
    seg, glb = m.column_path()
    want_seg = 88 <= N <= 104 or (forced and 44 <= N <= 52)
    want_glb = N >= 64 if col_global is None else bool(col_global)
    if (seg, glb) != (want_seg, want_glb):
        m.close()
        raise AssertionError("N = %d%s: column_path() = (segments %s, global scratch %s), expected (%s, %s)"
                             % (N, " forced" if forced else "", seg, glb, want_seg, want_glb))
    return m


def routine_list(cfg):
    """(id, routine, mode, outputs): test_gpu_parity's ROUTINE_CASES and, with
    KPP on, lmd_vmix at both time indices (test_gpu_lmd)."""
    out = []
    for name, mode, outs in ROUTINE_CASES:
        if name == "rho_eos" and cfg.nonlin_eos:
            outs = ["rho1", "qp1", "rhoA", "rhoS"]
        out.append((name, name, mode, outs))
    if cfg.lmd:
        out.append(("lmd_vmix_nstp", "lmd_vmix", None, LMD_OUT))
        out.append(("lmd_vmix_nrhs", "lmd_vmix", "corr", LMD_OUT))
    return out


_ROUTINE_CASE = {}   # one entry: the configuration last asked for


def routine_case(cfg, setup=None, tag=b""):
    """The oracle of configuration cfg after 3 steps with perturbed mixing and
    implicit fluxes, a copy of its whole state, and the per-routine reference
    outputs (filled on first use, shared by every model of the same
    configuration that follows: the default and the forced one).  setup(o)
    runs between init and the steps; tag tells its states from the plain one."""
    key = bytes(cfg) + tag
    if key in _ROUTINE_CASE:
        return _ROUTINE_CASE[key]
    o = oracle.Oracle(cfg)
    o.init()
    if setup is not None:
        setup(o)
    o.step(3)
    rng = np.random.default_rng(11)
    for name in ("Akv", "Akt"):
        a = o.field(name)
        a[...] = a * (1.0 + 0.5 * rng.random(a.shape))
    we, wi = o.field("We"), o.field("Wi")
    wi[...] = wi + 0.01 * float(np.abs(we).max()) * rng.standard_normal(wi.shape)
    snap = {n: o.field(n).copy() for n in romsgpu.FIELDS}
    _ROUTINE_CASE.clear()
    _ROUTINE_CASE[key] = cfg, o, snap, o.tindex(), {}
    return _ROUTINE_CASE[key]


def routine_errors(cfg, m, only=None, setup=None, tag=b""):
    """Every routine on the same state of configuration cfg, oracle and GPU:
    {(id, field): error} relative to the field's interior maximum (Wi: to
    We's, as in test_gpu_colseg.test_omega_blocks -- where the Courant split
    leaves Wi zero it is cancellation noise)."""
    cfg, o, snap, tix, refs = routine_case(cfg, setup, tag)
    iic, kstp, knew, nstp = tix[:4]
    errs = {}
    for rid, routine, mode, outs in routine_list(cfg):
        if only is not None and rid not in only:
            continue
        nrhs, nnew = (3, 3 - nstp) if mode == "corr" else (nstp, 3)
        for n, a in snap.items():
            o.field(n)[...] = a
        o.set_tindex([iic, kstp, knew, nstp, nrhs, nnew])
        copy_state(o, m)
        m.set_tindex(iic, kstp, knew, nstp, nrhs, nnew, nfast=o.nfast())
        if rid not in refs:
            if routine in ("rho_eos", "lmd_vmix"):
                o.call(routine, nrhs)
            else:
                o.call(routine)
            refs[rid] = {f: interior(o.field(f), cfg.LLm, cfg.MMm).copy() for f in set(outs) | {"We"}}
        if routine in ("rho_eos", "lmd_vmix"):
            getattr(m, routine)(nrhs)
        else:
            getattr(m, routine)()
        m.sync()
        for f in outs:
            a, ref = interior(m.get(f), cfg.LLm, cfg.MMm), refs[rid][f]
            if f == "Wi":
                e = float(np.abs(a - ref).max()) / float(np.abs(refs[rid]["We"]).max())
            else:
                e = relerr(a, ref)
            errs[rid, f] = float(e)
    return errs


@pytest.mark.parametrize("N,forced", CASES)
def test_depth_routine_parity(N, forced):
    """Each routine at depth N within RTOL_ROUTINE of the oracle (DEPTHS[N]
    names the paths); every failing (routine, field, error) is reported at once."""
    cfg = depth_cfg(N)
    m = depth_model(cfg, forced)
    try:
        errs = routine_errors(cfg, m)
    finally:
        m.close()
    for (rid, f), e in errs.items():
        print("N=%d%s %s %s %.3e" % (N, " colseg" if forced else "", rid, f, e))
    bad = [(rid, f, e) for (rid, f), e in errs.items() if not e <= RTOL_ROUTINE]
    assert not bad, (N, DEPTHS[N], bad)


@functools.lru_cache(maxsize=1)
def run_ref(N):
    cfg = depth_cfg(N)
    o = oracle.Oracle(cfg)
    o.init()
    o.step(12)
    return cfg, o


@pytest.mark.parametrize("N,forced", CASES)
def test_depth_run_rms(N, forced):
    """12 whole steps at depth N: field RMS against the oracle below RMS_RUN."""
    cfg, o = run_ref(N)
    m = depth_model(cfg, forced)
    try:
        m.step(12)
        m.sync()
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC, cfg.LLm, cfg.MMm, RMS_RUN, kind="rms")
    finally:
        m.close()
    print("N=%d%s" % (N, " colseg" if forced else ""), {k: "%.2e" % v for k, v in errs.items()})


@pytest.mark.parametrize("N,col_global", [(63, True), (64, False)])
def test_column_scratch_forms_bitwise(N, col_global):
    """The sequential column solvers are one set of templates over their
    scratch columns, in LDS (ColLds) or in global memory (ColGlb):
    ROMS_GPU_COL_GLOBAL=1 at N = 63 (the deepest grid whose two LDS columns
    fit the default 64 KiB) and =0 at N = 64 (the first that needs the raised
    LDS limit) give the bits of the default choice over 6 whole steps."""
    cfg = depth_cfg(N)
    out = []
    for cg in (None, col_global):
        m = depth_model(cfg, col_global=cg)
        try:
            m.step(6)
            out.append({n: m.get(n) for n in ("zeta", "ubar", "vbar", "u", "v", "t", "rufrc", "rvfrc", "Akv", "Akt")})
        finally:
            m.close()
    for n in out[0]:
        assert np.array_equal(out[0][n], out[1][n]), (N, n)
