"""Stores a whole step leaves out (ROMS_GPU_LEAN_ST, roms_gpu_lean_stores)
against every store (ROMS_GPU_LEAN_ST=0): bitwise equal fields.

Bit 1: the predictor's u, v(indx) = Hz*u(nstp).  On the buffer segment path
k_pre_uv_segb<false> neither keeps them in LDS nor stores them, and
k_uv1_segb<true>, their one reader in a step, forms each row's value again
from its LDS Hz pair and u(nstp) with the predictor's expression.
Bit 2: Akt(isalt).  Where it is Akt(itemp) bit for bit and the step's tracer
solvers are the pair kernels, k_kpp_int runs without the Ks chain and stores
and exchanges one slot; the library copies slot 1 over slot 2 before anything
reads it.  Covered:
  * whole steps on the smallest shapes that reach the segment path with
    16-column blocks -- 21x9x88 (a partial block in i, 11 rows per segment),
    21x9x104 (13 rows), 40x32x100 (several blocks both ways, 12/13 rows) --
    four steps from the analytic start: the eager first step (cf_bak = 0),
    graph capture, both nstp parities; masks 1, 2, 3 against 0 on every field
    m.get returns, all time slots of u, v and both slots of Akt among them;
    the launch counts say each store was left out with its bit on and never
    with it off;
  * the same under ROMS_GPU_GUARD=1 (NaN bands around every array: an access
    of the changed kernels outside an array's extent shows);
  * the routine entries: after whole steps with mask 3, pre_step3d called on
    its own still leaves u, v(indx) = Hz*u(nstp), and it and step3d_uv1 give
    the fields of mask 0;
  * Akt: after whole steps slot 2 reads as slot 1 and as mask 0's; a host
    write of an Akt whose slots differ is what a routine-level pre_step3d and
    step3d_t then see; the next whole step leaves the store out again;
  * Akt(isalt) is never left out with LMD_DDMIX, unequal backgrounds, one
    tracer, or ROMS_GPU_T_PAIR = 0, 1, 2;
  * calc_avg of AKt and AKs over two samples, a history record of both, a
    restart record, and a registered download of Akt;
  * a 2x1 decomposed run on one GPU: every rank's fields, halos and both Akt
    slots included.
"""
import ctypes

import numpy as np
import pytest

import oracle
import romsgpu
from test_ddmix import ddmix_cfg
from test_gpu_io import read
from test_gpu_lmd import lmd_basin_cfg
from test_gpu_multirank import run_decomposed
from test_gpu_register import host_model

pytestmark = pytest.mark.gpu

SHAPES = [(21, 9, 88), (21, 9, 104), (40, 32, 100)]
NSTEPS = 4


def _case_of(c):
    return dict(case_id=c.case_id, LLm=c.LLm, MMm=c.MMm, N=c.N, NT=c.NT, salinity=bool(c.salinity),
                nonlin_eos=bool(c.nonlin_eos), dt=c.dt, ndtfast=c.ndtfast, sizex=c.sizex, sizey=c.sizey, lmd=c.lmd,
                surf_flux=bool(c.surf_flux))


def _case(LLm, MMm, N):
    return _case_of(lmd_basin_cfg(surf_flux=1, LLm=LLm, MMm=MMm, N=N))


def _model(case, monkeypatch, mask):
    monkeypatch.setenv("ROMS_GPU_LEAN_ST", str(mask))
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")   # whole steps keep Hz_u, Hz_v: every field can be read
    m = romsgpu.Model.from_case(**case)
    assert m.column_path()[0]   # the segment solvers
    assert m.lean_stores() == (mask, (0, 0))
    return m


def _all_fields(m):
    return {n: m.get(n) for n in romsgpu.FIELDS}


def _assert_same(a, b, tag):
    diff = [n for n in a if not np.array_equal(a[n], b[n])]
    assert not diff, (tag, diff)


def _counts_ok(mask, n, steps):
    """The first step and one capture per nstp parity at least (lmd_vmix runs twice a step); never with the bit off."""
    uv = n[0] >= min(steps, 3) if mask & 1 else n[0] == 0
    akt = n[1] >= 2 * min(steps, 3) if mask & 2 else n[1] == 0
    return uv and akt


def _save_t(m):
    return romsgpu.Tlev.from_buffer_copy(m.t)


def _restore_t(m, saved):
    ctypes.memmove(ctypes.byref(m.t), ctypes.byref(saved), ctypes.sizeof(saved))


def _whole_steps(case, monkeypatch):
    outs = {}
    for mask in (0, 1, 2, 3):
        m = _model(case, monkeypatch, mask)
        m.step(NSTEPS)
        m.sync()
        got, n = m.lean_stores()
        assert got == mask and _counts_ok(mask, n, NSTEPS), (mask, n)
        outs[mask] = _all_fields(m)
        assert m.lean_stores() == (got, n)   # reading changes no count
        m.close()
    N = case["N"]
    assert outs[0]["u"].shape[0] == 3 * N and outs[0]["Akt"].shape[0] == 2 * (N + 1)   # every slot is compared
    assert np.all(np.isfinite(outs[0]["u"])) and np.any(outs[0]["u"] != 0.0)
    assert np.any(outs[0]["Akt"][N + 1:] != 0.0)
    for mask in (1, 2, 3):
        _assert_same(outs[0], outs[mask], "mask %d" % mask)


@pytest.mark.parametrize("LLm,MMm,N", SHAPES)
def test_whole_steps_bitwise(LLm, MMm, N, monkeypatch):
    _whole_steps(_case(LLm, MMm, N), monkeypatch)


@pytest.mark.parametrize("LLm,MMm,N", SHAPES)
def test_whole_steps_bitwise_guard(LLm, MMm, N, monkeypatch):
    monkeypatch.setenv("ROMS_GPU_GUARD", "1")
    _whole_steps(_case(LLm, MMm, N), monkeypatch)


@pytest.mark.parametrize("LLm,MMm,N", [(21, 9, 88), (40, 32, 100)])
def test_routine_entries_store_and_load(LLm, MMm, N, monkeypatch):
    case = _case(LLm, MMm, N)
    outs = []
    for mask in (0, 3):
        m = _model(case, monkeypatch, mask)
        m.step(NSTEPS)
        nstp, indx = m.t.nstp, 3 - m.t.nstp
        m.t.nrhs, m.t.nnew = nstp, 3   # the predictor's indices
        skipped = m.lean_stores()[1]
        m.pre_step3d()
        m.sync()
        assert m.lean_stores()[1] == skipped   # the routine stores
        pre = _all_fields(m)
        hz = pre["Hz"]
        u, v = pre["u"], pre["v"]
        # u(indx) = 0.5*(Hz(i) + Hz(i-1))*u(nstp) at i = 2..Lm, j = 1..Mm (array index i + 1, j + 1);
        # v(indx) with Hz(j-1) at i = 1..Lm, j = 2..Mm: the predictor's expression and order
        ju, iu = slice(2, MMm + 2), slice(3, LLm + 2)
        want_u = 0.5 * (hz[:, ju, iu] + hz[:, ju, 2:LLm + 1]) * u[(nstp - 1) * N:nstp * N, ju, iu]
        assert np.array_equal(u[(indx - 1) * N:indx * N, ju, iu], want_u)
        jv, iv = slice(3, MMm + 2), slice(2, LLm + 2)
        want_v = 0.5 * (hz[:, jv, iv] + hz[:, 2:MMm + 1, iv]) * v[(nstp - 1) * N:nstp * N, jv, iv]
        assert np.array_equal(v[(indx - 1) * N:indx * N, jv, iv], want_v)
        m.t.nrhs, m.t.nnew = 3, indx   # the corrector's
        m.step3d_uv1()
        m.sync()
        assert m.lean_stores()[1] == skipped
        outs.append((pre, _all_fields(m)))
        m.close()
    _assert_same(outs[0][0], outs[1][0], "pre_step3d")
    _assert_same(outs[0][1], outs[1][1], "step3d_uv1")
    assert not np.array_equal(outs[0][0]["u"], outs[0][1]["u"])


def test_akt_read_host_write_and_next_step(monkeypatch):
    LLm, MMm, N = 21, 9, 100
    case = _case(LLm, MMm, N)
    monkeypatch.setenv("ROMS_GPU_NO_GRAPH", "1")   # eager steps: every launch is counted, none replayed
    outs = []
    for mask in (0, 3):
        m = _model(case, monkeypatch, mask)
        m.step(NSTEPS)
        assert m.lean_stores()[1] == ((NSTEPS, 2 * NSTEPS) if mask else (0, 0))
        akt = m.get("Akt")
        assert np.array_equal(akt[N + 1:], akt[:N + 1]) and np.any(akt[:N + 1] != 0.0)
        saved = _save_t(m)
        host = akt.copy()
        host[N + 1:] = 2.0 * akt[:N + 1]   # slots that differ
        m.put("Akt", host)
        nstp, n0 = m.t.nstp, m.lean_stores()[1]
        m.t.nrhs, m.t.nnew = nstp, 3
        m.pre_step3d()
        m.t.nrhs, m.t.nnew = 3, 3 - nstp
        m.step3d_t()
        m.sync()
        routines = _all_fields(m)
        assert np.array_equal(routines["Akt"], host)   # the host's Akt is what they saw and what stays
        assert m.lean_stores()[1] == n0
        _restore_t(m, saved)
        m.step(1)
        m.sync()
        n1 = m.lean_stores()[1]
        assert n1[1] == (n0[1] + 2 if mask & 2 else 0) and n1[0] == (n0[0] + 1 if mask & 1 else 0), (n0, n1)
        outs.append((akt, routines, _all_fields(m)))
        m.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    _assert_same(outs[0][1], outs[1][1], "routines on the host's Akt")
    _assert_same(outs[0][2], outs[1][2], "the next whole step")
    t0 = outs[0][1]["t"]
    assert np.all(np.isfinite(t0)) and np.all(np.isfinite(outs[0][2]["t"]))


def _never(m, steps=3):
    m.step(steps)
    m.sync()
    mask, n = m.lean_stores()
    assert mask == 3 and n[1] == 0, n
    return n


def test_akt_kept_with_ddmix(monkeypatch):
    m = _model(_case_of(ddmix_cfg(LLm=21, MMm=9, N=100)), monkeypatch, 3)
    assert _never(m)[0] >= 3   # bit 1 does not depend on it
    m.close()


def test_akt_kept_with_unequal_backgrounds(monkeypatch):
    monkeypatch.setenv("ROMS_GPU_LEAN_ST", "3")
    cfg = lmd_basin_cfg(surf_flux=1, LLm=21, MMm=9, N=100)
    cfg.Akt_bak[1] = 2.0e-5
    o = oracle.Oracle(cfg)
    o.init()
    m, host = host_model(o, cfg)
    _never(m)
    akt = m.get("Akt")[:, 2:-2, 2:-2]
    assert not np.array_equal(akt[cfg.N + 1:], akt[:cfg.N + 1])
    m.close()


def test_akt_kept_with_one_tracer(monkeypatch):
    case = _case(21, 9, 100)
    case.update(NT=1, salinity=False)
    m = _model(case, monkeypatch, 3)
    _never(m)
    assert m.get("Akt").shape[0] == case["N"] + 1
    m.close()


@pytest.mark.parametrize("pair", [0, 1, 2])
def test_akt_kept_without_both_pair_kernels(pair, monkeypatch):
    case = _case(21, 9, 100)
    outs = []
    for mask in (0, 3):
        monkeypatch.setenv("ROMS_GPU_T_PAIR", str(pair))
        m = _model(case, monkeypatch, mask)
        m.step(3)
        m.sync()
        n = m.lean_stores()[1]
        assert n[1] == 0 and (n[0] >= 3 if mask else n[0] == 0), n
        outs.append(_all_fields(m))
        m.close()
    _assert_same(outs[0], outs[1], "T_PAIR %d" % pair)


def test_outputs_sample_a_current_akt(monkeypatch, tmp_path):
    """calc_avg of AKt and AKs over two samples, a history record with both, a restart record."""
    LLm, MMm, N = 21, 9, 100
    case = _case(LLm, MMm, N)
    bits = romsgpu.WRT["Akt"] | romsgpu.WRT["Aks"]
    outs = []
    for mask in (0, 3):
        m = _model(case, monkeypatch, mask)
        m.step(2)
        m.avg_begin(bits)
        m.step_avg(2, case["dt"])
        his, rst = str(tmp_path / ("his%d.nc" % mask)), str(tmp_path / ("rst%d.nc" % mask))
        m.wrt_his(his, 1, 1, m.time(case["dt"]), bits)
        m.wrt_rst(rst, 1, 1, m.time(case["dt"]))
        m.io_wait()
        assert _counts_ok(mask, m.lean_stores()[1], 4)
        got = {"avg_Akt": m.avg("Akt"), "avg_Aks": m.avg("Aks")}
        m.avg_begin(0)
        for tag, path in (("his", his), ("rst", rst)):
            for k, a in read(path).items():
                if not k.startswith("_"):
                    got[tag + "_" + k] = a
        outs.append(got)
        m.close()
    assert "his_AKs" in outs[0] and np.any(outs[0]["his_AKs"] != 0.0) and np.any(outs[0]["avg_Aks"] != 0.0)
    assert outs[0].keys() == outs[1].keys()
    _assert_same(outs[0], outs[1], "outputs")


def test_registered_download_of_akt(monkeypatch):
    cfg = lmd_basin_cfg(surf_flux=1, LLm=21, MMm=9, N=100)
    outs = []
    for mask in (0, 3):
        monkeypatch.setenv("ROMS_GPU_LEAN_ST", str(mask))
        o = oracle.Oracle(cfg)
        o.init()
        m, host = host_model(o, cfg)
        m.step(3)
        m.download("Akt")
        assert _counts_ok(mask, m.lean_stores()[1], 3)
        outs.append(host["Akt"].copy())
        m.close()
    N = cfg.N
    a = outs[0].reshape(2 * (N + 1), cfg.MMm + 4, cfg.LLm + 4)
    assert np.any(a[N + 1:] != 0.0)
    assert np.array_equal(outs[0], outs[1])


def test_decomposed_2x1_bitwise(monkeypatch):
    case = _case(40, 32, 100)
    monkeypatch.setenv("ROMS_GPU_HZ_UV", "1")
    parts = {}
    for mask in (0, 3):
        monkeypatch.setenv("ROMS_GPU_LEAN_ST", str(mask))
        parts[mask], _ = run_decomposed(case, 2, 1, NSTEPS, fields=tuple(romsgpu.FIELDS),
                                        probe=lambda m: m.lean_stores())
    N = case["N"]
    for rank in range(2):
        a, b = parts[0][rank], parts[3][rank]
        assert a[:4] == b[:4]
        assert a[5] == (0, (0, 0)) and b[5][0] == 3 and _counts_ok(3, b[5][1], NSTEPS), (a[5], b[5])
        _assert_same(a[4], b[4], "rank %d" % rank)   # whole arrays: halo rows and both Akt slots too
        akt = b[4]["Akt"]
        assert akt.shape[0] == 2 * (N + 1)
        # the rank boundary's halo columns hold the neighbour's values in both slots
        hal = slice(-2, None) if rank == 0 else slice(0, 2)
        assert np.any(akt[:N + 1, 2:-2, hal] != 0.0) and np.array_equal(akt[N + 1:, :, hal], akt[:N + 1, :, hal])
