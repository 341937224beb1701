"""One file of every kind the library writes, from the Filament 32 x 24 x 16 run of tests/test_gpu_wvlcty.py (TINY;
NT = 2 with salinity where a second tracer is needed), each after 3 steps: the recipe behind
tests/golden/out_files_sha256.json (tests/golden/out_files_golden.py records it, tests/test_gpu_out_files.py
compares).  Only calls of romsgpu that the recording commit has are used.
"""
import hashlib
import os

import numpy as np

import romsgpu

TINY = dict(case_id=0, LLm=32, MMm=24, N=16, NT=1, salinity=False, nonlin_eos=False, dt=5.0, ndtfast=60, sizex=12.8e3,
            sizey=3.2e3)
TINY2 = dict(TINY, NT=2, salinity=True)
DT = TINY["dt"]
Z = romsgpu.ZSL_T | romsgpu.ZSL_U | romsgpu.ZSL_V


def _depths(m):
    """Three depths: near the surface, mid-water and below every bottom."""
    h = float(m.get("h").max())
    return [-0.05 * h, -0.4 * h, -2.0 * h]


def _objects():
    """One rho, one u and one v object of five points; binary fractions."""
    k = np.arange(5.0)
    ang = lambda a0: a0 + 0.07 * k
    return [("chd_south_r", 3.25 + k, np.full(5, 2.375), None, "zeta, temp"),
            ("chd_south_u", 3.75 + k, np.full(5, 2.375), ang(0.1), "ubar, u"),
            ("chd_south_v", 3.25 + k, np.full(5, 2.875), ang(-0.2), "vbar, v")]


def write_all(d):
    """Writes the files into directory d; returns {name: (bytes, sha256)}."""
    p = lambda name: os.path.join(str(d), name)
    # restart (records 1 and 2: create, then append) and history with every variable
    m = romsgpu.Model.from_case(**TINY)
    m.step(3)
    m.wrt_rst(p("rst.nc"), 1, 1, m.time(DT))
    m.wrt_his(p("his.nc"), 1, 1, m.time(DT), mask=romsgpu.WRT_ALL)
    m.step(1)
    m.wrt_rst(p("rst.nc"), 2, 2, m.time(DT))
    m.io_wait()
    m.close()
    # averages: two windows
    m = romsgpu.Model.from_case(**TINY)
    m.avg_begin(romsgpu.WRT_ALL)
    m.step_avg(3, DT)
    m.wrt_avg(p("avg.nc"), 1, 1, 3 * DT)
    m.step_avg(2, DT)
    m.wrt_avg(p("avg.nc"), 2, 2, 2 * DT)
    m.io_wait()
    m.close()
    # slices: the means of three samples, then a snapshot of the same state
    m = romsgpu.Model.from_case(**TINY2)
    dep = _depths(m)
    m.zslice_begin(dep, Z, (1, 2), avg=True)
    for _ in range(3):
        m.step(1)
        m.calc_zslice()
    m.wrt_zslice(p("zsl_avg.nc"), 1, 1, m.time(DT))
    m.zslice_begin(dep, Z, (1, 2))
    m.wrt_zslice(p("zsl.nc"), 1, 1, m.time(DT))
    m.io_wait()
    m.close()
    # tracer-only diagnostics, means
    m = romsgpu.Model.from_case(**TINY2)
    m.tdiag_begin((2, 1), avg=True)
    m.step(3)
    m.wrt_tdiag(p("tdia_avg.nc"), 1, 1, m.time(DT), 3 * DT)
    m.io_wait()
    m.close()
    # momentum diagnostics with one armed tracer: last sample, and means
    for avg, name in ((False, "dia.nc"), (True, "dia_avg.nc")):
        m = romsgpu.Model.from_case(**TINY2)
        m.uvdiag_begin(avg=avg)
        m.tdiag_begin((2,), avg=avg)
        m.step(3)
        m.wrt_diag(p(name), 1, 1, m.time(DT), 3 * DT if avg else 0.0)
        m.io_wait()
        m.close()
    # extraction with the vertical remap
    m = romsgpu.Model.from_case(**TINY)
    m.extract_begin(5, 5.0, 1.5, 40.0)
    for name, ip, jp, ang, ov in _objects():
        m.extract_add(name, ip, jp, ov, ang=ang)
    m.step(3)
    m.wrt_extract(p("ext.nc"), 1, 1, m.time(DT))
    m.io_wait()
    m.close()
    out = {}
    for name in sorted(os.listdir(str(d))):
        raw = open(p(name), "rb").read()
        out[name] = (len(raw), hashlib.sha256(raw).hexdigest())
    return out
