"""CPU-side checks of the tracer-budget entry points (include/roms_gpu.h, ABI 30): the header, the Fortran module
and the Python mirror declare them and the ROMS_TDIA_* terms in the reference's order (diagnostics.F:83-88), the
by-value arguments are by value in Fortran, and on a library that was never initialised each returns an error with
a message instead of touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdiag_begin", "tdiag_sample", "tdiag_state", "tdiag_copy_out", "wrt_tdiag", "time_tdiag")
TERMS = dict(ADVX=1, ADVY=2, ADVZ=3, MIXX=4, MIXY=5, MIXZ=6, SNAP=7)


def test_header_fortran_module_and_python_declare_the_entries_and_the_terms():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 30
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 30
    for n in NAMES:
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
        assert hasattr(romsgpu.load_library(), "roms_gpu_" + n) and getattr(romsgpu.load_library(), "roms_gpu_" + n).argtypes
    for k, v in TERMS.items():
        assert re.search(r"#define ROMS_TDIA_%s\s+%d\b" % (k, v), h), k
        assert re.search(r"\bROMS_TDIA_%s = %d\b" % (k, v), f), k
        assert romsgpu.TDIA[k.lower()] == v
    for meth in ("tdiag_begin", "tdiag_sample", "tdiag_state", "tdiag", "wrt_tdiag", "time_tdiag"):
        assert callable(getattr(romsgpu.Model, meth))
    # the by-value arguments of the C prototypes are by value in Fortran too
    blk = f[f.index("function roms_gpu_tdiag_begin("):f.index("function roms_gpu_tdiag_sample(")]
    assert re.search(r"integer\(c_int\), value :: ntd, do_avg", blk) and re.search(r"intent\(in\) :: itrc\(\*\)", blk)
    blk = f[f.index("function roms_gpu_tdiag_copy_out("):f.index("function roms_gpu_wrt_tdiag(")]
    assert re.search(r"integer\(c_int\), value :: itrc, term", blk) and re.search(r"integer\(c_long\), value :: count", blk)
    blk = f[f.index("function roms_gpu_wrt_tdiag("):f.index("function roms_gpu_time_tdiag(")]
    assert re.search(r"real\(c_double\), value :: time, period", blk) and re.search(r"integer\(c_int\), value :: rec, total_rec", blk)
    blk = f[f.index("function roms_gpu_time_tdiag("):f.index("function roms_gpu_zslice_begin(")]
    assert re.search(r"integer\(c_int\), value :: n\b", blk) and re.search(r"intent\(out\) :: ms\(3\)", blk)


def test_uninitialised_calls_fail_with_a_message_and_touch_nothing():
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    ms = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    one = (ctypes.c_int * 1)(1)
    st = [ctypes.c_int(7) for _ in range(4)]
    calls = {
        "tdiag_begin": lambda: L.roms_gpu_tdiag_begin(1, one, 0),
        "tdiag_sample": lambda: L.roms_gpu_tdiag_sample(1),
        "tdiag_state": lambda: L.roms_gpu_tdiag_state(*[ctypes.byref(x) for x in st]),
        "tdiag_copy_out": lambda: L.roms_gpu_tdiag_copy_out(1, 1, buf, 4),
        "wrt_tdiag": lambda: L.roms_gpu_wrt_tdiag(b"/nonexistent/dia.nc", 1, 1, 0.0, 0.0, ctypes.byref(t)),
        "time_tdiag": lambda: L.roms_gpu_time_tdiag(3, ctypes.byref(t), ms),
    }
    assert set(NAMES) == set(calls)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert list(buf) == [7.0] * 4 and list(ms) == [7.0] * 3 and [x.value for x in st] == [7] * 4
    m = romsgpu.Model()
    m.N, m.shape2 = 4, (10, 13)
    for fn, args in ((m.tdiag_begin, ((1,),)), (m.tdiag_state, ()), (m.tdiag, (1, "advx")), (m.time_tdiag, (3,))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
