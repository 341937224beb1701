"""CPU-side checks of the momentum-budget entry points (include/roms_gpu.h, ABI 31): the header, the Fortran module
and the Python mirror declare them and the ROMS_UVD_* terms in the reference's order (diagnostics.F:56-63), the
by-value arguments are by value in Fortran, and on a library that was never initialised each returns an error with
a message instead of touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("uvdiag_begin", "uvdiag_sample", "uvdiag_state", "uvdiag_copy_out", "wrt_diag", "time_uvdiag")
TERMS = dict(PGR=1, COR=2, ADV=3, DIS=4, HMX=5, VMX=6, CPL=7, PREV=8)


def test_header_fortran_module_and_python_declare_the_entries_and_the_terms():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 31
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 31
    for n in NAMES:
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
        assert hasattr(romsgpu.load_library(), "roms_gpu_" + n) and getattr(romsgpu.load_library(), "roms_gpu_" + n).argtypes
    for k, v in TERMS.items():
        assert re.search(r"#define ROMS_UVD_%s\s+%d\b" % (k, v), h), k
        assert re.search(r"\bROMS_UVD_%s = %d\b" % (k, v), f), k
        assert romsgpu.UVD[k.lower()] == v
    for k, v in (("U", 0), ("V", 1)):
        assert re.search(r"#define ROMS_UVD_%s\s+%d\b" % (k, v), h) and re.search(r"\bROMS_UVD_%s = %d\b" % (k, v), f)
        assert romsgpu.UVD_COMP[k.lower()] == v
    for meth in ("uvdiag_begin", "uvdiag_sample", "uvdiag_state", "uvdiag", "wrt_diag", "time_uvdiag"):
        assert callable(getattr(romsgpu.Model, meth))
    # the by-value arguments of the C prototypes are by value in Fortran too
    blk = f[f.index("function roms_gpu_uvdiag_begin("):f.index("function roms_gpu_uvdiag_sample(")]
    assert re.search(r"integer\(c_int\), value :: on, do_avg", blk)
    blk = f[f.index("function roms_gpu_uvdiag_copy_out("):f.index("function roms_gpu_wrt_diag(")]
    assert re.search(r"integer\(c_int\), value :: comp, term", blk) and re.search(r"integer\(c_long\), value :: count", blk)
    blk = f[f.index("function roms_gpu_wrt_diag("):f.index("function roms_gpu_time_uvdiag(")]
    assert re.search(r"real\(c_double\), value :: time, period", blk) and re.search(r"integer\(c_int\), value :: rec, total_rec", blk)
    blk = f[f.index("function roms_gpu_time_uvdiag("):f.index("function roms_gpu_zslice_begin(")]
    assert re.search(r"integer\(c_int\), value :: n\b", blk) and re.search(r"intent\(out\) :: ms\(4\)", blk)


def test_uninitialised_calls_fail_with_a_message_and_touch_nothing():
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    ms = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    st = [ctypes.c_int(7) for _ in range(4)]
    calls = {
        "uvdiag_begin": lambda: L.roms_gpu_uvdiag_begin(1, 0),
        "uvdiag_sample": lambda: L.roms_gpu_uvdiag_sample(1),
        "uvdiag_state": lambda: L.roms_gpu_uvdiag_state(*[ctypes.byref(x) for x in st]),
        "uvdiag_copy_out": lambda: L.roms_gpu_uvdiag_copy_out(0, 1, buf, 4),
        "wrt_diag": lambda: L.roms_gpu_wrt_diag(b"/nonexistent/dia.nc", 1, 1, 0.0, 0.0, ctypes.byref(t)),
        "time_uvdiag": lambda: L.roms_gpu_time_uvdiag(3, ctypes.byref(t), ms),
    }
    assert set(NAMES) == set(calls)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert list(buf) == [7.0] * 4 and list(ms) == [7.0] * 4 and [x.value for x in st] == [7] * 4
    m = romsgpu.Model()
    m.N, m.shape2 = 4, (10, 13)
    for fn, args in ((m.uvdiag_begin, ()), (m.uvdiag_state, ()), (m.uvdiag, ("u", "pgr")), (m.time_uvdiag, (3,))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
    with pytest.raises(ValueError):
        m.uvdiag("w", "pgr")
