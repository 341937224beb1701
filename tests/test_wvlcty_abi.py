"""CPU-side checks of the true-vertical-velocity entry points (include/roms_gpu.h,
ABI 29): the header, the Fortran module and the Python mirror declare them and
the ROMS_WRT_W bit, the by-value arguments are by value in Fortran, and on a
library that was never initialised each returns an error with a message
instead of touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wvlcty", "wvlcty_copy_out", "time_wvlcty")


def test_header_fortran_module_and_python_declare_the_entries_and_the_bit():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 29
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 29
    for n in NAMES:
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
    assert re.search(r"#define ROMS_WRT_W\s+8192\b", h) and re.search(r"#define ROMS_WRT_DEFAULT 63\b", h)
    assert re.search(r"\bROMS_WRT_W = 8192\b", f)
    assert romsgpu.WRT["W"] == 8192 and romsgpu.WRT_ALL == 16383 and romsgpu.WRT_DEFAULT == 63
    assert romsgpu.AVG_FIELDS["w"] == (8192, 1)
    assert romsgpu.AVG_FIELDS["omega"] == (128, 2)   # omega keeps its name and its N+1 levels
    # extraction objects still do not produce w
    assert "w" in romsgpu.EXT and "w" not in romsgpu.EXT_3D
    # the by-value arguments of the C prototypes are by value in Fortran too
    blk = f[f.index("function roms_gpu_wvlcty_copy_out("):f.index("function roms_gpu_time_wvlcty(")]
    assert re.search(r"integer\(c_long\), value :: count", blk) and re.search(r"intent\(out\) :: dst\(\*\)", blk)
    blk = f[f.index("function roms_gpu_time_wvlcty("):f.index("function roms_gpu_zslice_begin(")]
    assert re.search(r"integer\(c_int\), value :: n\b", blk) and re.search(r"intent\(out\) :: ms\(2\)", blk)
    blk = f[f.index("function roms_gpu_wvlcty("):f.index("function roms_gpu_wvlcty_copy_out(")]
    assert re.search(r"type\(roms_tlev\), intent\(in\) :: t", blk) and "value" not in blk


def test_uninitialised_calls_fail_with_a_message_and_touch_nothing():
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    ms = (ctypes.c_double * 2)(7.0, 7.0)
    calls = {
        "wvlcty": lambda: L.roms_gpu_wvlcty(ctypes.byref(t)),
        "wvlcty_copy_out": lambda: L.roms_gpu_wvlcty_copy_out(buf, 4),
        "time_wvlcty": lambda: L.roms_gpu_time_wvlcty(3, ctypes.byref(t), ms),
        "avg_copy_out(W)": lambda: L.roms_gpu_avg_copy_out(romsgpu.WRT["W"], 0, buf, 4),
        "avg_begin(W)": lambda: L.roms_gpu_avg_begin(romsgpu.WRT["W"]),
    }
    assert set(NAMES) <= set(calls)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert list(buf) == [7.0] * 4 and list(ms) == [7.0, 7.0]
    m = romsgpu.Model()
    m.N, m.shape2 = 4, (10, 13)
    for fn, args in ((m.wvlcty, ()), (m.time_wvlcty, (3,)), (m.avg, ("w",))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
