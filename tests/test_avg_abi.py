"""CPU-side checks of the averaging entry points (include/roms_gpu.h, ABI 25):
the Fortran module declares them, the Python mirror binds them, and on a
library that was never initialised each returns an error with a message
instead of touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("avg_begin", "calc_avg", "wrt_avg", "avg_state", "avg_copy_out")


def test_header_and_fortran_module_declare_the_averaging_entries():
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 25
    for n in NAMES + ("time_calc_avg",):
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
    # the by-value arguments of the C prototypes are by value in Fortran too
    blk = f[f.index("function roms_gpu_wrt_avg("):f.index("function roms_gpu_avg_state(")]
    assert re.search(r"integer\(c_int\), value :: rec, total_rec", blk) and re.search(r"real\(c_double\), value :: period", blk)
    blk = f[f.index("function roms_gpu_calc_avg("):f.index("function roms_gpu_wrt_avg(")]
    assert re.search(r"real\(c_double\), value :: time", blk)


def test_uninitialised_averaging_calls_fail_with_a_message(tmp_path):
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    navg, mask, tavg = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_double(7.0)
    buf = (ctypes.c_double * 4)()
    p = str(tmp_path / "never.nc")
    calls = {
        "avg_begin": lambda: L.roms_gpu_avg_begin(63),
        "calc_avg": lambda: L.roms_gpu_calc_avg(ctypes.byref(t), 5.0),
        "wrt_avg": lambda: L.roms_gpu_wrt_avg(p.encode(), 1, 1, 5.0, ctypes.byref(t)),
        "avg_state": lambda: L.roms_gpu_avg_state(ctypes.byref(navg), ctypes.byref(tavg), ctypes.byref(mask)),
        "avg_copy_out": lambda: L.roms_gpu_avg_copy_out(1, 0, buf, 4),
    }
    assert set(calls) == set(NAMES)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert (navg.value, mask.value, tavg.value) == (7, 7, 7.0) and not os.path.exists(p)
    m = romsgpu.Model()
    for fn, args in ((m.avg_begin, ()), (m.calc_avg, (5.0,)), (m.wrt_avg, (p, 1, 1, 5.0)), (m.avg_state, ())):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)


def test_python_mirror_names_every_wrt_bit():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    bits = {n: int(v) for n, v in re.findall(r"#define ROMS_WRT_(\w+)\s+(\d+)", h)}
    default = bits.pop("DEFAULT")
    assert default == romsgpu.WRT_DEFAULT
    assert sum(bits.values()) == romsgpu.WRT_ALL
    assert {b for b, _ in romsgpu.AVG_FIELDS.values()} == set(bits.values())
