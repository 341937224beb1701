"""CPU-side checks of the particle entry points (include/roms_gpu.h, ABI 32):
the header, the Fortran module and the Python mirror declare them and
ROMS_PART_SORT, the by-value arguments are by value in Fortran, and on a
library that was never initialised each returns an error with a message
instead of touching the device or its buffers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("part_begin", "part_add", "do_particles", "part_state", "part_copy_out", "wrt_part", "time_do_particles")


def test_header_fortran_module_and_python_declare_the_entries():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 32
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 32
    for n in NAMES:
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
        assert hasattr(romsgpu.load_library(), "roms_gpu_" + n), n
    assert re.search(r"#define ROMS_PART_SORT\s+1\b", h) and re.search(r"\bROMS_PART_SORT = 1\b", f)
    assert romsgpu.PART_SORT == 1 and romsgpu.PART_NPV == 13 and len(romsgpu.PART_WORDS) == 13
    assert romsgpu.PART_BIG_NUMBER == 10000000 and len(romsgpu.PART_STATE) == 8
    for n in ("part_begin", "part_add", "do_particles", "part_state", "particles", "wrt_part", "time_do_particles"):
        assert callable(getattr(romsgpu.Model, n)), n
    assert callable(romsgpu.part_full_seed)

    def block(name):
        s = f.index("function roms_gpu_%s(" % name)
        return f[s:f.index("end function", s)]

    # the by-value arguments of the C prototypes are by value in Fortran too, the arrays are not
    b = block("part_begin")
    assert re.search(r"integer\(c_long\), value :: npmx", b) and re.search(r"real\(c_double\), value :: fac_x, fac_y, fac_c", b)
    assert re.search(r"integer\(c_int\), value :: flags", b)
    b = block("part_add")
    assert re.search(r"integer\(c_long\), value :: n\b", b) and re.search(r"integer\(c_int\), value :: zmode", b)
    assert re.search(r"real\(c_double\), intent\(in\) :: px\(\*\), py\(\*\), pz\(\*\)", b)
    b = block("do_particles")
    assert re.search(r"type\(roms_tlev\), intent\(in\) :: t", b) and "value" not in b
    b = block("part_state")
    assert re.search(r"integer\(c_long\), intent\(out\) :: out\(8\)", b) and "value" not in b
    b = block("part_copy_out")
    assert re.search(r"integer\(c_long\), value :: count", b) and re.search(r"integer\(c_int\), value :: global", b)
    assert re.search(r"intent\(out\) :: dst\(\*\)", b)
    b = block("wrt_part")
    assert re.search(r"integer\(c_int\), value :: rec, total_rec", b) and re.search(r"real\(c_double\), value :: time", b)
    b = block("time_do_particles")
    assert re.search(r"integer\(c_int\), value :: n\b", b) and re.search(r"intent\(out\) :: ms\(2\)", b)


def test_uninitialised_calls_fail_with_a_message_and_touch_nothing(tmp_path):
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    buf = (ctypes.c_double * 13)(*([7.0] * 13))
    ms = (ctypes.c_double * 2)(7.0, 7.0)
    out = (ctypes.c_long * 8)(*([7] * 8))
    p = np.array([1.0])
    path = str(tmp_path / "none_part.nc")
    calls = {
        "part_begin": lambda: L.roms_gpu_part_begin(100, 0.0, 0.0, 0.0, 0),
        "part_add": lambda: L.roms_gpu_part_add(1, p.ctypes.data, p.ctypes.data, p.ctypes.data, 0),
        "do_particles": lambda: L.roms_gpu_do_particles(ctypes.byref(t)),
        "part_state": lambda: L.roms_gpu_part_state(out),
        "part_copy_out": lambda: L.roms_gpu_part_copy_out(buf, 13, 0),
        "wrt_part": lambda: L.roms_gpu_wrt_part(path.encode(), 1, 1, 0.0),
        "time_do_particles": lambda: L.roms_gpu_time_do_particles(3, ctypes.byref(t), ms),
    }
    assert set(NAMES) == set(calls)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert list(buf) == [7.0] * 13 and list(ms) == [7.0, 7.0] and list(out) == [7] * 8 and p[0] == 1.0
    assert not os.path.exists(path)
    m = romsgpu.Model()
    m.N, m.shape2 = 4, (10, 13)
    for fn, args in ((m.part_begin, (10,)), (m.part_add, ([1.0], [1.0], [1.0])), (m.do_particles, ()), (m.part_state, ()),
                     (m.particles, ()), (m.wrt_part, (path, 1, 1, 0.0)), (m.time_do_particles, (2,))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
