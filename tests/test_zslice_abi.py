"""CPU-side checks of the z-slice entry points (include/roms_gpu.h, ABI 26): the
header and the Fortran module declare them with by-value arguments by value,
the Python mirror binds them, and on a library that was never initialised each
returns an error with a message instead of touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zslice_begin", "calc_zslice", "wrt_zslice", "zslice_state", "zslice_copy_out", "time_calc_zslice")


def _block(f, name):
    a = f.index("function roms_gpu_%s(" % name)
    return f[a:f.index("end function", a)]


def test_header_and_fortran_module_declare_the_zslice_entries():
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 26
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 26
    for n in NAMES:
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
    bits = {n: int(v) for n, v in re.findall(r"#define ROMS_ZSL_(\w+)\s+(\d+)", h)}
    assert bits == dict(T=1, U=2, V=4, MAXDEP=32)
    # the by-value arguments of the C prototypes are by value in Fortran too, the arrays and outputs are not
    blk = _block(f, "zslice_begin")
    assert re.search(r"integer\(c_int\), value :: what, ndep, nt_z, do_avg", blk)
    assert re.search(r"real\(c_double\), intent\(in\) :: vecdep\(\*\)", blk)
    assert re.search(r"integer\(c_int\), intent\(in\) :: trc2zsc\(\*\)", blk)
    blk = _block(f, "wrt_zslice")
    assert re.search(r"integer\(c_int\), value :: rec, total_rec", blk) and re.search(r"real\(c_double\), value :: time", blk)
    blk = _block(f, "zslice_copy_out")
    assert re.search(r"integer\(c_int\), value :: what_bit, q", blk) and re.search(r"integer\(c_long\), value :: count", blk)
    assert re.search(r"integer\(c_int\), value :: n\b", _block(f, "time_calc_zslice"))
    assert "value" not in _block(f, "zslice_state") and "value" not in _block(f, "calc_zslice")


def test_uninitialised_zslice_calls_fail_with_a_message(tmp_path):
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    q = [ctypes.c_int(7) for _ in range(4)]
    dep = (ctypes.c_double * 2)(-1.0, -2.0)
    trc = (ctypes.c_int * 1)(1)
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    ms = ctypes.c_double(7.0)
    p = str(tmp_path / "never.nc")
    calls = {
        "zslice_begin": lambda: L.roms_gpu_zslice_begin(7, 2, dep, 1, trc, 0),
        "calc_zslice": lambda: L.roms_gpu_calc_zslice(ctypes.byref(t)),
        "wrt_zslice": lambda: L.roms_gpu_wrt_zslice(p.encode(), 1, 1, 5.0, ctypes.byref(t)),
        "zslice_state": lambda: L.roms_gpu_zslice_state(*[ctypes.byref(x) for x in q]),
        "zslice_copy_out": lambda: L.roms_gpu_zslice_copy_out(2, 0, buf, 4),
        "time_calc_zslice": lambda: L.roms_gpu_time_calc_zslice(3, ctypes.byref(t), ctypes.byref(ms)),
    }
    assert set(calls) == set(NAMES)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert [x.value for x in q] == [7] * 4 and list(buf) == [7.0] * 4 and ms.value == 7.0 and not os.path.exists(p)
    m = romsgpu.Model()
    m.shape2 = (6, 6)
    for fn, args in ((m.zslice_begin, ([-1.0],)), (m.calc_zslice, ()), (m.wrt_zslice, (p, 1, 1, 5.0)),
                     (m.zslice_state, ()), (m.zslice, ("u",))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
    assert not os.path.exists(p)


def test_python_mirror_names_the_bits():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    bits = {n: int(v) for n, v in re.findall(r"#define ROMS_ZSL_(\w+)\s+(\d+)", h)}
    assert (romsgpu.ZSL_T, romsgpu.ZSL_U, romsgpu.ZSL_V, romsgpu.ZSL_MAXDEP) == (bits["T"], bits["U"], bits["V"], bits["MAXDEP"])
