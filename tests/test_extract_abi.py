"""CPU-side checks of the extraction entry points (include/roms_gpu.h, ABI 27):
the header and the Fortran module declare them and the ROMS_EXT_* bits with
by-value arguments by value, the Python mirror binds them, and on a library
that was never initialised each returns an error with a message instead of
touching the device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("extract_begin", "extract_angler", "extract_add_object", "extract_objects_file", "calc_extract", "wrt_extract",
         "extract_state", "extract_object_info", "extract_object_coef", "extract_child_cs", "extract_copy_out",
         "time_calc_extract")
BITS = dict(ZETA=1, UBAR=2, VBAR=4, U=8, V=16, TEMP=32, SALT=64, UP=128, VP=256, W=512, BGC=1024)


def _block(f, name):
    a = f.index("function roms_gpu_%s(" % name)
    return f[a:f.index("end function", a)]


def test_header_and_fortran_module_declare_the_extraction_entries():
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 27
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 27
    for n in NAMES + ("extract_locate",):
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
    assert {n: int(v) for n, v in re.findall(r"#define ROMS_EXT_(\w+)\s+(\d+)", h)} == BITS
    assert {n: int(v) for n, v in re.findall(r"ROMS_EXT_(\w+) = (\d+)", f)} == BITS
    # the by-value arguments of the C prototypes are by value in Fortran too, the arrays and outputs are not
    blk = _block(f, "extract_begin")
    assert re.search(r"integer\(c_int\), value :: N_chd", blk)
    assert re.search(r"real\(c_double\), value :: theta_s_chd, theta_b_chd, hc_chd", blk)
    blk = _block(f, "extract_add_object")
    assert re.search(r"integer\(c_long\), value :: np_global", blk) and re.search(r"type\(c_ptr\), value :: ang", blk)
    assert re.search(r"real\(c_double\), intent\(in\) :: ipos\(\*\), jpos\(\*\)", blk)
    blk = _block(f, "wrt_extract")
    assert re.search(r"integer\(c_int\), value :: rec, total_rec", blk) and re.search(r"real\(c_double\), value :: time", blk)
    blk = _block(f, "extract_copy_out")
    assert re.search(r"integer\(c_int\), value :: iobj, var_bit", blk) and re.search(r"integer\(c_long\), value :: count", blk)
    assert re.search(r"integer\(c_int\), value :: iobj\b", _block(f, "extract_object_info"))
    assert re.search(r"integer\(c_int\), value :: iobj, grid", _block(f, "extract_object_coef"))
    assert re.search(r"integer\(c_int\), value :: n\b", _block(f, "time_calc_extract"))
    blk = _block(f, "extract_locate")
    assert re.search(r"integer\(c_int\), value :: nx, ny, iSW_corn, jSW_corn", blk)
    assert re.search(r"integer\(c_long\), value :: npg", blk) and re.search(r"intent\(out\) :: start_idx, np", blk)
    for n in ("extract_state", "calc_extract", "extract_child_cs"):
        assert "value" not in _block(f, n), n


def test_uninitialised_extraction_calls_fail_with_a_message(tmp_path):
    import romsgpu
    L = romsgpu.load_library()
    t = romsgpu.Tlev(iic=1, kstp=1, knew=1, nstp=1, nrhs=1, nnew=1)
    q = [ctypes.c_int(7) for _ in range(5)]
    pos = np.array([1.5, 2.5])
    ibuf = np.full(4, 7, dtype=np.int32)
    buf = np.full(8, 7.0)
    ms = (ctypes.c_double * 2)(7.0, 7.0)
    p = str(tmp_path / "never.nc")
    calls = {
        "extract_begin": lambda: L.roms_gpu_extract_begin(5, 6.0, 2.0, 25.0),
        "extract_angler": lambda: L.roms_gpu_extract_angler(buf.ctypes.data, 8),
        "extract_add_object": lambda: L.roms_gpu_extract_add_object(b"g_west_r", b"n", 2, pos.ctypes.data, pos.ctypes.data,
                                                                    None, b"zeta"),
        "extract_objects_file": lambda: L.roms_gpu_extract_objects_file(p.encode()),
        "calc_extract": lambda: L.roms_gpu_calc_extract(ctypes.byref(t)),
        "wrt_extract": lambda: L.roms_gpu_wrt_extract(p.encode(), 1, 1, 5.0, ctypes.byref(t)),
        "extract_state": lambda: L.roms_gpu_extract_state(*[ctypes.byref(x) for x in q]),
        "extract_object_info": lambda: L.roms_gpu_extract_object_info(1, *[ctypes.byref(x) for x in q]),
        "extract_object_coef": lambda: L.roms_gpu_extract_object_coef(1, 0, ibuf.ctypes.data, ibuf.ctypes.data, buf.ctypes.data,
                                                                      buf.ctypes.data, buf.ctypes.data),
        "extract_child_cs": lambda: L.roms_gpu_extract_child_cs(buf.ctypes.data),
        "extract_copy_out": lambda: L.roms_gpu_extract_copy_out(1, 1, buf.ctypes.data, 2),
        "time_calc_extract": lambda: L.roms_gpu_time_calc_extract(3, ctypes.byref(t), ms),
    }
    assert set(calls) == set(NAMES)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert [x.value for x in q] == [7] * 5 and (buf == 7.0).all() and (ibuf == 7).all() and list(ms) == [7.0, 7.0]
    assert not os.path.exists(p)
    m = romsgpu.Model()
    m.N = 5
    for fn, args in ((m.extract_begin, (5, 6.0, 2.0, 25.0)), (m.extract_add, ("g_west_r", pos, pos, "zeta")),
                     (m.extract_objects_file, (p,)), (m.calc_extract, ()), (m.wrt_extract, (p, 1, 1, 5.0)),
                     (m.extract_state, ()), (m.extract_info, (1,)), (m.extract_coef, (1, "r")), (m.extract_child_cs, ()),
                     (m.extract, (1, "zeta")), (m.time_calc_extract, (2,))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
    assert not os.path.exists(p)


def test_python_mirror_names_the_bits():
    import romsgpu
    assert romsgpu.EXT == {k.lower(): v for k, v in BITS.items()}
    assert set(romsgpu.EXT_3D) == {"u", "v", "temp", "salt"}
