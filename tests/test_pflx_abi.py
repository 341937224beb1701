"""CPU-side checks of the pressure-flux entry points (include/roms_gpu.h, ABI 34): the header, the Fortran module and
the Python mirror declare them and the ROMS_PFLX_* ids, the by-value arguments are by value in Fortran, enum roms_field
got no new id, and on a library that was never initialised each entry returns an error with a message instead of
touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pflx_begin", "pflx_state", "pflx_path", "pflx_copy_out", "pflx_copy_in", "time_pflx")
IDS = dict(UP=1, VP=2, U_SLOW=3, V_SLOW=4, P_SLOW=5)
NFIELDS = 111  # enum roms_field before ABI 34: the filter states are no model fields


def test_header_fortran_module_and_python_declare_the_entries_and_the_ids():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    f = open(os.path.join(ROOT, "fortran", "roms_gpu_mod.F90")).read()
    assert int(re.search(r"#define ROMS_GPU_ABI_VERSION (\d+)", h).group(1)) >= 34
    assert int(re.search(r"ROMS_GPU_ABI = (\d+)", f).group(1)) >= 34
    L = romsgpu.load_library()
    for n in NAMES:
        assert re.search(r"\bint roms_gpu_%s\(" % n, h), n
        assert re.search(r"integer\(c_int\) function roms_gpu_%s\([\w, ]*\) bind\(c\)" % n, f), n
        assert hasattr(L, "roms_gpu_" + n) and getattr(L, "roms_gpu_" + n).argtypes
    for k, v in IDS.items():
        assert re.search(r"#define ROMS_PFLX_%s\s+%d\b" % (k, v), h), k
        assert re.search(r"\bROMS_PFLX_%s = %d\b" % (k, v), f), k
        assert romsgpu.PFLX[k.lower()] == v
    for meth in ("pflx_begin", "pflx_state", "pflx_path", "pflx", "pflx_set", "time_pflx"):
        assert callable(getattr(romsgpu.Model, meth))
    blk = f[f.index("function roms_gpu_pflx_begin("):f.index("function roms_gpu_pflx_state(")]
    assert re.search(r"real\(c_double\), value :: timescale", blk) and re.search(r"integer\(c_int\), value :: on", blk)
    for a, b in (("pflx_copy_out", "pflx_copy_in"), ("pflx_copy_in", "time_pflx")):
        blk = f[f.index("function roms_gpu_%s(" % a):f.index("function roms_gpu_%s(" % b)]
        assert re.search(r"integer\(c_int\), value :: which", blk) and re.search(r"integer\(c_long\), value :: count", blk)
    blk = f[f.index("function roms_gpu_time_pflx("):f.index("function roms_gpu_zslice_begin(")]
    assert re.search(r"integer\(c_int\), value :: n\b", blk) and re.search(r"intent\(out\) :: ms\(2\)", blk)


def test_enum_roms_field_is_unchanged_in_length():
    import romsgpu
    h = open(os.path.join(ROOT, "include", "roms_gpu.h")).read()
    body = h[h.index("enum roms_field"):h.index("ROMS_NFIELDS")]
    ids = [i for i in re.findall(r"ROMS_(\w+)", body) if i != "ALL"]
    assert len(ids) == NFIELDS == len(romsgpu.FIELDS + romsgpu.ISO_FIELDS)
    assert not [i for i in ids if "slow" in i.lower() or i.lower() in ("up", "vp")]


def test_uninitialised_calls_fail_with_a_message_and_touch_nothing():
    import romsgpu
    L = romsgpu.load_library()
    buf = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    ms = (ctypes.c_double * 2)(7.0, 7.0)
    armed, alpha, ns = ctypes.c_int(7), ctypes.c_double(7.0), ctypes.c_long(7)
    calls = {
        "pflx_begin": lambda: L.roms_gpu_pflx_begin(0.0, 1),
        "pflx_state": lambda: L.roms_gpu_pflx_state(ctypes.byref(armed), ctypes.byref(alpha), ctypes.byref(ns)),
        "pflx_path": lambda: L.roms_gpu_pflx_path(ctypes.byref(ns), ctypes.byref(ns)),
        "pflx_copy_out": lambda: L.roms_gpu_pflx_copy_out(1, buf, 4),
        "pflx_copy_in": lambda: L.roms_gpu_pflx_copy_in(3, buf, 4),
        "time_pflx": lambda: L.roms_gpu_time_pflx(3, ms),
    }
    assert set(NAMES) == set(calls)
    for n, call in calls.items():
        assert call() < 0, n
        assert b"not initialised" in L.roms_gpu_last_error(), n
    assert list(buf) == [7.0] * 4 and list(ms) == [7.0] * 2 and (armed.value, alpha.value, ns.value) == (7, 7.0, 7)
    m = romsgpu.Model()
    m.N, m.shape2 = 4, (10, 13)
    for fn, args in ((m.pflx_begin, ()), (m.pflx_state, ()), (m.pflx, ("up",)), (m.pflx, ("p_slow",)),
                     (m.pflx_set, ("u_slow", [0.0])), (m.time_pflx, (3,))):
        with pytest.raises(romsgpu.RomsGpuError):
            fn(*args)
    with pytest.raises(ValueError):
        m.pflx("dzt")
