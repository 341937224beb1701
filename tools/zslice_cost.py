"""Cost of the device z-slices on the C3 case of bench.py,
one box, one session:

  * roms_gpu_calc_zslice alone, HIP events on the library stream over
    --samples samples, U+V+T+S at the reference's six depths
    (zslice_output.opt), without and with do_avg (one untimed sample opens the
    window, so every timed one reads the old mean): ms per sample,
    algorithmic bytes, TB/s, and its ratio to the copy probe recorded in
    profiles/avg_cost.txt,
  * the same with z_r / z_w streamed instead of formed (a host write of z_r
    ends VGrid's validity),
  * the step with and without a sample after it, five alternations.

Algorithmic bytes of one sample of the search-then-gather kernel: per field
and depth two level reads and one plane written, with do_avg also the old mean
read and the new one written, over interior cells; the 2-D inputs of the
search (z_sd, h, hinv, rmask) are left out.  `walk_bytes` is the same count for
a level walk, N level reads per field, the shape the kept kernel was measured
against (the record's A/B lines came from a build that held both).

usage: python tools/zslice_cost.py [--samples 20] [--steps 10]
"""
import argparse
import ctypes
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ucla-roms_amd"))

import bench  # noqa: E402  (C3 constants, HBM_PEAK_GBS)

DEPTHS = (-2.0, -15.0, -30.0, -60.0, -120.0, -250.0)   # zslice_output.opt vecdep
NFIELDS = 4                                            # u, v, temp, salt


def gather_bytes(I, J, ndep, nfields, avg):
    return 8.0 * I * J * ndep * nfields * (5 if avg else 3)


def walk_bytes(I, J, N, ndep, nfields, avg):
    return 8.0 * I * J * nfields * (N + ndep * (3 if avg else 1))


def copy_probe():
    """GB/s of the copy yardstick recorded with the averaging kernel (same box class)."""
    txt = open(os.path.join(ROOT, "profiles", "avg_cost.txt")).read()
    return float(re.search(r"copy yardstick: ([\d.]+) GB/s", txt).group(1))


def time_samples(m, n):
    ms = ctypes.c_double()
    for _ in range(2):   # the second figure is reported (first: cold caches, clocks)
        m._chk(m.L.roms_gpu_time_calc_zslice(n, ctypes.byref(m.t), ctypes.byref(ms)), "time_calc_zslice")
    return ms.value / n


def c3_model():
    import romsgpu
    L, N, NT, dt = bench.C3_L, bench.C3_N, bench.NT, bench.C3_DT
    m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, NT, salinity=True, nonlin_eos=True, lmd=romsgpu.LMD_ICELAND,
                                dt=dt, ndtfast=bench.NDTFAST, sizex=bench.C3_DX * L, sizey=bench.C3_DX * L)
    m.step(4)
    m.sync()
    return m


def report(name, per, nb, copy):
    gbs = nb / (per * 1e-3) / 1e9
    print("calc_zslice %-34s %7.3f ms/sample  %6.3f GB  %6.3f TB/s  %.3f of peak  %.3f of copy" %
          (name, per, nb / 1e9, gbs / 1e3, gbs / bench.HBM_PEAK_GBS, gbs / copy))


def main():
    import romsgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    copy = copy_probe()
    m = c3_model()
    L, N, dt = bench.C3_L, bench.C3_N, bench.C3_DT
    what = romsgpu.ZSL_T | romsgpu.ZSL_U | romsgpu.ZSL_V
    print("C3 %dx%dx%d, U+V+T+S at %s, %d samples per figure; copy probe %.1f GB/s (profiles/avg_cost.txt)" %
          (L, L, N, list(DEPTHS), args.samples, copy))
    for avg in (False, True):
        m.zslice_begin(DEPTHS, what, (1, 2), avg=avg)
        m.calc_zslice()
        report("VGrid%s" % (", do_avg" if avg else ""), time_samples(m, args.samples),
               gather_bytes(L, L, len(DEPTHS), NFIELDS, avg), copy)
    print("  (a level walk would read %.3f GB per sample, %.3f GB with do_avg)" %
          (walk_bytes(L, L, N, len(DEPTHS), NFIELDS, False) / 1e9, walk_bytes(L, L, N, len(DEPTHS), NFIELDS, True) / 1e9))
    # the step with and without a sample after it (VGrid valid)
    m.zslice_begin(DEPTHS, what, (1, 2), avg=True)

    def run(sampling):
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.step(1)
            if sampling:
                m.calc_zslice()
        m.sync()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    run(True)
    print("step alone / step + do_avg sample, ms per step over %d steps, five alternations:" % args.steps)
    a, b = [], []
    for _ in range(5):
        a.append(run(False))
        b.append(run(True))
        print("  %8.3f  %8.3f" % (a[-1], b[-1]))
    ma, mb = sorted(a)[2], sorted(b)[2]
    print("medians %8.3f  %8.3f  -> sampling adds %.3f ms = %.1f %% of the step" % (ma, mb, mb - ma, 100 * (mb - ma) / ma))
    # z_r, z_w streamed: the fallback when the host has written the grid
    m.put("z_r", m.get("z_r"))
    for avg in (False, True):
        m.zslice_begin(DEPTHS, what, (1, 2), avg=avg)
        m.calc_zslice()
        report("streamed z%s" % (", do_avg" if avg else ""), time_samples(m, args.samples),
               gather_bytes(L, L, len(DEPTHS), NFIELDS, avg), copy)
    m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
