"""Cost of the device vertical velocity on the C3 case of
bench.py, one box, one session; writes profiles/wvlcty_cost.txt:

  * tools/membw's streaming figures (the copy lines are the yardstick),
  * roms_gpu_calc_avg's default mask (k_calc_avg, the other yardstick),
  * k_wvlcty alone, HIP events on the library stream over --samples launches
    (roms_gpu_time_wvlcty): the store sink and the running-mean sink with the
    old mean read, ms per launch, counted bytes, TB/s, share of 8 TB/s,
  * the A/B of the two forms of an averages sample of w, alternated
    --alternations times: fused = one launch with the mean as the sink (six
    counted passes), unfused = the store sink followed by k_calc_avg's plain
    copy sweep over one 3-D field (eight passes: the sweep is timed on u's
    mean, the same kernel, element count and alignment a mean of the work array
    would take),
  * the step with and without a sample of the default mask + w after it.

Counted bytes of one launch, over interior cells as bench.py counts: FlxU,
FlxV, u, v read and w written (five passes of I*J*N*8 B) for the store sink,
the old mean besides for the mean sink (six).  z_r is formed from the free
surface (VGrid), pm and pn are 2-D: neither is counted.

usage: python tools/wvlcty_cost.py [--samples 20] [--steps 10] [--alternations 3] [--no-membw]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ucla-roms_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import avg_cost  # noqa: E402  (membw(), sample_bytes())
import bench  # noqa: E402  (C3 constants, HBM_PEAK_GBS)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--no-membw", action="store_true")
    args = ap.parse_args()
    say("Device vertical velocity (roms_gpu_wvlcty, k_wvlcty): cost at C3 on one MI355X, one session.")
    say("Produced by: python tools/wvlcty_cost.py")
    say()
    copy = None
    if not args.no_membw:   # its own process, before this one opens the GPU
        out, copy = avg_cost.membw()
        say("tools/membw (845 MB arrays):")
        say(out.rstrip())
        say("copy yardstick: %.1f GB/s = %.3f of %.0f GB/s" % (copy, copy / bench.HBM_PEAK_GBS, bench.HBM_PEAK_GBS))
    import ctypes

    import romsgpu
    avg_cost.romsgpu = romsgpu
    W = romsgpu.WRT
    L, N, NT, dt = bench.C3_L, bench.C3_N, bench.NT, bench.C3_DT
    m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, NT, salinity=True, nonlin_eos=True, lmd=romsgpu.LMD_ICELAND,
                                dt=dt, ndtfast=bench.NDTFAST, sizex=bench.C3_DX * L, sizey=bench.C3_DX * L)
    m.step(4)
    m.sync()
    n = args.samples
    c3 = 8.0 * L * L * N
    peak = bench.HBM_PEAK_GBS
    say("C3 %dx%dx%d NT=%d, %d launches per figure" % (L, L, N, NT, n))

    def rate(ms, nbytes):
        g = nbytes / (ms * 1e-3) / 1e9
        return "%7.3f ms  %6.2f GB  %6.3f TB/s  %.3f of peak%s" % (ms, nbytes / 1e9, g / 1e3, g / peak,
                                                                 "  %.3f of copy" % (g / copy) if copy else "")

    def calc_avg_ms(mask):
        m.avg_begin(mask)
        m.calc_avg(m.time(dt))   # opens the window: the timed samples all read the old mean
        ms = ctypes.c_double()
        for _ in range(2):       # the second figure is reported (first: cold caches, clocks)
            m._chk(m.L.roms_gpu_time_calc_avg(n, ctypes.byref(m.t), ctypes.byref(ms)), "time_calc_avg")
        return ms.value / n

    def wvl_ms():
        m.avg_begin(W["W"])
        m.calc_avg(m.time(dt))
        for _ in range(2):
            st, mean = m.time_wvlcty(n)
        return st / n, mean / n

    d = calc_avg_ms(romsgpu.WRT_DEFAULT)
    say("calc_avg default mask (Z Ub Vb U V T)   " + rate(d, avg_cost.sample_bytes(romsgpu.WRT_DEFAULT, L, L, N, NT)))
    say("A/B of an averages sample of w, %d alternations (ms per launch):" % args.alternations)
    say("   store sink   copy sweep   unfused = sum   fused (mean sink)")
    rows = []
    for _ in range(args.alternations):
        sweep = calc_avg_ms(W["U"])
        st, mean = wvl_ms()
        rows.append((st, sweep, st + sweep, mean))
        say("   %9.3f   %10.3f   %13.3f   %9.3f" % rows[-1])
    med = [sorted(r[q] for r in rows)[len(rows) // 2] for q in range(4)]
    say("medians:")
    say("k_wvlcty store sink  (5 passes)         " + rate(med[0], 5 * c3))
    say("k_wvlcty mean sink   (6 passes)         " + rate(med[3], 6 * c3))
    say("copy sweep, one 3-D field (3 passes)    " + rate(med[1], 3 * c3))
    say("unfused sample of w  (8 passes)         " + rate(med[2], 8 * c3))
    say("fused / unfused time: %.3f" % (med[3] / med[2]))
    # the step with and without a sample after it
    mask = romsgpu.WRT_DEFAULT | W["W"]
    m.avg_begin(mask)

    def run(sampling):
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.step(1)
            if sampling:
                m.calc_avg(m.time(dt))
        m.sync()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    run(True)
    say("step alone / step + sample of the default mask and w, ms per step over %d steps, five alternations:" % args.steps)
    a, b = [], []
    for _ in range(5):
        a.append(run(False))
        b.append(run(True))
        say("  %8.3f  %8.3f" % (a[-1], b[-1]))
    ma, mb = sorted(a)[2], sorted(b)[2]
    say("medians %8.3f  %8.3f  -> sampling adds %.3f ms = %.1f %% of the step" % (ma, mb, mb - ma, 100 * (mb - ma) / ma))
    m.close()
    with open(os.path.join(ROOT, "profiles", "wvlcty_cost.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
