"""Cost of the device momentum budget terms on the C3 case of bench.py, one box, one
session; writes profiles/uvdiag_cost.txt:

  * the kernels alone, HIP events on the library stream over --samples launches a window (roms_gpu_time_uvdiag),
    --repeats windows after a warm-up window, median and range: for the store sinks and for the running-mean sinks
    with the old mean read, ms per launch, counted bytes, TB/s, share of 8 TB/s,
  * step3d_uv1 + visc3d + step3d_uv2 by roms_gpu_time_routine, unarmed and armed (store and mean sinks), alternated,
  * whole steps, wall clock around --wsteps calls of roms_gpu_step and a sync, unarmed (replayed graphs) and armed
    (enqueued step by step, prsgrd unfused, u, v(indx) stored: what an armed, sampling run does), alternated.

Counted bytes per launch, over interior cells as bench.py counts (I*J*N*8 B a pass).  The snapshots read ru, rv,
u, v(nnew) and write four arrays (8 passes).  k_uvdiag_rhs reads u, v(nrhs), FlxU, FlxV, We, Wi, Hz, ru, rv, the
four snapshots and u, v(nnew) and writes ten terms (25; the mean sink reads ten old means besides: 35).
k_uvdiag_hmx reads u, v(nstp) and Hz and writes two terms (5; mean 7); k_uvdiag_cpl reads u, v(nnew) and Hz and
writes two (5; mean 7).  The 2-D factors and the stencils' neighbours are counted once: neither adds a pass.

usage: python tools/uvdiag_cost.py [--samples 20] [--repeats 5] [--steps 3] [--wsteps 20] [--alternations 3]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "ucla-roms_amd"))

import bench  # noqa: E402  (C3 constants, HBM_PEAK_GBS)

LINES = []
KERNELS = ("snapshots", "k_uvdiag_rhs", "k_uvdiag_hmx", "k_uvdiag_cpl")
PASSES = {"snapshots": (8, 8), "k_uvdiag_rhs": (25, 35), "k_uvdiag_hmx": (5, 7), "k_uvdiag_cpl": (5, 7)}   # (store, mean)
ROUTINES = ("step3d_uv1", "visc3d", "step3d_uv2")


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def c3_model():
    import romsgpu
    L, N, NT = bench.C3_L, bench.C3_N, bench.NT
    m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, NT, salinity=True, nonlin_eos=True,
                                lmd=romsgpu.LMD_ICELAND, dt=bench.C3_DT, ndtfast=bench.NDTFAST, sizex=bench.C3_DX * L,
                                sizey=bench.C3_DX * L)
    m.step(4)
    m.sync()
    return m


def routines_ms(m, steps):
    return sum(m.time_routine(r, steps)[0] for r in ROUTINES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--wsteps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    args = ap.parse_args()
    say("Device momentum budget terms (roms_gpu_uvdiag_*, k_uvdiag.hip): cost at C3 on one MI355X, one session.")
    say("Produced by: python tools/uvdiag_cost.py")
    say()
    m = c3_model()
    L, N, NT = bench.C3_L, bench.C3_N, bench.NT
    n, c3, peak = args.samples, 8.0 * L * L * N, bench.HBM_PEAK_GBS
    say("C3 %dx%dx%d NT=%d; a window is %d launches, one warm-up window, then %d: median [min .. max] ms per launch"
        % (L, L, N, NT, n, args.repeats))

    def rate(ms, nbytes):
        g = nbytes / (ms * 1e-3) / 1e9
        return "%6.2f GB  %6.3f TB/s  %.3f of peak" % (nbytes / 1e9, g / 1e3, g / peak)

    for avg in (False, True):
        m.uvdiag_begin(avg=avg)
        m.step(1)
        m.time_uvdiag(n)      # warm-up window: cold caches, clocks
        wins = [m.time_uvdiag(n) for _ in range(args.repeats)]
        for q, k in enumerate(KERNELS):
            x = sorted(w[q] / n for w in wins)
            med = x[len(x) // 2]
            say("%-13s %-5s sink (%2d passes)  %7.3f [%7.3f .. %7.3f] ms  " % (
                k, "mean" if avg else "store", PASSES[k][avg], med, x[0], x[-1]) + rate(med, PASSES[k][avg] * c3))
    say()
    say("step3d_uv1 + visc3d + step3d_uv2 (roms_gpu_time_routine, %d steps a figure), ms per call of the three, "
        "%d alternations:" % (args.steps, args.alternations))
    say("   unarmed   armed, store   armed, mean")
    rows = []
    for _ in range(args.alternations):
        m.uvdiag_begin(on=False)
        a = routines_ms(m, args.steps)
        m.uvdiag_begin()
        b = routines_ms(m, args.steps)
        m.uvdiag_begin(avg=True)
        c = routines_ms(m, args.steps)
        rows.append((a, b, c))
        say("  %8.3f   %12.3f   %11.3f" % rows[-1])
    med = [sorted(r[q] for r in rows)[len(rows) // 2] for q in range(3)]
    say("medians %8.3f %12.3f %11.3f  -> armed / unarmed: store %.3f, mean %.3f" % (med[0], med[1], med[2],
                                                                                   med[1] / med[0], med[2] / med[0]))

    def whole(steps):
        m.sync()
        t0 = time.perf_counter()
        m.step(steps)
        m.sync()
        return 1e3 * (time.perf_counter() - t0) / steps

    say()
    say("whole steps (wall clock over %d roms_gpu_step and a sync), ms per step, %d alternations:" % (args.wsteps, args.alternations))
    say("   unarmed (graph replay)   armed, store (eager)   armed, mean (eager)")
    rows = []
    for _ in range(args.alternations):
        r = []
        for on, avg in ((False, False), (True, False), (True, True)):
            m.uvdiag_begin(avg=avg, on=on)
            whole(2)
            r.append(whole(args.wsteps))
        rows.append(tuple(r))
        say("  %12.3f   %20.3f   %18.3f" % rows[-1])
    med = [sorted(r[q] for r in rows)[len(rows) // 2] for q in range(3)]
    say("medians %8.3f %22.3f %20.3f  -> armed adds %.3f ms = %.1f %% (store), %.3f ms = %.1f %% (mean) of the step" % (
        med[0], med[1], med[2], med[1] - med[0], 100 * (med[1] - med[0]) / med[0], med[2] - med[0],
        100 * (med[2] - med[0]) / med[0]))
    m.uvdiag_begin(on=False)
    m.close()
    with open(os.path.join(HERE, "profiles", "uvdiag_cost.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
