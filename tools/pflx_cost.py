"""Cost of the device pressure fluxes on the C3 and C2 cases of bench.py, one box, one
session; writes profiles/pflx_cost.txt:

  * tools/membw's copy rate (the yardstick of the other cost files),
  * the two kernels alone, HIP events on the library stream over --samples launches a window (roms_gpu_time_pflx),
    --repeats windows after a warm-up window, median and range: ms per call, counted bytes, TB/s, share of 8 TB/s and
    of the copy rate,
  * whole steps, wall clock around --wsteps calls of roms_gpu_step and a sync, not armed (replayed graphs: the
    launches, the graph and the bits of the parent commit's step, timed on this commit's build, not on a build of
    the parent) and armed (enqueued step by step), alternated,
  * at C3 the host alternative: the seven 3-D arrays a host would download every step to form the filters itself
    (u, v(nrhs), rho1, qp1, FlxU, FlxV, Hz), at the measured rate of roms_gpu_copy_out.

Counted bytes per call, over interior cells as bench.py counts (I*J*N*8 B a pass).  k_pflx_p reads rho1, qp1 and
p_slow and writes p_slow and p_fast (5 passes; 6 when it streams z_r: after a host write of the grid only; without
SPLIT_EOS rho alone stands for rho1 and qp1: 4).  k_pflx_uv reads FlxU, FlxV, u, v, Hz, p_fast, u_slow, v_slow and
writes u_slow, v_slow (10 passes).  The 2-D factors, up, vp and the stencils' neighbours are counted once: none adds
a pass.

usage: python tools/pflx_cost.py [--samples 10] [--repeats 3] [--wsteps 10] [--alternations 2] [--no-membw]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "ucla-roms_amd"))
sys.path.insert(0, os.path.join(HERE, "tools"))

import avg_cost  # noqa: E402  (membw())
import bench  # noqa: E402  (C2, C3 constants, HBM_PEAK_GBS)

LINES = []
KERNELS = ("k_pflx_p", "k_pflx_uv")


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def model(case):
    import romsgpu
    if case == "C3":
        L, N = bench.C3_L, bench.C3_N
        m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, bench.NT, salinity=True, nonlin_eos=True,
                                    lmd=romsgpu.LMD_ICELAND, dt=bench.C3_DT, ndtfast=bench.NDTFAST,
                                    sizex=bench.C3_DX * L, sizey=bench.C3_DX * L)
        passes = {"k_pflx_p": 5, "k_pflx_uv": 10}
    else:
        L, N = bench.C2_L, bench.C2_N
        m = romsgpu.Model.from_case(romsgpu.CASE_FILAMENT, L, L, N, bench.NT, salinity=True, dt=bench.C2_DT,
                                    ndtfast=bench.NDTFAST, sizex=bench.C2_DX * L, sizey=bench.C2_DY * L)
        passes = {"k_pflx_p": 4, "k_pflx_uv": 10}   # no SPLIT_EOS: rho
    m.step(4)
    m.sync()
    return m, L, N, passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--wsteps", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--no-membw", action="store_true")
    args = ap.parse_args()
    say("Device pressure fluxes (roms_gpu_pflx_*, k_pflx.hip): cost on one MI355X, one session.")
    say("Produced by: python tools/pflx_cost.py")
    copy = None
    if not args.no_membw:   # its own process, before this one opens the GPU
        _, copy = avg_cost.membw()
        say("tools/membw copy yardstick: %.1f GB/s = %.3f of %.0f GB/s" % (copy, copy / bench.HBM_PEAK_GBS,
                                                                          bench.HBM_PEAK_GBS))
    peak, n = bench.HBM_PEAK_GBS, args.samples

    def rate(ms, nbytes):
        g = nbytes / (ms * 1e-3) / 1e9
        s = "%6.2f GB  %6.3f TB/s  %.3f of peak" % (nbytes / 1e9, g / 1e3, g / peak)
        return s + ("  %.3f of copy" % (g / copy) if copy else "")

    for case in ("C3", "C2"):
        m, L, N, passes = model(case)
        cells = 8.0 * L * L * N
        say()
        say("%s %dx%dx%d; a window is %d launches of each kernel, one warm-up window, then %d: median [min .. max] ms "
            "per call" % (case, L, L, N, n, args.repeats))
        m.pflx_begin()
        m.step(1)
        m.time_pflx(n)
        wins = [m.time_pflx(n) for _ in range(args.repeats)]
        tot = 0.0
        for q, k in enumerate(KERNELS):
            x = sorted(w[q] / n for w in wins)
            med = x[len(x) // 2]
            tot += med
            say("%-10s (%2d passes)  %7.3f [%7.3f .. %7.3f] ms  " % (k, passes[k], med, x[0], x[-1])
                + rate(med, passes[k] * cells))
        say("both       (%2d passes)  %7.3f ms  " % (sum(passes.values()), tot) + rate(tot, sum(passes.values()) * cells))

        def whole(steps):
            m.sync()
            t0 = time.perf_counter()
            m.step(steps)
            m.sync()
            return 1e3 * (time.perf_counter() - t0) / steps

        say("whole steps (wall clock over %d roms_gpu_step and a sync), ms per step, %d alternations:"
            % (args.wsteps, args.alternations))
        say("   not armed: this commit's step, which is the parent commit's -- the same launches in the same replayed graph, the")
        say("   same bits (tests/test_gpu_pflx.py::test_not_armed_is_the_parent_behaviour); the change adds one host test of a flag")
        say("   not armed (graph replay)                      armed (eager)")
        rows = []
        for _ in range(args.alternations):
            r = []
            for on in (False, True):
                m.pflx_begin(on=on)
                whole(2)
                r.append(whole(args.wsteps))
            rows.append(tuple(r))
            say("  %12.3f   %36.3f" % rows[-1])
        med = [sorted(r[q] for r in rows)[len(rows) // 2] for q in range(2)]
        say("medians %8.3f %38.3f  -> armed adds %.3f ms = %.1f %% of the step" % (
            med[0], med[1], med[1] - med[0], 100 * (med[1] - med[0]) / med[0]))
        m.pflx_begin(on=False)
        if case == "C3":
            say("the host alternative: seven 3-D arrays a step through roms_gpu_copy_out (one slot of u, v; rho1, qp1, "
                "FlxU, FlxV, Hz)")
            got = []
            for name in ("rho1", "qp1", "FlxU", "FlxV", "Hz"):
                m.get(name)   # first touch of the pageable buffer
                t0 = time.perf_counter()
                a = m.get(name)
                dt = time.perf_counter() - t0
                got.append(a.nbytes / dt / 1e9)
                say("copy_out %-5s %8.1f MB  %7.1f ms  %6.2f GB/s" % (name, a.nbytes / 1e6, 1e3 * dt, got[-1]))
            r = sorted(got)[len(got) // 2]
            one = 8.0 * (L + 4) * (L + 4) * N
            say("seven arrays of %.1f MB at the median %.2f GB/s: %.0f ms a step, against %.3f ms on the device"
                % (one / 1e6, r, 7 * one / r / 1e6, tot))
        m.close()
    with open(os.path.join(HERE, "profiles", "pflx_cost.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
