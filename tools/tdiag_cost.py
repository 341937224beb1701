"""Cost of the device tracer budget terms on the C3 case of bench.py, T and S armed, one
box, one session; writes profiles/tdiag_cost.txt:

  * the three kernels alone, HIP events on the library stream over --samples launches a window
    (roms_gpu_time_tdiag), --repeats windows after a warm-up window, median and range: for the store sinks and for
    the running-mean sinks with the old mean read, ms per launch (both tracers), counted bytes, TB/s, share of
    8 TB/s,
  * the corrector step3d_t by roms_gpu_time_routine, unarmed and armed (store and mean sinks), alternated; with
    --parent-tree also the unarmed corrector of a built checkout of the parent commit (this file run with
    --tree pointing at it), in a process of its own before this one opens the GPU,
  * whole steps, wall clock around --wsteps calls of roms_gpu_step and a sync, unarmed (replayed graphs) and armed
    (enqueued step by step, which is what an armed, sampling run does), alternated.

Counted bytes per launch and armed tracer, over interior cells as bench.py counts (I*J*N*8 B a pass): k_tdiag_snap
reads t(nnew) and writes the snapshot (2 passes); k_tdiag_h reads t(nrhs), FlxU, FlxV and writes four terms (7; the
mean sink reads four old means besides: 11); k_tdiag_v reads t(nrhs), Hz, We, the snapshot and t(nnew) and writes
two terms (7; mean sink 9).  Masks, pm and pn are 2-D and the stencil's neighbours are counted once: neither adds
a pass.

usage: python tools/tdiag_cost.py [--samples 40] [--repeats 5] [--steps 3] [--wsteps 20] [--alternations 3]
       [--parent-tree DIR]
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree DIR: measure the library and package of another checkout (the parent commit's) with this file
ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ucla-roms_amd"))

import bench  # noqa: E402  (C3 constants, HBM_PEAK_GBS)

LINES = []
PASSES = {"snap": (2, 2), "h": (7, 11), "v": (7, 9)}   # (store, mean) per armed tracer


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


def corrector_ms(m, steps):
    ms, calls = m.time_routine("step3d_t", steps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--wsteps", type=int, default=20)
    ap.add_argument("--tree", default=None, help="with --unarmed-only: the checkout whose library is measured")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--unarmed-only", action="store_true", help="print the unarmed corrector's ms per call and exit")
    args = ap.parse_args()
    if args.unarmed_only:
        m = c3_model()
        corrector_ms(m, args.steps)
        print("UNARMED " + " ".join("%.4f" % corrector_ms(m, args.steps) for _ in range(args.alternations)))
        m.close()
        return 0
    say("Device tracer budget terms (roms_gpu_tdiag_*, k_tdiag.hip): cost at C3 on one MI355X, one session.")
    say("Produced by: python tools/tdiag_cost.py" + (" --parent-tree <a built checkout of the parent commit>" if args.parent_tree else ""))
    say()
    parent = None
    if args.parent_tree:   # its own process, before this one opens the GPU
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--unarmed-only", "--tree", args.parent_tree,
                              "--steps", str(args.steps), "--alternations", str(args.alternations)],
                             capture_output=True, text=True, timeout=300)
        line = [l for l in out.stdout.splitlines() if l.startswith("UNARMED ")]
        if out.returncode or not line:
            sys.stderr.write(out.stdout + out.stderr)
            return 1
        parent = [float(x) for x in line[0].split()[1:]]
    m = c3_model()
    L, N, NT = bench.C3_L, bench.C3_N, bench.NT
    n, c3, peak = args.samples, 8.0 * L * L * N, bench.HBM_PEAK_GBS
    say("C3 %dx%dx%d NT=%d, temp and salt armed; a window is %d launches (each launch: both tracers), one warm-up "
        "window, then %d: median [min .. max] ms per launch" % (L, L, N, NT, n, args.repeats))

    def rate(ms, nbytes):
        g = nbytes / (ms * 1e-3) / 1e9
        return "%6.2f GB  %6.3f TB/s  %.3f of peak" % (nbytes / 1e9, g / 1e3, g / peak)

    for avg in (False, True):
        m.tdiag_begin((1, 2), avg=avg)
        m.step(1)
        m.time_tdiag(n)      # warm-up window: cold caches, clocks
        wins = [m.time_tdiag(n) for _ in range(args.repeats)]
        for q, k in enumerate(("snap", "h", "v")):
            x = sorted(w[q] / n for w in wins)
            med = x[len(x) // 2]
            say("k_tdiag_%-4s %-5s sink (%2d passes a tracer)  %7.3f [%7.3f .. %7.3f] ms  " % (
                k, "mean" if avg else "store", PASSES[k][avg], med, x[0], x[-1]) + rate(med, 2 * PASSES[k][avg] * c3))
    say()
    say("step3d_t (roms_gpu_time_routine, %d steps a figure), ms per call, %d alternations:" % (args.steps, args.alternations))
    say("   unarmed   armed, store   armed, mean")
    rows = []
    for _ in range(args.alternations):
        m.tdiag_begin(())
        a = corrector_ms(m, args.steps)
        m.tdiag_begin((1, 2))
        b = corrector_ms(m, args.steps)
        m.tdiag_begin((1, 2), avg=True)
        c = corrector_ms(m, args.steps)
        rows.append((a, b, c))
        say("  %8.3f   %12.3f   %11.3f" % rows[-1])
    med = [sorted(r[q] for r in rows)[len(rows) // 2] for q in range(3)]
    say("medians %8.3f %12.3f %11.3f  -> armed / unarmed: store %.3f, mean %.3f" % (med[0], med[1], med[2],
                                                                                   med[1] / med[0], med[2] / med[0]))
    if parent:
        pm = sorted(parent)[len(parent) // 2]
        say("the parent commit's library, unarmed, its own process: " + " ".join("%.3f" % x for x in parent)
            + "  median %.3f  -> armed / parent: store %.3f, mean %.3f" % (pm, med[1] / pm, med[2] / pm))
    import time

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
        for arm in ((), (1, 2), (1, 2)):
            m.tdiag_begin(arm, avg=len(r) == 2)
            whole(2)
            r.append(whole(args.wsteps))
        rows.append(tuple(r))
        say("  %12.3f   %20.3f   %18.3f" % rows[-1])
    med = [sorted(r[q] for r in rows)[len(rows) // 2] for q in range(3)]
    say("medians %8.3f %22.3f %20.3f  -> armed adds %.3f ms = %.1f %% (store), %.3f ms = %.1f %% (mean) of the step" % (
        med[0], med[1], med[2], med[1] - med[0], 100 * (med[1] - med[0]) / med[0], med[2] - med[0],
        100 * (med[2] - med[0]) / med[0]))
    m.tdiag_begin(())
    m.close()
    with open(os.path.join(HERE, "profiles", "tdiag_cost.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
