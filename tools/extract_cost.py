"""Cost of the device extraction on the C3 case of bench.py,
one box, one session, written to profiles/extract_cost.txt (--out):

  * roms_gpu_time_calc_extract over --samples samples for an Iceland-like set
    -- four sides x (r, u, v) objects of 1024 points each, N_chd = 20, every
    supported variable (r: zeta, temp, salt; u: ubar, u; v: vbar, v) -- split
    into its two launches (interpolation, remap), ms per sample,
  * the alternative's cost: roms_gpu_copy_out of the 3-D arrays a host-side
    extraction would fetch (u, v, t, Hz, Hz_u, Hz_v as the ABI hands them out,
    every slot), and the same bytes-per-second applied to seven one-slot
    arrays (u, v, T, S, Hz, Hz_u, Hz_v),
  * the step with and without a sample after it, five alternations.

usage: python tools/extract_cost.py [--samples 20] [--steps 10] [--out profiles/extract_cost.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ucla-roms_amd"))

import bench  # noqa: E402  (C3 constants)

CHILD = (20, 5.0, 2.0, 250.0)   # N_chd of Iceland's child; the stretching of extract_data.opt
NPTS = 1024
INSET = 8.375                   # the child's boundary, this many parent cells inside the domain


def iceland_like(L):
    """Four sides x (r, u, v): (name, ipos, jpos, ang or None, output_vars)."""
    run = 0.25 + np.arange(float(NPTS)) * ((L - 1.0) / NPTS)
    objs = []
    for side, (ip, jp) in dict(south=(run, np.full(NPTS, INSET)), north=(run, np.full(NPTS, L - INSET)),
                               west=(np.full(NPTS, INSET), run), east=(np.full(NPTS, L - INSET), run)).items():
        ang = 0.05 + 1e-4 * np.arange(NPTS)
        objs.append(("grid1_%s_r" % side, ip, jp, None, "zeta, temp, salt"))
        objs.append(("grid1_%s_u" % side, ip + 0.5, jp, ang, "ubar, u"))
        objs.append(("grid1_%s_v" % side, ip, jp + 0.5, ang, "vbar, v"))
    return objs


def main():
    import romsgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_cost.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    L, N, NT, dt = bench.C3_L, bench.C3_N, bench.NT, bench.C3_DT
    m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, NT, salinity=True, nonlin_eos=True, lmd=romsgpu.LMD_ICELAND,
                                dt=dt, ndtfast=bench.NDTFAST, sizex=bench.C3_DX * L, sizey=bench.C3_DX * L)
    objs = iceland_like(L)
    m.extract_begin(*CHILD)
    for name, ip, jp, ang, ov in objs:
        m.extract_add(name, ip, jp, ov, ang=ang)
    m.step(4)
    m.sync()
    nobj, mismatch, nchd, nptot, huv = m.extract_state()
    say("Child-boundary extraction (roms_gpu_calc_extract, k_ext_interp + k_ext_remap): cost at C3 on one MI355X.")
    say("Produced by: python tools/extract_cost.py")
    say("C3 %dx%dx%d; %d objects, %d points, N_chd = %d, remap %s, Hz_u/Hz_v stored %s; %d samples per figure" %
        (L, L, N, nobj, nptot, nchd, mismatch, huv, args.samples))
    m.calc_extract()
    for trial in range(2):   # the second figure is the one to read (first: cold caches, clocks)
        a, b = m.time_calc_extract(args.samples)
        say("calc_extract pass %d: interpolation %7.3f ms/sample   remap %7.3f ms/sample   both %7.3f ms/sample" %
            (trial + 1, a / args.samples, b / args.samples, (a + b) / args.samples))
    sample_ms = (a + b) / args.samples
    # the alternative: the host fetches the 3-D arrays and interpolates itself
    tot_b, tot_s = 0.0, 0.0
    for name in ("u", "v", "t", "Hz", "Hz_u", "Hz_v"):
        m.sync()
        t0 = time.perf_counter()
        arr = m.get(name)
        dts = time.perf_counter() - t0
        tot_b += arr.nbytes
        tot_s += dts
        say("copy_out %-5s %8.1f MB  %8.1f ms  %6.2f GB/s" % (name, arr.nbytes / 1e6, 1e3 * dts, arr.nbytes / dts / 1e9))
        del arr
    one = 8.0 * (L + 4) * (L + 4) * N
    seven_ms = 1e3 * 7 * one / (tot_b / tot_s)
    say("copy_out total %.1f MB in %.1f ms (%.2f GB/s); seven one-slot arrays (%.1f MB each) at that rate: %.1f ms" %
        (tot_b / 1e6, 1e3 * tot_s, tot_b / tot_s / 1e9, one / 1e6, seven_ms))
    say("extraction on the device: %.3f ms per sample = 1/%.0f of the seven-array download" % (sample_ms, seven_ms / sample_ms))

    def run(sampling):
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.step(1)
            if sampling:
                m.calc_extract()
        m.sync()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    run(True)
    say("step (Hz_u/Hz_v stored) alone / step + sample, ms per step over %d steps, five alternations:" % args.steps)
    p, q = [], []
    for _ in range(5):
        p.append(run(False))
        q.append(run(True))
        say("  %8.3f  %8.3f" % (p[-1], q[-1]))
    mp, mq = sorted(p)[2], sorted(q)[2]
    say("medians %8.3f  %8.3f  -> sampling adds %.3f ms = %.2f %% of the step" % (mp, mq, mq - mp, 100 * (mq - mp) / mp))
    # the same step with nothing armed: what storing Hz_u, Hz_v costs
    m.extract_begin(*CHILD)
    r = [run(False) for _ in range(5)]
    say("step with nothing armed (Hz_u/Hz_v not stored): median %8.3f ms of %s" % (sorted(r)[2], ["%.3f" % x for x in r]))
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
