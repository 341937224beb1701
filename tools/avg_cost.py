"""Cost of the device averaging on the C3 case of bench.py,
one box, one session:

  * tools/membw's streaming figures (the copy lines are the yardstick),
  * roms_gpu_calc_avg alone, HIP events on the library stream over --samples
    full samples (the old mean read: one untimed sample opens the window),
    default mask and full mask: ms per sample, algorithmic bytes, TB/s,
  * set_HUV as bench.py --full measures it (Model.time_routine, bench.py's
    pass count): the streaming routine the sample kernel is judged against,
  * the step with and without a sample after it, five alternations.

Algorithmic bytes of one sample: 3 passes per plain field (source read, old
mean read, new mean written), 5 for rho under SPLIT_EOS (rho1, qp1, z_r), 4
for omega (We, Wi), 6 for w (ROMS_WRT_W: FlxU, FlxV, u, v, old mean, new mean,
a launch of k_wvlcty of its own; tools/wvlcty_cost.py times it alone), over
interior cells as bench.py counts them; the coef == 1 saving is left out.
"Full mask" is romsgpu.WRT_ALL, which holds w since ABI 29: figures recorded
before that (profiles/avg_cost.txt) are without it.

usage: python tools/avg_cost.py [--samples 20] [--steps 10] [--no-membw]
"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ucla-roms_amd"))

import bench  # noqa: E402  (C3 constants, routine_passes, HBM_PEAK_GBS)


def membw():
    exe = os.path.join(ROOT, "tools", "membw")
    if not os.path.exists(exe):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", exe + ".hip", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300).stdout
    copy = [float(m.group(1)) for m in re.finditer(r"^copy .*?([\d.]+) GB/s", out, re.M)]
    return out, (max(copy) if copy else None)


def sample_bytes(mask, I, J, N, NT):
    W = romsgpu.WRT
    c2, c3, c3w = 8.0 * I * J, 8.0 * I * J * N, 8.0 * I * J * (N + 1)
    b = 0.0
    for k in ("Z", "Ub", "Vb", "Hbls", "Hbbl"):
        b += 3 * c2 if mask & W[k] else 0.0
    for k in ("U", "V"):
        b += 3 * c3 if mask & W[k] else 0.0
    b += 3 * c3 * NT if mask & W["T"] else 0.0
    b += 5 * c3 if mask & W["R"] else 0.0
    b += 4 * c3w if mask & W["O"] else 0.0
    b += 6 * c3 if mask & W.get("W", 0) else 0.0
    for k in ("Akv", "Akt", "Aks"):
        b += 3 * c3w if mask & W[k] else 0.0
    return b


def main():
    global romsgpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-membw", action="store_true")
    args = ap.parse_args()
    copy = None
    if not args.no_membw:   # its own process, before this one opens the GPU
        out, copy = membw()
        print("tools/membw (845 MB arrays):")
        print(out.rstrip())
        print("copy yardstick: %.1f GB/s = %.3f of %.0f GB/s" % (copy, copy / bench.HBM_PEAK_GBS, bench.HBM_PEAK_GBS))
    import ctypes

    import romsgpu
    L, N, NT, dt = bench.C3_L, bench.C3_N, bench.NT, bench.C3_DT
    m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, NT, salinity=True, nonlin_eos=True, lmd=romsgpu.LMD_ICELAND,
                                dt=dt, ndtfast=bench.NDTFAST, sizex=bench.C3_DX * L, sizey=bench.C3_DX * L)
    m.step(4)
    m.sync()
    print("C3 %dx%dx%d NT=%d, %d samples per figure" % (L, L, N, NT, args.samples))
    res = {}
    for name, mask in (("default mask (Z Ub Vb U V T)", romsgpu.WRT_DEFAULT), ("full mask", romsgpu.WRT_ALL)):
        m.avg_begin(mask)
        m.calc_avg(m.time(dt))   # opens the window: the timed samples all read the old mean
        ms = ctypes.c_double()
        for _ in range(2):       # the second figure is reported (first: cold caches, clocks)
            m._chk(m.L.roms_gpu_time_calc_avg(args.samples, ctypes.byref(m.t), ctypes.byref(ms)), "time_calc_avg")
        per = ms.value / args.samples
        nb = sample_bytes(mask, L, L, N, NT)
        gbs = nb / (per * 1e-3) / 1e9
        res[name] = gbs
        print("calc_avg %-30s %7.3f ms/sample  %6.2f GB  %6.3f TB/s  %.3f of peak%s" %
              (name, per, nb / 1e9, gbs / 1e3, gbs / bench.HBM_PEAK_GBS,
               "  %.3f of copy" % (gbs / copy) if copy else ""))
    # set_HUV as bench.py --full times it
    hms, hn = m.time_routine("set_HUV", 3)
    hb = 8.0 * bench.routine_passes(NT, bench.NT_TS, lmd=True)["set_HUV"] * L * L * N
    hg = hb / (hms * 1e-3) / 1e9
    print("set_HUV (time_routine, %d calls)         %7.3f ms/call    %6.2f GB  %6.3f TB/s  %.3f of peak%s" %
          (hn, hms, hb / 1e9, hg / 1e3, hg / bench.HBM_PEAK_GBS, "  %.3f of copy" % (hg / copy) if copy else ""))
    # the step with and without a sample after it
    m.avg_begin(romsgpu.WRT_DEFAULT)

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
    print("step alone / step + default-mask sample, ms per step over %d steps, five alternations:" % args.steps)
    a, b = [], []
    for _ in range(5):
        a.append(run(False))
        b.append(run(True))
        print("  %8.3f  %8.3f" % (a[-1], b[-1]))
    ma, mb = sorted(a)[2], sorted(b)[2]
    print("medians %8.3f  %8.3f  -> sampling adds %.3f ms = %.1f %% of the step" % (ma, mb, mb - ma, 100 * (mb - ma) / ma))
    m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
