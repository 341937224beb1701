"""Cost of the device particles on the C3 case of bench.py,
one box, one session; writes profiles/part_cost.txt (--out):

  * tools/membw's copy rate, the yardstick of the streaming part (13 words
    read and 13 written per particle and call),
  * at two densities of romsgpu.part_full_seed chosen to give about 1e6 and
    1e7 particles, and in three list orders -- as seeded (column after column),
    shuffled (the worst case of an unsorted list) and cell-sorted
    (ROMS_PART_SORT) -- roms_gpu_time_do_particles over --samples calls: ms per
    whole call and ms of the rhs and advance kernel alone,
  * which of sort + sorted gather and unsorted gather wins at each density,
  * the whole call against the step it follows (roms_gpu_time_steps) and
    against the five 3-D downloads per step a host-side float code would need,
    at the PCIe rate of DESIGN.md section 6 (2.5 GB in 50 ms).

--pmc-run ORDER,NP seeds, arms and makes three calls and exits: the run to put
under  rocprofv3 --pmc FETCH_SIZE  (a pass of its own) for the rhs kernel's
fetched bytes per particle; --pmc-append ORDER,NP,CSV then appends the figure
of that pass's counter_collection.csv to the report (FETCH_SIZE is in KB; the
factor 2 of tools/pmc_traffic.py for wide coalesced reads is not applied to
this gather: with it the kernel would exceed the copy rate).

usage: python tools/part_cost.py [--samples 10] [--steps 10] [--no-membw] [--out profiles/part_cost.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ucla-roms_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402  (C3 constants)

PCIE_GBS = 2.5 / 0.050   # 2.5 GB in about 50 ms
SEED = 20260


def model():
    import romsgpu
    L, N = bench.C3_L, bench.C3_N
    m = romsgpu.Model.from_case(romsgpu.CASE_BASIN, L, L, N, bench.NT, salinity=True, nonlin_eos=True,
                                lmd=romsgpu.LMD_ICELAND, dt=bench.C3_DT, ndtfast=bench.NDTFAST, sizex=bench.C3_DX * L,
                                sizey=bench.C3_DX * L)
    m.step(4)
    m.sync()
    return m


def ppm3_for(m, target):
    """The density at which the columns' floor(h/(pm*pn)*ppm3) sum to about `target`."""
    inner = (slice(2, m.Mm + 2), slice(2, m.Lm + 2))
    vol = m.get("h")[0][inner] / (m.get("pm")[0][inner] * m.get("pn")[0][inner])
    ppm3 = target / vol.sum()
    for _ in range(8):
        ppm3 *= target / max(np.floor(vol * ppm3).sum(), 1.0)
    return ppm3


def arm(m, target, order):
    """The list of about `target` particles in `order`: seeded, shuffled or sorted.  Returns np."""
    import romsgpu
    rng = np.random.default_rng(SEED)
    npmx = int(1.2 * target) + 1000
    m.part_begin(npmx, sort=order == "sorted")
    n = romsgpu.part_full_seed(m, ppm3_for(m, target), rng)
    if order == "shuffled":
        P = m.particles()
        q = rng.permutation(P.shape[0])
        m.part_begin(npmx)
        m.part_add(P[q, 1], P[q, 2], P[q, 3])
    m.do_particles()   # the start call; with the flag the list is cell-sorted from here
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-membw", action="store_true")
    ap.add_argument("--pmc-run", default="")
    ap.add_argument("--pmc-append", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_cost.txt"))
    args = ap.parse_args()
    if args.pmc_append:
        import csv
        order, npart, path = args.pmc_append.split(",")
        v = [float(r["Counter_Value"]) for r in csv.DictReader(open(path))
             if "k_part_rhs_adv" in r["Kernel_Name"] and r["Counter_Name"] == "FETCH_SIZE"]
        with open(args.out, "a") as f:
            f.write("FETCH_SIZE of k_part_rhs_adv, %-8s order, np %s: %.0f KB per launch (mean of %d) = %.0f B per particle\n"
                    % (order, npart, sum(v) / len(v), len(v), 1024.0 * sum(v) / len(v) / float(npart)))
        return 0
    if args.pmc_run:
        order, target = args.pmc_run.split(",")
        m = model()
        n = arm(m, float(target), order)
        for _ in range(3):
            m.do_particles()
        print("pmc run: %s order, np %d, 4 calls" % (order, n))
        m.close()
        return 0
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Device particles (roms_gpu_do_particles, k_particles.hip): cost at C3 on one MI355X, one session.")
    say("Produced by: python tools/part_cost.py")
    copy = None
    if not args.no_membw:   # its own process, before this one opens the GPU
        import avg_cost
        out, copy = avg_cost.membw()
        say("tools/membw copy yardstick: %.1f GB/s" % copy)
    m = model()
    L, N = bench.C3_L, bench.C3_N
    ms = m.time_steps(args.steps)
    step_ms = (ms[0] if isinstance(ms, (tuple, list)) else ms) / args.steps
    field_mb = 8.0 * (L + 4) * (L + 4) * N / 1e6
    pcie_ms = 5 * field_mb / 1e3 / PCIE_GBS * 1e3
    say("C3 %dx%dx%d: step %.3f ms; five 3-D downloads (%.0f MB each) at %.0f GB/s: %.1f ms per step" %
        (L, L, N, step_ms, field_mb, PCIE_GBS, pcie_ms))
    n = args.samples
    for target in (1e6, 1e7):
        res = {}
        for order in ("seeded", "shuffled", "sorted"):
            np_ = arm(m, target, order)
            for _ in range(2):   # the second figure is reported (first: cold caches, clocks)
                whole, rhs = m.time_do_particles(n)
            res[order] = (whole / n, rhs / n)
            stream = 26 * 8.0 * np_ / 1e9   # 13 words read and written
            say("np %9d  %-8s  do_particles %8.3f ms   rhs+advance kernel %8.3f ms  (%5.1f ns/particle; streaming part "
                "%.3f GB%s)" % (np_, order, whole / n, rhs / n, 1e6 * rhs / n / np_, stream,
                                 " = %.3f ms at the copy rate" % (stream / copy * 1e3) if copy else ""))
        sort_cost = res["sorted"][0] - res["sorted"][1]
        base = res["seeded"][0] - res["seeded"][1]
        say("np ~%.0e: sort + permute adds %.3f ms per call; sorted call %.3f ms against %.3f ms as seeded and %.3f ms "
            "shuffled -> %s" % (target, sort_cost - base, res["sorted"][0], res["seeded"][0], res["shuffled"][0],
                                "the sort wins" if res["sorted"][0] < min(res["seeded"][0], res["shuffled"][0])
                                else "the sort wins only over a shuffled list" if res["sorted"][0] < res["shuffled"][0]
                                else "the unsorted list wins"))
        say("np ~%.0e: the call as seeded is %.2f %% of the step and 1/%.0f of the downloads" %
            (target, 100 * res["seeded"][0] / step_ms, pcie_ms / res["seeded"][0]))
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
