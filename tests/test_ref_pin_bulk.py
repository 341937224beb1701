"""or_bulk_flux against the reference's own calc_all_bulk_forces.

oracle/ref/build_ref.sh compiles bulk_frc.F from the reference tree,
unchanged, against stand-ins for its two I/O modules; set_bulk_frc is called
with the atmosphere already in its arrays (tests/branch_states.bulk_state):
  analytic  the atmosphere of or_ana_forces on a mid-run basin, which runs
            one arm of most branches (unstable air, delW <= 10, rain, no
            land, no ice);
  arms      stable and unstable air, no wind at all over a quarter of the
            basin (Wgus at its floor of 0.2 where stable), all three Charnock
            ranges, both sides of the current-feedback threshold, no rain
            over half, a block of land, surface water below and exactly at
            -1.8 degC.  bulk_arms restates these conditions from the inputs
            and the test asserts that every one holds somewhere.

The routine carries exp, log, sqrt, atan and powers, so bitwise agreement is
not promised between two runtimes.  Measured here, oracle (gcc, glibc)
against reference (flang, its runtime over the same glibc), largest
|a - b| / max|b| per field, both states, nrhs = nstp and nrhs = 3:

    sustr 0  svstr 0  sustr_r 0  svstr_r 0  stflx 0  swflx 0  srflx 0

every element equal.  The bound per field is four times the measured value
and no less than 8 ulp, so 8 * 2**-52 = 1.8e-15 throughout, well under the
1e-13 that keeps GPU-to-oracle at 1e-12 meaning GPU-to-reference.

Before this test the oracle (and k_bulk.hip) left out SEA_ICE_NOFLUX, which
set_global_definitions.h defines for every case: stflx(itemp) = 0, and
srflx = 0 under LMD_KPP, where t(N) <= -1.8.  On the 'arms' state that was
a relative difference of 0.86 in stflx and 0.77 in srflx at the nine cold
cells.

srflx is compared on the extended bounds 0:Lm+1 x 0:Mm+1 that the routine
works on: outside them the reference holds whatever set_frc_data read, the
oracle what srflx held before.  Not marked gpu.  Skips only where neither
the library nor the reference tree exists.
"""
import numpy as np
import pytest

import branch_states as bs
import oracle.ref as ref

ULP = 2.0 ** -52
MEASURED = {n: 0.0 for n in bs.BULK_OUT}
BOUND = {n: max(4.0 * MEASURED[n], 8.0 * ULP) for n in bs.BULK_OUT}
assert max(BOUND.values()) <= 1.0e-13

pytestmark = pytest.mark.skipif(not (ref.have_tree() or ref.available(ref.BULK)),
                                reason="neither oracle/_ref/libref_bulk.so nor a reference tree")


def run_reference(o):
    """set_bulk_frc on the state of the Oracle o (before or_bulk_flux has run on it)."""
    assert ref.available(ref.BULK)
    r = ref.RefLib(ref.BULK)
    r.load(o, any_sides=True)
    return r.bulk({n: o.field(n).copy() for n in bs.BULK_ATM}, {n: o.field(n).copy() for n in bs.BULK_OUT})


def written(name, a):
    return a[..., 1:-1, 1:-1] if name == "srflx" else a


def rel(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


@pytest.mark.parametrize("mode", ["nstp", "corr"])
@pytest.mark.parametrize("kind", ["analytic", "arms"])
def test_bulk_flux(kind, mode):
    cfg, o, tix = bs.bulk_state(kind, mode)
    arms = bs.bulk_arms(o, cfg, tix)
    if kind == "arms":
        missing = [k for k, v in arms.items() if not bool(np.any(v))]
        assert not missing, missing
    else:   # what the second state is for
        assert not np.any(arms["stable (Ri >= 0)"]) and not np.any(arms["land"]) and not np.any(arms["no rain"])
    for n in bs.BULK_OUT:   # start from a value no flux takes, to see what the routine writes
        o.field(n)[...] = 0.125
    before = {n: o.field(n).copy() for n in bs.BULK_OUT}
    out = run_reference(o)
    o.call("bulk_flux")
    errs = {n: rel(written(n, o.field(n)), written(n, out[n])) for n in bs.BULK_OUT}
    print(kind, mode, errs)
    bad = {n: e for n, e in errs.items() if not e <= BOUND[n]}
    assert not bad, bad
    for n in bs.BULK_OUT:   # the routine ran: every field moved, and stayed finite
        assert np.all(np.isfinite(out[n])) and not np.array_equal(written(n, out[n]), written(n, before[n])), n
    if kind == "arms":      # the sea-ice arm shows in the result
        E = (slice(1, -1), slice(1, -1))
        ice = arms["ice: t < -1.8"] | arms["ice: t = -1.8"]
        assert np.all(out["stflx"][0][E][ice] == 0.0) and np.all(out["srflx"][0][E][ice] == 0.0)
        assert np.all(out["stflx"][0][E][arms["no ice"]] != 0.0)
