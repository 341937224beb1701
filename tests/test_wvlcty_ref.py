"""tests/wvlcty_ref.py, the numpy restatement every GPU test of w takes its
expected values from, is pinned here to the reference's own routine:
tests/golden/wvlcty_golden.npz holds the output of src/wvlcty.F, compiled
unchanged (cpp | mpc.py | flang -O2 -ffp-contract=off) in two builds, closed and
EW_PERIODIC + NS_PERIODIC, on a 9 x 6 x 4 grid with fixed pseudo-random FlxU,
FlxV, u, v, z_r, pm, pn (tests/golden/wvlcty_golden.py recorded it; the inputs
are in the file).  The routine got its Wvlc(.., 0:N) filled with a sentinel, so
the recording also shows which cells it leaves alone."""
import os

import numpy as np
import pytest

import wvlcty_ref

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wvlcty_golden.npz"))
SENT = float(G["sentinel"])


def run(name, **kw):
    Lm, Mm, N, ewp, nsp, nstp = (int(x) for x in G["dims_" + name])
    out = np.full((N, Mm + 4, Lm + 4), SENT)
    w = wvlcty_ref.wvlcty(G["FlxU"], G["FlxV"], G["u"][nstp - 1], G["v"][nstp - 1], G["z_r"], G["pm"], G["pn"],
                          bool(ewp), bool(nsp), out=out, **kw)
    return w, G["Wvlc_" + name], (Lm, Mm, N, ewp, nsp, nstp)


@pytest.mark.parametrize("name", ["closed", "periodic"])
def test_restatement_equals_the_reference_routine_bitwise(name):
    w, gold, (Lm, Mm, N, ewp, nsp, nstp) = run(name)
    assert (Lm, Mm, N) == (9, 6, 4) and (ewp, nsp) == ((1, 1) if name == "periodic" else (0, 0))
    assert np.all(gold[0] == SENT)                  # level 0 of (.., 0:N) is never written
    assert np.array_equal(w, gold[1:])              # computed cells, copies, corners and the cells left alone
    # the cells written are rows/columns 0..Mm+1 x 0..Lm+1 in both builds: computed 1..Lm plus the edge copies
    # when closed, computed 0..Lm+1 (the widened range) and no copies when periodic
    wrote = gold[1:] != SENT
    want = np.zeros_like(wrote)
    want[:, 1:Mm + 3, 1:Lm + 3] = True
    assert np.array_equal(wrote, want)
    inner = gold[1:, 2:Mm + 2, 2:Lm + 2]
    assert np.abs(inner).max() > 0
    if name == "closed":   # edges and corners are gradient copies
        g = gold[1:]
        assert np.array_equal(g[:, 2:Mm + 2, 1], g[:, 2:Mm + 2, 2]) and np.array_equal(g[:, 2:Mm + 2, Lm + 2], g[:, 2:Mm + 2, Lm + 1])
        assert np.array_equal(g[:, 1, 2:Lm + 2], g[:, 2, 2:Lm + 2]) and np.array_equal(g[:, Mm + 2, 2:Lm + 2], g[:, Mm + 1, 2:Lm + 2])
        assert np.array_equal(g[:, 1, 1], g[:, 2, 2]) and np.array_equal(g[:, Mm + 2, Lm + 2], g[:, Mm + 1, Lm + 1])
        assert np.array_equal(g[:, 1, Lm + 2], g[:, 2, Lm + 1]) and np.array_equal(g[:, Mm + 2, 1], g[:, Mm + 1, 2])
    else:                  # the rim is computed, not copied
        g = gold[1:]
        assert not np.array_equal(g[:, 2:Mm + 2, 1], g[:, 2:Mm + 2, 2])


def test_the_pin_is_sensitive():
    """Negative controls: the other slot of u, v, and the closed build's ranges on the periodic build, differ."""
    w, gold, (Lm, Mm, N, ewp, nsp, nstp) = run("closed")
    out = np.full_like(w, SENT)
    other = wvlcty_ref.wvlcty(G["FlxU"], G["FlxV"], G["u"][2 - nstp], G["v"][2 - nstp], G["z_r"], G["pm"], G["pn"],
                              False, False, out=out)
    assert not np.array_equal(other, gold[1:])
    out = np.full_like(w, SENT)
    closed_on_periodic = wvlcty_ref.wvlcty(G["FlxU"], G["FlxV"], G["u"][nstp - 1], G["v"][nstp - 1], G["z_r"], G["pm"],
                                           G["pn"], False, False, out=out)
    assert not np.array_equal(closed_on_periodic, G["Wvlc_periodic"][1:])


def test_fewer_than_two_levels_is_refused():
    with pytest.raises(ValueError):
        wvlcty_ref.wvlcty(G["FlxU"][:1], G["FlxV"][:1], G["u"][0][:1], G["v"][0][:1], G["z_r"][:1], G["pm"], G["pn"],
                          False, False)
