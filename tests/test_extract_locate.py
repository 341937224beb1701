"""find_local_points of extract_data.F on the CPU (no GPU needed): the host-only
entry roms_gpu_extract_locate against a Python restatement, on an 18 x 12
domain split 3 x 2.  A rank keeps the first contiguous run of an object's
points inside its subdomain, as the reference does (it assumes contiguity)."""
import numpy as np
import pytest

import romsgpu as R

LLM, MMM, NPX, NPE = 18, 12, 3, 2


def ranks():
    for r in range(NPX * NPE):
        jn, inn = divmod(r, NPX)
        nx, isw = R.rank_extent(LLM, NPX, inn)
        ny, jsw = R.rank_extent(MMM, NPE, jn)
        yield r, nx, ny, isw, jsw


def find_local_points(nx, ny, isw, jsw, gi, gj):
    """The reference's loops; (start_idx 1-based, np), (0, 0) when no point is inside."""
    li, lj = np.asarray(gi, float) - isw, np.asarray(gj, float) - jsw
    inside = [(li[q] >= 0 and li[q] < nx and lj[q] >= 0 and lj[q] < ny) for q in range(len(li))]
    if True not in inside:
        return 0, 0
    s = inside.index(True)
    e = len(inside) - 1
    for q in range(s, len(inside)):
        if not inside[q]:
            e = q - 1
            break
    return s + 1, e - s + 1


def both(nx, ny, isw, jsw, gi, gj):
    got = R.extract_locate(nx, ny, isw, jsw, gi, gj)
    assert got == find_local_points(nx, ny, isw, jsw, gi, gj)
    return got


def test_diagonal_line_is_split_into_disjoint_contiguous_ranges():
    n = 61
    gi = np.linspace(0.25, LLM - 0.25, n)
    gj = np.linspace(0.25, MMM - 0.25, n)
    owner = np.zeros(n, int)
    for r, nx, ny, isw, jsw in ranks():
        s, c = both(nx, ny, isw, jsw, gi, gj)
        if c:
            owner[s - 1:s - 1 + c] += 1
            li, lj = gi[s - 1:s - 1 + c] - isw, gj[s - 1:s - 1 + c] - jsw
            assert (li >= 0).all() and (li < nx).all() and (lj >= 0).all() and (lj < ny).all()
    # a monotonic diagonal enters every subdomain at most once: each point has exactly one owner
    assert (owner == 1).all()


def test_points_on_the_subdomain_edges_follow_the_inequalities():
    for r, nx, ny, isw, jsw in ranks():
        j = jsw + 0.5 * ny
        gi = np.array([isw - 1.0, isw + 0.0, isw + nx - 0.5, isw + nx + 0.0, isw + nx + 1.0])
        s, c = both(nx, ny, isw, jsw, gi, np.full(5, j))
        assert (s, c) == (2, 2)   # 0 is inside (>= 0), nx is not (< nx)
        i = isw + 0.5 * nx
        gj = np.array([jsw + 0.0, jsw + ny - 1e-9, jsw + ny + 0.0])
        assert both(nx, ny, isw, jsw, np.full(3, i), gj) == (1, 2)


def test_a_line_that_re_enters_keeps_its_first_run_only():
    _, nx, ny, isw, jsw = next(ranks())
    gi = np.array([0.5, 1.5, 2.5, nx + 0.5, nx + 1.5, 3.5, 4.5, 5.5]) + isw
    gj = np.full(gi.size, jsw + 1.5)
    assert both(nx, ny, isw, jsw, gi, gj) == (1, 3)
    # starting outside: the first run begins where the line first enters
    gi = np.array([nx + 0.5, 0.5, 1.5, nx + 0.5, 2.5]) + isw
    assert both(nx, ny, isw, jsw, gi, np.full(5, jsw + 1.5)) == (2, 2)


def test_a_line_outside_has_no_points_and_nan_is_outside():
    for r, nx, ny, isw, jsw in ranks():
        gi = np.linspace(-5.0, -0.5, 7)
        assert both(nx, ny, isw, jsw, gi, np.full(7, jsw + 1.0)) == (0, 0)
        assert both(nx, ny, isw, jsw, [np.nan, isw + 1.0], [jsw + 1.0, np.nan]) == (0, 0)
    assert R.extract_locate(6, 6, 0, 0, [], []) == (0, 0)
    with pytest.raises(ValueError):
        R.extract_locate(0, 6, 0, 0, [1.0], [1.0])
