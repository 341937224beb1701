"""The particle messages over the two transports that tests/test_gpu_part.py
does not reach with its threads (halo_exchange_messages, halo.hip): RCCL, as
one process that sends all eight messages to itself (ROMS_GPU_RCCL_SELF, the
way tests/test_gpu_multirank.py covers the field exchanges: RCCL refuses two
ranks on one GPU), and the host channel with one process per rank through a
file allgather, as tests/test_gpu_ipc.py runs it.  The list is the
eight-direction list of tests/test_part_ref.py on its analytic flow; expected
values come from the restatement (host channel) and from the on-device wrap of
a rank without a communicator (RCCL), which test_gpu_part.py holds to the
restatement."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import part_ref
from part_ref import Rank, Ranks
from test_part_ref import CALLS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "ucla-roms_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
sys.path.insert(0, sys.argv[1])
import numpy as np, romsgpu, part_ref
from test_part_ref import CALLS, eight_list, quadrant_flow
case = dict(case_id=0, LLm=32, MMm=24, N=16, NT=1, salinity=False, nonlin_eos=False, dt=5.0, ndtfast=60, sizex=12.8e3,
            sizey=3.2e3)
LL, MM = case["LLm"], case["MMm"]
gx, gy, gz = eight_list(LL, MM, 16, 12, True)

def run(m, lists):
    mine = (gx >= m.iSW) & (gx < m.iSW + m.Lm) & (gy >= m.jSW) & (gy < m.jSW + m.Mm)
    m.part_begin(4 * gx.size)
    m.part_add(gx[mine] - m.iSW, gy[mine] - m.jSW, gz[mine])
    m.step(1)
    u, v = quadrant_flow(m.N, m.shape2, case["dt"], m.get("pm")[0][3, 3], m.get("pn")[0][3, 3])
    for name, a in (("u", u), ("v", v)):
        f, s = m.get(name), m.t.nnew
        f[(s - 1) * m.N:s * m.N] = a
        m.put(name, f)
    for _ in range(CALLS):
        m.do_particles()
        lists.append(m.particles())
    return m.part_state()
"""

RCCL_SCRIPT = COMMON + r"""
a, b = [], []
m = romsgpu.Model.from_case(**case)
sa = run(m, a)
m.close()
h = romsgpu.comm_create(romsgpu.comm_unique_id(), 1, 0, 0)
m = romsgpu.Model.from_case(np_xi=1, np_eta=1, comm=h, rank=0, **case)
sb = run(m, b)
m.close()
romsgpu.comm_destroy(h)
assert sa == sb and sa["n_moved"] >= 8 and sa["n_lost"] == 0, (sa, sb)
for c, (x, y) in enumerate(zip(a, b)):
    assert x.shape == y.shape and np.array_equal(x, y), c
print("PART_RCCL_OK", sa["n_moved"])
"""

HOST_SCRIPT = COMMON + r"""
rank, chan = int(sys.argv[2]), sys.argv[3]
ag = romsgpu.FileAllgather(chan, 4, rank)
h = romsgpu.comm_create_host(4, rank, ag)
m = romsgpu.Model.from_case(np_xi=2, np_eta=2, comm=h, rank=rank, **case)
lists = []
st = run(m, lists)
r = part_ref.Rank(m.Lm, m.Mm, m.N, case["dt"])
part_ref.of_model(m, r)
np.savez(os.path.join(chan, "out%d.npz" % rank), geo=np.array([m.Lm, m.Mm, m.iSW, m.jSW]),
         state=np.array([st[k] for k in romsgpu.PART_STATE]), **{"list%d" % c: x for c, x in enumerate(lists)}, **r.F)
m.close()
romsgpu.comm_destroy(h)
print("PART_HOST_OK")
"""


def test_rccl_self_routed_messages_equal_the_on_device_wrap():
    env = dict(os.environ, ROMS_GPU_RCCL_SELF="1")
    r = subprocess.run([sys.executable, "-c", RCCL_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "PART_RCCL_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_host_channel_processes_equal_the_restatement():
    from test_part_ref import eight_list
    LL, MM, N, dt = 32, 24, 16, 5.0
    gx, gy, gz = eight_list(LL, MM, 16, 12, True)
    with tempfile.TemporaryDirectory() as td:
        ps = [subprocess.Popen([sys.executable, "-c", HOST_SCRIPT, ROOT, str(q), td], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True) for q in range(4)]
        outs = []
        for p in ps:
            try:
                o, e = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for q in ps:
                    q.kill()
                raise
            outs.append((p.returncode, o, e))
        for rc, o, e in outs:
            assert rc == 0 and "PART_HOST_OK" in o, (rc, o[-2000:], e[-3000:])
        got = [dict(np.load(os.path.join(td, "out%d.npz" % q))) for q in range(4)]
    ranks = []
    for q in range(4):
        nx, ny, isw, jsw = (int(x) for x in got[q]["geo"])
        r = Rank(nx, ny, N, dt, exch=part_ref.exch_flags(2, 2, q, True, True), mynode=q)
        r.F = {k: got[q][k] for k in ("u", "v", "We", "Wi", "Hz", "pm", "pn")}
        mine = (gx >= isw) & (gx < isw + nx) & (gy >= jsw) & (gy < jsw + ny)
        r.add(gx[mine] - isw, gy[mine] - jsw, gz[mine])
        ranks.append(r)
    R = Ranks(ranks, 2, 2, True, True)
    for c in range(CALLS):
        R.do_particles()
        for q, r in enumerate(ranks):
            x = got[q]["list%d" % c]
            assert x.shape == r.part.shape and np.array_equal(x, r.part), (c, q)
    import romsgpu
    for q, r in enumerate(ranks):
        assert dict(zip(romsgpu.PART_STATE, (int(v) for v in got[q]["state"]))) == r.state(), q
    assert sum(r.count["n_moved"] for r in ranks) >= 8 and all(r.count["n_lost"] == 0 for r in ranks)
