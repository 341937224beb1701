"""do_particles of particles.F restated in numpy, one particle at a time in
the reference's order of operations: rhs_particles (:475-573) with interp_2D /
interp_3D (:621-659), advance_particles (:213-267), exchange_particles
(:661-840) and sort_particles (:902-931).  The expected values of every GPU
test of the particles come from here, never from the library.

One deviation, the library's own: Wp, which the
reference interpolates but never fills (:499-502 are commented out), is
((We + Wi) * pm) * pn, formed from the eight corners -- what those lines say.
For pz == nz the level pair of Wp is clamped to (nz-1, nz).  Where the
reference stops (:524-535, :675-682) the particle gets zero increments and is
counted (n_range), and a full message keeps what fits (n_overflow).

Arrays are in the model's layout, as Model.get returns them: (levels, Mm+4,
Lm+4), element (i, j) at [j+1, i+1]; u, v are one time slot (N levels), We,
Wi, Hz the stored arrays, pm, pn planes.  A particle is 13 words (WORDS).
Several ranks run in one process: `Ranks` holds each rank's fields and list
and moves the messages itself.
"""
import math

import numpy as np

WORDS = ("tag", "px", "py", "pz", "pu", "pv", "pw", "prx", "pry", "prz", "prxm", "prym", "przm")
NPV = 13
BIG_NUMBER = 10000000
DIRS = ("w", "e", "s", "n", "sw", "se", "nw", "ne")          # the library's message directions
OPP = dict(w="e", e="w", s="n", n="s", sw="ne", ne="sw", se="nw", nw="se")
ARRIVE = ("sw", "s", "se", "w", "e", "nw", "n", "ne")          # :746-838
STEP = dict(w=(-1, 0), e=(1, 0), s=(0, -1), n=(0, 1), sw=(-1, -1), se=(1, -1), nw=(-1, 1), ne=(1, 1))


def interp3(f, x, y, z):
    """interp_3D: weights as products left to right, the sum in array-element order (first index fastest)."""
    wt = ((1 - x) * (1 - y) * (1 - z), x * (1 - y) * (1 - z), (1 - x) * y * (1 - z), x * y * (1 - z),
          (1 - x) * (1 - y) * z, x * (1 - y) * z, (1 - x) * y * z, x * y * z)
    s = f[0] * wt[0]
    for q in range(1, 8):
        s = s + f[q] * wt[q]
    return s


def interp2(f, x, y):
    wt = ((1 - x) * (1 - y), x * (1 - y), (1 - x) * y, x * y)
    s = f[0] * wt[0]
    for q in range(1, 4):
        s = s + f[q] * wt[q]
    return s


def box3(a, i, j, k0):
    """a(i:i+1, j:j+1, k:k+1) in array-element order; k0 is the array's first index of level k."""
    return [float(a[k0 + c, j + 1 + b, i + 1 + q]) for c in (0, 1) for b in (0, 1) for q in (0, 1)]


def box2(a, i, j):
    return [float(a[j + 1 + b, i + 1 + q]) for b in (0, 1) for q in (0, 1)]


class Rank:
    """One rank: its fields, its list and the counters the library reports."""

    def __init__(self, nx, ny, nz, dt, exch=(0, 0, 0, 0), mynode=0, npmx=1 << 30, caps=None, sort=False):
        self.nx, self.ny, self.nz, self.dt = nx, ny, nz, float(dt)
        self.exch = dict(zip("wesn", exch))      # west, east, south, north_msg_exch
        self.mynode, self.npmx, self.sort = mynode, npmx, sort
        self.caps = caps or {d: 1 << 30 for d in DIRS}
        self.part = np.zeros((0, NPV))
        self.first = True
        self.ntag = 0
        self.count = dict(n_sur=0, n_bot=0, n_lost=0, n_moved=0, n_range=0, n_overflow=0)
        self.F = None

    def fields(self, u, v, We, Wi, Hz, pm, pn):
        self.F = dict(u=u, v=v, We=We, Wi=Wi, Hz=Hz, pm=pm, pn=pn)

    def add(self, px, py, pz):
        """part_add with zmode 0: tags go on from ntag; zero velocities and increments (:179-185, :347-354)."""
        n = len(px)
        new = np.zeros((n, NPV))
        new[:, 0] = np.arange(1, n + 1) + self.ntag + BIG_NUMBER * self.mynode
        new[:, 1], new[:, 2], new[:, 3] = px, py, pz
        self.part = np.vstack([self.part, new])
        self.ntag += n

    # ---- rhs_particles :475-573 ----
    def rhs(self):
        F, nx, ny, nz, dt = self.F, self.nx, self.ny, self.nz, self.dt
        for p in self.part:
            px, py, pz = float(p[1]), float(p[2]), float(p[3])
            if not pz < 2 * nz:
                p[7] = p[8] = p[9] = 0.0
                continue
            if not (-0.5 <= px <= nx + 0.5 and -0.5 <= py <= ny + 0.5 and 0.0 <= pz <= nz):   # the reference stops
                self.count["n_range"] += 1
                p[7] = p[8] = p[9] = 0.0
                continue
            i, j = math.floor(px + 0.5), math.floor(py + 0.5)
            k = min(max(math.floor(pz + 0.5), 1), nz - 1)
            iu, jv = math.floor(px + 1.0), math.floor(py + 1.0)
            kw = min(math.floor(pz), nz - 1)
            x, y, z = px - i + 0.5, py - j + 0.5, pz - k + 0.5
            xu, yv, zw = px - iu + 1.0, py - jv + 1.0, pz - kw
            pm, pn = box2(F["pm"], i, j), box2(F["pn"], i, j)
            we, wi = box3(F["We"], i, j, kw), box3(F["Wi"], i, j, kw)
            wp = [((we[q] + wi[q]) * pm[q & 3]) * pn[q & 3] for q in range(8)]
            pu = interp3(box3(F["u"], iu, j, k - 1), xu, y, z)
            pv = interp3(box3(F["v"], i, jv, k - 1), x, yv, z)
            pw = interp3(wp, x, y, zw)
            pdxi, pdyi = interp2(pm, x, y), interp2(pn, x, y)
            pdz = interp3(box3(F["Hz"], i, j, k - 1), x, y, z)
            p[4], p[5], p[6] = pu, pv, pw
            p[7], p[8], p[9] = dt * pu * pdxi, dt * pv * pdyi, dt * pw / pdz

    # ---- advance_particles :213-267 ----
    def advance(self):
        self.rhs()
        P = self.part
        if self.first:
            self.first = False
            P[:, 10:13] = P[:, 7:10]
        for p in P:
            for a in (1, 2, 3):
                p[a] = float(p[a]) + 1.5 * float(p[a + 6]) - 0.5 * float(p[a + 9])
            if p[3] < 0:
                p[3] = 0.02
                self.count["n_bot"] += 1
            if p[3] > self.nz:
                p[3] = self.nz - 0.02
                self.count["n_sur"] += 1
        P[:, 10:13] = P[:, 7:10]

    # ---- exchange_particles :684-732: who leaves, where to, with which coordinates ----
    def pack(self, active):
        """Marks the leavers dead (pz = 10*nz) and returns {direction: [particle, ..]} in list order.  `active`:
        the directions in which exchange_data sends (:958-1072); a corner message of the west branch that is
        never sent loses its particles."""
        nx, ny, nz, ex = self.nx, self.ny, self.nz, self.exch
        out = {d: [] for d in DIRS}
        for p in self.part:
            if not p[3] < nz:
                continue
            d = None
            if p[1] > nx:
                if ex["e"]:
                    if p[2] > ny and ex["n"]:
                        p[1] -= nx
                        p[2] -= ny
                        d = "ne"
                    elif p[2] < 0 and ex["s"]:
                        p[1] -= nx
                        d = "se"
                    else:
                        p[1] -= nx
                        d = "e"
            elif p[1] < 0.0:
                if ex["w"]:
                    if p[2] > ny:
                        p[2] -= ny
                        d = "nw"
                    elif p[2] < 0:
                        d = "sw"
                    else:
                        d = "w"
            elif p[2] > ny:
                if ex["n"]:
                    p[2] -= ny
                    d = "n"
            elif p[2] < 0.0:
                if ex["s"]:
                    d = "s"
            else:
                continue
            if d is not None and active[d]:
                if len(out[d]) < self.caps[d]:
                    out[d].append(p.copy())
                    self.count["n_moved"] += 1
                else:
                    self.count["n_overflow"] += 1
            else:
                self.count["n_lost"] += 1
            p[3] = 10 * nz
        return out

    def receive(self, msgs):
        """:746-838: msgs[h] came from direction h; appended in the order sw, s, se, w, e, nw, n, ne."""
        rows = [self.part[self.part[:, 3] < 2 * self.nz]]   # remsort: the dead go (order kept)
        for h in ARRIVE:
            for p in msgs.get(h, []):
                q = p.copy()
                if "e" in h:
                    q[1] += self.nx
                if "n" in h:
                    q[2] += self.ny
                rows.append(q[None, :])
        self.part = np.vstack(rows)
        if len(self.part) > self.npmx:
            self.count["n_overflow"] += len(self.part) - self.npmx
            self.part = self.part[:self.npmx]

    # ---- sort_particles :902-931 (the dead are gone already); np.argsort(kind="stable") stands for qsort ----
    def order(self):
        P = self.part
        key = np.floor(P[:, 1]) + np.floor(P[:, 2]) * self.nx + np.floor(P[:, 3]) * self.nx * self.ny
        self.part = P[np.argsort(key, kind="stable")]

    def state(self):
        return dict(self.count, np=len(self.part), ntag=self.ntag)


class Ranks:
    """np_xi x np_eta ranks of one grid (rank = inode + jnode*np_xi, mpi_setup.F); a periodic direction makes the
    end ranks neighbours, on one rank its own."""

    def __init__(self, ranks, np_xi=1, np_eta=1, ew_periodic=False, ns_periodic=False):
        self.r, self.npx, self.npe, self.ewp, self.nsp = ranks, np_xi, np_eta, ew_periodic, ns_periodic

    def peer(self, rank, d):
        jn, i_n = divmod(rank, self.npx)
        di, dj = STEP[d]
        ok_i = di == 0 or self.ewp or 0 <= i_n + di < self.npx
        ok_j = dj == 0 or self.nsp or 0 <= jn + dj < self.npe
        if not (ok_i and ok_j):
            return None
        return (i_n + di) % self.npx + ((jn + dj) % self.npe) * self.npx

    def do_particles(self):
        sent = []
        for q, r in enumerate(self.r):
            r.advance()
            sent.append(r.pack({d: self.peer(q, d) is not None for d in DIRS}))
        for q, r in enumerate(self.r):
            msgs = {}
            for h in DIRS:
                p = self.peer(q, h)
                if p is not None:
                    msgs[h] = sent[p][OPP[h]]
            r.receive(msgs)
            if r.sort:
                r.order()


def exch_flags(np_xi, np_eta, rank, ew_periodic, ns_periodic):
    """west, east, south, north_msg_exch of a rank."""
    jn, i_n = divmod(rank, np_xi)
    return (int(ew_periodic or i_n > 0), int(ew_periodic or i_n < np_xi - 1), int(ns_periodic or jn > 0),
            int(ns_periodic or jn < np_eta - 1))


def rank_extent(LL, np_, node):
    """(length, SW-corner offset) of a subdomain along one direction (mpi_setup.F:110-154)."""
    base = (LL + np_ - 1) // np_
    off = np_ * base - LL
    sw = 0 if node == 0 else node * base - off // 2
    n = base - (off // 2 if node == 0 else 0) - ((off + 1) // 2 if node == np_ - 1 else 0)
    return n, sw


def cut(a, isw, jsw, nx, ny):
    """A rank's array with its halos out of the single domain's (periodic halos must be filled in `a`)."""
    return np.ascontiguousarray(a[..., jsw:jsw + ny + 4, isw:isw + nx + 4])


def of_model(m, rank_obj):
    """Hands a Rank the fields do_particles reads, downloaded from the model: u, v(nnew), We, Wi, Hz, pm, pn."""
    N, s = m.N, m.t.nnew
    rank_obj.fields(m.get("u")[(s - 1) * N:s * N], m.get("v")[(s - 1) * N:s * N], m.get("We"), m.get("Wi"), m.get("Hz"),
                    m.get("pm")[0], m.get("pn")[0])
