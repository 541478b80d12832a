"""Test infrastructure: plain numpy restatements around the sharded single-linkage reduction --
the pair distances from the oracle, MSTPrim's recurrence (reference tree/MSTPrim.cpp:356-533), and the
local half of a Boruvka round over a row block.  Nothing in famsa_amd/ imports this."""
import numpy as np

from famsa_amd.lcsgpu import MST_EDGE, MST_KEY

M64 = (1 << 64) - 1
NO_D = 0x7FEFFFFFFFFFFFFF


def pair_distances(oracle, codes, offsets, kind=1):
    """D[i, j] = D[j, i] = Transform<double>(LCS(ref = max(i,j), partner = min(i,j))): the triangle's orientation."""
    n = len(offsets) - 1
    lens = np.diff(offsets.astype(np.int64))
    tri = oracle.triangle(codes, offsets)
    fn = oracle.lib.oracle_dist_indel075_f64 if kind == 1 else oracle.lib.oracle_dist_indel_f64
    D = np.zeros((n, n), np.float64)
    for i in range(1, n):
        row = tri[i * (i - 1) // 2: i * (i - 1) // 2 + i]
        D[i, :i] = [fn(int(l), int(lens[i]), int(lens[j])) for j, l in enumerate(row)]
        D[:i, i] = D[i, :i]
    return D


def prim_edges(D):
    """MSTPrim::run_view's recurrence over symmetric distances: keys (d, ~pack(min, max)) compared
    lexicographically; returns MST_EDGE[n-1] in insertion order."""
    n = len(D)
    key = [(np.finfo(np.float64).max, 0)] * n
    alive = set(range(1, n))
    cur, out = 0, np.zeros(max(n - 1, 0), MST_EDGE)
    k = 0
    while alive:
        for v in alive:
            d = float(D[cur, v])
            if d <= key[v][0]:
                a, b = min(cur, v), max(cur, v)
                s = (d, M64 ^ ((a << 32) + b))
                if s < key[v]:
                    key[v] = s
        best = min(alive, key=lambda v: key[v])
        packed = M64 ^ key[best][1]
        out[k] = (packed >> 32, packed & 0xFFFFFFFF, key[best][0])
        k += 1
        alive.remove(best)
        cur = best
    return out


def block_best(D, comp, r0, r1):
    """Local half of a Boruvka round over the row block [r0, r1): for every vertex v the smallest key
    (distance bits, ~pack) among the pairs (u, v) the block holds -- (u < v, v in the block) and
    (u > v, u in the block) -- with comp[u] != comp[v]."""
    n = len(D)
    out = np.zeros(n, MST_KEY)
    out["dist_bits"] = NO_D
    out["id"] = M64
    bits = D.view(np.uint64)
    for v in range(n):
        best = (NO_D, M64)
        us = list(range(0, v)) if r0 <= v < r1 else []
        us += list(range(max(v + 1, r0), r1))
        for u in us:
            if comp[u] == comp[v]:
                continue
            a, b = min(u, v), max(u, v)
            k = (int(bits[u, v]), M64 ^ ((a << 32) + b))
            if k < best:
                best = k
        out[v] = best
    return out


HUGE = np.nextafter(np.finfo(np.float64).max, 0.0)  # Transform's value for an LCS of 0
_POW075 = {}


def _pow075_table(oracle, n_entries):
    """t[indel] = the oracle's own scalar Transform<double, indel075_div_lcs> at l = 1 (pow(indel, 0.75) / 1.0), filled once."""
    t = _POW075.get("t")
    if t is None or len(t) < n_entries:
        fn = oracle.lib.oracle_dist_indel075_f64
        t = np.array([fn(1, i + 2, 0) for i in range(n_entries)], np.float64)  # indel = (i + 2) + 0 - 2 * 1
        _POW075["t"] = t
    return t


def square_lcs(lcs, n):
    """A packed lower triangle (row i at i (i - 1) / 2) as a symmetric square of the same integer type; a square is
    symmetrised from its lower triangle (ref = the larger id: the triangle's orientation)."""
    lcs = np.asarray(lcs)
    if lcs.ndim == 1:
        assert len(lcs) == n * (n - 1) // 2
        sq = np.zeros((n, n), lcs.dtype)
        for i in range(1, n):
            sq[i, :i] = lcs[i * (i - 1) // 2: i * (i - 1) // 2 + i]
    else:
        assert lcs.shape == (n, n)
        sq = np.tril(lcs, -1)
    return sq + sq.T


class DistanceRows:
    """The rows of distances_from_lcs made one at a time from a symmetric LCS square (9000^2 doubles are not kept)."""

    def __init__(self, sq, lens, kind, oracle):
        self.sq, self.lens, self.kind = sq, np.asarray(lens, np.int64), kind
        self.table = _pow075_table(oracle, 2 * int(self.lens.max(initial=0)) + 1) if kind == 1 else None

    def __len__(self):
        return len(self.lens)

    def __getitem__(self, i):
        l = self.sq[i].astype(np.int64)
        indel = self.lens[i] + self.lens - 2 * l
        num = self.table[indel] if self.kind == 1 else indel.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = num / l.astype(np.float64)  # IEEE division: the bits of the scalar form
        d[l == 0] = HUGE
        d[i] = 0.0
        return d


def distances_from_lcs(lcs, lens, kind, oracle):
    """pair_distances from LCS values already in hand (a packed lower triangle or a square whose lower triangle is
    used): the symmetric float64 matrix, bit for bit what the oracle's scalar Transform gives pair by pair."""
    n = len(lens)
    rows = DistanceRows(square_lcs(lcs, n), lens, kind, oracle)
    D = np.zeros((n, n), np.float64)
    for i in range(n):
        D[i] = rows[i]
    return D


def prim_edges_fast(D):
    """prim_edges with one numpy pass per step: the same recurrence, the same key order (d, ~pack(min, max)), the same
    insertion order from vertex 0.  D: a matrix or anything whose D[i] is row i (DistanceRows)."""
    n = len(D)
    out = np.zeros(max(n - 1, 0), MST_EDGE)
    if n < 2:
        return out
    ids = np.arange(n, dtype=np.uint64)
    kd = np.full(n, np.finfo(np.float64).max)
    kid = np.zeros(n, np.uint64)
    alive = np.ones(n, bool)
    alive[0] = False
    cur = 0
    for k in range(n - 1):
        d = np.asarray(D[cur], np.float64)
        c = np.uint64(cur)
        cid = ~((np.minimum(ids, c) << np.uint64(32)) + np.maximum(ids, c))
        upd = alive & ((d < kd) | ((d == kd) & (cid < kid)))
        kd[upd] = d[upd]
        kid[upd] = cid[upd]
        m = np.where(alive, kd, np.inf)
        cand = np.nonzero(m == m.min())[0]
        best = int(cand[np.argmin(kid[cand])])
        packed = M64 ^ int(kid[best])
        out[k] = (packed >> 32, packed & 0xFFFFFFFF, kd[best])
        alive[best] = False
        cur = best
    return out
