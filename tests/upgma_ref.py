"""Test infrastructure: UPGMA::computeTree (reference tree/UPGMA.cpp:114-295) restated in numpy float32, one vector
operation per merge, over a square float32 matrix -- the nearest-neighbour-array form with its strict '<' scans in
ascending index (numpy's argmin returns the first minimum) and its deliberately stale row minima.  Both averages:
(x + y) * 0.5f and 0.05f * (x + y) + 0.9f * min(x, y), one float32 rounding per operation.  Distances come from
oracle.dist_triangle_f32 (Transform<float, kind> in the oracle's C).  A helper for the tests of lcsgpu_upgma_batch, pinned
by test_upgma_ref.py; nothing in famsa_amd/ imports this."""
import numpy as np

BIG = np.float32(1e29)   # UPGMA::BIG_DIST
NONE = 0x7FFFFFFF


def dist_square(oracle, lcs_square, lens, kind=1):
    """The symmetric float32 matrix UPGMA::computeDistances fills, from lcs_square[k, c] = LCS(ref = member k, partner =
    member c): pair (i, j), j < i, takes the value with the LATER member as the ref.  The diagonal is +inf (never read)."""
    lcs_square = np.asarray(lcs_square)
    m = len(lens)
    ii, jj = np.tril_indices(m, -1)  # row-major over the lower triangle: i (i - 1) / 2 + j
    tri = oracle.dist_triangle_f32(lcs_square[ii, jj], lens, kind)
    D = np.full((m, m), np.inf, np.float32)
    D[ii, jj] = tri
    D[jj, ii] = tri
    return D


def upgma_tree(D, modified=False):
    """(left, right, ok): children of the internal nodes m .. 2m - 2 in the order they are made.  ok = False when a step
    finds no alive row with a key below BIG_DIST -- where the reference would pick nothing (and read out of bounds); the
    records from that step on are unspecified.  D is not changed."""
    D = np.array(D, np.float32, copy=True)
    m = len(D)
    left, right = np.zeros(max(m - 1, 0), np.int32), np.zeros(max(m - 1, 0), np.int32)
    if m < 2:
        return left, right, True
    idx = np.arange(m)
    np.fill_diagonal(D, np.inf)
    # the double loop at UPGMA.cpp:198-215 shows row r every other row once, in ascending index, with a strict '<'
    near = D.argmin(axis=1)
    mn = D[idx, near].copy()
    bad = ~(mn < BIG)
    mn[bad] = BIG
    near[bad] = NONE
    node = idx.copy()
    alive = np.ones(m, bool)
    half, c005, c09 = np.float32(0.5), np.float32(0.05), np.float32(0.9)
    for step in range(m - 1):
        keys = np.where(alive, mn, BIG)
        lmin = int(keys.argmin())
        if not keys[lmin] < BIG:
            return left, right, False
        rmin = int(near[lmin])
        others = alive.copy()
        others[lmin] = others[rmin] = False
        x, y = D[lmin], D[rmin]
        with np.errstate(over="ignore"):  # FLT_MAX + FLT_MAX = +inf, as in the reference
            new = c005 * (x + y) + c09 * np.minimum(x, y) if modified else (x + y) * half
        near[others & (near == rmin)] = lmin
        D[lmin, others] = new[others]
        D[others, lmin] = new[others]
        cand = np.where(others, new, np.float32(np.inf))
        j = int(cand.argmin())
        if cand[j] < BIG:
            mn[lmin], near[lmin] = cand[j], j
        else:
            mn[lmin], near[lmin] = BIG, NONE
        left[step], right[step] = node[lmin], node[rmin]
        node[lmin] = m + step
        alive[rmin] = False
    return left, right, True
